// sm_k_retire.h -- retirement (DESIGN.md "4e. Retirement"): move the surfels that are out of fusion's reach out of the model.
// Included by sm_retire.hip only.  Four kernels, all streaming and bound by HBM:
//   k_retire_mark    per live slot 16 B pos_conf + 4 B time + 1 bit alive in; 1 bit retired-mask + 4 B per tile out.  Changes
//                    nothing in the model: a dry run ends after the scan and leaves no trace.
//   k_retire_scan    exclusive prefix of the per-tile counts (one workgroup; a model has at most 24 415 tiles)
//   k_retire_gather  per retired surfel 44 B of the five planes in, one 48-byte AoS record out at base + rank, staged through
//                    LDS so that every wave writes whole 16-byte lanes of consecutive lines
//   k_retire_clear   clears the retired bits in `alive` and books them as dead slots, exactly as a marking cull does
//                    (k_cull_lazy); the existing compaction then closes the gaps.  Its own launch, because the periodic
//                    policy must have the records on disk before the model changes.
#pragma once

#include "sm_device.h"

namespace sm {

// the predicate's constants, all fp32 (sm_c_api.h "sm_retire"): evaluated in exactly the order the header states
struct RetireArgs {
    float tick;          // float(tick): the time stamp the next frame will carry
    float min_age;       // float(min_age)
    float cx, cy, cz;    // camera centre (pose[12..14])
    float md2;           // min_distance * min_distance, rounded to fp32 once (on the host)
    int use_dist;        // 0: min_distance <= 0, the age gate alone
};

__device__ __forceinline__ bool retire_test(const RetireArgs &ra, const float4 &pc, float t_last)
{
    const float age = ra.tick - t_last;                  // index_map.vert:45 reads the same word
    const bool old = age > ra.min_age;
    const float dx = pc.x - ra.cx, dy = pc.y - ra.cy, dz = pc.z - ra.cz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const bool far = !ra.use_dist || d2 > ra.md2;
    return old && far;                                   // every comparison is false on a NaN
}

// One 1024-slot tile per workgroup iteration; each wave settles four 64-slot words (the layout of k_cull_lazy).
__global__ __launch_bounds__(256) void k_retire_mark(Model M, const DevState *__restrict__ st, RetireArgs ra,
                                                     const uint64_t *__restrict__ alive, uint64_t *__restrict__ mask,
                                                     uint32_t *__restrict__ tile_ret)
{
    __shared__ uint32_t s_cnt[4];
    const uint32_t N = st->count;
    const SurfelSet cur = M.s[st->cur];
    const uint32_t ntiles = (N + TILE - 1) / TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        float4 pv[4];
        float tv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {                    // unconditional, clamped: all loads of the lane in flight together
            const uint32_t kc = min((tile * TILE_WORDS + r * 4 + wave) * 64u + lane, N - 1u);
            pv[r] = cur.pos_conf[kc];
            tv[r] = cur.time[kc];
        }
        uint32_t cnt = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t word = tile * TILE_WORDS + (uint32_t)(r * 4 + wave);
            const uint64_t base = (uint64_t)word * 64u;
            uint64_t range = 0ull;
            if (base < N) { const uint64_t rem = (uint64_t)N - base; range = rem >= 64 ? ~0ull : ((1ull << rem) - 1ull); }
            // slots a deferred-compaction cull has killed are neither retired nor kept
            const uint64_t m = __ballot(retire_test(ra, pv[r], tv[r])) & range & alive[word];
            if (lane == 0) mask[word] = m;
            cnt += (uint32_t)__popcll(m);
        }
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) tile_ret[tile] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);   // partials, no same-address atomics
        __syncthreads();
    }
}

// tile_base[t] = retired surfels in the tiles before t; total[0] = all of them, total[1] = the occupied slots they were counted over
__global__ __launch_bounds__(1024) void k_retire_scan(const DevState *__restrict__ st, const uint32_t *__restrict__ tile_ret,
                                                      uint32_t *__restrict__ tile_base, uint32_t *__restrict__ total)
{
    __shared__ uint32_t s_scan[17];
    const uint32_t N = st->count;
    const uint32_t ntiles = (N + TILE - 1) / TILE;
    uint32_t run = 0;
    for (uint32_t b = 0; b < ntiles; b += 1024u) {
        const uint32_t t = b + threadIdx.x;
        const uint32_t v = t < ntiles ? tile_ret[t] : 0u;
        uint32_t tot;
        const uint32_t excl = block_scan_1024(v, &tot, s_scan);
        if (t < ntiles) tile_base[t] = run + excl;
        run += tot;
    }
    if (threadIdx.x == 0) { total[0] = run; total[1] = N; }
}

// The records with rank in [r0, r1) go to dst[(rank - r0) * 3 ..]: the caller's whole buffer in one launch, or one staging chunk
// per launch.  A tile's retired surfels are consecutive in the output, so the tile is laid out in LDS as it will lie in memory
// and then stored by all 256 threads, 16 bytes per lane, consecutive lanes on consecutive addresses.
__global__ __launch_bounds__(256) void k_retire_gather(Model M, const DevState *__restrict__ st, const uint64_t *__restrict__ mask,
                                                       const uint32_t *__restrict__ tile_ret, const uint32_t *__restrict__ tile_base,
                                                       const uint32_t *__restrict__ total, float4 *__restrict__ dst, uint32_t r0,
                                                       uint32_t r1)
{
    __shared__ float4 s_rec[TILE * 3];                   // 48 KiB
    __shared__ uint64_t s_mask[TILE_WORDS];
    const uint32_t N = total[1];                         // the slots the masks were made over
    const SurfelSet cur = M.s[st->cur];
    const uint32_t ntiles = (N + TILE - 1) / TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t cnt = tile_ret[tile], gb = tile_base[tile];            // workgroup-uniform
        if (cnt == 0u || gb >= r1 || gb + cnt <= r0) continue;
        if (threadIdx.x < TILE_WORDS) s_mask[threadIdx.x] = mask[tile * TILE_WORDS + threadIdx.x];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int w = r * 4 + wave;
            const uint64_t m = s_mask[w];
            if ((m >> lane) & 1ull) {
                uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                for (int x = 0; x < w; ++x) rank += (uint32_t)__popcll(s_mask[x]);
                const uint32_t k = (tile * TILE_WORDS + (uint32_t)w) * 64u + lane;      // < N: the mask has no bit beyond
                s_rec[rank * 3 + 0] = cur.pos_conf[k];
                s_rec[rank * 3 + 1] = make_float4(__uint_as_float(cur.color[k]), 0.0f, cur.init_time[k], cur.time[k]);
                s_rec[rank * 3 + 2] = cur.norm_rad[k];
            }
        }
        __syncthreads();
        const uint32_t lo = (max(gb, r0) - gb) * 3u, hi = (min(gb + cnt, r1) - gb) * 3u;   // float4s of this tile inside the window
        const size_t off = (size_t)gb * 3u;
        for (uint32_t i = lo + threadIdx.x; i < hi; i += 256u) dst[off + i - (size_t)r0 * 3u] = s_rec[i];
        __syncthreads();
    }
}

// one thread per mask word; the retired become dead slots (alive bit 0, tile_dead, DevState::garbage) for the next compaction
__global__ __launch_bounds__(256) void k_retire_clear(DevState *__restrict__ st, const uint64_t *__restrict__ mask,
                                                      const uint32_t *__restrict__ tile_ret, const uint32_t *__restrict__ total,
                                                      uint64_t *__restrict__ alive, uint32_t *__restrict__ tile_dead)
{
    const uint32_t N = total[1];
    const uint32_t nwords = ((N + TILE - 1) / TILE) * TILE_WORDS;
    for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < nwords; w += gridDim.x * 256u) {
        const uint64_t m = mask[w];
        if (m) alive[w] &= ~m;
        if ((w % TILE_WORDS) == 0u) {
            const uint32_t c = tile_ret[w / TILE_WORDS];
            if (c) tile_dead[w / TILE_WORDS] += c;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) st->garbage += total[0];
}

}  // namespace sm
