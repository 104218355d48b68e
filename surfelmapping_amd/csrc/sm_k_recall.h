// sm_k_recall.h -- paging in (DESIGN.md "4g. Paging in"): the records of map files that lie within `radius` of the camera come
// back into the model.  Included by sm_recall.hip only.  A chunk is at most 2^20 records of one file, a block 256 of them
// (at most 4096 blocks per chunk).  Three kernels, all streaming and bound by HBM:
//   k_recall_mark    per block 768 float4s of records in (through LDS: consecutive lanes on consecutive addresses); four 64-bit
//                    near-masks, one count and one box of the finite centres out.  Changes nothing anywhere else: a COUNT
//                    call ends after the scan.
//   k_recall_scan    one workgroup: the exclusive prefix of the block counts, the chunk's total, the box of the chunk, and the
//                    running total of the call (so that the placement needs no host round trip between chunks)
//   k_recall_place   append: the near records of a block go into the SoA planes at base + running total + prefix + rank, in
//                    file order, straight from the LDS copy; slots at or above MAX_VERTICES are not written (the host then
//                    reports SM_E_CAPACITY and never publishes the count).  keep (MOVE only): the records that stay are
//                    packed in LDS as they will lie in memory and stored 16 bytes per lane to device staging.
#pragma once

#include "sm_device.h"

namespace sm {

constexpr int RECALL_BLOCK = 256;                        // records per workgroup
constexpr int RECALL_MAX_BLOCKS = 4096;                  // blocks of a full chunk (2^20 records)

// the predicate's constants, all fp32 (sm_c_api.h "sm_recall"): evaluated in exactly the order the header states
struct RecallArgs {
    float cx, cy, cz;    // camera centre (pose[12..14])
    float r2;            // radius * radius, rounded to fp32 once (on the host)
};

// the complement of retire_test's `far` for finite rows (sm_k_retire.h): the same expression, the comparison turned round
__device__ __forceinline__ bool recall_test(const RecallArgs &ra, const float4 &pc)
{
    const float dx = pc.x - ra.cx, dy = pc.y - ra.cy, dz = pc.z - ra.cz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 <= ra.r2;                                  // false on a NaN; an infinite d2 is above every finite r2
}

// what the scan leaves per chunk (read back by the host): total near records, the running total BEFORE this chunk, and the
// box of the chunk's finite centres (lo = +inf, hi = -inf if it has none), and the largest non-NaN last-update time of its records
// (-inf if it has none: what sm_warp_by_time's file skip asks the index)
struct RecallChunk { uint32_t total, run_before; float lx, ly, lz, hx, hy, hz, tmax; };

__device__ __forceinline__ float recall_wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float recall_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// a block's 768 float4s into LDS, consecutive lanes on consecutive addresses (k_maps_intake's load)
__device__ __forceinline__ void recall_load_block(const float4 *__restrict__ rec, uint32_t first, uint32_t m, float4 *s_rec)
{
    const float4 *src = rec + (size_t)first * 3;
    for (uint32_t i = threadIdx.x; i < m * 3u; i += 256u) s_rec[i] = src[i];
}

// mask[4 * b + w]: near bits of records 256 b + 64 w ...; blk_cnt[b]: their number; box[2 b], box[2 b + 1]: min / max of the
// finite centres of the block; box[2 b + 1].w: the largest non-NaN time of the block
__global__ __launch_bounds__(256) void k_recall_mark(const float4 *__restrict__ rec, uint32_t n, RecallArgs ra, uint64_t *__restrict__ mask,
                                                     uint32_t *__restrict__ blk_cnt, float4 *__restrict__ box)
{
    __shared__ float4 s_rec[RECALL_BLOCK * 3];           // 12 KiB
    __shared__ float s_red[4][7];
    __shared__ uint32_t s_cnt[4];
    const uint32_t first = blockIdx.x * (uint32_t)RECALL_BLOCK;
    const uint32_t m = min((uint32_t)RECALL_BLOCK, n - first);              // >= 1: the grid is ceil(n / 256)
    recall_load_block(rec, first, m, s_rec);
    __syncthreads();
    const bool have = threadIdx.x < m;
    const float4 pc = have ? s_rec[threadIdx.x * 3] : make_float4(0, 0, 0, 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t near = __ballot(have && recall_test(ra, pc));
    const float INF = __uint_as_float(0x7F800000u);
    // the box bounds the rows that can be near: those whose three coordinates are finite (x - x is 0 for a finite x only)
    const bool fin = have && (pc.x - pc.x == 0.0f) && (pc.y - pc.y == 0.0f) && (pc.z - pc.z == 0.0f);
    const float lx = recall_wave_min(fin ? pc.x : INF), ly = recall_wave_min(fin ? pc.y : INF), lz = recall_wave_min(fin ? pc.z : INF);
    const float hx = recall_wave_max(fin ? pc.x : -INF), hy = recall_wave_max(fin ? pc.y : -INF), hz = recall_wave_max(fin ? pc.z : -INF);
    const float tau = have ? s_rec[threadIdx.x * 3 + 1].w : -INF;
    const float tm = recall_wave_max(tau == tau ? tau : -INF);
    if (lane == 0) {
        mask[(size_t)blockIdx.x * 4 + wave] = near;
        s_cnt[wave] = (uint32_t)__popcll(near);
        s_red[wave][0] = lx; s_red[wave][1] = ly; s_red[wave][2] = lz;
        s_red[wave][3] = hx; s_red[wave][4] = hy; s_red[wave][5] = hz; s_red[wave][6] = tm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_cnt[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);   // partials, no same-address atomics
        float4 lo, hi;
        lo.x = fminf(fminf(s_red[0][0], s_red[1][0]), fminf(s_red[2][0], s_red[3][0]));
        lo.y = fminf(fminf(s_red[0][1], s_red[1][1]), fminf(s_red[2][1], s_red[3][1]));
        lo.z = fminf(fminf(s_red[0][2], s_red[1][2]), fminf(s_red[2][2], s_red[3][2]));
        lo.w = 0.0f;
        hi.x = fmaxf(fmaxf(s_red[0][3], s_red[1][3]), fmaxf(s_red[2][3], s_red[3][3]));
        hi.y = fmaxf(fmaxf(s_red[0][4], s_red[1][4]), fmaxf(s_red[2][4], s_red[3][4]));
        hi.z = fmaxf(fmaxf(s_red[0][5], s_red[1][5]), fmaxf(s_red[2][5], s_red[3][5]));
        hi.w = fmaxf(fmaxf(s_red[0][6], s_red[1][6]), fmaxf(s_red[2][6], s_red[3][6]));
        box[2 * (size_t)blockIdx.x] = lo;
        box[2 * (size_t)blockIdx.x + 1] = hi;
    }
}

// blk_base[b] = near records in the blocks before b; *out = the chunk's tally; *run (the call's running total) += the total
__global__ __launch_bounds__(1024) void k_recall_scan(uint32_t nblk, const uint32_t *__restrict__ blk_cnt, const float4 *__restrict__ box,
                                                      uint32_t *__restrict__ blk_base, uint32_t *__restrict__ run, RecallChunk *__restrict__ out)
{
    __shared__ uint32_t s_scan[17];
    __shared__ float s_red[16][7];
    const float INF = __uint_as_float(0x7F800000u);
    float lx = INF, ly = INF, lz = INF, hx = -INF, hy = -INF, hz = -INF, tm = -INF;
    uint32_t sum = 0;
    for (uint32_t b0 = 0; b0 < nblk; b0 += 1024u) {      // at most four rounds
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < nblk ? blk_cnt[b] : 0u;
        uint32_t tot;
        const uint32_t excl = block_scan_1024(v, &tot, s_scan);
        if (b < nblk) {
            blk_base[b] = sum + excl;
            const float4 lo = box[2 * (size_t)b], hi = box[2 * (size_t)b + 1];
            lx = fminf(lx, lo.x); ly = fminf(ly, lo.y); lz = fminf(lz, lo.z);
            hx = fmaxf(hx, hi.x); hy = fmaxf(hy, hi.y); hz = fmaxf(hz, hi.z); tm = fmaxf(tm, hi.w);
        }
        sum += tot;
    }
    lx = recall_wave_min(lx); ly = recall_wave_min(ly); lz = recall_wave_min(lz);
    hx = recall_wave_max(hx); hy = recall_wave_max(hy); hz = recall_wave_max(hz); tm = recall_wave_max(tm);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = lx; s_red[wave][1] = ly; s_red[wave][2] = lz;
        s_red[wave][3] = hx; s_red[wave][4] = hy; s_red[wave][5] = hz; s_red[wave][6] = tm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            lx = fminf(lx, s_red[w][0]); ly = fminf(ly, s_red[w][1]); lz = fminf(lz, s_red[w][2]);
            hx = fmaxf(hx, s_red[w][3]); hy = fmaxf(hy, s_red[w][4]); hz = fmaxf(hz, s_red[w][5]); tm = fmaxf(tm, s_red[w][6]);
        }
        const uint32_t before = *run;
        *run = before + sum;
        *out = RecallChunk{sum, before, lx, ly, lz, hx, hy, hz, tm};
    }
}

// Block b of the chunk: its near records to slots base0 + run_before + blk_base[b] + rank of the model's planes,
// its other records to keep[(256 b - blk_base[b] + rank among them) * 3 ..] (keep != null).  Both ranks follow file order.
// `cap`: MAX_VERTICES -- a slot at or above it is not written; the caller sees the overflow in the running total.
__global__ __launch_bounds__(256) void k_recall_place(const float4 *__restrict__ rec, uint32_t n, Model M, const DevState *__restrict__ st,
                                                      const uint64_t *__restrict__ mask, const uint32_t *__restrict__ blk_cnt,
                                                      const uint32_t *__restrict__ blk_base, const RecallChunk *__restrict__ chunk,
                                                      uint32_t base0, uint32_t cap, float4 *__restrict__ keep)
{
    __shared__ float4 s_rec[RECALL_BLOCK * 3];           // 12 KiB
    const uint32_t cnt = blk_cnt[blockIdx.x];            // workgroup-uniform
    const uint32_t first = blockIdx.x * (uint32_t)RECALL_BLOCK;
    const uint32_t m = min((uint32_t)RECALL_BLOCK, n - first);
    if (cnt == 0u && !keep) return;
    recall_load_block(rec, first, m, s_rec);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m0 = mask[(size_t)blockIdx.x * 4 + 0], m1 = mask[(size_t)blockIdx.x * 4 + 1], m2 = mask[(size_t)blockIdx.x * 4 + 2],
                   m3 = mask[(size_t)blockIdx.x * 4 + 3];
    const uint64_t mw = wave == 0 ? m0 : wave == 1 ? m1 : wave == 2 ? m2 : m3;
    // near records before this one in the block
    uint32_t rank = (uint32_t)__popcll(mw & ((1ull << lane) - 1ull));
    if (wave > 0) rank += (uint32_t)__popcll(m0);
    if (wave > 1) rank += (uint32_t)__popcll(m1);
    if (wave > 2) rank += (uint32_t)__popcll(m2);
    const bool have = threadIdx.x < m;
    const bool near = (mw >> lane) & 1ull;               // no bit beyond m: the mark tested `have`
    float4 pc = make_float4(0, 0, 0, 0), ct = pc, nr = pc;
    if (have) { pc = s_rec[threadIdx.x * 3 + 0]; ct = s_rec[threadIdx.x * 3 + 1]; nr = s_rec[threadIdx.x * 3 + 2]; }
    const uint32_t bb = blk_base[blockIdx.x];
    if (near) {
        const uint64_t k = (uint64_t)base0 + chunk->run_before + bb + rank;
        if (k < cap) store_record(M.s[st->cur], (uint32_t)k, pc, ct, nr);
    }
    if (!keep || cnt == m) return;                       // (workgroup-uniform)
    __syncthreads();                                     // every lane holds its record: the LDS copy may be overwritten
    if (have && !near) {
        const uint32_t kr = threadIdx.x - rank;          // records that stay before this one in the block
        s_rec[kr * 3 + 0] = pc; s_rec[kr * 3 + 1] = ct; s_rec[kr * 3 + 2] = nr;
    }
    __syncthreads();
    float4 *dst = keep + ((size_t)first - bb) * 3u;
    const uint32_t hi = (m - cnt) * 3u;
    for (uint32_t i = threadIdx.x; i < hi; i += 256u) dst[i] = s_rec[i];
}

}  // namespace sm
