// sm_k_tile.h -- spatial tiling of a map set (DESIGN.md "4s. Spatial tiling"; the specification is sm_c_api.h's "tiling").
// Included by sm_tile.hip only.  The grid, the probe and the claim are sm_d_simplify.h's; sm_voxel.hip ranks the
// records a reading keeps (k_rank_scan) between k_tile_mark and k_tile_select, and sorts a batch's (key, idx) pairs (pair_sort).
// Records come as 48-byte AoS rows (three float4), a chunk of a map file or the exported model.
//   k_tile_count        pass 1: per placed record its tile; the lanes of a wave with one tile are counted together, and only the
//                       lowest of them claims the tile in the open-addressing table (64-bit atomicCAS, a probe loop bounded by
//                       the table size) and adds their number to its count.  Loose records are tallied, one add per wave.
//   k_tile_list         the table's occupied slots as (tile, count) pairs, in any order: the host sorts them
//   k_tile_mark<LOOSE>  pass 2: how many records of each block of 256 a reading keeps -- those whose tile lies in the batch's range,
//                       or the loose ones -- and, of the former, the OR and the AND of their keys (at most one atomic each per wave)
//   k_tile_select<LOOSE> every kept record to slot `rank` of the batch (three 16-byte stores), its key to key[rank], rank to idx[rank];
//                       ranks run on across chunks and files, so the batch fills in global-id order
//   k_tile_gather       out[i] = rec[idx[i]]: three lanes per record, consecutive lanes store consecutive 16-byte pieces
// No lane waits for another.  Integer atomics only.
#pragma once

#include "sm_d_simplify.h"

namespace sm {

struct TileRange { unsigned long long lo, hi; int shift3; };   // tiles lo..hi (lo > hi: none); shift3 = 3 * tile_shift

// bit i of u to bit 3 i (u < 2^21)
__device__ __forceinline__ unsigned long long tile_spread(uint32_t u)
{
    unsigned long long x = u;
    x = (x | x << 32) & 0x001F00000000FFFFull;
    x = (x | x << 16) & 0x001F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// placed: the 51-bit Morton key of the record's cell; false: the record is loose.  Only the position is examined.
__device__ __forceinline__ bool tile_key(const SimplifyArgs &a, const float4 &pc, unsigned long long &M)
{
    const float p[3] = {pc.x, pc.y, pc.z};
    M = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double d = (double)p[k] - (double)a.origin[k];
        if (!(fabs(d) < 16777216.0)) return false;       // (NaN and inf fail here)
        const long long X = (long long)floor(d * 65536.0);
        long long c = X / a.V;
        if (X - c * a.V < 0) --c;                        // floor division
        if (c < -65536 || c > 65535) return false;
        M |= tile_spread((uint32_t)(c + 65536)) << k;
    }
    return true;
}

// ---- pass 1: T has key and n (the count) only
__global__ __launch_bounds__(256) void k_tile_count(const float4 *__restrict__ rec, uint32_t n, SimplifyArgs a, int shift3, SimplifyTable T)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned long long tile = SIMP_EMPTY;
    bool placed = false;
    if (t < n) {
        unsigned long long M;
        placed = tile_key(a, rec[(size_t)t * 3], M);
        if (placed) tile = M >> shift3;
    }
    // the lanes of the wave with one tile, consecutive or not, are counted by the lowest of them: a loop over the wave's distinct
    // tiles (one or two for a file in drive order, the tiles a wave straddles otherwise), wave-uniform
    bool head = placed && !a.combine;
    uint32_t len = 1u;
    for (unsigned long long todo = a.combine ? __ballot(placed) : 0ull; todo;) {
        const int first = __ffsll(todo) - 1;
        const unsigned long long same = __ballot(placed && tile == __shfl(tile, first));
        if (lane == first) { head = true; len = (uint32_t)__popcll(same); }
        todo &= ~same;
    }
    simp_claim(a, T, tile, head, [&](uint32_t sl) { atomicAdd(&T.n[sl], len); });
    const unsigned long long loose = __ballot(t < n && !placed);
    if (loose && lane == 0) atomicAdd(&T.tally[SIMP_N_LOOSE], (uint32_t)__popcll(loose));
}

// tally[SIMP_RUN] counts the pairs; there are at most `cap` (the table's distinct tiles, checked by the host before)
__global__ __launch_bounds__(256) void k_tile_list(SimplifyTable T, uint32_t cap, unsigned long long *__restrict__ tiles, uint32_t *__restrict__ counts)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long key = sl <= T.mask ? T.key[sl] : SIMP_EMPTY;
    const bool has = key != SIMP_EMPTY;
    const unsigned long long m = __ballot(has);
    if (!m) return;
    uint32_t base = 0;
    if (lane == __ffsll(m) - 1) base = atomicAdd(&T.tally[SIMP_RUN], (uint32_t)__popcll(m));
    base = __shfl(base, __ffsll(m) - 1);
    const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (has && at < cap) { tiles[at] = key; counts[at] = T.n[sl]; }
}

// ---- pass 2.  LOOSE: the reading keeps the loose records; otherwise those of the tiles r.lo..r.hi
template <bool LOOSE>
__device__ __forceinline__ bool tile_kept(const SimplifyArgs &a, const TileRange &r, const float4 &pc, unsigned long long &M)
{
    const bool placed = tile_key(a, pc, M);
    if constexpr (LOOSE) return !placed;
    const unsigned long long tile = M >> r.shift3;
    return placed && tile >= r.lo && tile <= r.hi;
}

// bits[0] |= every kept key, bits[1] &= every kept key (not LOOSE)
template <bool LOOSE>
__global__ __launch_bounds__(256) void k_tile_mark(const float4 *__restrict__ rec, uint32_t n, SimplifyArgs a, TileRange r, uint32_t *__restrict__ blk_cnt,
                                                   unsigned long long *__restrict__ bits)
{
    __shared__ uint32_t s_cnt[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long M = 0;
    const bool kept = t < n && tile_kept<LOOSE>(a, r, rec[(size_t)t * 3], M);
    const unsigned long long m = __ballot(kept);
    if constexpr (!LOOSE) {
        if (m) {                                         // wave-uniform
            unsigned long long o = kept ? M : 0ull, d = kept ? M : ~0ull;
#pragma unroll
            for (int x = 32; x; x >>= 1) { o |= __shfl_xor(o, x); d &= __shfl_xor(d, x); }
            // (OR only grows and AND only shrinks, so a value read earlier that already holds this wave's bits settles it)
            if (lane == 0) {
                const unsigned long long seen_or = __atomic_load_n(&bits[0], __ATOMIC_RELAXED), seen_and = __atomic_load_n(&bits[1], __ATOMIC_RELAXED);
                if ((seen_or | o) != seen_or) atomicOr(&bits[0], o);
                if ((seen_and & d) != seen_and) atomicAnd(&bits[1], d);
            }
        }
    }
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// cap: the slots of out, key and idx; a rank beyond it is dropped (the host compares the ranks given with its plan)
template <bool LOOSE>
__global__ __launch_bounds__(256) void k_tile_select(const float4 *__restrict__ rec, uint32_t n, SimplifyArgs a, TileRange r,
                                                     const uint32_t *__restrict__ blk_base, uint32_t cap, float4 *__restrict__ out,
                                                     unsigned long long *__restrict__ key, uint32_t *__restrict__ idx)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    unsigned long long M = 0;
    float4 pc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool kept = false;
    if (t < n) {
        pc = rec[(size_t)t * 3];
        kept = tile_kept<LOOSE>(a, r, pc, M);
    }
    const uint32_t rank = simp_rank_in_chunk(kept, blk_base, nullptr);
    if (!kept || rank >= cap) return;
    out[(size_t)rank * 3] = pc;
    out[(size_t)rank * 3 + 1] = rec[(size_t)t * 3 + 1];
    out[(size_t)rank * 3 + 2] = rec[(size_t)t * 3 + 2];
    if constexpr (!LOOSE) { key[rank] = M; idx[rank] = rank; }
}

// ---- out[i] = rec[idx[first + i]], i < n: lane t moves 16-byte piece t % 3 of record t / 3.  cap: the records at rec
__global__ __launch_bounds__(256) void k_tile_gather(const float4 *__restrict__ rec, const uint32_t *__restrict__ idx, uint32_t first, uint32_t n,
                                                     uint32_t cap, float4 *__restrict__ out)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n * 3u) return;
    const uint32_t i = t / 3u, piece = t - i * 3u;
    const uint32_t from = idx[first + i];
    if (from < cap) out[t] = rec[(size_t)from * 3 + piece];
}

}  // namespace sm
