// sm_k_simplify.h -- voxel-cell simplification (DESIGN.md "4p. Simplification"; the specification is sm_c_api.h's "sm_simplify").
// Included by sm_simplify.hip only; the table and what fills and reads it are sm_d_simplify.h's, which the lookup tables share
// (sm_k_voxel.h); between flag and emit sm_voxel.hip ranks the representatives.
// Records come as 48-byte AoS rows (three float4), a chunk of a map file or the exported model.
//   k_simplify_insert  pass 1: per regular record the key into the open-addressing table (64-bit atomicCAS, a probe loop bounded
//                      by the table size) and the contribution into the key's accumulators (integer atomics, no return value).
//                      With `combine` the lanes of a wave that follow each other with one key -- a source column of one frame --
//                      are summed by a segmented shuffle reduction first and only the run's first lane goes to memory.
//   k_simplify_flag    pass 2: per record its code (not a representative | loose | the slot of the cell it is `first` of), the
//                      representatives per block of 256, and the call's tallies (one atomic per wave)
//   k_simplify_emit    every representative writes its finished record at its rank (simp_rank_in_chunk): three 16-byte stores
// No kernel waits for another lane: the accumulators are initialised before pass 1 starts (two memsets), so a claimed key can be
// added to at once, and a key that finds no slot sets the sticky error word and gives up.
#pragma once

#include "sm_d_simplify.h"

namespace sm {

// ---- pass 1: n records at rec, ids gid0 + t
__global__ __launch_bounds__(256) void k_simplify_insert(const float4 *__restrict__ rec, uint32_t n, uint32_t gid0, SimplifyArgs a, SimplifyTable T)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    unsigned long long key = SIMP_EMPTY;
    bool reg = false;
    SimpContrib c{};
    if (t < n) {
        const float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
        uint32_t off[3];
        reg = simp_classify(a, pc, ct, nr, key, off);
        if (reg) simp_contribution(pc, ct, nr, off, gid0 + t, c);
        else key = SIMP_EMPTY;
    }
    simp_insert<true>(a, T, key, reg, c);
}

// ---- pass 2
__global__ __launch_bounds__(256) void k_simplify_flag(const float4 *__restrict__ rec, uint32_t n, uint32_t gid0, SimplifyArgs a, SimplifyTable T,
                                                       uint32_t *__restrict__ code, uint32_t *__restrict__ blk_cnt)
{
    __shared__ uint32_t s_cnt[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t c = SIMP_NONE, cell_n = 0;
    bool lost = false;
    if (t < n) {
        const float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
        unsigned long long key;
        uint32_t off[3], sl = 0;
        bool claimed;
        if (!simp_classify(a, pc, ct, nr, key, off)) c = SIMP_LOOSE;
        else if (!simp_probe(T, key, false, sl, claimed)) lost = true;
        else if (T.first[sl] == gid0 + t) { c = sl; cell_n = T.n[sl]; }
        code[t] = c;
    }
    const unsigned long long reps = __ballot(c != SIMP_NONE), loose = __ballot(c == SIMP_LOOSE), merged = __ballot(cell_n >= 2u);
    uint32_t largest = cell_n;
#pragma unroll
    for (int o = 32; o; o >>= 1) largest = max(largest, (uint32_t)__shfl_xor(largest, o));
    if (lane == 0) {
        s_cnt[wave] = (uint32_t)__popcll(reps);
        if (loose) atomicAdd(&T.tally[SIMP_N_LOOSE], (uint32_t)__popcll(loose));
        if (merged) atomicAdd(&T.tally[SIMP_MERGED], (uint32_t)__popcll(merged));
        if (largest > 1u) atomicMax(&T.tally[SIMP_LARGEST], largest);
    }
    if (lost) atomicOr(&T.tally[SIMP_ERR], 4u);
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// out[(rank - base) * 3 ..]: base = info->x (a chunk's output begins at out), 0 without info (out is the whole output)
__global__ __launch_bounds__(256) void k_simplify_emit(const float4 *__restrict__ rec, uint32_t n, SimplifyArgs a, SimplifyTable T,
                                                       const uint32_t *__restrict__ code, const uint32_t *__restrict__ blk_base,
                                                       const uint2 *__restrict__ info, float4 *__restrict__ out)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t c = t < n ? code[t] : SIMP_NONE;
    const uint32_t rank = simp_rank_in_chunk(c != SIMP_NONE, blk_base, info);
    if (c == SIMP_NONE) return;
    float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
    if (c != SIMP_LOOSE && T.n[c] >= 2u) simp_finish(a, T, c, nr, pc, ct, nr);
    out[(size_t)rank * 3] = pc;
    out[(size_t)rank * 3 + 1] = ct;
    out[(size_t)rank * 3 + 2] = nr;
}

}  // namespace sm
