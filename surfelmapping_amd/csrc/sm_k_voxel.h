// sm_k_voxel.h -- the kernels of sm_voxel.hip, which alone includes this: what registration (DESIGN.md "4q") and change detection
// ("4r") do alike to a lookup table, and what simplification ("4p") and change detection do alike to rank a chunk's output.  The
// device functions are sm_d_simplify.h's and sm_d_register.h's.
//   k_lut_insert  per chunk of records: every regular record's key (the class kept or taken as 0) with its SW, SP, SN into the
//                 table's sums (simp_insert<false>: the in-wave combination, the claim, then atomics); COVER: from the same read
//                 of the record the key of its cover cell claimed in the cover table, which has keys only (simp_head, simp_claim:
//                 a read, an atomicCAS where the slot is empty, one tally add per wave)
//   k_lut_finish  one lane per slot: the sums become the lookup record -- key, position, normal in 32 aligned bytes, so a probe
//                 that hits has the representative in the line it has just read
//   k_rank_scan   exclusive prefix of the per-block counts on top of the running rank (one workgroup, block_scan_1024)
// No lane waits for another: a probe walk ends at the key, at an empty slot or after mask + 1 slots.  Integer atomics only.
#pragma once

#include "sm_d_register.h"

namespace sm {

// a, T: the grid (split faces) and its table; ac, TC: the cover grid (no faces) and its table, of which key, mask and tally exist
template <bool COVER, bool KEEP_CLASS>
__global__ __launch_bounds__(256) void k_lut_insert(const float4 *__restrict__ rec, uint32_t n, SimplifyArgs a, SimplifyTable T, SimplifyArgs ac,
                                                    SimplifyTable TC)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    unsigned long long key = SIMP_EMPTY, ckey = SIMP_EMPTY;
    bool reg = false, creg = false;
    SimpContrib c{};
    if (t < n) {
        const float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
        uint32_t off[3];
        reg = simp_classify(a, pc, ct, nr, key, off);
        if (reg) { simp_contribution(pc, ct, nr, off, 0u, c); if (!KEEP_CLASS) key &= ~0xFFull; }
        else key = SIMP_EMPTY;
        if constexpr (COVER) {
            creg = simp_classify(ac, pc, ct, nr, ckey, off);
            ckey = creg ? ckey & ~0xFFull : SIMP_EMPTY;
        }
    }
    simp_insert<false>(a, T, key, reg, c);
    if constexpr (COVER) simp_claim(ac, TC, ckey, simp_head(ac, ckey, creg), [](uint32_t) {});
}

__global__ __launch_bounds__(256) void k_lut_finish(SimplifyArgs a, SimplifyTable T, RegCell *__restrict__ lut)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    if (sl > T.mask) return;
    lut[sl] = reg_cell_of(a, T, sl);
}

// blk_base[b] = the rank of block b's first kept record in the whole output; info (may be null): (this chunk's first rank, its count)
__global__ __launch_bounds__(1024) void k_rank_scan(const uint32_t *__restrict__ blk_cnt, uint32_t nblk, uint32_t *__restrict__ blk_base,
                                                    uint32_t *__restrict__ tally, uint2 *__restrict__ info)
{
    simp_scan_ranks(blk_cnt, nblk, blk_base, tally, info);
}

}  // namespace sm
