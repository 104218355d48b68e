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
//   k_pair_sort_hist    one pass of the LSD radix sort of (key, idx) pairs, 8 bits: per block of 8192 keys the digits' histogram,
//                       built in LDS
//   k_pair_sort_scan    ... the exclusive scan over (digit, block) in place, one workgroup, block_scan_1024 over steps of 4096 entries
//   k_pair_sort_scatter ... (key, idx) to their places, stable: a block takes its keys in 32 rounds of 256; per round a wave matches
//                       its lanes on the digit (ballots over the 8 bits) and the waves' counts per digit go through LDS
// No lane waits for another: a probe walk ends at the key, at an empty slot or after mask + 1 slots.  Integer atomics only.
#pragma once

#include "sm_d_register.h"

namespace sm {

constexpr uint32_t PAIR_SORT_BLOCK = 8192u;              // keys per workgroup of a sort pass: 32 rounds of 256
constexpr uint32_t PAIR_SCAN_TILE = 4096u;               // entries per step of k_pair_sort_scan: four per lane

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

// ---- the pair sort: block b of a pass has the keys [b * 8192, b * 8192 + 8192) of n; hist[digit * nblk + b]
__global__ __launch_bounds__(256) void k_pair_sort_hist(const unsigned long long *__restrict__ key, uint32_t n, int shift, uint32_t nblk,
                                                        uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * PAIR_SORT_BLOCK;
#pragma unroll
    for (uint32_t r = 0; r < PAIR_SORT_BLOCK / 256u; ++r) {
        const uint32_t i = first + r * 256u + threadIdx.x;
        if (i < n) atomicAdd(&s_h[(uint32_t)(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[threadIdx.x * nblk + blockIdx.x] = s_h[threadIdx.x];
}

// entries: a multiple of 4 (256 digits per block)
__global__ __launch_bounds__(1024) void k_pair_sort_scan(uint32_t *__restrict__ hist, uint32_t entries)
{
    __shared__ uint32_t s_scan[17];
    uint32_t run = 0;
    for (uint32_t b = 0; b < entries; b += PAIR_SCAN_TILE) {
        const uint32_t i = b + threadIdx.x * 4u;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i < entries) v = *(const uint4 *)(hist + i);
        uint32_t tot;
        const uint32_t at = run + block_scan_1024((v.x + v.y) + (v.z + v.w), &tot, s_scan);
        if (i < entries) *(uint4 *)(hist + i) = make_uint4(at, at + v.x, at + v.x + v.y, at + v.x + v.y + v.z);
        run += tot;
    }
}

__global__ __launch_bounds__(256) void k_pair_sort_scatter(const unsigned long long *__restrict__ key_in, const uint32_t *__restrict__ idx_in, uint32_t n,
                                                           int shift, uint32_t nblk, const uint32_t *__restrict__ hist,
                                                           unsigned long long *__restrict__ key_out, uint32_t *__restrict__ idx_out)
{
    __shared__ uint32_t s_run[256];                      // per digit: where the block's next key with it goes
    __shared__ uint32_t s_wave[4][256];                  // per wave and digit: the keys of this round
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s_run[threadIdx.x] = hist[threadIdx.x * nblk + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) s_wave[w][threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t first = blockIdx.x * PAIR_SORT_BLOCK;
    for (uint32_t r = 0; r < PAIR_SORT_BLOCK / 256u; ++r) {
        if (first + r * 256u >= n) break;                // (the same for every lane of the block)
        const uint32_t i = first + r * 256u + threadIdx.x;
        const bool valid = i < n;
        const unsigned long long k = valid ? key_in[i] : 0ull;
        const uint32_t d = (uint32_t)(k >> shift) & 255u;
        unsigned long long m = __ballot(valid);          // the wave's lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool on = (d >> b) & 1u;
            const unsigned long long bb = __ballot(on);
            m &= on ? bb : ~bb;
        }
        const uint32_t below = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (valid && below == 0u) s_wave[wave][d] = (uint32_t)__popcll(m);
        __syncthreads();
        if (valid) {
            uint32_t at = s_run[d] + below;
            for (int w = 0; w < wave; ++w) at += s_wave[w][d];
            if (at < n) { key_out[at] = k; idx_out[at] = idx_in[i]; }
        }
        __syncthreads();
        s_run[threadIdx.x] += (s_wave[0][threadIdx.x] + s_wave[1][threadIdx.x]) + (s_wave[2][threadIdx.x] + s_wave[3][threadIdx.x]);
#pragma unroll
        for (int w = 0; w < 4; ++w) s_wave[w][threadIdx.x] = 0u;
        __syncthreads();
    }
}

}  // namespace sm
