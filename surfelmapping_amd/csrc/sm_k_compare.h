// sm_k_compare.h -- change detection between two map sets (DESIGN.md "4r. Change detection"; the specification is sm_c_api.h's
// "sm_compare_maps").  Included by sm_compare.hip only.  The tables, the claim-and-add and the ranks are the simplification's
// (sm_d_simplify.h); the lookup record, the moved point and its candidate cells are registration's (sm_d_register.h).
//   k_compare_insert    per chunk of the reference: every regular record's fine key (the class kept or taken as 0) with its SW,
//                       SP, SN into the fine table (simp_insert<false>), and the key of its cover cell claimed in the cover
//                       table, which has keys only (cmp_claim: a read, an atomicCAS where the slot is empty, one tally add per wave)
//   k_compare_finish    one lane per fine slot: the sums become the 32-byte lookup record (reg_cell_of)
//   k_compare_classify  one lane per query record of a chunk: the label byte, the keep flag, the kept records per block of 256
//                       and the label counts (one atomic per wave and label).  The eight first probes of the primary face are
//                       issued together; a secondary face is probed only by lanes that have one and are not supported yet, the
//                       cover table only by lanes that no face supports
//   k_compare_scan      the kept records' ranks: simp_scan_ranks on top of the call's running rank
//   k_compare_emit      every kept record, verbatim, at its rank: three 16-byte stores
// No lane waits for another: a probe walk ends at the key, at an empty slot or after mask + 1 slots.  Integer atomics only.
#pragma once

#include "sm_d_register.h"

namespace sm {

enum { CMP_SUPPORTED = 0, CMP_CHANGED = 1, CMP_OUTSIDE = 2, CMP_LOOSE = 3, CMP_LABELS = 4 };
// the tally's words: the fine table's (SIMP_RUN of it: the running rank), the cover table's, the label counts
enum { CMP_FINE = 0, CMP_COVER = SIMP_TALLY_WORDS, CMP_COUNTS = 2 * SIMP_TALLY_WORDS, CMP_TALLY_WORDS = 2 * SIMP_TALLY_WORDS + CMP_LABELS };

struct CmpParams {
    const RegCell *lut;                // the fine table's lookup records
    const unsigned long long *cover;   // the cover table's keys
    uint32_t mask, cmask;
    long long V0, V1;
    float origin[3];
    int match_class;
    uint32_t write_mask;               // 0: nothing is kept
    double T[16];                      // query world -> reference world, column-major
    double reach, cos_angle, plane;    // metres, a cosine, metres
};

// ---- the reference's tables ----

// a regular record's cover key into the table of keys (all 64 lanes of a wave call it; reg: the lane has one)
__device__ __forceinline__ void cmp_claim(const SimplifyArgs &a, const SimplifyTable &T, unsigned long long key, bool reg)
{
    const int lane = threadIdx.x & 63;
    bool head = reg;
    if (a.combine) {                                     // a lane whose neighbour below has its key leaves the claim to it
        const unsigned long long prev = __shfl_up(key, 1);
        head = reg && !(lane > 0 && prev == key);
    }
    bool claimed = false, lost = false;
    if (head) {
        uint32_t sl = 0;
        lost = !simp_probe(T, key, true, sl, claimed);
    }
    const unsigned long long cb = __ballot(claimed);
    if (cb && lane == __ffsll(cb) - 1) {
        const uint32_t m = (uint32_t)__popcll(cb);
        if (atomicAdd(&T.tally[SIMP_CELLS], m) + m > a.max_cells) atomicOr(&T.tally[SIMP_ERR], 1u);
    }
    if (lost) atomicOr(&T.tally[SIMP_ERR], 2u);
}

// aF, TF: the fine grid (split faces) and its table; aC, TC: the cover grid (no faces) and its table, of which key, mask and tally exist
__global__ __launch_bounds__(256) void k_compare_insert(const float4 *__restrict__ rec, uint32_t n, SimplifyArgs aF, SimplifyTable TF, int keep_class,
                                                        SimplifyArgs aC, SimplifyTable TC)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    unsigned long long key = SIMP_EMPTY, ckey = SIMP_EMPTY;
    bool reg = false, creg = false;
    SimpContrib c{};
    if (t < n) {
        const float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
        uint32_t off[3];
        reg = simp_classify(aF, pc, ct, nr, key, off);
        if (reg) { simp_contribution(pc, ct, nr, off, 0u, c); if (!keep_class) key &= ~0xFFull; }
        else key = SIMP_EMPTY;
        creg = simp_classify(aC, pc, ct, nr, ckey, off);
        ckey = creg ? ckey & ~0xFFull : SIMP_EMPTY;
    }
    simp_insert<false>(aF, TF, key, reg, c);
    cmp_claim(aC, TC, ckey, creg);
}

__global__ __launch_bounds__(256) void k_compare_finish(SimplifyArgs a, SimplifyTable T, RegCell *__restrict__ lut)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    if (sl > T.mask) return;
    lut[sl] = reg_cell_of(a, T, sl);
}

// ---- the query's labels ----

// does a representative of the eight candidate cells with the key bits `low` (face << 8 | class) pass the three gates?
__device__ __forceinline__ bool cmp_face_supports(const CmpParams &cp, const long long cell[3][2], const double q[3], const double nq[3],
                                                  unsigned long long low)
{
    // every first probe is on its way before one is looked at
    unsigned long long ck[8], cur[8];
    uint32_t sl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bool valid;
        ck[j] = reg_candidate(cell, j, low, valid);
        sl[j] = (uint32_t)simp_hash(ck[j]) & cp.mask;
        cur[j] = valid ? cp.lut[sl[j]].key : SIMP_EMPTY;
    }
    bool sup = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        unsigned long long c = cur[j];
        uint32_t s = sl[j];
        bool hit = false;
        for (uint32_t w = 0; w <= cp.mask; ++w) {        // (at most the table's slots)
            if (c == SIMP_EMPTY) break;
            if (c == ck[j]) { hit = true; break; }
            s = (s + 1u) & cp.mask;
            c = cp.lut[s].key;
        }
        if (!hit) continue;
        const RegCell &rc = cp.lut[s];
        const double e0 = q[0] - (double)rc.p[0], e1 = q[1] - (double)rc.p[1], e2 = q[2] - (double)rc.p[2];
        const double m0 = rc.n[0], m1 = rc.n[1], m2 = rc.n[2];
        const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
        const double r = (m0 * e0 + m1 * e1) + m2 * e2;
        const double dot = (nq[0] * m0 + nq[1] * m1) + nq[2] * m2;
        sup = sup || (sqrt(d2) <= cp.reach && dot >= cp.cos_angle && fabs(r) <= cp.plane);
    }
    return sup;
}

// does the cover table hold one of the eight cover cells?
__device__ __forceinline__ bool cmp_covered(const CmpParams &cp, const long long cell[3][2])
{
    unsigned long long ck[8], cur[8];
    uint32_t sl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bool valid;
        ck[j] = reg_candidate(cell, j, 0ull, valid);
        sl[j] = (uint32_t)simp_hash(ck[j]) & cp.cmask;
        cur[j] = valid ? cp.cover[sl[j]] : SIMP_EMPTY;
    }
    bool near = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        unsigned long long c = cur[j];
        uint32_t s = sl[j];
        for (uint32_t w = 0; w <= cp.cmask; ++w) {
            if (c == SIMP_EMPTY) break;
            if (c == ck[j]) { near = true; break; }
            s = (s + 1u) & cp.cmask;
            c = cp.cover[s];
        }
    }
    return near;
}

__device__ __forceinline__ uint32_t cmp_label(const CmpParams &cp, const float4 &pc, const float4 &ct, const float4 &nr)
{
    if (!simp_fields_ok(pc, ct, nr)) return CMP_LOOSE;
    double q[3], nq[3];
    reg_move(cp.T, pc, nr, q, nq);
    long long cell[3][2], cov[3][2];   // per axis the cell and its neighbour towards q, fine and cover
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!reg_cells(q[k], cp.origin[k], cp.V0, cell[k][0], cell[k][1])) return CMP_OUTSIDE;
        if (!reg_cells(q[k], cp.origin[k], cp.V1, cov[k][0], cov[k][1])) return CMP_OUTSIDE;
    }
    // the primary face is the simplification's of nq; an axis with 4 |nq[a]| >= max |nq| gives a face as well
    double m = fabs(nq[0]);
    int ax = 0;
    if (fabs(nq[1]) > m) { m = fabs(nq[1]); ax = 1; }
    if (fabs(nq[2]) > m) { m = fabs(nq[2]); ax = 2; }
    const unsigned long long cls = cp.match_class ? (unsigned long long)(__float_as_uint(ct.x) >> 24) : 0ull;
    bool sup = false;
#pragma unroll 1
    for (int pass = 0; pass < 3 && !sup; ++pass) {
        const int a = pass == 0 ? ax : pass == 1 ? (ax == 0 ? 1 : 0) : (ax == 2 ? 1 : 2);
        const double na = a == 0 ? nq[0] : a == 1 ? nq[1] : nq[2];
        if (pass && !(4.0 * fabs(na) >= m)) continue;
        const unsigned long long face = 2ull * (unsigned long long)a + (na < 0.0 ? 1ull : 0ull);
        sup = cmp_face_supports(cp, cell, q, nq, (face << 8) | cls);
    }
    if (sup) return CMP_SUPPORTED;
    return cmp_covered(cp, cov) ? CMP_CHANGED : CMP_OUTSIDE;
}

__global__ __launch_bounds__(256) void k_compare_classify(const float4 *__restrict__ rec, uint32_t n, CmpParams cp, uint8_t *__restrict__ label,
                                                          uint8_t *__restrict__ keep, uint32_t *__restrict__ blk_cnt, uint32_t *__restrict__ tally)
{
    __shared__ uint32_t s_cnt[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t lab = CMP_LABELS;                           // (no record)
    bool kp = false;
    if (t < n) {
        const float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
        lab = cmp_label(cp, pc, ct, nr);
        kp = ((cp.write_mask >> lab) & 1u) != 0u;
        label[t] = (uint8_t)lab;
        keep[t] = kp ? 1 : 0;
    }
#pragma unroll
    for (uint32_t l = 0; l < CMP_LABELS; ++l) {
        const unsigned long long b = __ballot(lab == l);
        if (b && lane == 0) atomicAdd(&tally[CMP_COUNTS + l], (uint32_t)__popcll(b));
    }
    const unsigned long long kept = __ballot(kp);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(kept);
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// blk_base[b] = the rank of block b's first kept record in the whole output; info: (this chunk's first rank, its count)
__global__ __launch_bounds__(1024) void k_compare_scan(const uint32_t *__restrict__ blk_cnt, uint32_t nblk, uint32_t *__restrict__ blk_base,
                                                       uint32_t *__restrict__ tally, uint2 *__restrict__ info)
{
    simp_scan_ranks(blk_cnt, nblk, blk_base, tally, info);
}

// out[(rank - info->x) * 3 ..]: a chunk's output begins at out
__global__ __launch_bounds__(256) void k_compare_emit(const float4 *__restrict__ rec, uint32_t n, const uint8_t *__restrict__ keep,
                                                      const uint32_t *__restrict__ blk_base, const uint2 *__restrict__ info, float4 *__restrict__ out)
{
    __shared__ uint32_t s_cnt[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool kp = t < n && keep[t] != 0;
    const unsigned long long kept = __ballot(kp);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(kept);
    __syncthreads();
    if (!kp) return;
    uint32_t rank = blk_base[blockIdx.x] - info->x + (uint32_t)__popcll(kept & ((1ull << lane) - 1ull));
    for (int x = 0; x < wave; ++x) rank += s_cnt[x];
    out[(size_t)rank * 3] = rec[(size_t)t * 3];
    out[(size_t)rank * 3 + 1] = rec[(size_t)t * 3 + 1];
    out[(size_t)rank * 3 + 2] = rec[(size_t)t * 3 + 2];
}

}  // namespace sm
