// sm_k_compare.h -- change detection between two map sets (DESIGN.md "4r. Change detection"; the specification is sm_c_api.h's
// "sm_compare_maps").  Included by sm_compare.hip only.  The reference's fine table with its cover table is a lookup table, filled
// and finished by sm_voxel.hip, which also ranks the kept records; the lookup record, the moved point, its candidate cells and
// their lookup are sm_d_register.h's.
//   k_compare_classify  one lane per query record of a chunk: the label byte, the keep flag, the kept records per block of 256
//                       and the label counts (one atomic per wave and label).  The eight first probes of the primary face are
//                       issued together; a secondary face is probed only by lanes that have one and are not supported yet, the
//                       cover table only by lanes that no face supports
//   k_compare_emit      every kept record, verbatim, at its rank (simp_rank_in_chunk): three 16-byte stores
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

// ---- the query's labels ----

// does a representative of the eight candidate cells with the key bits `low` (face << 8 | class) pass the three gates?
__device__ __forceinline__ bool cmp_face_supports(const CmpParams &cp, const long long cell[3][2], const double q[3], const double nq[3],
                                                  unsigned long long low)
{
    bool sup = false;
    reg_lookup8(cell, low, cp.mask, [&](uint32_t s) { return cp.lut[s].key; }, [&](int, unsigned long long, uint32_t s) {
        const RegCell &rc = cp.lut[s];
        const double e0 = q[0] - (double)rc.p[0], e1 = q[1] - (double)rc.p[1], e2 = q[2] - (double)rc.p[2];
        const double m0 = rc.n[0], m1 = rc.n[1], m2 = rc.n[2];
        const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
        const double r = (m0 * e0 + m1 * e1) + m2 * e2;
        const double dot = (nq[0] * m0 + nq[1] * m1) + nq[2] * m2;
        sup = sup || (sqrt(d2) <= cp.reach && dot >= cp.cos_angle && fabs(r) <= cp.plane);
    });
    return sup;
}

// does the cover table hold one of the eight cover cells?
__device__ __forceinline__ bool cmp_covered(const CmpParams &cp, const long long cell[3][2])
{
    bool near = false;
    reg_lookup8(cell, 0ull, cp.cmask, [&](uint32_t s) { return cp.cover[s]; }, [&](int, unsigned long long, uint32_t) { near = true; });
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

// out[(rank - info->x) * 3 ..]: a chunk's output begins at out
__global__ __launch_bounds__(256) void k_compare_emit(const float4 *__restrict__ rec, uint32_t n, const uint8_t *__restrict__ keep,
                                                      const uint32_t *__restrict__ blk_base, const uint2 *__restrict__ info, float4 *__restrict__ out)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const bool kp = t < n && keep[t] != 0;
    const uint32_t rank = simp_rank_in_chunk(kp, blk_base, info);
    if (!kp) return;
    out[(size_t)rank * 3] = rec[(size_t)t * 3];
    out[(size_t)rank * 3 + 1] = rec[(size_t)t * 3 + 1];
    out[(size_t)rank * 3 + 2] = rec[(size_t)t * 3 + 2];
}

}  // namespace sm
