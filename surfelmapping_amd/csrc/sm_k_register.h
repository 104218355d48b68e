// sm_k_register.h -- registration of one map set against another (DESIGN.md "4q. Registration"; the specification is
// sm_c_api.h's "sm_register_maps").  Included by sm_register.hip only.  The target's tables are lookup tables, filled and finished
// by sm_voxel.hip; their lookup is sm_d_register.h's; the 29-value system, its fixed-order sums and the solve are the trackers'
// (sm_d_track.h).
//   k_register_gather  per chunk of the source: record id goes to sample id / stride if stride divides it (no scan)
//   k_register_reduce  one lane per sample: the moved point, its eight candidate keys, their first probes issued together, the
//                      nearest representative, the gates, the 28 float32 products into fp64 sums; track_block_sum per workgroup
//   k_register_solve   one workgroup: track_sum_parts, then one lane: statuses, LDLT, the step about the pivot, convergence, the
//                      next level.  Launches after the end return at once (RegState::done), so the host waits once.
// No lane waits for another: a probe walk ends at the key, at an empty slot or after mask + 1 slots.
#pragma once

#include "sm_d_register.h"
#include "sm_d_track.h"

namespace sm {

constexpr int REG_MAX_LEVELS = 4;
enum { REG_OK = 0, REG_LOST = 1, REG_DEGENERATE = 2, REG_NO_TARGET = 3, REG_NO_SOURCE = 4 };

struct RegLevel {
    const RegCell *lut;
    uint32_t mask;
    long long V;
    double reach;                      // metres
};

struct RegParams {
    RegLevel lv[REG_MAX_LEVELS];
    int levels;
    float origin[3];
    double pivot[3];
    double cos_angle;
    uint32_t n_samples;
    int nb;                            // workgroups of k_register_reduce
    uint32_t min_inliers;
    int max_iters;                     // per level
    double degenerate_bound;
};

struct RegState {
    double T[16];                      // the estimate, source world -> target world, column-major
    double guess[16];
    double sys[32];                    // the last system summed (TRACK_NSYS used)
    double rmse, pivot_ratio, step_rot, step_trans;
    int32_t status, done, level, iter; // level: the one the next system is summed on; iter: iterations made on it
    int32_t iters[REG_MAX_LEVELS];
    uint32_t inliers, pad;
};

// ---- the source's samples: pos.w = 1 regular, 0 not ----

__global__ __launch_bounds__(256) void k_register_gather(const float4 *__restrict__ rec, uint32_t n, uint32_t gid0, uint32_t stride,
                                                         float4 *__restrict__ pos, float4 *__restrict__ nrm, uint32_t *__restrict__ regular)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    bool ok = false;
    if (t < n) {
        const uint32_t gid = gid0 + t, i = gid / stride;
        if (gid - i * stride == 0u) {
            const float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
            ok = simp_fields_ok(pc, ct, nr);
            pos[i] = make_float4(pc.x, pc.y, pc.z, ok ? 1.0f : 0.0f);
            nrm[i] = make_float4(nr.x, nr.y, nr.z, 0.0f);
        }
    }
    const unsigned long long m = __ballot(ok);
    if (m && (int)(threadIdx.x & 63u) == __ffsll(m) - 1) atomicAdd(regular, (uint32_t)__popcll(m));
}

// ---- one Gauss-Newton iteration ----

// the pair of sample i at the pose T on level L: false if it does not count
__device__ __forceinline__ bool reg_pair(uint32_t i, const double *T, const RegParams &rp, const RegLevel &L, const float4 *__restrict__ pos,
                                         const float4 *__restrict__ nrm, float *J, float &r)
{
    const float4 pf = pos[i];
    if (pf.w == 0.0f) return false;
    const float4 nf = nrm[i];
    double q[3], nq[3];
    reg_move(T, pf, nf, q, nq);
    long long cell[3][2];              // the cell and its neighbour towards q
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (!reg_cells(q[k], rp.origin[k], L.V, cell[k][0], cell[k][1])) return false;
    int ax = 0;
    if (fabs(nq[1]) > fabs(nq[ax])) ax = 1;
    if (fabs(nq[2]) > fabs(nq[ax])) ax = 2;
    const unsigned long long face = 2ull * (unsigned long long)ax + (nq[ax] < 0.0 ? 1ull : 0ull);

    // the nearest representative among the eight candidates; of two equally near the one with the smaller key
    double best = 0.0, e[3] = {0.0, 0.0, 0.0};
    float nc[3] = {0.0f, 0.0f, 0.0f};
    unsigned long long best_key = SIMP_EMPTY;
    reg_lookup8(cell, face << 8, L.mask, [&](uint32_t s) { return L.lut[s].key; }, [&](int, unsigned long long key, uint32_t s) {
        const RegCell &rc = L.lut[s];
        const double e0 = q[0] - (double)rc.p[0], e1 = q[1] - (double)rc.p[1], e2 = q[2] - (double)rc.p[2];
        const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
        if (best_key == SIMP_EMPTY || d2 < best || (d2 == best && key < best_key)) {
            best = d2; best_key = key;
            e[0] = e0; e[1] = e1; e[2] = e2;
            nc[0] = rc.n[0]; nc[1] = rc.n[1]; nc[2] = rc.n[2];
        }
    });
    if (best_key == SIMP_EMPTY) return false;
    if (!(sqrt(best) <= L.reach)) return false;
    const double m0 = nc[0], m1 = nc[1], m2 = nc[2];
    if (!((nq[0] * m0 + nq[1] * m1) + nq[2] * m2 >= rp.cos_angle)) return false;
    r = (float)((m0 * e[0] + m1 * e[1]) + m2 * e[2]);
    const double u0 = q[0] - rp.pivot[0], u1 = q[1] - rp.pivot[1], u2 = q[2] - rp.pivot[2];
    J[0] = nc[0]; J[1] = nc[1]; J[2] = nc[2];
    J[3] = (float)(u1 * m2 - u2 * m1);
    J[4] = (float)(u2 * m0 - u0 * m2);
    J[5] = (float)(u0 * m1 - u1 * m0);
    return true;
}

// every workgroup: its lanes take samples blockIdx * 256 + tid + k * nb * 256 (fixed), so partials do not depend on timing.
// level < 0: the state's.
__global__ __launch_bounds__(TRACK_BLOCK) void k_register_reduce(RegParams rp, const float4 *__restrict__ pos, const float4 *__restrict__ nrm,
                                                                 const RegState *__restrict__ st, double *__restrict__ part)
{
    if (st->done) return;
    __shared__ double s_w[TRACK_BLOCK / 64][TRACK_NSYS];
    double T[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) T[e] = st->T[e];
    const RegLevel L = rp.lv[st->level];
    double acc[TRACK_NSYS];
#pragma unroll
    for (int e = 0; e < TRACK_NSYS; ++e) acc[e] = 0.0;
    const uint32_t step = (uint32_t)rp.nb * TRACK_BLOCK;
    for (uint32_t i = blockIdx.x * TRACK_BLOCK + threadIdx.x; i < rp.n_samples; i += step) {
        float J[6], r;
        if (!reg_pair(i, T, rp, L, pos, nrm, J, r)) continue;
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[e++] += (double)(J[a] * J[b]);
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] += (double)(J[a] * r);
        acc[27] += (double)(r * r);
        acc[28] += 1.0;
    }
    track_block_sum(acc, s_w, rp.nb, part);
}

__device__ inline void reg_fail(RegState *__restrict__ st, int status)
{
    for (int e = 0; e < 16; ++e) st->T[e] = st->guess[e];
    st->status = status;
    st->done = 1;
}

// T <- Tr(pivot) * exp(xi) * Tr(-pivot) * T
__device__ inline void reg_apply(const double *xi, const double *pivot, RegState *__restrict__ st)
{
    double R[3][3], tt[3], tp[3];
    track_exp(xi, R, tt);
    for (int r = 0; r < 3; ++r) tp[r] = (tt[r] + pivot[r]) - ((R[r][0] * pivot[0] + R[r][1] * pivot[1]) + R[r][2] * pivot[2]);
    const double *T = st->T;                                  // column-major: T[c * 4 + r]
    double Tn[16];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Tn[c * 4 + r] = (R[r][0] * T[c * 4 + 0] + R[r][1] * T[c * 4 + 1]) + R[r][2] * T[c * 4 + 2];
        Tn[12 + r] = ((R[r][0] * T[12] + R[r][1] * T[13]) + R[r][2] * T[14]) + tp[r];
    }
    Tn[3] = 0.0; Tn[7] = 0.0; Tn[11] = 0.0; Tn[15] = 1.0;
    for (int k = 0; k < 16; ++k) st->T[k] = Tn[k];
    st->step_rot = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
    st->step_trans = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
}

// one workgroup.  sum_only: only the fixed-order sum into st->sys (sm_register_debug)
__global__ __launch_bounds__(256) void k_register_solve(RegParams rp, const double *__restrict__ part, RegState *__restrict__ st, int sum_only)
{
    if (st->done) return;
    __shared__ double s_p[TRACK_NSYS][8];
    double sys[TRACK_NSYS];
    track_sum_parts(part, rp.nb, s_p, sys);
    if (threadIdx.x != 0) return;
    for (int e = 0; e < TRACK_NSYS; ++e) st->sys[e] = sys[e];
    if (sum_only) return;
    const double cnt = sys[28];
    const int level = st->level;
    st->iter += 1;
    st->iters[level] += 1;
    st->inliers = (uint32_t)cnt;
    st->rmse = cnt > 0.0 ? sqrt(sys[27] / cnt) : 0.0;
    if (cnt < (double)rp.min_inliers || cnt < 6.0) { reg_fail(st, REG_LOST); return; }
    double A[6][6], b[6], xi[6];
    track_unpack(sys, A, b);
    if (!track_solve_xi(A, b, xi)) { reg_fail(st, REG_DEGENERATE); return; }
    reg_apply(xi, rp.pivot, st);
    const bool converged = st->step_rot < 1e-6 && st->step_trans < 1e-6;
    if (!converged && st->iter < rp.max_iters) return;
    if (level > 0) { st->level = level - 1; st->iter = 0; return; }
    // the end: the last system is judged about the pivot, where its rows were taken
    const double zero[3] = {0.0, 0.0, 0.0};
    st->pivot_ratio = track_pivot_ratio(A, zero);
    if (!(st->pivot_ratio >= rp.degenerate_bound)) { reg_fail(st, REG_DEGENERATE); return; }
    st->done = 1;
}

}  // namespace sm
