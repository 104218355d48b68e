// sm_k_track.h -- camera tracking: projective frame-to-model point-to-plane ICP (DESIGN.md "4d. Tracking").
// Included by sm_track.hip only; the sums and the solve of the normal equations are sm_d_track.h's, which sm_k_register.h shares.
// The reference has no tracker (its header promises one:
// src/SurfelMapping.h:31-34); the vertex / normal rule is the frame's own (geometry.glsl:5-24 as local_surfel restates it).
//
// One tracked frame:
//   k_track_splat    one pass over the occupied slots: every live surfel (alive bit set) whose centre lies in front of the
//                    prediction camera T_prev with near < z < far lands on pixel (floor(fx*x/z + cx + 0.5), floor(fy*y/z + cy + 0.5))
//                    by a 64-bit atomicMin of (float bits of z) << 32 | slot: the nearest surfel, ties to the lower slot.
//   k_track_resolve  key -> slot (-1 = empty), row-major W*H int32.
//   (with a time window -- sm_track_*_old, sm_track_*_window -- the splat's instantiation that also gates on the surfel's time,
//   and k_track_anchor after the resolve)
//   k_track_vertex   the current frame's metric depth (p0a's rule), vertex and normal of every pixel of the strided grid.
//   then max_iters times:
//   k_track_reduce   associate + residual + the 29 values of the normal equations per inlier, fp32 terms accumulated in fp64,
//                    wave shuffle + LDS reduction to one fp64 partial per workgroup (fixed order: bit-reproducible).
//   k_track_solve    one workgroup: fixed-order sum of the partials, LDLT in double, T <- exp(xi) T, convergence / failure
//                    (LOST at any iteration; DEGENERATE when the system of the converged or last iteration is).
// A device-side `done` word makes every launch after convergence or failure a no-op, so the host waits once per frame.

#pragma once

#include "sm_device.h"
#include "sm_d_track.h"

namespace sm {


enum { TRACK_OK = 0, TRACK_LOST = 1, TRACK_DEGENERATE = 2, TRACK_NO_MODEL = 3 };

struct TrackParams {
    float tinv_prev[16];      // world -> prediction camera, column-major: [R^T | -R^T t] of T_prev in double, rounded to float
    float fx, fy, cx, cy, inv_fx, inv_fy;
    float near_clip, far_clip, stereo_border;
    int W, H;
    int stride, ni, nj, n;    // the strided pixel grid: columns 0, s, 2s, ... (ni of them) x rows 0, s, ... (nj); n = ni * nj
    float dist, cos_angle;    // association gates
    uint32_t min_inliers;
    double degenerate_bound;  // smallest / largest LDLT pivot of the scaled, camera-centred system
    double c[3];              // prediction camera centre (the translation of T_prev)
    int nb;                   // workgroups of k_track_reduce
    int max_iters;
};

struct TrackState {
    double T[16];             // the estimate, camera -> world, column-major
    double guess[16];
    double sys[32];           // the last system summed by k_track_solve (TRACK_NSYS used)
    double rmse, pivot_ratio, step_rot, step_trans;
    int32_t status, iterations, done, pad;
    uint32_t in_view, inliers;
};

// ---- the prediction ----

// USE_MIN / USE_MAX: the surfel's last-update time is held to min_time < m[7] <= max_time (sm_track_*_old, sm_track_*_window).  The
// gates are compile-time so that the open-ended forms are the plain kernel by construction: an open end makes no comparison (a NaN
// time passes there; both comparisons are false on a NaN), and with both ends open the time plane is not loaded at all.
template <bool USE_MIN, bool USE_MAX>
__global__ __launch_bounds__(256) void k_track_splat(Model M, const DevState *__restrict__ st, const uint64_t *__restrict__ alive,
                                                     TrackParams tp, float min_time, float max_time, uint64_t *__restrict__ key,
                                                     TrackState *__restrict__ ts)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    bool in_view = false;
    if (k < st->count && ((alive[k >> 6] >> (k & 63u)) & 1ull)) {
        bool inside = true;
        if constexpr (USE_MIN || USE_MAX) {
            const float t = M.s[st->cur].time[k];
            if constexpr (USE_MIN) inside = t > min_time;
            if constexpr (USE_MAX) inside = inside && t <= max_time;
        }
        if (inside) {
            const float4 pc = M.s[st->cur].pos_conf[k];
            const float3 c = xform3(tp.tinv_prev, pc.x, pc.y, pc.z);
            if (c.z > tp.near_clip && c.z < tp.far_clip) {
                const float fu = floorf(((tp.fx * c.x) / c.z + tp.cx) + 0.5f);
                const float fv = floorf(((tp.fy * c.y) / c.z + tp.cy) + 0.5f);
                if (fu >= 0.0f && fu < (float)tp.W && fv >= 0.0f && fv < (float)tp.H) {
                    in_view = true;
                    const size_t p = (size_t)(int)fv * tp.W + (int)fu;
                    atomicMin((unsigned long long *)&key[p], (unsigned long long)(((uint64_t)__float_as_uint(c.z) << 32) | k));
                }
            }
        }
    }
    const uint64_t m = __ballot(in_view);                     // one atomic per wave
    if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll((unsigned long long)m) - 1))
        atomicAdd(&ts->in_view, (uint32_t)__popcll(m));
}

__global__ void k_track_resolve(const uint64_t *__restrict__ key, int npix, int32_t *__restrict__ slot)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const uint64_t kk = key[p];
    slot[p] = kk == KEY_EMPTY ? -1 : (int32_t)(uint32_t)(kk & 0xFFFFFFFFull);
}

// *anchor = max over the resolved slots of f2ord(last-update time); 0 (no float's code but a NaN's) stays where the prediction is
// empty.  One wave reduction and at most one atomic per wave.
__global__ __launch_bounds__(256) void k_track_anchor(Model M, const DevState *__restrict__ st, const int32_t *__restrict__ slot, int npix,
                                                      uint32_t *__restrict__ anchor)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    uint32_t v = 0u;
    if (p < npix) {
        const int32_t k = slot[p];
        if (k >= 0) v = f2ord(M.s[st->cur].time[k]);
    }
    v = wave_max_u32(v);                                      // (all 64 lanes active: nobody has returned)
    if ((threadIdx.x & 63u) == 0u && v) atomicMax(anchor, v);
}

// ---- the current frame: vertex (xyz, 1 = valid) and normal per grid point ----

// metriciseDepth (p0a: sm_k_prep.h, prep_image_block) of pixel (i, j) of the row-major millimetre image
__device__ __forceinline__ float track_depth(const uint16_t *__restrict__ mm, int i, int j, const TrackParams &tp)
{
    const uint32_t lo = (uint32_t)(tp.near_clip * 1000.0f);
    const uint32_t hi = (uint32_t)((tp.far_clip - 0.001f) * 1000.0f);
    const uint32_t v = mm[(size_t)j * tp.W + i];
    if ((float)i + 0.5f < tp.stereo_border) return 0.0f;
    return (v > lo && v < hi) ? (float)v / 1000.0f : 0.0f;
}

__global__ __launch_bounds__(256) void k_track_vertex(const uint16_t *__restrict__ mm, const float *__restrict__ xs,
                                                      const float *__restrict__ ys, TrackParams tp, float4 *__restrict__ vmap,
                                                      float4 *__restrict__ nmap)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= tp.n) return;
    const int gj = idx / tp.ni;
    const int i = (idx - gj * tp.ni) * tp.stride, j = gj * tp.stride;
    const int W = tp.W, H = tp.H;
    // clamp-to-edge neighbours, as the frame's surfels (local_surfel)
    const float z = track_depth(mm, i, j, tp);
    const float zl = track_depth(mm, i > 0 ? i - 1 : i, j, tp), zr = track_depth(mm, i < W - 1 ? i + 1 : i, j, tp);
    const float zu = track_depth(mm, i, j > 0 ? j - 1 : j, tp), zd = track_depth(mm, i, j < H - 1 ? j + 1 : j, tp);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // checkNeighbours + range (data.vert:33-52,87); no checkerboard: every grid pixel is a measurement
    if (z > 0.0f && zl != 0.0f && zu != 0.0f && zr != 0.0f && zd != 0.0f) {
        FrameParams fp;                                       // (get_vertex reads cx, cy only)
        fp.cx = tp.cx; fp.cy = tp.cy;
        const float x = xs[i], y = ys[j];
        const float3 p = get_vertex(z, x, y, fp, tp.inv_fx, tp.inv_fy);
        const float3 xf = get_vertex(zr, x + 1.0f, y, fp, tp.inv_fx, tp.inv_fy);
        const float3 xb = get_vertex(zl, x - 1.0f, y, fp, tp.inv_fx, tp.inv_fy);
        const float3 yf = get_vertex(zd, x, y + 1.0f, fp, tp.inv_fx, tp.inv_fy);
        const float3 yb = get_vertex(zu, x, y - 1.0f, fp, tp.inv_fx, tp.inv_fy);
        const float3 del_x = make_float3(xb.x - xf.x, xb.y - xf.y, xb.z - xf.z);
        const float3 del_y = make_float3(yb.x - yf.x, yb.y - yf.y, yb.z - yf.z);
        const float3 n = normalize3(cross3(del_x, del_y));
        if (isfinite(n.x) && isfinite(n.y) && isfinite(n.z)) {
            v = make_float4(p.x, p.y, p.z, 1.0f);
            nn = make_float4(n.x, n.y, n.z, 0.0f);
        }
    }
    vmap[idx] = v;
    nmap[idx] = nn;
}

// ---- one Gauss-Newton iteration ----

// the estimate in float, column-major (rounded from the double state)
__device__ __forceinline__ void track_pose_f(const TrackState *__restrict__ ts, float *m)
{
#pragma unroll
    for (int e = 0; e < 16; ++e) m[e] = (float)ts->T[e];
}

// association and residual of grid point idx under the pose `m`: false if not an inlier
__device__ __forceinline__ bool track_pair(int idx, const float *m, const TrackParams &tp, const float4 *__restrict__ vmap,
                                           const float4 *__restrict__ nmap, const int32_t *__restrict__ pred, const SurfelSet &cur,
                                           float *J, float &r)
{
    const float4 v = vmap[idx];
    if (v.w == 0.0f) return false;
    const float4 n = nmap[idx];
    const float3 w = xform3(m, v.x, v.y, v.z);                // T v
    const float3 nw = rot3(m, n.x, n.y, n.z);                 // R n
    const float3 c = xform3(tp.tinv_prev, w.x, w.y, w.z);     // into the prediction camera
    if (!(c.z > 0.0f)) return false;
    const float fu = floorf(((tp.fx * c.x) / c.z + tp.cx) + 0.5f);
    const float fv = floorf(((tp.fy * c.y) / c.z + tp.cy) + 0.5f);
    if (!(fu >= 0.0f && fu < (float)tp.W && fv >= 0.0f && fv < (float)tp.H)) return false;
    const int32_t s = pred[(size_t)(int)fv * tp.W + (int)fu];
    if (s < 0) return false;
    const float4 pm = cur.pos_conf[s];
    const float4 nm = cur.norm_rad[s];
    const float3 d = make_float3(w.x - pm.x, w.y - pm.y, w.z - pm.z);
    if (!(sqrtf(dot3(d, d)) <= tp.dist)) return false;
    const float3 nm3 = make_float3(nm.x, nm.y, nm.z);
    if (!(dot3(nw, nm3) >= tp.cos_angle)) return false;
    r = dot3(nm3, d);
    const float3 wn = cross3(w, nm3);
    J[0] = nm.x; J[1] = nm.y; J[2] = nm.z; J[3] = wn.x; J[4] = wn.y; J[5] = wn.z;
    return true;
}

// every workgroup: its lanes take grid points idx = blockIdx*256 + tid + k * nb*256 (fixed), so partials do not depend on timing
__device__ __forceinline__ void track_reduce_body(const Model &M, const DevState *__restrict__ st, const TrackParams &tp,
                                                  const float4 *__restrict__ vmap, const float4 *__restrict__ nmap,
                                                  const int32_t *__restrict__ pred, const TrackState *__restrict__ ts,
                                                  double *__restrict__ part, double (*s_w)[TRACK_NSYS])
{
    float m[16];
    track_pose_f(ts, m);
    const SurfelSet cur = M.s[st->cur];
    double acc[TRACK_NSYS];
#pragma unroll
    for (int e = 0; e < TRACK_NSYS; ++e) acc[e] = 0.0;
    const int step = tp.nb * TRACK_BLOCK;
    for (int idx = blockIdx.x * TRACK_BLOCK + threadIdx.x; idx < tp.n; idx += step) {
        float J[6], r;
        if (!track_pair(idx, m, tp, vmap, nmap, pred, cur, J, r)) continue;
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
    track_block_sum(acc, s_w, tp.nb, part);
}

__global__ __launch_bounds__(TRACK_BLOCK) void k_track_reduce(Model M, const DevState *__restrict__ st, TrackParams tp,
                                                              const float4 *__restrict__ vmap, const float4 *__restrict__ nmap,
                                                              const int32_t *__restrict__ pred, const TrackState *__restrict__ ts,
                                                              double *__restrict__ part)
{
    if (ts->done) return;                                     // converged or failed: the remaining launches are no-ops
    __shared__ double s_w[TRACK_BLOCK / 64][TRACK_NSYS];
    track_reduce_body(M, st, tp, vmap, nmap, pred, ts, part, s_w);
}

// Gauss-Newton step: track_solve_xi, T <- exp(xi) T, the step's norms into ts; false if A is not positive definite
__device__ inline bool track_step(const double A[6][6], const double *b, TrackState *__restrict__ ts)
{
    double xi[6];
    if (!track_solve_xi(A, b, xi)) return false;
    double R[3][3], tt[3];
    track_exp(xi, R, tt);
    const double *T = ts->T;                                  // column-major: T[c * 4 + r]
    double Tn[16];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Tn[c * 4 + r] = R[r][0] * T[c * 4 + 0] + R[r][1] * T[c * 4 + 1] + R[r][2] * T[c * 4 + 2];
        Tn[12 + r] = R[r][0] * T[12] + R[r][1] * T[13] + R[r][2] * T[14] + tt[r];
    }
    Tn[3] = 0.0; Tn[7] = 0.0; Tn[11] = 0.0; Tn[15] = 1.0;
    for (int k = 0; k < 16; ++k) ts->T[k] = Tn[k];
    ts->step_rot = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
    ts->step_trans = sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
    return true;
}

__device__ inline void track_fail(TrackState *__restrict__ ts, int status)
{
    for (int e = 0; e < 16; ++e) ts->T[e] = ts->guess[e];
    ts->status = status;
    ts->done = 1;
}

// one workgroup.  sum_only: only the fixed-order sum into ts->sys (sm_track_debug)
__global__ __launch_bounds__(256) void k_track_solve(TrackParams tp, const double *__restrict__ part, TrackState *__restrict__ ts,
                                                     int sum_only)
{
    if (ts->done) return;
    __shared__ double s_p[TRACK_NSYS][8];
    double sys[TRACK_NSYS];
    track_sum_parts(part, tp.nb, s_p, sys);
    if (threadIdx.x != 0) return;
    for (int e = 0; e < TRACK_NSYS; ++e) ts->sys[e] = sys[e];
    if (sum_only) return;
    const double cnt = sys[28];
    ts->iterations += 1;
    ts->inliers = (uint32_t)cnt;
    ts->rmse = cnt > 0.0 ? sqrt(sys[27] / cnt) : 0.0;
    if (ts->iterations == 1 && ts->in_view == 0u) { track_fail(ts, TRACK_NO_MODEL); return; }
    if (cnt < (double)tp.min_inliers || cnt < 6.0) { track_fail(ts, TRACK_LOST); return; }
    double A[6][6], b[6];
    track_unpack(sys, A, b);
    ts->pivot_ratio = track_pivot_ratio(A, tp.c);
    // (judged on the system of the last iteration: a poor guess can pair mostly ground and walls in the first ones)
    const bool degenerate = !(ts->pivot_ratio >= tp.degenerate_bound);
    if (!track_step(A, b, ts)) { track_fail(ts, TRACK_DEGENERATE); return; }
    const bool converged = ts->step_rot < 1e-6 && ts->step_trans < 1e-6;
    if ((converged || ts->iterations >= tp.max_iters) && degenerate) { track_fail(ts, TRACK_DEGENERATE); return; }
    if (converged) ts->done = 1;
}

}  // namespace sm
