// sm_track.hip -- camera tracking: projective frame-to-model point-to-plane ICP (sm_track_*; DESIGN.md "4d. Tracking").
// Kernels: sm_k_track.h.
#include "sm_ctx.h"
#include "sm_k_track.h"

#include <cmath>

using namespace sm;

namespace {
// [R^T | -R^T t] of a column-major rigid pose, double
void rigid_inv_d(const double *m, double *o)
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[c * 4 + r] = m[r * 4 + c];
        o[12 + r] = -((m[r * 4 + 0] * m[12] + m[r * 4 + 1] * m[13]) + m[r * 4 + 2] * m[14]);
    }
    o[3] = 0.0; o[7] = 0.0; o[11] = 0.0; o[15] = 1.0;
}

// column-major rigid product a * b, double
void mul_rigid_d(const double *a, const double *b, double *o)
{
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r)
            o[c * 4 + r] = ((a[r] * b[c * 4] + a[4 + r] * b[c * 4 + 1]) + a[8 + r] * b[c * 4 + 2]) + (c == 3 ? a[12 + r] : 0.0);
    o[3] = 0.0; o[7] = 0.0; o[11] = 0.0; o[15] = 1.0;
}

// the rotation of a column-major pose made orthonormal (Gram-Schmidt on columns 0 and 1, column 2 = 0 x 1), double.  Float
// poses are orthonormal to ~1e-7 only; products of them (the constant-velocity guess, exp(xi) * guess) would carry and, frame
// after frame, multiply that error, so every product starts from orthonormal factors.
void orthonormalize_d(double *m)
{
    double *a = m, *b = m + 4, *c = m + 8;
    const double na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (int k = 0; k < 3; ++k) a[k] /= na;
    const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    for (int k = 0; k < 3; ++k) b[k] -= ab * a[k];
    const double nb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    for (int k = 0; k < 3; ++k) b[k] /= nb;
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
    m[3] = 0.0; m[7] = 0.0; m[11] = 0.0; m[15] = 1.0;
}

// constant velocity T_prev * (T_prev2^-1 * T_prev) of the orthonormalised poses; one processed pose: that pose; none: the identity
void track_guess(const sm_ctx *s, float *g)
{
    if (s->trk.n_hist == 0) {
        for (int e = 0; e < 16; ++e) g[e] = (e % 5 == 0) ? 1.0f : 0.0f;
        return;
    }
    if (s->trk.n_hist == 1) { memcpy(g, s->trk.hist[0], 64); return; }
    double p[16], p2[16], p2i[16], rel[16], out[16];
    for (int e = 0; e < 16; ++e) { p[e] = s->trk.hist[0][e]; p2[e] = s->trk.hist[1][e]; }
    orthonormalize_d(p);
    orthonormalize_d(p2);
    rigid_inv_d(p2, p2i);
    mul_rigid_d(p2i, p, rel);
    mul_rigid_d(p, rel, out);
    for (int e = 0; e < 16; ++e) g[e] = (float)out[e];
}

int track_alloc(sm_ctx *s)
{
    if (s->trk.d_state) return SM_OK;
    const size_t P = (size_t)s->P;
    Dev<uint16_t> depth; Dev<float4> v, n; Dev<uint64_t> key; Dev<int32_t> pred; Dev<double> part; Dev<TrackState> d;
    Host<TrackState> h;
    int rc;
    if ((rc = dalloc(depth, P)) || (rc = dalloc(v, P)) || (rc = dalloc(n, P)) || (rc = dalloc(key, P)) || (rc = dalloc(pred, P)) ||
        (rc = dalloc(part, (size_t)TRACK_NSYS * TRACK_MAX_PARTS)) || (rc = dalloc(d, 1)))
        return rc;
    HIPCK(hipHostMalloc(h.put(), sizeof(TrackState)));
    s->trk.d_depth = std::move(depth); s->trk.d_v = std::move(v); s->trk.d_n = std::move(n); s->trk.d_key = std::move(key);
    s->trk.d_pred = std::move(pred); s->trk.d_part = std::move(part); s->trk.h_state = std::move(h);
    s->trk.d_state = std::move(d);              // last: it marks the set complete
    return SM_OK;
}

int track_check(sm_ctx *s, const char *fn)
{
    if (s->ss_on) { g_err = std::string(fn) + ": a sharded context holds only its rank's surfels; tracking is not supported"; return SM_E_UNSUPPORTED; }
    if (s->pending_cull) { g_err = std::string(fn) + " between sm_stage_conflict and sm_stage_cull"; return SM_E_ARG; }
    return SM_OK;
}

TrackParams track_params(const sm_ctx *s, const sm_track_params &p)
{
    TrackParams tp;
    memset(&tp, 0, sizeof tp);
    double prev[16], inv[16];
    for (int e = 0; e < 16; ++e) prev[e] = s->trk.n_hist ? (double)s->trk.hist[0][e] : ((e % 5 == 0) ? 1.0 : 0.0);
    rigid_inv_d(prev, inv);
    for (int e = 0; e < 16; ++e) tp.tinv_prev[e] = (float)inv[e];
    for (int k = 0; k < 3; ++k) tp.c[k] = prev[12 + k];
    const sm_config &c = s->cfg;
    tp.fx = c.fx; tp.fy = c.fy; tp.cx = c.cx; tp.cy = c.cy;
    tp.inv_fx = (float)(1.0 / (double)c.fx);
    tp.inv_fy = (float)(1.0 / (double)c.fy);
    tp.near_clip = c.near_clip; tp.far_clip = c.far_clip; tp.stereo_border = c.stereo_border;
    tp.W = s->W; tp.H = s->H;
    tp.stride = p.pixel_stride;
    tp.ni = (s->W + p.pixel_stride - 1) / p.pixel_stride;
    tp.nj = (s->H + p.pixel_stride - 1) / p.pixel_stride;
    tp.n = tp.ni * tp.nj;
    tp.dist = p.dist_thresh;
    tp.cos_angle = (float)std::cos((double)p.angle_thresh * (3.14159265358979323846 / 180.0));
    tp.min_inliers = (uint32_t)p.min_inliers;
    tp.degenerate_bound = SM_TRACK_DEGENERATE_BOUND;
    tp.max_iters = p.max_iters;
    tp.nb = (int)std::min<long>(TRACK_MAX_PARTS, std::max<long>(1, ((long)tp.n + TRACK_BLOCK * 4 - 1) / (TRACK_BLOCK * 4)));
    return tp;
}

int track_event(sm_ctx *s, size_t i)
{
    if (!s->trk.timed) return SM_OK;
    while (s->trk.ev.size() <= i) {
        Event e;
        HIPCK(hipEventCreate(e.put()));
        s->trk.ev.push_back(std::move(e));
    }
    HIPCK(hipEventRecord(s->trk.ev[i], s->stream));
    return SM_OK;
}

// the state, the prediction at T_prev and the vertex / normal stage, enqueued (the model's state has been pulled)
int track_prepare(sm_ctx *s, const uint16_t *depth_mm, const TrackParams &tp, const float *T0, const float *guess, bool ortho)
{
    const size_t P = (size_t)s->P;
    TrackState &h = *s->trk.h_state;
    memset(&h, 0, sizeof h);
    for (int e = 0; e < 16; ++e) { h.T[e] = T0[e]; h.guess[e] = guess[e]; }
    if (ortho) orthonormalize_d(h.T);
    h.status = TRACK_OK;
    HIPCK(hipMemcpyAsync(s->trk.d_state, &h, sizeof h, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(s->trk.d_depth, depth_mm, P * 2, hipMemcpyHostToDevice, s->stream));
    const char *te = std::getenv("SM_TRACK_TIMING");
    s->trk.timed = te && te[0] == '1';
    s->trk.ev_iters = 0;
    int rc;
    if ((rc = track_event(s, 0))) return rc;
    const unsigned pblocks = (unsigned)((P + 255) / 256);
    fill_keys(s, s->trk.d_key, P);
    const uint32_t slots = s->h_state->count;
    if (slots)
        hipLaunchKernelGGL(k_track_splat, dim3((slots + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, s->d_alive, tp,
                           s->trk.d_key, s->trk.d_state);
    hipLaunchKernelGGL(k_track_resolve, dim3(pblocks), dim3(256), 0, s->stream, s->trk.d_key, (int)P, s->trk.d_pred);
    if ((rc = track_event(s, 1))) return rc;
    hipLaunchKernelGGL(k_track_vertex, dim3((tp.n + 255) / 256), dim3(256), 0, s->stream, s->trk.d_depth, s->d_xs, s->d_ys, tp,
                       s->trk.d_v, s->trk.d_n);
    HIPCK(hipGetLastError());
    return track_event(s, 2);
}

int track_iteration(sm_ctx *s, const TrackParams &tp, int sum_only)
{
    hipLaunchKernelGGL(k_track_reduce, dim3(tp.nb), dim3(TRACK_BLOCK), 0, s->stream, s->M, s->d_state, tp, s->trk.d_v, s->trk.d_n,
                       s->trk.d_pred, s->trk.d_state, s->trk.d_part);
    int rc;
    if ((rc = track_event(s, 3 + 2 * (size_t)s->trk.ev_iters))) return rc;
    hipLaunchKernelGGL(k_track_solve, dim3(1), dim3(256), 0, s->stream, tp, s->trk.d_part, s->trk.d_state, sum_only);
    HIPCK(hipGetLastError());
    if ((rc = track_event(s, 4 + 2 * (size_t)s->trk.ev_iters))) return rc;
    s->trk.ev_iters++;
    return SM_OK;
}
}  // namespace

extern "C" {

int sm_default_track_params(sm_track_params *p)
{
    if (!p) return SM_E_ARG;
    p->max_iters = 15;
    p->dist_thresh = 0.3f;
    p->angle_thresh = 30.0f;
    p->min_inliers = 1000;
    p->pixel_stride = 1;
    return SM_OK;
}

int sm_track_frame(sm_ctx *s, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params, float *pose16_out,
                   sm_track_info *info)
{
    if (!s || !depth_mm || !pose16_out) { g_err = "sm_track_frame: null argument"; return SM_E_ARG; }
    sm_track_params p;
    if (params) p = *params;
    else sm_default_track_params(&p);
    if (p.max_iters < 1 || p.max_iters > SM_TRACK_MAX_ITERS || !(p.dist_thresh > 0.0f) || !std::isfinite(p.dist_thresh) ||
        !(p.angle_thresh > 0.0f && p.angle_thresh <= 180.0f) || p.min_inliers < 0 || p.pixel_stride < 1 ||
        p.pixel_stride > std::min(s->W, s->H)) {
        g_err = "sm_track_frame: parameter out of range (max_iters 1..100, dist_thresh > 0, angle_thresh in (0, 180], "
                "min_inliers >= 0, pixel_stride 1..min(W, H))";
        return SM_E_ARG;
    }
    int rc = track_check(s, "sm_track_frame");
    if (rc) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = pull_state(s))) return rc;                      // waits for frames in flight: the model after the last frame
    float g[16];
    if (guess16) memcpy(g, guess16, 64);
    else track_guess(s, g);
    sm_track_info inf;
    memset(&inf, 0, sizeof inf);
    memcpy(inf.guess, g, 64);
    const uint32_t live = s->h_state->count - s->h_state->garbage;
    if (s->trk.n_hist == 0 || live == 0) {
        inf.status = SM_TRACK_NO_MODEL;
        memcpy(pose16_out, g, 64);
        if (info) *info = inf;
        return SM_OK;
    }
    if ((rc = track_alloc(s))) return rc;
    const TrackParams tp = track_params(s, p);
    if ((rc = track_prepare(s, depth_mm, tp, g, g, true))) return rc;    // (iterates from the orthonormalised guess)
    for (int it = 0; it < p.max_iters; ++it)
        if ((rc = track_iteration(s, tp, 0))) return rc;
    HIPCK(hipMemcpyAsync(s->trk.h_state, s->trk.d_state, sizeof(TrackState), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));                   // the one wait of a tracked frame
    const TrackState &h = *s->trk.h_state;
    for (int e = 0; e < 16; ++e) pose16_out[e] = (float)h.T[e];
    inf.status = h.status;
    inf.iterations = h.iterations;
    inf.inliers = h.inliers;
    inf.rmse = (float)h.rmse;
    if (info) *info = inf;
    return SM_OK;
}

int sm_track_debug(sm_ctx *s, const uint16_t *depth_mm, const float *pose16_eval, int32_t *pred_slot, double *sys29)
{
    if (!s || !depth_mm || !pose16_eval) { g_err = "sm_track_debug: null argument"; return SM_E_ARG; }
    int rc = track_check(s, "sm_track_debug");
    if (rc) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = pull_state(s))) return rc;
    if ((rc = track_alloc(s))) return rc;
    sm_track_params p;
    sm_default_track_params(&p);
    const TrackParams tp = track_params(s, p);
    if ((rc = track_prepare(s, depth_mm, tp, pose16_eval, pose16_eval, false))) return rc;   // (the pose as given)
    if ((rc = track_iteration(s, tp, 1))) return rc;
    if (pred_slot) HIPCK(hipMemcpyAsync(pred_slot, s->trk.d_pred, (size_t)s->P * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(s->trk.h_state, s->trk.d_state, sizeof(TrackState), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    if (sys29) memcpy(sys29, s->trk.h_state->sys, TRACK_NSYS * sizeof(double));
    return SM_OK;
}

// Diagnostic, deliberately not part of include/sm_c_api.h (tools/track_probe.py): device times of the last sm_track_frame /
// sm_track_debug call made with SM_TRACK_TIMING=1, in ms: ms[0] prediction (key fill, splat, resolve), ms[1] vertex stage, then per
// launched iteration its reduction and its solve (a no-op once converged); *n = values written (0 if that call was not timed).
int sm_debug_track_stats(sm_ctx *s, float *ms, int cap, int *n)
{
    if (!s || !ms || !n) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipStreamSynchronize(s->stream));
    *n = 0;
    if (!s->trk.timed) return SM_OK;
    const int total = 2 + 2 * s->trk.ev_iters;
    for (int i = 0; i < total && i < cap; ++i) {
        HIPCK(hipEventElapsedTime(&ms[i], s->trk.ev[i], s->trk.ev[i + 1]));
        *n = i + 1;
    }
    return SM_OK;
}

}  // extern "C"
