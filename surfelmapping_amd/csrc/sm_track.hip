// sm_track.hip -- camera tracking: projective frame-to-model point-to-plane ICP (sm_track_*; DESIGN.md "4d. Tracking").
// Kernels: sm_k_track.h; the colour term (sm_track_frame_rgb): sm_k_track_rgb.h.
#include "sm_ctx.h"
#include "sm_k_track.h"
#include "sm_k_track_rgb.h"
#include "sm_k_loop.h"
#include "sm_pose.h"

#include <cmath>

using namespace sm;
using sm_pose::orthonormalize_d;
using sm_pose::rigid_inv_d;

namespace {
// constant velocity T_prev * (T_prev2^-1 * T_prev) of the orthonormalised poses; one processed pose: that pose; none: the identity
void track_guess(const sm_ctx *s, float *g)
{
    if (s->trk.n_hist == 0) { sm_pose::identity(g); return; }
    if (s->trk.n_hist == 1) { memcpy(g, s->trk.hist[0], 64); return; }
    double p[16], p2[16], p2i[16], rel[16], out[16];
    sm_pose::widen(s->trk.hist[0], p);
    sm_pose::widen(s->trk.hist[1], p2);
    orthonormalize_d(p);
    orthonormalize_d(p2);
    rigid_inv_d(p2, p2i);
    sm_pose::mul_rigid_d(p2i, p, rel);
    sm_pose::mul_rigid_d(p, rel, out);
    for (int e = 0; e < 16; ++e) g[e] = (float)out[e];
}

int track_alloc(sm_ctx *s)
{
    if (s->trk.d_state) return SM_OK;
    const size_t P = (size_t)s->P;
    Dev<uint16_t> depth; Dev<float4> v, n; Dev<uint64_t> key; Dev<int32_t> pred; Dev<double> part; Dev<TrackState> d;
    Dev<uint32_t> anchor;
    Host<TrackState> h;
    int rc;
    if ((rc = dalloc(anchor, 1)) || (rc = dalloc(depth, P)) || (rc = dalloc(v, P)) || (rc = dalloc(n, P)) || (rc = dalloc(key, P)) || (rc = dalloc(pred, P)) ||
        (rc = dalloc(part, (size_t)TRACK_NSYS * TRACK_MAX_PARTS)) || (rc = dalloc(d, 1)))
        return rc;
    HIPCK(hipHostMalloc(h.put(), sizeof(TrackState)));
    s->trk.d_depth = std::move(depth); s->trk.d_v = std::move(v); s->trk.d_n = std::move(n); s->trk.d_key = std::move(key);
    s->trk.d_pred = std::move(pred); s->trk.d_part = std::move(part); s->trk.h_state = std::move(h);
    s->trk.d_anchor = std::move(anchor);
    s->trk.d_state = std::move(d);              // last: it marks the set complete
    return SM_OK;
}

int track_check(sm_ctx *s, const char *fn)
{
    if (s->ss_on) { g_err = std::string(fn) + ": a sharded context holds only its rank's surfels; tracking is not supported"; return SM_E_UNSUPPORTED; }
    if (int rc = check_not_mid_cull(s, fn)) return rc;
    return SM_OK;
}

int track_params_check(const sm_ctx *s, const sm_track_params &p, const char *fn)
{
    if (p.max_iters < 1 || p.max_iters > SM_TRACK_MAX_ITERS || !(p.dist_thresh > 0.0f) || !std::isfinite(p.dist_thresh) ||
        !(p.angle_thresh > 0.0f && p.angle_thresh <= 180.0f) || p.min_inliers < 0 || p.pixel_stride < 1 ||
        p.pixel_stride > std::min(s->W, s->H)) {
        g_err = std::string(fn) + ": parameter out of range (max_iters 1..100, dist_thresh > 0, angle_thresh in (0, 180], "
                                  "min_inliers >= 0, pixel_stride 1..min(W, H))";
        return SM_E_ARG;
    }
    return SM_OK;
}

// pred16 (null: T_prev) is the camera the prediction is drawn at
TrackParams track_params(const sm_ctx *s, const sm_track_params &p, const float *pred16 = nullptr)
{
    TrackParams tp;
    memset(&tp, 0, sizeof tp);
    double prev[16], inv[16];
    if (pred16) sm_pose::widen(pred16, prev);                         // (sm_search_pose_at: the prediction is drawn elsewhere)
    else if (s->trk.n_hist) sm_pose::widen(s->trk.hist[0], prev);
    else sm_pose::identity(prev);
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

// the state, the prediction at T_prev and the vertex / normal stage, enqueued (the model's state has been pulled).
// win (sm_track_*_old, sm_track_*_window; null otherwise): the prediction holds only surfels last updated inside it, and the
// newest time it holds is left in d_anchor
int track_prepare(sm_ctx *s, const uint16_t *depth_mm, const TrackParams &tp, const float *T0, const float *guess, bool ortho,
                  const TrackWindow *win)
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
    // (an open end is not compared: both open is exactly sm_track_frame's prediction, whatever the times are, and an open
    // lower end exactly sm_track_frame_old's)
    const bool use_min = win && win->lo != INT32_MIN, use_max = win && win->hi != INT32_MAX;
    const auto splat = use_min ? (use_max ? k_track_splat<true, true> : k_track_splat<true, false>)
                               : (use_max ? k_track_splat<false, true> : k_track_splat<false, false>);
    if (slots)
        hipLaunchKernelGGL(splat, dim3((slots + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, s->d_alive, tp,
                           use_min ? (float)win->lo : 0.0f, use_max ? (float)win->hi : 0.0f, s->trk.d_key, s->trk.d_state);
    hipLaunchKernelGGL(k_track_resolve, dim3(pblocks), dim3(256), 0, s->stream, s->trk.d_key, (int)P, s->trk.d_pred);
    if (win) {
        HIPCK(hipMemsetAsync(s->trk.d_anchor, 0, 4, s->stream));
        hipLaunchKernelGGL(k_track_anchor, dim3(pblocks), dim3(256), 0, s->stream, s->M, s->d_state, s->trk.d_pred, (int)P, s->trk.d_anchor);
    }
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

// ---- the colour term ----

enum { RGB_EV_PYRAMID = 2, RGB_EV_GATHER = 3, RGB_EV_VERTEX = 4, RGB_EV_ICP = 5, RGB_EV_PHOTO = 6, RGB_EV_SOLVE = 7 };

int track_rgb_alloc(sm_ctx *s)
{
    if (s->trk.d_rstate) return SM_OK;
    const size_t P = (size_t)s->P;
    Dev<uint8_t> rgb; Dev<float> pyr; Dev<float4> plane; Dev<double> part; Dev<TrackRgbState> d;
    Host<TrackRgbState> h;
    int rc;
    // (levels 1.. hold at most P / 3 pixels together)
    if ((rc = dalloc(rgb, P * 3)) || (rc = dalloc(pyr, P + P / 3 + 1)) || (rc = dalloc(plane, P)) ||
        (rc = dalloc(part, (size_t)TRACK_NSYS * TRACK_MAX_PARTS)) || (rc = dalloc(d, 1)))
        return rc;
    HIPCK(hipHostMalloc(h.put(), sizeof(TrackRgbState)));
    s->trk.d_rgb = std::move(rgb); s->trk.d_pyr = std::move(pyr); s->trk.d_plane = std::move(plane);
    s->trk.d_part_rgb = std::move(part); s->trk.h_rstate = std::move(h);
    s->trk.d_rstate = std::move(d);             // last: it marks the set complete
    return SM_OK;
}

// the event that closes an interval of kind `kind` at `level` (after track_prepare's events 0..2)
int track_rgb_event(sm_ctx *s, int kind, int level)
{
    if (!s->trk.timed) return SM_OK;
    s->trk.ev_kind.push_back(kind | (level << 4));
    return track_event(s, 2 + s->trk.ev_kind.size());
}

const char *track_rgb_check(const sm_ctx *s, const sm_track_params &p, const sm_track_rgb_params &q)
{
    if (q.levels < 1 || q.levels > TRACK_RGB_LEVELS) return "levels outside 1..6";
    long sum = 0;
    for (int l = 0; l < q.levels; ++l) {
        if (q.iters[l] < 1) return "iters[l] < 1 for a used level";
        sum += q.iters[l];
    }
    if (sum > SM_TRACK_MAX_ITERS) return "the sum of iters exceeds SM_TRACK_MAX_ITERS";
    if (!(q.rgb_weight >= 0.0f) || !std::isfinite(q.rgb_weight)) return "rgb_weight negative or not finite";
    if (!(q.rgb_max_residual > 0.0f)) return "rgb_max_residual <= 0";
    if ((s->W >> (q.levels - 1)) < 8 || (s->H >> (q.levels - 1)) < 8) return "the coarsest level is smaller than 8 x 8";
    if ((long)p.pixel_stride << (q.levels - 1) > std::min(s->W, s->H)) return "pixel_stride * 2^(levels-1) exceeds min(W, H)";
    return nullptr;
}

TrackRgbParams track_rgb_params(const sm_ctx *s, const sm_track_rgb_params &q)
{
    TrackRgbParams rp;
    memset(&rp, 0, sizeof rp);
    rp.levels = q.levels;
    int off = 0;
    for (int l = 0; l < TRACK_RGB_LEVELS; ++l) {
        rp.iters[l] = q.iters[l];
        rp.lw[l] = s->W >> l; rp.lh[l] = s->H >> l;
        rp.off[l] = off;
        off += rp.lw[l] * rp.lh[l];
    }
    rp.max_residual = q.rgb_max_residual;
    rp.lambda = (double)q.rgb_weight;
    return rp;
}

TrackParams track_level_params(const sm_ctx *s, sm_track_params p, int level, const float *pred16 = nullptr)
{
    p.pixel_stride <<= level;
    return track_params(s, p, pred16);
}

// sm_track_frame's preparation on the coarsest level's grid, then the pyramid and the gathered prediction (the rgb upload precedes event 0, as the depth's)
int track_rgb_prepare(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const TrackParams &tpc, const TrackRgbParams &rp,
                      const float *T0, const float *guess, bool ortho, int first_level, const TrackWindow *win)
{
    const size_t P = (size_t)s->P;
    TrackRgbState &h = *s->trk.h_rstate;
    memset(&h, 0, sizeof h);
    h.level = first_level;
    HIPCK(hipMemcpyAsync(s->trk.d_rstate, &h, sizeof h, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(s->trk.d_rgb, rgb, P * 3, hipMemcpyHostToDevice, s->stream));
    s->trk.ev_kind.clear();
    int rc;
    if ((rc = track_prepare(s, depth_mm, tpc, T0, guess, ortho, win))) return rc;
    hipLaunchKernelGGL(k_track_luma_pyr, dim3((s->W + TRACK_RGB_TILE - 1) / TRACK_RGB_TILE, (s->H + TRACK_RGB_TILE - 1) / TRACK_RGB_TILE),
                       dim3(256), 0, s->stream, s->trk.d_rgb, s->W, s->H, rp, s->trk.d_pyr);
    if ((rc = track_rgb_event(s, RGB_EV_PYRAMID, 0))) return rc;
    hipLaunchKernelGGL(k_track_gather, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s->stream, s->M, s->d_state, s->trk.d_pred,
                       (int)P, s->trk.d_plane);
    HIPCK(hipGetLastError());
    return track_rgb_event(s, RGB_EV_GATHER, 0);
}

// the vertex stage of a level's grid (the coarsest level's is track_prepare's own)
int track_rgb_level(sm_ctx *s, const TrackParams &tpl, int level)
{
    hipLaunchKernelGGL(k_track_vertex, dim3((tpl.n + 255) / 256), dim3(256), 0, s->stream, s->trk.d_depth, s->d_xs, s->d_ys, tpl,
                       s->trk.d_v, s->trk.d_n);
    HIPCK(hipGetLastError());
    return track_rgb_event(s, RGB_EV_VERTEX, level);
}

int track_rgb_iteration(sm_ctx *s, const TrackParams &tpl, const TrackRgbParams &rp, int level, int sum_only)
{
    int rc;
    hipLaunchKernelGGL(k_track_rgb_icp, dim3(tpl.nb), dim3(TRACK_BLOCK), 0, s->stream, s->M, s->d_state, tpl, level, s->trk.d_v,
                       s->trk.d_n, s->trk.d_pred, s->trk.d_state, s->trk.d_rstate, s->trk.d_part);
    if ((rc = track_rgb_event(s, RGB_EV_ICP, level))) return rc;
    hipLaunchKernelGGL(k_track_rgb_photo, dim3(tpl.nb), dim3(TRACK_BLOCK), 0, s->stream, tpl, rp, level, s->trk.d_depth,
                       s->trk.d_plane, s->trk.d_pyr, s->trk.d_state, s->trk.d_rstate, s->trk.d_part_rgb);
    if ((rc = track_rgb_event(s, RGB_EV_PHOTO, level))) return rc;
    hipLaunchKernelGGL(k_track_rgb_solve, dim3(1), dim3(256), 0, s->stream, tpl, rp, level, s->trk.d_part, s->trk.d_part_rgb,
                       s->trk.d_state, s->trk.d_rstate, sum_only);
    HIPCK(hipGetLastError());
    return track_rgb_event(s, RGB_EV_SOLVE, level);
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

}  // extern "C"

namespace {
// a prediction slot code of k_track_anchor as the time it stands for (-1: the prediction is empty)
float anchor_of(uint32_t code)
{
    if (!code) return -1.0f;
    const uint32_t b = (code & 0x80000000u) ? (code & 0x7FFFFFFFu) : ~code;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// one iteration's system at the pose as given, with the default parameters: sm_track_debug* (rgb null; level and which are not
// read) and sm_track_rgb_debug* (which 0 = joint, 1 = the geometric term, 2 = the photometric term).  pred_slot may be null.
int track_debug(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16_eval, int level, int which,
                const TrackWindow *win, int32_t *pred_slot, double *sys29, const char *fn)
{
    if (!s || !depth_mm || !pose16_eval) { g_err = std::string(fn) + ": null argument"; return SM_E_ARG; }
    sm_track_params p;
    sm_default_track_params(&p);
    sm_track_rgb_params q;
    if (rgb) {
        sm_default_track_rgb_params(&q);
        q.levels = level + 1;                                 // (the pyramid up to that level; its size is checked below)
        if (level < 0 || level >= TRACK_RGB_LEVELS || which < 0 || which > 2) {
            g_err = std::string(fn) + ": level outside 0..5 or which outside 0..2";
            return SM_E_ARG;
        }
        if (const char *why = track_rgb_check(s, p, q)) { g_err = std::string(fn) + ": " + why; return SM_E_ARG; }
    }
    int rc = track_check(s, fn);
    if (rc) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = pull_state(s))) return rc;
    if ((rc = track_alloc(s)) || (rgb && (rc = track_rgb_alloc(s)))) return rc;
    const double *src = s->trk.h_state->sys;
    if (rgb) {
        const TrackRgbParams rp = track_rgb_params(s, q);
        const TrackParams tpl = track_level_params(s, p, level);
        if ((rc = track_rgb_prepare(s, rgb, depth_mm, tpl, rp, pose16_eval, pose16_eval, false, level, win))) return rc;   // (the pose as given)
        if ((rc = track_rgb_iteration(s, tpl, rp, level, 1))) return rc;
        if (which) src = which == 1 ? s->trk.h_rstate->sys_icp : s->trk.h_rstate->sys_rgb;
    } else {
        const TrackParams tp = track_params(s, p);
        if ((rc = track_prepare(s, depth_mm, tp, pose16_eval, pose16_eval, false, win))) return rc;   // (the pose as given)
        if ((rc = track_iteration(s, tp, 1))) return rc;
    }
    if (pred_slot) HIPCK(hipMemcpyAsync(pred_slot, s->trk.d_pred, (size_t)s->P * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(s->trk.h_state, s->trk.d_state, sizeof(TrackState), hipMemcpyDeviceToHost, s->stream));
    if (rgb) HIPCK(hipMemcpyAsync(s->trk.h_rstate, s->trk.d_rstate, sizeof(TrackRgbState), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    if (sys29) memcpy(sys29, src, TRACK_NSYS * sizeof(double));
    return SM_OK;
}

// what an entry point of the colour forms says to a null image (rgb null selects the depth forms in the bodies)
int null_argument(const char *fn)
{
    g_err = std::string(fn) + ": null argument";
    return SM_E_ARG;
}
}  // namespace

// ---- one tracked frame, every form: rgb null is the depth schedule (max_iters iterations on the pixel_stride grid; rgb_params and
// rgb_info are not read), otherwise the colour term's pyramid schedule; win null is the whole model (anchor_time may be null).
// fn: the public entry point the call came through -- it does not consult the policy of sm_set_auto_loop.
int sm_impl::track_windowed(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params,
                            const sm_track_rgb_params *rgb_params, const TrackWindow *win, float *pose16_out, sm_track_info *info,
                            sm_track_rgb_info *rgb_info, float *anchor_time, const char *fn, const float *pred16)
{
    if (!s || !depth_mm || !pose16_out) { g_err = std::string(fn) + ": null argument"; return SM_E_ARG; }
    sm_track_params p;
    if (params) p = *params;
    else sm_default_track_params(&p);
    sm_track_rgb_params q;
    if (rgb_params) q = *rgb_params;
    else sm_default_track_rgb_params(&q);
    int rc;
    // (max_iters is sm_track_frame's: checked as there in the colour forms too, whose schedule is iters[])
    if ((rc = track_params_check(s, p, fn))) return rc;
    if (rgb)
        if (const char *why = track_rgb_check(s, p, q)) { g_err = std::string(fn) + ": " + why; return SM_E_ARG; }
    if ((rc = track_check(s, fn))) return rc;
    if (anchor_time) *anchor_time = -1.0f;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = pull_state(s))) return rc;                      // waits for frames in flight: the model after the last frame
    float g[16];
    if (guess16) memcpy(g, guess16, 64);
    else track_guess(s, g);
    sm_track_info inf;
    sm_track_rgb_info rinf;
    memset(&inf, 0, sizeof inf);
    memset(&rinf, 0, sizeof rinf);
    memcpy(inf.guess, g, 64);
    const uint32_t live = s->h_state->count - s->h_state->garbage;
    if (s->trk.n_hist == 0 || live == 0) {
        inf.status = SM_TRACK_NO_MODEL;
        memcpy(pose16_out, g, 64);
        if (info) *info = inf;
        if (rgb && rgb_info) *rgb_info = rinf;
        return SM_OK;
    }
    if ((rc = track_alloc(s)) || (rgb && (rc = track_rgb_alloc(s)))) return rc;
    if (rgb) {
        const TrackRgbParams rp = track_rgb_params(s, q);
        // (the preparation's vertex stage is the coarsest level's; the prediction does not depend on the stride)
        const TrackParams tpc = track_level_params(s, p, q.levels - 1, pred16);
        if ((rc = track_rgb_prepare(s, rgb, depth_mm, tpc, rp, g, g, true, q.levels - 1, win))) return rc;
        for (int l = q.levels - 1; l >= 0; --l) {
            const TrackParams tpl = track_level_params(s, p, l, pred16);
            if (l < q.levels - 1 && (rc = track_rgb_level(s, tpl, l))) return rc;
            for (int it = 0; it < q.iters[l]; ++it)
                if ((rc = track_rgb_iteration(s, tpl, rp, l, 0))) return rc;
        }
    } else {
        const TrackParams tp = track_params(s, p, pred16);
        if ((rc = track_prepare(s, depth_mm, tp, g, g, true, win))) return rc;     // (iterates from the orthonormalised guess)
        for (int it = 0; it < p.max_iters; ++it)
            if ((rc = track_iteration(s, tp, 0))) return rc;
    }
    uint32_t anchor = 0;
    if (win) HIPCK(hipMemcpyAsync(&anchor, s->trk.d_anchor, 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(s->trk.h_state, s->trk.d_state, sizeof(TrackState), hipMemcpyDeviceToHost, s->stream));
    if (rgb) HIPCK(hipMemcpyAsync(s->trk.h_rstate, s->trk.d_rstate, sizeof(TrackRgbState), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));                   // the one wait of a tracked frame
    const TrackState &h = *s->trk.h_state;
    for (int e = 0; e < 16; ++e) pose16_out[e] = (float)h.T[e];
    inf.status = h.status;
    inf.iterations = h.iterations;
    inf.inliers = h.inliers;
    inf.rmse = (float)h.rmse;
    if (info) *info = inf;
    if (rgb && rgb_info) {
        const TrackRgbState &hr = *s->trk.h_rstate;
        rinf.rgb_inliers = hr.rgb_inliers;
        rinf.rgb_rmse = (float)hr.rgb_rmse;
        rinf.pivot_ratio = h.pivot_ratio;
        for (int l = 0; l < TRACK_RGB_LEVELS; ++l) rinf.level_iterations[l] = hr.level_iterations[l];
        *rgb_info = rinf;
    }
    if (anchor_time) *anchor_time = anchor_of(anchor);
    return SM_OK;
}

// ---- what the pose search takes from the preparation (sm_search.hip) ----
int sm_impl::search_prepare(sm_ctx *s, const uint16_t *depth_mm, const sm_track_params &params, int32_t stride, int32_t min_time,
                            int32_t max_time, bool fresh, SearchFrame *f, SearchBufs *b, bool *no_model, const char *fn, const float *pred16)
{
    sm_track_params p = params;
    p.pixel_stride = stride;
    int rc;
    if ((rc = track_params_check(s, p, fn)) || (rc = track_check(s, fn))) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = pull_state(s))) return rc;                      // waits for frames in flight: the model after the last frame
    *no_model = s->trk.n_hist == 0 || s->h_state->count == s->h_state->garbage;
    if (*no_model) return SM_OK;
    if ((rc = track_alloc(s))) return rc;
    const TrackParams tp = track_params(s, p, pred16);
    if (fresh) {
        float eye[16];
        sm_pose::identity(eye);
        const TrackWindow win{min_time, max_time};
        if ((rc = track_prepare(s, depth_mm, tp, eye, eye, false, &win))) return rc;   // (no estimate is iterated)
    } else {
        hipLaunchKernelGGL(k_track_vertex, dim3((tp.n + 255) / 256), dim3(256), 0, s->stream, s->trk.d_depth, s->d_xs, s->d_ys, tp,
                           s->trk.d_v, s->trk.d_n);
        HIPCK(hipGetLastError());
    }
    memcpy(f->tinv_prev, tp.tinv_prev, sizeof f->tinv_prev);
    f->fx = tp.fx; f->fy = tp.fy; f->cx = tp.cx; f->cy = tp.cy;
    f->W = tp.W; f->H = tp.H;
    f->stride = tp.stride; f->ni = tp.ni; f->nj = tp.nj; f->n = tp.n;
    f->dist = tp.dist; f->cos_angle = tp.cos_angle;
    b->v = s->trk.d_v; b->n = s->trk.d_n; b->pred = s->trk.d_pred;
    b->in_view = &s->trk.d_state.get()->in_view;
    return SM_OK;
}

// sm_track_frame (rgb null) and sm_track_frame_rgb: the track -- the auto-loop policy's while it is on -- and then the place policy
static int track_with_policies(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params,
                               const sm_track_rgb_params *rgb_params, float *pose16_out, sm_track_info *info, sm_track_rgb_info *rgb_info,
                               const char *fn)
{
    if (!s || !s->place.auto_on) {
        if (s && s->aloop.on) return auto_loop_track(s, rgb, depth_mm, guess16, params, rgb_params, pose16_out, info, rgb_info);
        return track_windowed(s, rgb, depth_mm, guess16, params, rgb_params, nullptr, pose16_out, info, rgb_info, nullptr, fn);
    }
    sm_track_info inf;
    const uint32_t closed_before = s->aloop.stats.closed;
    int rc = s->aloop.on ? auto_loop_track(s, rgb, depth_mm, guess16, params, rgb_params, pose16_out, &inf, rgb_info)
                         : track_windowed(s, rgb, depth_mm, guess16, params, rgb_params, nullptr, pose16_out, &inf, rgb_info, nullptr, fn);
    if (rc) return rc;
    if (info) *info = inf;
    return auto_place_after_track(s, rgb, depth_mm, params, rgb_params, pose16_out, inf.status, s->aloop.on && s->aloop.stats.closed != closed_before);
}

extern "C" {

int sm_track_frame(sm_ctx *s, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params, float *pose16_out,
                   sm_track_info *info)
{
    return track_with_policies(s, nullptr, depth_mm, guess16, params, nullptr, pose16_out, info, nullptr, "sm_track_frame");
}

int sm_track_frame_old(sm_ctx *s, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params, int32_t max_time,
                       float *pose16_out, sm_track_info *info, float *anchor_time)
{
    const TrackWindow win{INT32_MIN, max_time};
    return track_windowed(s, nullptr, depth_mm, guess16, params, nullptr, &win, pose16_out, info, nullptr, anchor_time, "sm_track_frame_old");
}

int sm_track_frame_window(sm_ctx *s, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params, int32_t min_time,
                          int32_t max_time, float *pose16_out, sm_track_info *info, float *anchor_time)
{
    const TrackWindow win{min_time, max_time};
    return track_windowed(s, nullptr, depth_mm, guess16, params, nullptr, &win, pose16_out, info, nullptr, anchor_time, "sm_track_frame_window");
}

int sm_track_frame_rgb(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params,
                       const sm_track_rgb_params *rgb_params, float *pose16_out, sm_track_info *info, sm_track_rgb_info *rgb_info)
{
    if (!rgb) return null_argument("sm_track_frame_rgb");
    return track_with_policies(s, rgb, depth_mm, guess16, params, rgb_params, pose16_out, info, rgb_info, "sm_track_frame_rgb");
}

int sm_track_frame_rgb_window(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params,
                              const sm_track_rgb_params *rgb_params, int32_t min_time, int32_t max_time, float *pose16_out,
                              sm_track_info *info, sm_track_rgb_info *rgb_info, float *anchor_time)
{
    if (!rgb) return null_argument("sm_track_frame_rgb_window");
    const TrackWindow win{min_time, max_time};
    return track_windowed(s, rgb, depth_mm, guess16, params, rgb_params, &win, pose16_out, info, rgb_info, anchor_time,
                          "sm_track_frame_rgb_window");
}

int sm_track_debug(sm_ctx *s, const uint16_t *depth_mm, const float *pose16_eval, int32_t *pred_slot, double *sys29)
{
    return track_debug(s, nullptr, depth_mm, pose16_eval, 0, 0, nullptr, pred_slot, sys29, "sm_track_debug");
}

int sm_track_debug_old(sm_ctx *s, const uint16_t *depth_mm, const float *pose16_eval, int32_t max_time, int32_t *pred_slot, double *sys29)
{
    const TrackWindow win{INT32_MIN, max_time};
    return track_debug(s, nullptr, depth_mm, pose16_eval, 0, 0, &win, pred_slot, sys29, "sm_track_debug_old");
}

int sm_track_debug_window(sm_ctx *s, const uint16_t *depth_mm, const float *pose16_eval, int32_t min_time, int32_t max_time,
                          int32_t *pred_slot, double *sys29)
{
    const TrackWindow win{min_time, max_time};
    return track_debug(s, nullptr, depth_mm, pose16_eval, 0, 0, &win, pred_slot, sys29, "sm_track_debug_window");
}

int sm_track_rgb_debug(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16_eval, int level, int which,
                       double *sys29)
{
    if (!rgb) return null_argument("sm_track_rgb_debug");
    return track_debug(s, rgb, depth_mm, pose16_eval, level, which, nullptr, nullptr, sys29, "sm_track_rgb_debug");
}

int sm_track_rgb_debug_window(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16_eval, int level, int which,
                              int32_t min_time, int32_t max_time, int32_t *pred_slot, double *sys29)
{
    if (!rgb) return null_argument("sm_track_rgb_debug_window");
    const TrackWindow win{min_time, max_time};
    return track_debug(s, rgb, depth_mm, pose16_eval, level, which, &win, pred_slot, sys29, "sm_track_rgb_debug_window");
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

int sm_default_track_rgb_params(sm_track_rgb_params *p)
{
    if (!p) return SM_E_ARG;
    static const int32_t iters[TRACK_RGB_LEVELS] = {10, 5, 4, 4, 4, 4};
    p->levels = 3;
    memcpy(p->iters, iters, sizeof iters);
    p->rgb_weight = 0.01f;
    p->rgb_max_residual = 0.25f;
    return SM_OK;
}

// ---- the census of old surfels in view (DESIGN.md "4i. Closing loops unasked") ----

int sm_old_in_view(sm_ctx *s, const float *pose16, int32_t max_time, uint32_t *n)
{
    const char *fn = "sm_old_in_view";
    if (!s || !pose16 || !n) { g_err = std::string(fn) + ": null argument"; return SM_E_ARG; }
    int rc;
    if ((rc = check_pose(pose16, fn)) || (rc = track_check(s, fn))) return rc;
    if (s->rig_on) { g_err = std::string(fn) + ": a rig context holds only its own surfels"; return SM_E_UNSUPPORTED; }
    *n = 0;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = pull_state(s))) return rc;                      // waits for frames in flight: the model after the last frame
    const char *te = std::getenv("SM_TRACK_TIMING");
    s->trk.census_timed = false;
    const uint32_t slots = s->h_state->count;
    if (!slots) return SM_OK;
    if (!s->trk.d_census && (rc = dalloc(s->trk.d_census, 1))) return rc;
    sm_track_params p;
    sm_default_track_params(&p);
    TrackParams tp = track_params(s, p);
    double pose[16], inv[16];
    sm_pose::widen(pose16, pose);
    rigid_inv_d(pose, inv);
    for (int e = 0; e < 16; ++e) tp.tinv_prev[e] = (float)inv[e];
    const bool timed = te && te[0] == '1';
    if (timed && !s->trk.ev_census[0]) {
        Event e0, e1;
        HIPCK(hipEventCreate(e0.put()));
        HIPCK(hipEventCreate(e1.put()));
        s->trk.ev_census[0] = std::move(e0); s->trk.ev_census[1] = std::move(e1);
    }
    HIPCK(hipMemsetAsync(s->trk.d_census, 0, 4, s->stream));
    if (timed) HIPCK(hipEventRecord(s->trk.ev_census[0], s->stream));
    const unsigned grid = (unsigned)std::min<uint32_t>((slots + 255u) / 256u, (uint32_t)LOOP_CENSUS_GRID);
    hipLaunchKernelGGL(k_loop_census, dim3(grid), dim3(256), 0, s->stream, s->M, (const DevState *)s->d_state.get(),
                       (const uint64_t *)s->d_alive.get(), tp, (float)max_time, s->trk.d_census.get());
    HIPCK(hipGetLastError());
    if (timed) HIPCK(hipEventRecord(s->trk.ev_census[1], s->stream));
    uint32_t got = 0;
    HIPCK(hipMemcpyAsync(&got, s->trk.d_census, 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    s->trk.census_timed = timed;
    *n = got;
    return SM_OK;
}

// Diagnostic, deliberately not part of include/sm_c_api.h (tools/auto_loop_probe.py): the device time in ms of k_loop_census in the
// last sm_old_in_view made with SM_TRACK_TIMING=1 (-1 if that call was not timed or launched nothing)
int sm_debug_census_ms(sm_ctx *s, float *ms)
{
    if (!s || !ms) return SM_E_ARG;
    *ms = -1.0f;
    if (!s->trk.census_timed) return SM_OK;
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipEventElapsedTime(ms, s->trk.ev_census[0], s->trk.ev_census[1]));
    return SM_OK;
}

// Diagnostic, deliberately not part of include/sm_c_api.h (tools/track_rgb_probe.py): device times of the last sm_track_frame_rgb /
// sm_track_rgb_debug call made with SM_TRACK_TIMING=1, in ms, with what each covers: kind[i] & 15 = 0 prediction, 1 vertex stage of
// the coarsest level, 2 luminance pyramid, 3 gather, 4 a finer level's vertex stage, 5 geometric reduction, 6 photometric reduction,
// 7 solve (5..7 are no-ops once their level has ended); kind[i] >> 4 = the level.  *n = values written (0 if not timed).
int sm_debug_track_rgb_stats(sm_ctx *s, float *ms, int *kind, int cap, int *n)
{
    if (!s || !ms || !kind || !n) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipStreamSynchronize(s->stream));
    *n = 0;
    if (!s->trk.timed || s->trk.ev_kind.empty()) return SM_OK;
    const int total = 2 + (int)s->trk.ev_kind.size();
    for (int i = 0; i < total && i < cap; ++i) {
        HIPCK(hipEventElapsedTime(&ms[i], s->trk.ev[i], s->trk.ev[i + 1]));
        kind[i] = i < 2 ? i : s->trk.ev_kind[i - 2];
        *n = i + 1;
    }
    return SM_OK;
}

}  // extern "C"
