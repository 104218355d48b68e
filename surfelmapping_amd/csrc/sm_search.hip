// sm_search.hip -- pose search before the tracker (sm_score_poses_window, sm_search_pose; DESIGN.md "4j. Pose search").
// Kernels: sm_k_search.h.  The prediction and the grid's vertex stage are the trackers' (sm_track.hip, search_prepare); the
// refinement runs through the trackers' one frame body (track_windowed).
#include "sm_ctx.h"
#include "sm_k_search.h"

#include <chrono>
#include <cmath>

using namespace sm;

namespace {
constexpr double DEG = 3.14159265358979323846 / 180.0;

int search_alloc(sm_ctx *s, size_t n_cand)
{
    Search &q = s->srch;
    const size_t P = (size_t)s->P;
    int rc;
    if (!q.d_nsamp) {
        Dev<uint8_t> rgb; Dev<float4> samp, plane; Dev<uint32_t> ns;
        Event e0, e1;
        if ((rc = dalloc(rgb, P * 3)) || (rc = dalloc(samp, 2 * P)) || (rc = dalloc(plane, 2 * P)) || (rc = dalloc(ns, 1))) return rc;
        HIPCK(hipEventCreate(e0.put()));
        HIPCK(hipEventCreate(e1.put()));
        q.d_rgb = std::move(rgb); q.d_samp = std::move(samp); q.d_plane = std::move(plane);
        q.ev[0] = std::move(e0); q.ev[1] = std::move(e1);
        q.d_nsamp = std::move(ns);                            // last: it marks the set complete
    }
    if (q.cand_cap < n_cand) {
        Dev<float> cand; Dev<uint32_t> scores;
        if ((rc = dalloc(cand, n_cand * 12)) || (rc = dalloc(scores, n_cand))) return rc;
        q.d_cand = std::move(cand); q.d_scores = std::move(scores);
        q.cand_cap = n_cand;
    }
    return SM_OK;
}

int check_candidates(const float *cand16, uint32_t n, const char *fn)
{
    if (n == 0 || n > SM_SEARCH_MAX_CANDIDATES) { g_err = std::string(fn) + ": the number of candidates is outside 1..2^20"; return SM_E_ARG; }
    for (size_t i = 0; i < (size_t)n * 16; ++i)
        if (!std::isfinite(cand16[i])) { g_err = std::string(fn) + ": non-finite candidate"; return SM_E_ARG; }
    return SM_OK;
}

// One scored list (arguments checked).  fresh: upload the frame and build the prediction; otherwise the last call's stand and
// only the grid changes.  *in_view: the surfels of the window in view of the prediction camera; *ms: the scoring kernels' time.
int score(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *cand16, uint32_t n, const sm_track_params &tp,
          int32_t stride, float colour_thresh, int32_t min_time, int32_t max_time, bool fresh, uint32_t *scores, bool *no_model,
          uint32_t *in_view, float *ms, const char *fn, const float *pred16 = nullptr)
{
    SearchFrame f;
    SearchBufs b;
    int rc;
    *in_view = 0;
    *ms = 0.0f;
    if ((rc = search_prepare(s, depth_mm, tp, stride, min_time, max_time, fresh, &f, &b, no_model, fn, pred16))) return rc;
    if (*no_model) { memset(scores, 0, (size_t)n * 4); return SM_OK; }
    if ((rc = search_alloc(s, n))) return rc;
    Search &q = s->srch;
    const size_t P = (size_t)s->P;
    if (fresh) {
        if (rgb) HIPCK(hipMemcpyAsync(q.d_rgb, rgb, P * 3, hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(k_search_gather, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s->stream, s->M,
                           (const DevState *)s->d_state.get(), b.pred, (int)P, q.d_plane.get());
        HIPCK(hipGetLastError());
    }
    std::vector<float> c12((size_t)n * 12);
    for (size_t i = 0; i < n; ++i)
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 3; ++r) c12[i * 12 + c * 3 + r] = cand16[i * 16 + c * 4 + r];
    HIPCK(hipMemcpyAsync(q.d_cand, c12.data(), c12.size() * 4, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemsetAsync(q.d_nsamp, 0, 4, s->stream));
    HIPCK(hipMemsetAsync(q.d_scores, 0, (size_t)n * 4, s->stream));
    uint32_t n_chunks = ((uint32_t)f.n + SEARCH_CHUNK - 1) / SEARCH_CHUNK;
    if (n_chunks >= 8) n_chunks = (n_chunks + 7u) & ~7u;      // a chunk's workgroups on one XCD (k_search_score)
    const uint32_t runs = (n + SEARCH_RUN - 1) / SEARCH_RUN;
    HIPCK(hipEventRecord(q.ev[0], s->stream));
    hipLaunchKernelGGL(k_search_samples, dim3((f.n + 255) / 256), dim3(256), 0, s->stream, b.v, b.n,
                       rgb ? (const uint8_t *)q.d_rgb.get() : (const uint8_t *)nullptr, f, q.d_samp.get(), q.d_nsamp.get());
    hipLaunchKernelGGL(k_search_score, dim3(n_chunks * runs), dim3(SEARCH_BLOCK), 0, s->stream, (const float4 *)q.d_samp.get(),
                       (const uint32_t *)q.d_nsamp.get(), (const float4 *)q.d_plane.get(), (const float *)q.d_cand.get(), n, n_chunks, f,
                       rgb ? 1 : 0, colour_thresh, q.d_scores.get());
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(q.ev[1], s->stream));
    HIPCK(hipMemcpyAsync(scores, q.d_scores, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(in_view, b.in_view, 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    HIPCK(hipEventElapsedTime(ms, q.ev[0], q.ev[1]));
    return SM_OK;
}

// ---- the candidate grids, all in double ----
// (A * B)[i][j] = (A[i][0]*B[0][j] + A[i][1]*B[1][j]) + A[i][2]*B[2][j]
void mul3(const double A[3][3], const double B[3][3], double O[3][3])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) O[i][j] = (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j];
}

// Ry(b) * Rx(a) * Rz(c) of angles in degrees
void delta_rot(double a, double b, double c, double R[3][3])
{
    const double ra = a * DEG, rb = b * DEG, rc = c * DEG;
    const double ca = std::cos(ra), sa = std::sin(ra), cb = std::cos(rb), sb = std::sin(rb), cc = std::cos(rc), sc = std::sin(rc);
    const double Rx[3][3] = {{1.0, 0.0, 0.0}, {0.0, ca, -sa}, {0.0, sa, ca}};
    const double Ry[3][3] = {{cb, 0.0, sb}, {0.0, 1.0, 0.0}, {-sb, 0.0, cb}};
    const double Rz[3][3] = {{cc, -sc, 0.0}, {sc, cc, 0.0}, {0.0, 0.0, 1.0}};
    double yx[3][3];
    mul3(Ry, Rx, yx);
    mul3(yx, Rz, R);
}

// base (a float pose widened) * [R | t], rounded to float once
void compose(const float *base16, const double R[3][3], const double t[3], float *out16)
{
    double a[16];
    for (int e = 0; e < 16; ++e) a[e] = (double)base16[e];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) out16[c * 4 + r] = (float)((a[r] * R[0][c] + a[4 + r] * R[1][c]) + a[8 + r] * R[2][c]);
    for (int r = 0; r < 3; ++r) out16[12 + r] = (float)(((a[r] * t[0] + a[4 + r] * t[1]) + a[8 + r] * t[2]) + a[12 + r]);
    out16[3] = 0.0f; out16[7] = 0.0f; out16[11] = 0.0f; out16[15] = 1.0f;
}

// the nested loops over (rot x, rot y, rot z, trans x, trans y, trans z), the last fastest: offsets (k + k0[a]) * step[a], k = 0..n[a]-1
void append_grid(const float *base16, const int n[6], const double k0[6], const double step[6], std::vector<float> &out)
{
    double o[6];
    int k[6];
    for (k[0] = 0; k[0] < n[0]; ++k[0])
        for (k[1] = 0; k[1] < n[1]; ++k[1])
            for (k[2] = 0; k[2] < n[2]; ++k[2]) {
                for (int a = 0; a < 3; ++a) o[a] = ((double)k[a] + k0[a]) * step[a];
                double R[3][3];
                delta_rot(o[0], o[1], o[2], R);
                for (k[3] = 0; k[3] < n[3]; ++k[3])
                    for (k[4] = 0; k[4] < n[4]; ++k[4])
                        for (k[5] = 0; k[5] < n[5]; ++k[5]) {
                            for (int a = 3; a < 6; ++a) o[a] = ((double)k[a] + k0[a]) * step[a];
                            out.resize(out.size() + 16);
                            compose(base16, R, o + 3, out.data() + out.size() - 16);
                        }
            }
}

// rank: score descending, then index ascending; kept only if score * stride^2 >= min_inliers; the first top_k kept
std::vector<uint32_t> rank_kept(const std::vector<uint32_t> &scores, int32_t stride, int32_t min_inliers, int32_t top_k)
{
    std::vector<uint32_t> idx;
    const uint64_t need = (uint64_t)std::max(min_inliers, 0), s2 = (uint64_t)stride * (uint64_t)stride;
    for (uint32_t i = 0; i < scores.size(); ++i)
        if ((uint64_t)scores[i] * s2 >= need) idx.push_back(i);
    const size_t k = std::min<size_t>(idx.size(), (size_t)top_k);
    std::partial_sort(idx.begin(), idx.begin() + k, idx.end(),
                      [&](uint32_t a, uint32_t b) { return scores[a] != scores[b] ? scores[a] > scores[b] : a < b; });
    idx.resize(k);
    return idx;
}
}  // namespace

int sm_impl::check_search_params(const sm_search_params &p, const char *who)
{
    const char *why = nullptr;
    if (p.levels < 1 || p.levels > 4) why = "levels outside 1..4";
    else if (p.refine < 1) why = "refine < 1";
    else if (p.top_k < 1 || p.top_k > 16) why = "top_k outside 1..16";
    else if (p.stride0 < 1) why = "stride0 < 1";
    else if (!(p.colour_thresh >= 0.0f) || !std::isfinite(p.colour_thresh)) why = "colour_thresh negative or not finite";
    for (int a = 0; a < 3 && !why; ++a) {
        const float v[4] = {p.trans_half[a], p.trans_step[a], p.rot_half_deg[a], p.rot_step_deg[a]};
        for (float x : v)
            if (!(x >= 0.0f) || !std::isfinite(x)) why = "a half or step is negative or not finite";
    }
    if (why) { g_err = std::string(who) + ": " + why; return SM_E_ARG; }
    // the sizes of the lists, before anything runs
    double n0 = 1.0, n1 = (double)p.top_k;
    for (int a = 0; a < 3; ++a) {
        const float half[2] = {p.rot_half_deg[a], p.trans_half[a]}, step[2] = {p.rot_step_deg[a], p.trans_step[a]};
        for (int k = 0; k < 2; ++k)
            if (half[k] > 0.0f && step[k] > 0.0f) {
                n0 *= 2.0 * std::floor((double)half[k] / (double)step[k]) + 1.0;
                n1 *= 2.0 * (double)p.refine + 1.0;
            }
    }
    if (n0 > (double)SM_SEARCH_MAX_CANDIDATES || (p.levels > 1 && n1 > (double)SM_SEARCH_MAX_CANDIDATES)) {
        g_err = std::string(who) + ": a level has more than 2^20 candidates";
        return SM_E_ARG;
    }
    return SM_OK;
}

extern "C" {

int sm_default_search_params(sm_search_params *p)
{
    if (!p) return SM_E_ARG;
    p->levels = 2;
    p->trans_half[0] = 2.0f; p->trans_half[1] = 0.0f; p->trans_half[2] = 2.0f;
    p->rot_half_deg[0] = 0.0f; p->rot_half_deg[1] = 3.0f; p->rot_half_deg[2] = 0.0f;
    for (int a = 0; a < 3; ++a) { p->trans_step[a] = 0.25f; p->rot_step_deg[a] = 0.5f; }
    p->refine = 4;
    p->stride0 = 8;
    p->top_k = 4;
    p->colour_thresh = 0.1f;
    return SM_OK;
}

int sm_score_poses_window(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *cand16, uint32_t n,
                          const sm_track_params *tp, int32_t stride, float colour_thresh, int32_t min_time, int32_t max_time,
                          uint32_t *scores)
{
    const char *fn = "sm_score_poses_window";
    if (!s || !depth_mm || !cand16 || !scores) { g_err = std::string(fn) + ": null argument"; return SM_E_ARG; }
    int rc;
    if ((rc = check_whole_map(s, fn)) || (rc = check_candidates(cand16, n, fn))) return rc;
    if (stride < 1) { g_err = std::string(fn) + ": stride < 1"; return SM_E_ARG; }
    if (!(colour_thresh >= 0.0f)) { g_err = std::string(fn) + ": colour_thresh negative or not a number"; return SM_E_ARG; }
    sm_track_params p;
    if (tp) p = *tp;
    else sm_default_track_params(&p);
    bool no_model;
    uint32_t in_view;
    float ms;
    return score(s, rgb, depth_mm, cand16, n, p, stride, colour_thresh, min_time, max_time, true, scores, &no_model, &in_view, &ms, fn);
}

// Diagnostic, deliberately not part of include/sm_c_api.h (tools/search_probe.py): how many grid points the last scored list packed
int sm_debug_search_samples(sm_ctx *s, uint32_t *n)
{
    if (!s || !n) return SM_E_ARG;
    *n = 0;
    if (!s->srch.d_nsamp) return SM_OK;
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipMemcpy(n, s->srch.d_nsamp, 4, hipMemcpyDeviceToHost));
    return SM_OK;
}

int sm_search_pose(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *centre16, const sm_track_params *tp,
                   const sm_track_rgb_params *rp, const sm_search_params *sp, int32_t min_time, int32_t max_time, float *pose16_out,
                   sm_search_info *info)
{
    return search_pose(s, rgb, depth_mm, nullptr, centre16, tp, rp, sp, min_time, max_time, pose16_out, info, "sm_search_pose");
}

}  // extern "C"

int sm_impl::search_pose(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pred16, const float *centre16,
                         const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_search_params *sp, int32_t min_time,
                         int32_t max_time, float *pose16_out, sm_search_info *info, const char *fn)
{
    const auto t_start = std::chrono::steady_clock::now();
    if (!s || !depth_mm || !centre16 || !pose16_out) { g_err = std::string(fn) + ": null argument"; return SM_E_ARG; }
    int rc;
    if ((rc = check_whole_map(s, fn)) || (rc = check_pose(centre16, fn))) return rc;
    sm_search_params q;
    if (sp) q = *sp;
    else sm_default_search_params(&q);
    if ((rc = check_search_params(q, fn))) return rc;
    sm_track_params p;
    if (tp) p = *tp;
    else sm_default_track_params(&p);

    sm_search_info inf;
    memset(&inf, 0, sizeof inf);
    inf.winner_rank = -1;
    inf.anchor_time = -1.0f;
    memcpy(inf.track.guess, centre16, 64);
    memcpy(inf.start, centre16, 64);
    memcpy(pose16_out, centre16, 64);
    auto finish = [&](int status) {
        inf.status = status;
        inf.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        if (info) *info = inf;
        return SM_OK;
    };

    // the axes: rot x, y, z, trans x, y, z
    int n0[6];
    double k0[6], step0[6];
    bool active[6];
    for (int a = 0; a < 6; ++a) {
        const double half = a < 3 ? (double)q.rot_half_deg[a] : (double)q.trans_half[a - 3];
        step0[a] = a < 3 ? (double)q.rot_step_deg[a] : (double)q.trans_step[a - 3];
        active[a] = half > 0.0 && step0[a] > 0.0;
        n0[a] = active[a] ? 2 * (int)std::floor(half / step0[a]) + 1 : 1;
        k0[a] = -(double)((n0[a] - 1) / 2);
    }
    std::vector<float> cand, kept_pose;
    append_grid(centre16, n0, k0, step0, cand);
    std::vector<uint32_t> scores, kept;
    double pw = 1.0;
    for (int l = 0; l < q.levels; ++l) {
        const uint32_t n = (uint32_t)(cand.size() / 16);
        const int32_t stride = std::max(1, q.stride0 >> l);
        scores.assign(n, 0u);
        bool no_model = false;
        uint32_t in_view = 0;
        float ms = 0.0f;
        if ((rc = score(s, rgb, depth_mm, cand.data(), n, p, stride, q.colour_thresh, min_time, max_time, l == 0, scores.data(), &no_model,
                        &in_view, &ms, fn, pred16)))
            return rc;
        if (no_model) return finish(SM_TRACK_NO_MODEL);
        inf.levels_run = l + 1;
        inf.candidates[l] = n;
        inf.best_score[l] = *std::max_element(scores.begin(), scores.end());
        inf.score_ms += ms;
        if (in_view == 0u) return finish(SM_TRACK_NO_MODEL);
        kept = rank_kept(scores, stride, p.min_inliers, q.top_k);
        if (kept.empty()) { inf.track.status = SM_TRACK_LOST; return finish(SM_TRACK_LOST); }
        kept_pose.clear();
        for (uint32_t i : kept) kept_pose.insert(kept_pose.end(), cand.begin() + (size_t)i * 16, cand.begin() + (size_t)i * 16 + 16);
        if (l + 1 == q.levels) break;
        // the next level: +-refine steps of step / refine^(l+1) around every kept candidate
        pw *= (double)q.refine;
        int n1[6];
        double k1[6], step1[6];
        for (int a = 0; a < 6; ++a) {
            n1[a] = active[a] ? 2 * q.refine + 1 : 1;
            k1[a] = active[a] ? -(double)q.refine : 0.0;
            step1[a] = step0[a] / pw;
        }
        cand.clear();
        for (size_t r = 0; r < kept.size(); ++r) append_grid(kept_pose.data() + r * 16, n1, k1, step1, cand);
    }

    // the refinement: every kept candidate of the last level through the tracker
    bool have_ok = false;
    const TrackWindow win{min_time, max_time};
    for (size_t r = 0; r < kept.size(); ++r) {
        const float *g = kept_pose.data() + r * 16;
        float out[16], anchor = -1.0f;
        sm_track_info ti;
        if ((rc = track_windowed(s, rgb, depth_mm, g, &p, rp, &win, out, &ti, nullptr, &anchor,
                                 rgb ? "sm_track_frame_rgb_window" : "sm_track_frame_window", pred16)))
            return rc;
        const bool ok = ti.status == SM_TRACK_OK;
        if ((r == 0 && !ok) || (ok && (!have_ok || ti.inliers > inf.track.inliers))) {
            inf.track = ti;
            memcpy(inf.start, g, 64);
            inf.anchor_time = anchor;
            if (ok) { inf.winner_rank = (int32_t)r; memcpy(pose16_out, out, 64); have_ok = true; }
        }
    }
    return finish(inf.track.status);
}
