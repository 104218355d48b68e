// sm_warp.hip -- closing loops (DESIGN.md "4h. Closing loops"): sm_warp_by_time moves the live model and the records of map files
// by a table of world->world transforms indexed by each surfel's last-update time; sm_loop_spread makes the table of a loop
// closure.  Kernels: sm_k_warp.h.  The files stream through the context's MapStaging (MapStream), are warped IN its record
// buffers and copied back from them; the index, the opening, the temporaries and the replacement are sm_map_set.h's.
//
// Durability, in sm_recall MOVE's order: every file's new contents are complete in "<path>.warp.tmp" before the model is touched;
// then the model is warped; then each temporary is renamed over its file.  A temporary that cannot be written removes all
// temporaries and leaves everything as it was.  A rename that fails after the model was warped is reported (SM_E_ARG names the
// file), the other files are still renamed, and THAT FILE'S TEMPORARY IS LEFT IN PLACE: it holds the rows the model now agrees
// with, the file still holds the unwarped world, and an operator finishes the job with one mv "<path>.warp.tmp" "<path>".
#include "sm_map_stream.h"
#include "sm_k_warp.h"
#include "sm_pose.h"

#include <cstdlib>

using namespace sm;
using sm_mapfile::now_ms;
using sm_mapset::MapFile;

namespace {

constexpr uint32_t CHUNK = MapStaging::CHUNK;
static_assert(CHUNK / WARP_BLOCK == WARP_MAX_BLOCKS, "a chunk's blocks are folded by one workgroup");

int ensure_scratch(sm_ctx *s, uint32_t rows)
{
    Warp &w = s->warp;
    int rc;
    if (!w.h_chunk) {
        Dev<float4> box;
        Dev<uint32_t> sel;
        Dev<WarpChunk> chunk;
        Event e0, e1;
        if ((rc = dalloc(box, (size_t)WARP_MAX_BLOCKS * 2)) || (rc = dalloc(sel, 3)) || (rc = dalloc(chunk, 2))) return rc;
        HIPCK(hipEventCreate(e0.put()));
        HIPCK(hipEventCreate(e1.put()));
        HIPCK(hipHostMalloc((void **)w.h_chunk.put(), 2 * sizeof(WarpChunk), hipHostMallocDefault));
        w.d_box = std::move(box); w.d_sel = std::move(sel); w.d_chunk = std::move(chunk);
        w.ev[0] = std::move(e0); w.ev[1] = std::move(e1);
    }
    if (rows > w.corr_rows) {
        w.corr_rows = 0;
        if ((rc = dalloc(w.d_corr, (size_t)rows * 3))) return rc;
        w.corr_rows = rows;
    }
    return SM_OK;
}

// the row rule's selection on the host, for a stored pose of tick `tick`
bool select_row(int32_t tick, int32_t t0, uint32_t n, uint32_t &k)
{
    const float tau = (float)tick, t0f = (float)t0;
    if (!(tau >= t0f)) return false;
    const float d = tau - t0f;
    k = d >= (float)(n - 1u) ? n - 1u : (uint32_t)d;
    return true;
}

// P <- C * P for a camera->world pose (column-major) of a selected tick: in double from the widened floats, each element
// ((c0*p0 + c1*p1) + c2*p2) + c3*p3, rounded to float once; the last row of P stays
void warp_pose(float *P, int32_t tick, int32_t t0, uint32_t n, const float *corr12)
{
    uint32_t k;
    if (!select_row(tick, t0, n, k)) return;
    const float *C = corr12 + (size_t)k * 12;
    float out[16];
    memcpy(out, P, sizeof out);
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 3; ++i)
            out[i + 4 * j] = (float)((((double)C[4 * i] * (double)P[4 * j] + (double)C[4 * i + 1] * (double)P[4 * j + 1]) +
                                      (double)C[4 * i + 2] * (double)P[4 * j + 2]) + (double)C[4 * i + 3] * (double)P[4 * j + 3]);
    memcpy(P, out, sizeof out);
}

int warp_model(sm_ctx *s, const WarpArgs &wa, int32_t t0, uint32_t n, const float *corr12)
{
    Warp &w = s->warp;
    const uint32_t slots = s->h_state->count;            // occupied slots: live surfels and the dead ones among them
    HIPCK(hipMemsetAsync(w.d_sel.get() + 2, 0, 4, s->stream));
    HIPCK(hipEventRecord(w.ev[0], s->stream));
    if (slots) {
        const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)slots + 255) / 256, MAX_GRID);
        hipLaunchKernelGGL(k_warp_model, dim3(grid), dim3(256), 0, s->stream, s->M, (const DevState *)s->d_state.get(), (const uint64_t *)s->d_alive.get(), wa,
                           (const float4 *)w.d_corr.get(), w.d_sel.get() + 2);
        HIPCK(hipGetLastError());
    }
    HIPCK(hipEventRecord(w.ev[1], s->stream));
    uint32_t moved = 0;
    HIPCK(hipMemcpyAsync(&moved, w.d_sel.get() + 2, 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    float ms = 0.0f;
    HIPCK(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
    w.stats.device_ms += ms;
    w.stats.model_moved = moved;
    // the tile boxes of the whole model from the moved centres: the pass's tile skipping must not work with the old ones
    if (moved)
        if (int rc = rebuild_bounds(s, 0, slots)) return rc;
    // the stored poses move with the model: the last processed frame's (tick - 1) and the tracker's history
    if (s->ref_set && s->tick >= 1) {
        warp_pose(s->curr_pose, s->tick - 1, t0, n, corr12);
        warp_pose(s->last_pose, s->tick - 1, t0, n, corr12);
    }
    if (s->trk.n_hist >= 1) warp_pose(s->trk.hist[0], s->tick - 1, t0, n, corr12);
    if (s->trk.n_hist >= 2) warp_pose(s->trk.hist[1], s->tick - 2, t0, n, corr12);
    // ... and the keyframes of place recognition, each by its own time
    place_warp_poses(s, [&](float *P, int32_t time) { warp_pose(P, time, t0, n, corr12); });
    return SM_OK;
}

int check_args(sm_ctx *s, const sm_map_source *src, uint32_t n, const float *corr12, const char *who)
{
    if (!s || !src || !corr12) { g_err = std::string(who) + ": null context, source or table"; return SM_E_ARG; }
    if (int rc = check_whole_map(s, who)) return rc;
    if (n == 0) { g_err = std::string(who) + ": an empty table"; return SM_E_ARG; }
    for (size_t i = 0; i < (size_t)n * 12; ++i)
        if (!std::isfinite(corr12[i])) { g_err = std::string(who) + ": non-finite table entry"; return SM_E_ARG; }
    if (int rc = check_map_source(src, who)) return rc;
    if (int rc = check_not_mid_cull(s, who)) return rc;
    return sm_mapset::check_distinct_paths(src->paths, src->n_paths, who, g_err) ? SM_OK : SM_E_ARG;
}

int warp(sm_ctx *s, const sm_map_source *src, int32_t t0, uint32_t n, const float *corr12, const char *who)
{
    const double t_begin = now_ms();
    int rc = check_args(s, src, n, corr12, who);
    if (rc) return rc;
    Warp &w = s->warp;
    const WarpArgs wa{(float)t0, (float)(n - 1u), n};

    // ---- every file is checked before anything changes; the index skips a file none of whose rows is selected:
    // tau >= float(t0) fails for every non-NaN tau <= max_time, and for every NaN
    sm_mapset::RewriteSet set;
    std::vector<MapFile> &files = set.files;
    if (!sm_mapset::open_rewrite_set(src->paths, src->n_paths, CHUNK, s->index, -1,
                                     [&](const sm_mapset::FileIndex::Entry &en) { return en.max_time < wa.t0; }, who, set, g_err))
        return set.packed_refused ? SM_E_UNSUPPORTED : SM_E_ARG;
    sm_warp_stats_t st{};
    st.files_listed = set.listed; st.files_skipped = set.skipped; st.files_read = set.read;
    w.stats = st;
    w.stats_valid = true;
    if (set.jobs.empty() && !src->include_model) { w.stats.total_ms = (float)(now_ms() - t_begin); return SM_OK; }

    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = pull_state(s))) return rc;                 // (waits for frames in flight, flushes a held-back association)
    if ((rc = ensure_scratch(s, n))) return rc;
    HIPCK(hipMemcpyAsync(w.d_corr, corr12, (size_t)n * 48, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));              // (the caller's table is free again)
    if (!set.jobs.empty()) {
        if ((rc = maps_ensure_staging(s))) return rc;
        // (gone before the renames: an open handle would keep a replaced file's pages alive.  If the call fails, the stream drains
        // what is in flight and the temporaries go with `files`.)
        MapStream in(s, who, src->paths, {&w.stats.read_ms, &w.stats.copy_ms, &w.stats.device_ms});
        MapStaging &sg = s->staging;
        // the next chunk of the stream: its rows warped in the staging buffer, its tally on the way back, all asynchronous
        const auto enqueue = [&](MapStream::Chunk &ck) -> int {
            if (int e = in.next(ck)) return e;
            const int q = ck.q;
            const uint32_t m = ck.job->n;
            const unsigned nblk = (m + WARP_BLOCK - 1) / WARP_BLOCK;
            HIPCK(hipMemsetAsync(w.d_sel.get() + q, 0, 4, s->stream));
            hipLaunchKernelGGL(k_warp_rows, dim3(nblk), dim3(256), 0, s->stream, sg.d_rec[q].get(), m, wa, (const float4 *)w.d_corr.get(), w.d_box.get(),
                               w.d_sel.get() + q);
            hipLaunchKernelGGL(k_warp_fold, dim3(1), dim3(1024), 0, s->stream, nblk, (const float4 *)w.d_box.get(), (const uint32_t *)(w.d_sel.get() + q),
                               w.d_chunk.get() + q);
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpyAsync(w.h_chunk.get() + q, w.d_chunk.get() + q, sizeof(WarpChunk), hipMemcpyDeviceToHost, s->stream));
            if (int e = in.done(q)) return e;
            w.stats.chunks++;
            w.stats.records_read += m;
            return SM_OK;
        };
        // the chunk is through the device: its tally, and its rows into the file's temporary if the file has one by now
        const auto finish = [&](const MapStream::Chunk &ck) -> int {
            const int q = ck.q;
            if (int e = in.fold(q)) return e;                // (waits for the chunk's kernels and the copy of its tally)
            const WarpChunk wc = w.h_chunk.get()[q];
            MapFile &mf = files[ck.job->file];
            mf.fold(wc.lx, wc.ly, wc.lz, wc.hx, wc.hy, wc.hz, wc.tmax);
            w.stats.records_moved += wc.selected;
            const double t1 = now_ms();
            if (wc.selected) {
                // (the copy stream is idle or copying the next chunk into the other buffer; the kernels that wrote this one are over)
                HIPCK(hipMemcpyAsync(sg.h_rec[q], sg.d_rec[q], (size_t)ck.job->n * sm_mapfile::RECORD_BYTES, hipMemcpyDeviceToHost, sg.copy));
                HIPCK(hipStreamSynchronize(sg.copy));
            }
            // (a chunk without a selected row: as it was read)
            const bool ok = mf.keep(*ck.job, sg.h_rec[q].get(), ck.job->n, wc.selected != 0, ".warp.tmp", mf.h.count, who, g_err);
            w.stats.write_ms += (float)(now_ms() - t1);
            return ok ? SM_OK : SM_E_ARG;
        };
        if ((rc = sm_mapset::stream_files(in, set.jobs, enqueue, finish))) return rc;
    }

    // ---- all temporaries are complete: the model
    if (src->include_model && (rc = warp_model(s, wa, t0, n, corr12))) return rc;   // (a device error: the context is lost anyway)

    // ---- the files, last; what this read has learnt goes into the index
    const double t1 = now_ms();
    for (const MapFile &mf : files)
        if (!mf.skipped && !mf.tmp_done) mf.note_in(s->index);   // (read and left as it is)
    // (a file that could not be replaced: its temporary is left in place for the operator, and the index forgets the file)
    w.stats.files_rewritten += sm_mapset::replace_files(files, s->index, true, [&](const MapFile &mf) {
        if (rc == SM_OK)
            g_err = std::string(who) + ": " + mf.path + " could not be replaced; its warped rows are in " + mf.tmp.path() + " (rename it over the file)";
        rc = SM_E_ARG;
        s->index.erase(mf.path);
    });
    w.stats.write_ms += (float)(now_ms() - t1);
    w.stats.total_ms = (float)(now_ms() - t_begin);
    return rc;
}

// ---- sm_loop_spread: all in double
struct Rot { double m[3][3]; };

bool log_rotation(const Rot &R, double axis[3], double *angle)
{
    // within 1e-3 of orthonormal, proper
    double worst = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double g = (R.m[0][i] * R.m[0][j] + R.m[1][i] * R.m[1][j]) + R.m[2][i] * R.m[2][j];
            worst = std::max(worst, std::fabs(g - (i == j ? 1.0 : 0.0)));
        }
    const double det = (R.m[0][0] * (R.m[1][1] * R.m[2][2] - R.m[1][2] * R.m[2][1]) - R.m[0][1] * (R.m[1][0] * R.m[2][2] - R.m[1][2] * R.m[2][0])) +
                       R.m[0][2] * (R.m[1][0] * R.m[2][1] - R.m[1][1] * R.m[2][0]);
    if (!(worst <= 1e-3) || !(det > 0.0)) return false;
    const double v[3] = {R.m[2][1] - R.m[1][2], R.m[0][2] - R.m[2][0], R.m[1][0] - R.m[0][1]};   // 2 sin(angle) * axis
    const double nv = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double c = (((R.m[0][0] + R.m[1][1]) + R.m[2][2]) - 1.0) * 0.5;
    *angle = std::atan2(nv * 0.5, c);
    if (!(*angle <= 3.14159265358979323846 - 1e-3)) return false;
    if (nv > 0.0) { axis[0] = v[0] / nv; axis[1] = v[1] / nv; axis[2] = v[2] / nv; }
    else { axis[0] = axis[1] = axis[2] = 0.0; *angle = 0.0; }
    return true;
}

}  // namespace

extern "C" {

int sm_warp_by_time(sm_ctx *s, const sm_map_source *src, int32_t t0, uint32_t n, const float *corr12)
{
    return warp(s, src, t0, n, corr12, "sm_warp_by_time");
}

int sm_warp_stats(sm_ctx *s, sm_warp_stats_t *out)
{
    if (!s || !out) return SM_E_ARG;
    if (!s->warp.stats_valid) { g_err = "sm_warp_stats: no sm_warp_by_time call yet"; return SM_E_ARG; }
    *out = s->warp.stats;
    return SM_OK;
}

int sm_default_loop_params(const sm_config *c, sm_loop_params *p)
{
    if (!c || !p) return SM_E_ARG;
    p->min_age = c->time_delta;
    p->min_trans = 0.02f; p->min_rot_deg = 0.05f;
    p->max_trans = 2.0f; p->max_rot_deg = 10.0f;
    return SM_OK;
}

}  // extern "C"

int sm_impl::check_loop_params(const sm_loop_params &p, const char *who)
{
    const float bounds[4] = {p.min_trans, p.min_rot_deg, p.max_trans, p.max_rot_deg};
    for (float b : bounds)
        if (!(b >= 0.0f) || !std::isfinite(b)) { g_err = std::string(who) + ": a bound is negative or not finite"; return SM_E_ARG; }
    if (p.min_age < 1) { g_err = std::string(who) + ": min_age must be at least 1"; return SM_E_ARG; }
    return SM_OK;
}

int sm_impl::close_loop(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16, const sm_map_source *src,
                        const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_loop_params *lp, bool search,
                        const sm_search_params *sp, float *pose16_out, sm_loop_info *info, const char *who, const float *place16)
{
    if (!s || !depth_mm || !pose16 || !src || !pose16_out || !info) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    int rc;
    if ((rc = check_whole_map(s, who))) return rc;
    sm_loop_params p;
    if (lp) p = *lp;
    else sm_default_loop_params(&s->cfg, &p);
    if ((rc = check_loop_params(p, who)) || (rc = check_pose(pose16, who)) || (rc = check_map_source(src, who))) return rc;
    memset(info, 0, sizeof *info);
    sm_pose::identity(info->D);
    info->t_a = info->t_b = -1;
    memcpy(pose16_out, pose16, 64);
    const int64_t mt = (int64_t)s->tick - 1 - p.min_age;
    const int32_t max_time = (int32_t)std::max<int64_t>(mt, INT32_MIN);
    float t_old[16], anchor = -1.0f;
    if (search) {
        sm_search_info si;
        rc = search_pose(s, rgb, depth_mm, place16, place16 ? place16 : pose16, tp, rp, sp, INT32_MIN, max_time, t_old, &si,
                         place16 ? "sm_search_pose_at" : "sm_search_pose");
        if (rc) return rc;
        info->track = si.track;
        info->track.status = si.status;
        anchor = si.anchor_time;
    }
    else {
        const TrackWindow old{INT32_MIN, max_time};
        if ((rc = track_windowed(s, rgb, depth_mm, pose16, tp, rp, &old, t_old, &info->track, nullptr, &anchor,
                                 rgb ? "sm_track_frame_rgb_window" : "sm_track_frame_old")))
            return rc;
    }
    if (info->track.status == SM_TRACK_NO_MODEL) { info->status = SM_LOOP_NO_OLD_MAP; return SM_OK; }
    if (info->track.status != SM_TRACK_OK) { info->status = SM_LOOP_TRACK_FAILED; return SM_OK; }
    // D = T_old * pose16^-1, the inverse taken as a rigid pose's
    double pose[16], told[16], inv[16], D[16];
    sm_pose::widen(pose16, pose);
    sm_pose::widen(t_old, told);
    sm_pose::rigid_inv_d(pose, inv);
    sm_pose::mul_rigid_d(told, inv, D);
    for (int e = 0; e < 16; ++e) info->D[e] = (float)D[e];
    Rot R;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R.m[i][j] = (double)info->D[i + 4 * j];
    double axis[3], angle = 0.0;
    if (!log_rotation(R, axis, &angle)) { info->status = SM_LOOP_REJECTED; return SM_OK; }   // (no rotation a tracker step can be)
    const double dx = (double)t_old[12] - (double)pose16[12], dy = (double)t_old[13] - (double)pose16[13], dz = (double)t_old[14] - (double)pose16[14];
    const double trans = std::sqrt((dx * dx + dy * dy) + dz * dz), rot = angle * (180.0 / 3.14159265358979323846);
    if (trans < (double)p.min_trans && rot < (double)p.min_rot_deg) { info->status = SM_LOOP_NONE; return SM_OK; }
    if (trans > (double)p.max_trans || rot > (double)p.max_rot_deg) { info->status = SM_LOOP_REJECTED; return SM_OK; }
    const int32_t t_a = (int32_t)anchor, t_b = s->tick - 1;
    if (!(t_a < t_b)) { g_err = std::string(who) + ": the old map is not older than the last frame"; return SM_E_ARG; }
    const uint32_t n = (uint32_t)((int64_t)t_b - (int64_t)t_a) + 1u;
    std::vector<float> table((size_t)n * 12);
    if ((rc = sm_loop_spread(info->D, t_a, t_b, table.data()))) return rc;
    const sm_map_source all{src->paths, src->n_paths, 1};
    // Row 0, the identity, is not applied: the warp starts at t_a + 1 with the table from row 1 on.  The rows are the same for every
    // surfel newer than the anchor, and the old world keeps its BITS (1*x + 0*y + 0*z turns a -0.0 into +0.0, and fused normals hold many).
    if ((rc = warp(s, &all, t_a + 1, n - 1u, table.data() + 12, who))) return rc;
    // the corrected pose D * pose16, written out: it multiplies by the pose's own fourth row, which sm_pose.h's rigid product takes as (0, 0, 0, 1)
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r)
            pose16_out[c * 4 + r] = (float)((((double)info->D[r] * (double)pose16[c * 4] + (double)info->D[4 + r] * (double)pose16[c * 4 + 1]) +
                                             (double)info->D[8 + r] * (double)pose16[c * 4 + 2]) + (double)info->D[12 + r] * (double)pose16[c * 4 + 3]);
    info->status = SM_LOOP_CLOSED;
    info->t_a = t_a;
    info->t_b = t_b;
    return SM_OK;
}

extern "C" {

int sm_close_loop(sm_ctx *s, const uint16_t *depth_mm, const float *pose16, const sm_map_source *src, const sm_track_params *tp,
                  const sm_loop_params *lp, float *pose16_out, sm_loop_info *info)
{
    return close_loop(s, nullptr, depth_mm, pose16, src, tp, nullptr, lp, false, nullptr, pose16_out, info, "sm_close_loop");
}

int sm_close_loop_rgb(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16, const sm_map_source *src,
                      const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_loop_params *lp, float *pose16_out,
                      sm_loop_info *info)
{
    if (!rgb) { g_err = "sm_close_loop_rgb: null argument"; return SM_E_ARG; }
    return close_loop(s, rgb, depth_mm, pose16, src, tp, rp, lp, false, nullptr, pose16_out, info, "sm_close_loop_rgb");
}

int sm_close_loop_search(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16, const sm_map_source *src,
                         const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_loop_params *lp, const sm_search_params *sp,
                         float *pose16_out, sm_loop_info *info)
{
    return close_loop(s, rgb, depth_mm, pose16, src, tp, rp, lp, true, sp, pose16_out, info, "sm_close_loop_search");
}

int sm_loop_spread(const float *D16, int32_t t_a, int32_t t_b, float *corr12)
{
    const char *who = "sm_loop_spread";
    if (!D16 || !corr12) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if (t_b <= t_a) { g_err = std::string(who) + ": t_b must be above t_a"; return SM_E_ARG; }
    if (int rc = check_pose(D16, who)) return rc;
    Rot R;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R.m[i][j] = (double)D16[i + 4 * j];
    double a[3], angle;
    if (!log_rotation(R, a, &angle)) { g_err = std::string(who) + ": the rotation part is not orthonormal to 1e-3, or turns by more than pi - 1e-3"; return SM_E_ARG; }
    const double t[3] = {(double)D16[12], (double)D16[13], (double)D16[14]};
    const uint32_t span = (uint32_t)((int64_t)t_b - (int64_t)t_a);
    // K = the axis' cross-product matrix, K2 = K * K
    const double K[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
    double K2[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) K2[i][j] = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
    for (uint32_t k = 0; k <= span; ++k) {
        float *C = corr12 + (size_t)k * 12;
        if (k == span) {
            // fully due: D itself, as given (what exp(phi) equals up to the rounding of D's own entries)
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) C[4 * i + j] = D16[i + 4 * j];
            break;
        }
        if (k == 0) {                                    // not at all due: the identity, exactly
            for (int i = 0; i < 12; ++i) C[i] = (i % 5 == 0) ? 1.0f : 0.0f;
            continue;
        }
        const double wk = (double)k / (double)span, ak = wk * angle;
        const double sn = std::sin(ak), oc = 1.0 - std::cos(ak);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) C[4 * i + j] = (float)(((i == j ? 1.0 : 0.0) + sn * K[i][j]) + oc * K2[i][j]);
            C[4 * i + 3] = (float)(wk * t[i]);
        }
    }
    return SM_OK;
}

}  // extern "C"
