// sm_recall.hip -- paging in (sm_recall, the periodic policy of sm_set_auto_recall; DESIGN.md "4g. Paging in"): the records of
// map files that lie near the camera come back into the model, streamed through the context's MapStaging (MapStream); the host half
// of a rewrite of listed files (index, opening, temporaries, replacement) is sm_map_set.h's.  Kernels: sm_k_recall.h.
//
// One pass over the files.  The near records of every chunk are appended speculatively into the free slots above `count`
// (never at or above MAX_VERTICES); the count is published only when every file has been read and every temporary of a MOVE is
// complete, so a call that fails -- a file that cannot be read, a temporary that cannot be written, SM_E_CAPACITY -- leaves the
// model as it was: slots above `count` are nobody's.
#include "sm_map_stream.h"
#include "sm_k_recall.h"

#include <cstdlib>

using namespace sm;
using sm_mapfile::now_ms;
using sm_mapset::MapFile;

namespace {

constexpr uint32_t CHUNK = MapStaging::CHUNK;
static_assert(CHUNK / RECALL_BLOCK == RECALL_MAX_BLOCKS, "a chunk's blocks are scanned by one workgroup");

// ---------------------------------------------------------------------------------------------
// The file index's test.  True = no row of the file can be near, the file need not be opened.  Conservative by construction:
//
// (1) With a finite r2 only a row whose three coordinates are finite can be near: a NaN makes d2 a NaN, an infinity makes it
//     +inf or a NaN, and neither is <= r2.  The box [lo, hi] bounds exactly the rows with finite coordinates (k_recall_mark); a
//     file without any has lo = +inf, hi = -inf.  (A radius whose square overflows has r2 = +inf: the test below is then
//     never true and no file is skipped.)
// (2) Per axis, g = max(lo - c, c - hi, 0) evaluated in fp32.  For a row with lo <= q <= hi: if g = fl(lo - c) > 0 then
//     q - c >= lo - c in the reals, and rounding to nearest is monotone, so the predicate's own dx = fl(q - c) >= g; if
//     g = fl(c - hi) > 0 then c - q >= c - hi, fl(c - q) >= g, and fl(q - c) = -fl(c - q) because rounding is symmetric: |dx| >= g
//     either way (and trivially for g = 0).  c is finite (a non-finite pose is refused), so no operand is a NaN.
// (3) The bound is then put together exactly as the predicate puts d2 together: lb = (gx*gx + gy*gy) + gz*gz in fp32, without
//     contraction (the build's -ffp-contract=off covers the host).  Every step -- a product of two equal-signed operands, a sum of
//     two non-negative ones -- is monotone in each operand in the reals and stays monotone after rounding to nearest, overflow
//     to +inf included.  So lb <= d2 as the kernel evaluates it, for every row of the box: the rounding of the fp32 evaluation
//     is charged by making the same roundings in the same order, and no slack term is needed.
// (4) near needs d2 <= r2, so lb > r2 (strict, false on a NaN) rules every row out.
// tests/test_recall.py restates this in numpy and checks it against the predicate on random boxes and on rows at and next to
// d2 == r2.
// ---------------------------------------------------------------------------------------------
float axis_gap(float lo, float hi, float c)
{
    const float a = lo - c, b = c - hi;
    const float g = a > b ? a : b;
    return g > 0.0f ? g : 0.0f;
}

bool box_out_of_reach(const sm_mapset::FileIndex::Entry &e, const float *c, float r2)
{
    const float gx = axis_gap(e.lo[0], e.hi[0], c[0]), gy = axis_gap(e.lo[1], e.hi[1], c[1]), gz = axis_gap(e.lo[2], e.hi[2], c[2]);
    const float lb = (gx * gx + gy * gy) + gz * gz;
    return lb > r2;
}

int ensure_scratch(sm_ctx *s)
{
    Recall &r = s->rec;
    if (r.h_chunk) return SM_OK;
    Dev<uint64_t> mask;
    Dev<uint32_t> cnt, base, run;
    Dev<RecallChunk> chunk;
    Dev<float4> box;
    int rc;
    if ((rc = dalloc(box, (size_t)RECALL_MAX_BLOCKS * 2)) || (rc = dalloc(mask, (size_t)RECALL_MAX_BLOCKS * 4)) || (rc = dalloc(cnt, RECALL_MAX_BLOCKS)) || (rc = dalloc(base, RECALL_MAX_BLOCKS)) ||
        (rc = dalloc(run, 1)) || (rc = dalloc(chunk, 2)))
        return rc;
    HIPCK(hipHostMalloc((void **)r.h_chunk.put(), 2 * sizeof(RecallChunk), hipHostMallocDefault));
    r.d_mask = std::move(mask); r.d_blk_cnt = std::move(cnt); r.d_blk_base = std::move(base); r.d_run = std::move(run);
    r.d_chunk = std::move(chunk); r.d_box = std::move(box);
    return SM_OK;
}

int check_args(sm_ctx *s, const sm_map_source *src, const float *pose16, const sm_recall_params *p, int32_t mode, const uint32_t *n,
               const char *who)
{
    if (!s || !src || !n) { g_err = std::string(who) + ": null context, source or count"; return SM_E_ARG; }
    if (int rc = check_whole_map(s, who)) return rc;
    if (src->include_model) { g_err = std::string(who) + ": include_model must be 0"; return SM_E_ARG; }
    if (int rc = check_map_source(src, who)) return rc;
    if (mode != SM_RECALL_MOVE && mode != SM_RECALL_COPY && mode != SM_RECALL_COUNT) { g_err = std::string(who) + ": unknown mode"; return SM_E_ARG; }
    if (p && !(std::isfinite(p->radius) && p->radius > 0.0f)) { g_err = std::string(who) + ": radius must be finite and > 0"; return SM_E_ARG; }
    if (int rc = check_pose(pose16, who)) return rc;
    if (int rc = check_not_mid_cull(s, who)) return rc;
    if (mode == SM_RECALL_MOVE && !sm_mapset::check_distinct_paths(src->paths, src->n_paths, who, g_err)) return SM_E_ARG;
    return SM_OK;
}

// known_far: index of a path whose file is known to hold no near row (the policy's own file of this round), or -1
int recall(sm_ctx *s, const sm_map_source *src, const float *pose16, const sm_recall_params *params, int32_t mode, uint32_t *n, const char *who,
           int64_t known_far = -1)
{
    const double t_begin = now_ms();
    int rc = check_args(s, src, pose16, params, mode, n, who);
    if (rc) return rc;
    sm_recall_params p;
    if (params) p = *params;
    else sm_default_recall_params(&s->cfg, &p);
    if (!(std::isfinite(p.radius) && p.radius > 0.0f)) { g_err = std::string(who) + ": radius must be finite and > 0"; return SM_E_ARG; }
    const float *pose = pose16 ? pose16 : s->last_pose;
    Recall &r = s->rec;
    RecallArgs ra;
    ra.cx = pose[12]; ra.cy = pose[13]; ra.cz = pose[14];
    ra.r2 = p.radius * p.radius;
    const float c3[3] = {ra.cx, ra.cy, ra.cz};

    // ---- every file is checked before anything changes; the index skips a file whose box no near row can lie in
    sm_mapset::RewriteSet set;
    std::vector<MapFile> &files = set.files;
    if (!sm_mapset::open_rewrite_set(src->paths, src->n_paths, CHUNK, s->index, known_far,
                                     [&](const sm_mapset::FileIndex::Entry &en) { return box_out_of_reach(en, c3, ra.r2); }, who, set, g_err,
                                     mode == SM_RECALL_MOVE ? sm_mapfile::PLAIN_ONLY : sm_mapfile::PACKED_OK))
        return set.packed_refused ? SM_E_UNSUPPORTED : SM_E_ARG;
    sm_recall_stats_t st{};
    st.files_listed = set.listed; st.files_skipped = set.skipped; st.files_read = set.read;

    HIPCK(hipSetDevice(s->cfg.device));
    // COUNT leaves the model alone altogether; the others append to the rows a download would return
    if (mode != SM_RECALL_COUNT && (rc = ensure_compact(s))) return rc;
    if ((rc = pull_state(s))) return rc;                 // (waits for frames in flight, flushes a held-back association)
    const uint32_t cnt = s->h_state->count;              // |m|: where the first recalled record goes
    uint64_t total = 0;                                  // |R| so far
    r.stats = st;
    r.stats_valid = true;
    if (!set.jobs.empty()) {
        if ((rc = maps_ensure_staging(s)) || (rc = ensure_scratch(s))) return rc;
        uint32_t largest = 0;
        for (const sm_mapfile::Job &j : set.jobs) largest = std::max(largest, j.n);
        if (mode == SM_RECALL_MOVE && (rc = ensure_export(s, ((size_t)CHUNK + largest) * sm_mapfile::RECORD_BYTES))) return rc;   // two chunks of rows that stay
        HIPCK(hipMemsetAsync(r.d_run, 0, 4, s->stream));
        MapStaging &sg = s->staging;
        const auto stay = [&](int q) { return (float4 *)s->d_export.get() + (size_t)q * CHUNK * 3; };
        // (gone before the renames: an open handle would keep a replaced file's pages alive.  If the call fails, the stream drains
        // what is in flight and the temporaries go with `files`.)
        MapStream in(s, who, src->paths, {&r.stats.read_ms, &r.stats.copy_ms, &r.stats.device_ms});
        // the next chunk of the stream: the kernels and the read-back of the chunk's tally, all asynchronous
        const auto enqueue = [&](MapStream::Chunk &ck) -> int {
            if (int e = in.next(ck)) return e;
            const int q = ck.q;
            const uint32_t n = ck.job->n;
            const unsigned nblk = (n + RECALL_BLOCK - 1) / RECALL_BLOCK;
            hipLaunchKernelGGL(k_recall_mark, dim3(nblk), dim3(256), 0, s->stream, ck.d_rec, n, ra, r.d_mask.get(), r.d_blk_cnt.get(), sg.d_box.get());
            hipLaunchKernelGGL(k_recall_scan, dim3(1), dim3(1024), 0, s->stream, nblk, (const uint32_t *)r.d_blk_cnt.get(), (const float4 *)sg.d_box.get(),
                               r.d_blk_base.get(), r.d_run.get(), r.d_chunk.get() + q);
            if (mode != SM_RECALL_COUNT)
                hipLaunchKernelGGL(k_recall_place, dim3(nblk), dim3(256), 0, s->stream, ck.d_rec, n, s->M, (const DevState *)s->d_state.get(),
                                   (const uint64_t *)r.d_mask.get(), (const uint32_t *)r.d_blk_cnt.get(), (const uint32_t *)r.d_blk_base.get(),
                                   (const RecallChunk *)(r.d_chunk.get() + q), cnt, s->cap, mode == SM_RECALL_MOVE ? stay(q) : nullptr);
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpyAsync(r.h_chunk.get() + q, r.d_chunk.get() + q, sizeof(RecallChunk), hipMemcpyDeviceToHost, s->stream));
            if (int e = in.done(q)) return e;
            r.stats.chunks++;
            r.stats.records_read += n;
            return SM_OK;
        };
        // the chunk is through the device: its tally, its box, and (MOVE) its rows that stay into the file's temporary
        const auto finish = [&](const MapStream::Chunk &ck) -> int {
            const int q = ck.q;
            if (int e = in.fold(q)) return e;
            const RecallChunk t = r.h_chunk.get()[q];
            MapFile &mf = files[ck.job->file];
            total += t.total;
            mf.fold(t.lx, t.ly, t.lz, t.hx, t.hy, t.hz, t.tmax);
            if (mode != SM_RECALL_MOVE) return SM_OK;
            const double t0 = now_ms();
            const uint32_t kept = ck.job->n - t.total;
            if (t.total && kept) {
                // (the copy stream is idle or copying the next chunk in; the kernels that wrote the rows that stay are over)
                HIPCK(hipMemcpyAsync(sg.h_rec[q], stay(q), (size_t)kept * sm_mapfile::RECORD_BYTES, hipMemcpyDeviceToHost, sg.copy));
                HIPCK(hipStreamSynchronize(sg.copy));
            }
            // (a chunk that lost nothing: as it was read)
            const bool ok = mf.keep(*ck.job, sg.h_rec[q].get(), kept, t.total != 0, ".recall.tmp", sm_mapfile::Writer::UNKNOWN, who, g_err);
            r.stats.write_ms += (float)(now_ms() - t0);
            return ok ? SM_OK : SM_E_ARG;
        };
        if ((rc = sm_mapset::stream_files(in, set.jobs, enqueue, finish))) return rc;
    }
    r.stats.recalled = total;
    *n = (uint32_t)std::min<uint64_t>(total, 0xFFFFFFFFull);
    // what this read has learnt goes into the index, whatever becomes of the call: the files are as they were
    // (a MOVE only takes rows away: the box stays a superset, tmax an upper bound)
    for (const MapFile &mf : files)
        if (!mf.skipped) mf.note_in(s->index);
    if (mode == SM_RECALL_COUNT) { r.stats.total_ms = (float)(now_ms() - t_begin); return SM_OK; }
    if ((uint64_t)cnt + total > s->cap) {
        g_err = std::string(who) + ": " + std::to_string(cnt) + " surfels + " + std::to_string(total) + " recalled exceed MAX_VERTICES";
        r.stats.total_ms = (float)(now_ms() - t_begin);
        return SM_E_CAPACITY;
    }

    // ---- publish: the state an upload of concat(m, R) leaves; only the tiles that hold a recalled row get new boxes
    if ((rc = publish_dense(s, cnt + (uint32_t)total, cnt))) return rc;   // (a device error: the context is lost anyway)

    // ---- the files, last: a failure from here on leaves rows twice, never nowhere
    const double t0 = now_ms();
    // (a file that could not be replaced: its temporary goes with `files`; the first one's text stays)
    r.stats.files_rewritten += sm_mapset::replace_files(files, s->index, false, [&](const MapFile &mf) {
        if (rc == SM_OK) g_err = std::string(who) + ": " + mf.path + " could not be replaced; its recalled rows are in the model AND still in the file";
        rc = SM_E_ARG;
    });
    r.stats.write_ms += (float)(now_ms() - t0);
    r.stats.total_ms = (float)(now_ms() - t_begin);
    return rc;
}

}  // namespace

int sm_impl::check_recall_policy(float radius, const sm_retire_params &rp, const char *who)
{
    if (rp.min_distance > 0.0f && radius <= rp.min_distance) return SM_OK;
    g_err = std::string(who) + ": the recall policy needs 0 < radius <= min_distance of the retirement policy (what a round retires it must not recall)";
    return SM_E_ARG;
}

int sm_impl::recall_box_of(sm_ctx *s, const float *d_rec12, uint32_t n, float lo[3], float hi[3], float *max_time)
{
    Recall &r = s->rec;
    if (!n) return SM_OK;
    const unsigned nblk = (n + RECALL_BLOCK - 1) / RECALL_BLOCK;         // n <= a chunk: the caller's staging holds no more
    const RecallArgs none{0.0f, 0.0f, 0.0f, -1.0f};                       // (no d2 is <= -1: the masks stay empty)
    hipLaunchKernelGGL(k_recall_mark, dim3(nblk), dim3(256), 0, s->stream, (const float4 *)d_rec12, n, none, r.d_mask.get(), r.d_blk_cnt.get(),
                       r.d_box.get());
    hipLaunchKernelGGL(k_recall_scan, dim3(1), dim3(1024), 0, s->stream, nblk, (const uint32_t *)r.d_blk_cnt.get(), (const float4 *)r.d_box.get(),
                       r.d_blk_base.get(), r.d_run.get(), r.d_chunk.get());
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(r.h_chunk.get(), r.d_chunk.get(), sizeof(RecallChunk), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    const RecallChunk ck = r.h_chunk.get()[0];
    lo[0] = std::min(lo[0], ck.lx); lo[1] = std::min(lo[1], ck.ly); lo[2] = std::min(lo[2], ck.lz);
    hi[0] = std::max(hi[0], ck.hx); hi[1] = std::max(hi[1], ck.hy); hi[2] = std::max(hi[2], ck.hz);
    *max_time = std::max(*max_time, ck.tmax);
    return SM_OK;
}

int sm_impl::recall_ensure_scratch(sm_ctx *s) { return ensure_scratch(s); }

// The periodic policy, called by auto_retire_after_frame once that frame's retirement is complete: a MOVE recall at the frame's
// pose from every file the retirement policy has written.  The file this round has written is listed and not read: each of its
// rows was retired because d2 > min_distance^2 at this very pose, and radius <= min_distance (check_recall_policy), so by the
// complement property none of them is near; its box is in the index already (auto_retire_after_frame).
int sm_impl::auto_recall_after_retire(sm_ctx *s, bool wrote_file)
{
    Recall &r = s->rec;
    if (!(r.radius > 0.0f) || s->ret.files == 0) return SM_OK;
    std::vector<std::string> paths(s->ret.files);
    std::vector<const char *> ptrs(s->ret.files);
    for (uint32_t i = 0; i < s->ret.files; ++i) {
        paths[i] = sm_mapfile::policy_file(s->ret.prefix, i);
        ptrs[i] = paths[i].c_str();
    }
    const sm_map_source src{ptrs.data(), s->ret.files, 0};
    const sm_recall_params p{r.radius};
    uint32_t n = 0;
    const int rc = recall(s, &src, nullptr, &p, SM_RECALL_MOVE, &n, "sm_set_auto_recall", wrote_file ? (int64_t)s->ret.files - 1 : -1);
    if (rc) return rc;
    r.rounds++;
    r.surfels += n;
    return SM_OK;
}

extern "C" {

int sm_default_recall_params(const sm_config *c, sm_recall_params *p)
{
    if (!c || !p) return SM_E_ARG;
    p->radius = 1.5f * c->far_clip;
    return SM_OK;
}

int sm_recall(sm_ctx *s, const sm_map_source *src, const float *pose16, const sm_recall_params *params, int32_t mode, uint32_t *n)
{
    return recall(s, src, pose16, params, mode, n, "sm_recall");
}

int sm_recall_stats(sm_ctx *s, sm_recall_stats_t *out)
{
    if (!s || !out) return SM_E_ARG;
    if (!s->rec.stats_valid) { g_err = "sm_recall_stats: no sm_recall call yet"; return SM_E_ARG; }
    *out = s->rec.stats;
    return SM_OK;
}

int sm_set_auto_recall(sm_ctx *s, const sm_recall_params *params)
{
    if (!s) return SM_E_ARG;
    if (int rc = check_whole_map(s, "sm_set_auto_recall")) return rc;
    if (!params || params->radius <= 0.0f) { s->rec.radius = 0.0f; return SM_OK; }
    if (!std::isfinite(params->radius)) { g_err = "sm_set_auto_recall: radius must be finite"; return SM_E_ARG; }
    if (s->ret.every > 0)
        if (int rc = check_recall_policy(params->radius, s->ret.params, "sm_set_auto_recall")) return rc;
    // so that the frame that recalls first allocates nothing: the staging of the stream, the scratch, two chunks of rows that stay
    HIPCK(hipSetDevice(s->cfg.device));
    int rc;
    if ((rc = maps_ensure_staging(s)) || (rc = ensure_scratch(s)) || (rc = ensure_export(s, (size_t)CHUNK * 2 * sm_mapfile::RECORD_BYTES))) return rc;
    s->rec.radius = params->radius;
    return SM_OK;
}

int sm_auto_recall_stats(sm_ctx *s, uint32_t *rounds, uint64_t *surfels)
{
    if (!s) return SM_E_ARG;
    if (rounds) *rounds = s->rec.rounds;
    if (surfels) *surfels = s->rec.surfels;
    return SM_OK;
}

}  // extern "C"
