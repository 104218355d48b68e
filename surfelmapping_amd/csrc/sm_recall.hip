// sm_recall.hip -- paging in (sm_recall, the periodic policy of sm_set_auto_recall; DESIGN.md "4g. Paging in"): the records of
// map files that lie near the camera come back into the model, streamed through the staging of sm_render_maps.hip.
// Kernels: sm_k_recall.h.
//
// One pass over the files.  The near records of every chunk are appended speculatively into the free slots above `count`
// (never at or above MAX_VERTICES); the count is published only when every file has been read and every temporary of a MOVE is
// complete, so a call that fails -- a file that cannot be read, a temporary that cannot be written, SM_E_CAPACITY -- leaves the
// model as it was: slots above `count` are nobody's.
#include "sm_ctx.h"
#include "sm_k_recall.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <sys/stat.h>

using namespace sm;

namespace {

constexpr uint32_t CHUNK = RenderMaps::CHUNK;
static_assert(CHUNK / RECALL_BLOCK == RECALL_MAX_BLOCKS, "a chunk's blocks are scanned by one workgroup");

struct FileCloser { void operator()(FILE *f) const { if (f) fclose(f); } };
using File = std::unique_ptr<FILE, FileCloser>;

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

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

bool box_out_of_reach(const Recall::Entry &e, const float *c, float r2)
{
    const float gx = axis_gap(e.lo[0], e.hi[0], c[0]), gy = axis_gap(e.lo[1], e.hi[1], c[1]), gz = axis_gap(e.lo[2], e.hi[2], c[2]);
    const float lb = (gx * gx + gy * gy) + gz * gz;
    return lb > r2;
}

// one listed file through the call
struct MapFile {
    std::string path;
    uint64_t size = 0;                 // from stat(), as the index keeps it
    int64_t mtime_ns = 0;
    bool skipped = false;              // by the index: not opened
    uint32_t n = 0;                    // records (header)
    int32_t start_id = 0, end_id = 0;
    float lo[3], hi[3];                // box of this read
    uint32_t chunks_left = 0;
    // MOVE: the temporary, opened by the first chunk that loses a row
    FILE *tmp = nullptr;
    std::string tmp_path;
    bool tmp_made = false, tmp_done = false;
    uint32_t kept = 0;
};

struct Job { uint32_t file, first, n; };

int64_t mtime_of(const struct stat &st) { return (int64_t)st.st_mtim.tv_sec * 1000000000ll + (int64_t)st.st_mtim.tv_nsec; }

int ensure_scratch(sm_ctx *s)
{
    Recall &r = s->rec;
    if (r.h_chunk) return SM_OK;
    Dev<uint64_t> mask;
    Dev<uint32_t> cnt, base, run;
    Dev<RecallChunk> chunk;
    int rc;
    if ((rc = dalloc(mask, (size_t)RECALL_MAX_BLOCKS * 4)) || (rc = dalloc(cnt, RECALL_MAX_BLOCKS)) || (rc = dalloc(base, RECALL_MAX_BLOCKS)) ||
        (rc = dalloc(run, 1)) || (rc = dalloc(chunk, 2)))
        return rc;
    HIPCK(hipHostMalloc((void **)r.h_chunk.put(), 2 * sizeof(RecallChunk), hipHostMallocDefault));
    r.d_mask = std::move(mask); r.d_blk_cnt = std::move(cnt); r.d_blk_base = std::move(base); r.d_run = std::move(run);
    r.d_chunk = std::move(chunk);
    return SM_OK;
}

// the temporary of a file that is about to lose its first row: header (completed at the end), then the rows of the chunks
// before `first`, which lost nothing, from the file itself
int open_tmp(MapFile &mf, uint32_t first, const char *who)
{
    mf.tmp_path = mf.path + ".recall.tmp";
    mf.tmp = fopen(mf.tmp_path.c_str(), "wb");
    if (!mf.tmp) { g_err = std::string(who) + ": " + mf.tmp_path + " is not open!"; return SM_E_ARG; }
    mf.tmp_made = true;
    const uint32_t hdr[3] = {0u, (uint32_t)mf.start_id, (uint32_t)mf.end_id};
    bool ok = fwrite(hdr, 4, 3, mf.tmp) == 3;
    if (ok && first) {
        File f(fopen(mf.path.c_str(), "rb"));
        ok = f && fseek(f.get(), 12, SEEK_SET) == 0;
        std::vector<char> buf((size_t)48 << 14);
        for (uint64_t left = (uint64_t)first; ok && left;) {
            const size_t m = (size_t)std::min<uint64_t>(left, (uint64_t)1 << 14);
            ok = fread(buf.data(), 48, m, f.get()) == m && fwrite(buf.data(), 48, m, mf.tmp) == m;
            left -= m;
        }
        mf.kept = first;
    }
    if (!ok) { g_err = std::string(who) + ": " + mf.tmp_path + " saved err!!"; return SM_E_ARG; }
    return SM_OK;
}

struct Run {
    sm_ctx *s;
    const char *who;
    int32_t mode;
    RecallArgs ra;
    uint32_t base0;                    // |m|: where the first recalled record goes
    std::vector<MapFile> &files;
    std::vector<Job> jobs;
    uint64_t total = 0;                // |R| so far
    File in;                           // the file being read
    uint32_t in_file = 0xFFFFFFFFu;
};

// chunk c: the host's read, the copy, the kernels and the read-back of the chunk's tally, all asynchronous but the read
int enqueue(Run &R, uint32_t c)
{
    sm_ctx *s = R.s;
    RenderMaps &rm = s->maps;
    Recall &r = s->rec;
    const Job &j = R.jobs[c];
    MapFile &mf = R.files[j.file];
    const int q = (int)(c & 1u);
    if (R.in_file != j.file) {
        R.in.reset(fopen(mf.path.c_str(), "rb"));
        R.in_file = j.file;
        if (!R.in || fseek(R.in.get(), 12, SEEK_SET) != 0) { g_err = std::string(R.who) + ": " + mf.path + " is not open!"; return SM_E_ARG; }
    }
    const double t0 = now_ms();
    const size_t got = fread(rm.h_rec[q].get(), 48, j.n, R.in.get());
    r.stats.read_ms += (float)(now_ms() - t0);
    if (got != j.n) { g_err = std::string(R.who) + ": " + mf.path + " read err!!"; return SM_E_ARG; }
    // (buffer q is free on both sides: chunk c - 2 was finished, which waits for its kernels)
    HIPCK(hipEventRecord(rm.ev_copy0[q], rm.copy));
    HIPCK(hipMemcpyAsync(rm.d_rec[q], rm.h_rec[q], (size_t)j.n * 48, hipMemcpyHostToDevice, rm.copy));
    HIPCK(hipEventRecord(rm.ev_copied[q], rm.copy));
    HIPCK(hipStreamWaitEvent(s->stream, rm.ev_copied[q], 0));
    HIPCK(hipEventRecord(rm.ev_k0[q], s->stream));
    const unsigned nblk = (j.n + RECALL_BLOCK - 1) / RECALL_BLOCK;
    const float4 *rec = (const float4 *)rm.d_rec[q].get();
    hipLaunchKernelGGL(k_recall_mark, dim3(nblk), dim3(256), 0, s->stream, rec, j.n, R.ra, r.d_mask.get(), r.d_blk_cnt.get(), rm.d_box.get());
    hipLaunchKernelGGL(k_recall_scan, dim3(1), dim3(1024), 0, s->stream, nblk, (const uint32_t *)r.d_blk_cnt.get(), (const float4 *)rm.d_box.get(),
                       r.d_blk_base.get(), r.d_run.get(), r.d_chunk.get() + q);
    if (R.mode != SM_RECALL_COUNT) {
        float4 *keep = R.mode == SM_RECALL_MOVE ? (float4 *)s->d_export.get() + (size_t)q * CHUNK * 3 : nullptr;
        hipLaunchKernelGGL(k_recall_place, dim3(nblk), dim3(256), 0, s->stream, rec, j.n, s->M, (const DevState *)s->d_state.get(),
                           (const uint64_t *)r.d_mask.get(), (const uint32_t *)r.d_blk_cnt.get(), (const uint32_t *)r.d_blk_base.get(),
                           (const RecallChunk *)(r.d_chunk.get() + q), R.base0, s->cap, keep);
    }
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(r.h_chunk.get() + q, r.d_chunk.get() + q, sizeof(RecallChunk), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipEventRecord(rm.ev_k1[q], s->stream));
    r.stats.chunks++;
    r.stats.records_read += j.n;
    return SM_OK;
}

// chunk c is through the device: its tally, its box, and (MOVE) its rows that stay into the file's temporary
int finish(Run &R, uint32_t c)
{
    sm_ctx *s = R.s;
    RenderMaps &rm = s->maps;
    Recall &r = s->rec;
    const Job &j = R.jobs[c];
    MapFile &mf = R.files[j.file];
    const int q = (int)(c & 1u);
    float ms = 0.0f;
    HIPCK(hipEventSynchronize(rm.ev_k1[q]));
    HIPCK(hipEventElapsedTime(&ms, rm.ev_copy0[q], rm.ev_copied[q]));
    r.stats.copy_ms += ms;
    HIPCK(hipEventElapsedTime(&ms, rm.ev_k0[q], rm.ev_k1[q]));
    r.stats.device_ms += ms;
    const RecallChunk ck = r.h_chunk.get()[q];
    R.total += ck.total;
    mf.lo[0] = std::min(mf.lo[0], ck.lx); mf.lo[1] = std::min(mf.lo[1], ck.ly); mf.lo[2] = std::min(mf.lo[2], ck.lz);
    mf.hi[0] = std::max(mf.hi[0], ck.hx); mf.hi[1] = std::max(mf.hi[1], ck.hy); mf.hi[2] = std::max(mf.hi[2], ck.hz);
    mf.chunks_left--;
    if (R.mode != SM_RECALL_MOVE) return SM_OK;
    const double t0 = now_ms();
    int rc = SM_OK;
    if (ck.total && !mf.tmp_made) rc = open_tmp(mf, j.first, R.who);
    if (!rc && mf.tmp) {
        const uint32_t kept = j.n - ck.total;
        if (ck.total && kept) {
            // (the copy stream is idle or copying the next chunk in; the kernels that wrote the staging are over)
            HIPCK(hipMemcpyAsync(rm.h_rec[q], (const float4 *)s->d_export.get() + (size_t)q * CHUNK * 3, (size_t)kept * 48, hipMemcpyDeviceToHost, rm.copy));
            HIPCK(hipStreamSynchronize(rm.copy));
        }
        bool ok = kept == 0 || fwrite(rm.h_rec[q].get(), 48, kept, mf.tmp) == kept;   // (a chunk that lost nothing: as it was read)
        mf.kept += kept;
        if (ok && mf.chunks_left == 0) {
            ok = fseek(mf.tmp, 0, SEEK_SET) == 0 && fwrite(&mf.kept, 4, 1, mf.tmp) == 1;
            ok = (fclose(mf.tmp) == 0) && ok;
            mf.tmp = nullptr;
            mf.tmp_done = ok;
        }
        if (!ok) { g_err = std::string(R.who) + ": " + mf.tmp_path + " saved err!!"; rc = SM_E_ARG; }
    }
    r.stats.write_ms += (float)(now_ms() - t0);
    return rc;
}

int stream_files(Run &R)
{
    int rc;
    const uint32_t nj = (uint32_t)R.jobs.size();
    for (uint32_t c = 0; c < nj; ++c) {
        if ((rc = enqueue(R, c))) return rc;             // the host reads chunk c while the device works on chunk c - 1
        if (c && (rc = finish(R, c - 1))) return rc;     // ... and writes what stays of chunk c - 1 while it works on chunk c
    }
    if (nj && (rc = finish(R, nj - 1))) return rc;
    return SM_OK;
}

void drop_temporaries(std::vector<MapFile> &files)
{
    for (MapFile &mf : files) {
        if (mf.tmp) { fclose(mf.tmp); mf.tmp = nullptr; }
        if (mf.tmp_made) { std::remove(mf.tmp_path.c_str()); mf.tmp_made = false; }
    }
}

int check_args(sm_ctx *s, const sm_map_source *src, const float *pose16, const sm_recall_params *p, int32_t mode, const uint32_t *n,
               const char *who)
{
    if (!s || !src || !n) { g_err = std::string(who) + ": null context, source or count"; return SM_E_ARG; }
    if (s->ss_on || s->rig_on) { g_err = std::string(who) + ": a sharded or rig context holds only its own surfels"; return SM_E_UNSUPPORTED; }
    if (src->include_model) { g_err = std::string(who) + ": include_model must be 0"; return SM_E_ARG; }
    if (src->n_paths && !src->paths) { g_err = std::string(who) + ": null paths"; return SM_E_ARG; }
    for (uint32_t i = 0; i < src->n_paths; ++i)
        if (!src->paths[i]) { g_err = std::string(who) + ": null path"; return SM_E_ARG; }
    if (mode != SM_RECALL_MOVE && mode != SM_RECALL_COPY && mode != SM_RECALL_COUNT) { g_err = std::string(who) + ": unknown mode"; return SM_E_ARG; }
    if (p && !(std::isfinite(p->radius) && p->radius > 0.0f)) { g_err = std::string(who) + ": radius must be finite and > 0"; return SM_E_ARG; }
    if (pose16)
        for (int i = 0; i < 16; ++i)
            if (!std::isfinite(pose16[i])) { g_err = std::string(who) + ": non-finite pose"; return SM_E_ARG; }
    if (s->pending_cull) { g_err = std::string(who) + " between sm_stage_conflict and sm_stage_cull"; return SM_E_ARG; }
    if (mode == SM_RECALL_MOVE)
        for (uint32_t i = 0; i < src->n_paths; ++i)
            for (uint32_t k = 0; k < i; ++k)
                if (strcmp(src->paths[i], src->paths[k]) == 0) { g_err = std::string(who) + ": " + src->paths[i] + " is listed twice"; return SM_E_ARG; }
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
    const char *e = std::getenv("SM_RECALL_NO_INDEX");
    const bool use_index = !(e && e[0] == '1');
    RecallArgs ra;
    ra.cx = pose[12]; ra.cy = pose[13]; ra.cz = pose[14];
    ra.r2 = p.radius * p.radius;
    const float c3[3] = {ra.cx, ra.cy, ra.cz};

    // ---- every file is checked before anything changes: skipped by the index on its stat() alone, or its header against its length
    sm_recall_stats_t st{};
    st.files_listed = src->n_paths;
    std::vector<MapFile> files(src->n_paths);
    Run R{s, who, mode, ra, 0u, files, {}, 0, nullptr, 0xFFFFFFFFu};
    const float INF = __builtin_inff();
    for (uint32_t i = 0; i < src->n_paths; ++i) {
        MapFile &mf = files[i];
        mf.path = src->paths[i];
        for (int a = 0; a < 3; ++a) { mf.lo[a] = INF; mf.hi[a] = -INF; }
        struct stat sb;
        if ((int64_t)i == known_far) { mf.skipped = true; st.files_skipped++; continue; }
        if (use_index && stat(mf.path.c_str(), &sb) == 0) {
            auto it = r.index.find(mf.path);
            if (it != r.index.end() && it->second.size == (uint64_t)sb.st_size && it->second.mtime_ns == mtime_of(sb) &&
                box_out_of_reach(it->second, c3, ra.r2)) {
                mf.skipped = true;
                st.files_skipped++;
                continue;
            }
        }
        File f(fopen(mf.path.c_str(), "rb"));
        if (!f) { g_err = std::string(who) + ": " + mf.path + " is not open!"; return SM_E_ARG; }
        uint32_t hdr[3];
        if (fread(hdr, 4, 3, f.get()) != 3 || fstat(fileno(f.get()), &sb) != 0) {
            g_err = std::string(who) + ": " + mf.path + " read err!! (no header)"; return SM_E_ARG;
        }
        const uint64_t want = 12ull + 48ull * hdr[0];
        if ((uint64_t)sb.st_size != want) {
            g_err = std::string(who) + ": " + mf.path + " holds " + std::to_string((uint64_t)sb.st_size) + " bytes, its header's " +
                    std::to_string(hdr[0]) + " records need " + std::to_string(want);
            return SM_E_ARG;
        }
        mf.size = (uint64_t)sb.st_size; mf.mtime_ns = mtime_of(sb);
        mf.n = hdr[0]; mf.start_id = (int32_t)hdr[1]; mf.end_id = (int32_t)hdr[2];
        st.files_read++;
        for (uint32_t first = 0; first < mf.n; first += CHUNK) {
            R.jobs.push_back({i, first, std::min(CHUNK, mf.n - first)});
            mf.chunks_left++;
        }
    }

    HIPCK(hipSetDevice(s->cfg.device));
    // COUNT leaves the model alone altogether; the others append to the rows a download would return
    if (mode != SM_RECALL_COUNT && (rc = ensure_compact(s))) return rc;
    if ((rc = pull_state(s))) return rc;                 // (waits for frames in flight, flushes a held-back association)
    const uint32_t cnt = s->h_state->count;
    R.base0 = cnt;
    r.stats = st;
    r.stats_valid = true;
    if (!R.jobs.empty()) {
        if ((rc = maps_ensure_staging(s)) || (rc = ensure_scratch(s))) return rc;
        uint32_t largest = 0;
        for (const Job &j : R.jobs) largest = std::max(largest, j.n);
        if (mode == SM_RECALL_MOVE && (rc = ensure_export(s, (size_t)CHUNK * 48 + (size_t)largest * 48))) return rc;   // two chunks of rows that stay
        HIPCK(hipMemsetAsync(r.d_run, 0, 4, s->stream));
        rc = stream_files(R);
        R.in.reset();                                    // (before the renames: an open handle would keep a replaced file's pages alive)
        if (rc) {
            (void)hipStreamSynchronize(s->maps.copy);
            (void)hipStreamSynchronize(s->stream);
            drop_temporaries(files);
            return rc;
        }
    }
    r.stats.recalled = R.total;
    *n = (uint32_t)std::min<uint64_t>(R.total, 0xFFFFFFFFull);
    // what this read has learnt goes into the index, whatever becomes of the call: the files are as they were
    auto note = [&](const MapFile &mf) {
        Recall::Entry en{mf.size, mf.mtime_ns, {mf.lo[0], mf.lo[1], mf.lo[2]}, {mf.hi[0], mf.hi[1], mf.hi[2]}};
        r.index[mf.path] = en;
    };
    for (const MapFile &mf : files)
        if (!mf.skipped) note(mf);
    if (mode == SM_RECALL_COUNT) { r.stats.total_ms = (float)(now_ms() - t_begin); return SM_OK; }
    if ((uint64_t)cnt + R.total > s->cap) {
        drop_temporaries(files);
        g_err = std::string(who) + ": " + std::to_string(cnt) + " surfels + " + std::to_string(R.total) + " recalled exceed MAX_VERTICES";
        r.stats.total_ms = (float)(now_ms() - t_begin);
        return SM_E_CAPACITY;
    }

    // ---- publish: the state an upload of concat(m, R) leaves, with retirement's exceptions (retire_commit)
    DevState &d = *s->h_state;
    d.count = cnt + (uint32_t)R.total;
    d.offset = d.count;
    d.garbage = 0; d.garbage_prev = 0; d.first_live = 0; d.do_compact = 0;
    s->culls_since_compact = 0;
    if ((rc = push_state(s)) == SM_OK && R.total) rc = rebuild_bounds(s, cnt, d.count);
    if (rc == SM_OK) rc = pull_state(s);
    if (rc) { drop_temporaries(files); return rc; }      // (a device error: the context is lost anyway)

    // ---- the files, last: a failure from here on leaves rows twice, never nowhere
    const double t0 = now_ms();
    for (MapFile &mf : files) {
        if (!mf.tmp_done) continue;
        if (std::rename(mf.tmp_path.c_str(), mf.path.c_str()) != 0) {
            if (rc == SM_OK) g_err = std::string(who) + ": " + mf.path + " could not be replaced; its recalled rows are in the model AND still in the file";
            rc = SM_E_ARG;
            continue;                                    // (drop_temporaries below removes its temporary)
        }
        mf.tmp_made = false;
        r.stats.files_rewritten++;
        struct stat sb;
        if (stat(mf.path.c_str(), &sb) == 0) { mf.size = (uint64_t)sb.st_size; mf.mtime_ns = mtime_of(sb); note(mf); }   // (the old box: a superset)
        else r.index.erase(mf.path);
    }
    drop_temporaries(files);
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

int sm_impl::recall_box_of(sm_ctx *s, const float *d_rec12, uint32_t n, float lo[3], float hi[3])
{
    Recall &r = s->rec;
    if (!n) return SM_OK;
    const unsigned nblk = (n + RECALL_BLOCK - 1) / RECALL_BLOCK;         // n <= a chunk: the caller's staging holds no more
    const RecallArgs none{0.0f, 0.0f, 0.0f, -1.0f};                       // (no d2 is <= -1: the masks stay empty)
    hipLaunchKernelGGL(k_recall_mark, dim3(nblk), dim3(256), 0, s->stream, (const float4 *)d_rec12, n, none, r.d_mask.get(), r.d_blk_cnt.get(),
                       s->maps.d_box.get());
    hipLaunchKernelGGL(k_recall_scan, dim3(1), dim3(1024), 0, s->stream, nblk, (const uint32_t *)r.d_blk_cnt.get(), (const float4 *)s->maps.d_box.get(),
                       r.d_blk_base.get(), r.d_run.get(), r.d_chunk.get());
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(r.h_chunk.get(), r.d_chunk.get(), sizeof(RecallChunk), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    const RecallChunk ck = r.h_chunk.get()[0];
    lo[0] = std::min(lo[0], ck.lx); lo[1] = std::min(lo[1], ck.ly); lo[2] = std::min(lo[2], ck.lz);
    hi[0] = std::max(hi[0], ck.hx); hi[1] = std::max(hi[1], ck.hy); hi[2] = std::max(hi[2], ck.hz);
    return SM_OK;
}

void sm_impl::recall_note_written(sm_ctx *s, const std::string &path, const float lo[3], const float hi[3])
{
    struct stat sb;
    if (stat(path.c_str(), &sb) != 0) { s->rec.index.erase(path); return; }
    s->rec.index[path] = Recall::Entry{(uint64_t)sb.st_size, mtime_of(sb), {lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}};
}

// The periodic policy, called by auto_retire_after_frame once that frame's retirement is complete: a MOVE recall at the frame's
// pose from every file the retirement policy has written.  The file this round has written is listed and not read: each of its
// rows was retired because d2 > min_distance^2 at this very pose, and radius <= min_distance (check_recall_policy), so by the
// complement property none of them is near; its box is in the index already (recall_note_written).
int sm_impl::auto_recall_after_retire(sm_ctx *s, bool wrote_file)
{
    Recall &r = s->rec;
    if (!(r.radius > 0.0f) || s->ret.files == 0) return SM_OK;
    std::vector<std::string> paths(s->ret.files);
    std::vector<const char *> ptrs(s->ret.files);
    for (uint32_t i = 0; i < s->ret.files; ++i) {
        char name[32];
        snprintf(name, sizeof name, "_%06u.bin", i);
        paths[i] = s->ret.prefix + name;
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
    if (s->ss_on || s->rig_on) { g_err = "sm_set_auto_recall: a sharded or rig context holds only its own surfels"; return SM_E_UNSUPPORTED; }
    if (!params || params->radius <= 0.0f) { s->rec.radius = 0.0f; return SM_OK; }
    if (!std::isfinite(params->radius)) { g_err = "sm_set_auto_recall: radius must be finite"; return SM_E_ARG; }
    if (s->ret.every > 0)
        if (int rc = check_recall_policy(params->radius, s->ret.params, "sm_set_auto_recall")) return rc;
    // so that the frame that recalls first allocates nothing: the staging of the stream, the scratch, two chunks of rows that stay
    HIPCK(hipSetDevice(s->cfg.device));
    int rc;
    if ((rc = maps_ensure_staging(s)) || (rc = ensure_scratch(s)) || (rc = ensure_export(s, (size_t)CHUNK * 96))) return rc;
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
