// sm_simplify.hip -- voxel-cell simplification (sm_simplify, sm_simplify_maps; DESIGN.md "4p. Simplification"): the records of
// the live model or of a map set merged per cell of a world grid, in two passes over the records.  A map set's files go through
// the context's chunk stream twice, the live model through the export scratch.  Kernels: sm_k_simplify.h.
#include "sm_map_stream.h"
#include "sm_k_simplify.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

constexpr uint32_t CHUNK = MapStaging::CHUNK;

int check_params(const sm_simplify_params *p, const char *who)
{
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (!p) return bad("null params");
    if (p->voxel_mm < 10 || p->voxel_mm > 10000) return bad("voxel_mm outside 10..10000");
    if (p->split_normals != 0 && p->split_normals != 1) return bad("split_normals is 0 or 1");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k])) return bad("non-finite origin");
    if (p->max_cells == 0) return bad("max_cells is 0");
    return SM_OK;
}

// One call's device side: the table, the kernel arguments, the launches of both passes on the context's stream.
struct SimplifyJob {
    sm_ctx *s;
    Simplify &sp;
    const char *who;
    SimplifyArgs a{};
    SimplifyTable T{};
    Dev<uint8_t> table;                // freed when the call ends: up to 136 bytes per record
    uint32_t launches = 0;

    SimplifyJob(sm_ctx *s_, const char *who_) : s(s_), sp(s_->simp), who(who_) {}

    // the scratch every call shares, the table for `records` records, everything initialised
    int open(uint64_t records, const sm_simplify_params &p)
    {
        int rc;
        if (!sp.d_code) {
            if ((rc = dalloc(sp.d_code, CHUNK)) || (rc = dalloc(sp.d_blk_cnt, CHUNK / 256)) || (rc = dalloc(sp.d_blk_base, CHUNK / 256)) ||
                (rc = dalloc(sp.d_tally, SIMP_TALLY_WORDS)) || (rc = dalloc(sp.d_info, 2)))
                return rc;
            HIPCK(hipHostMalloc((void **)sp.h_info.put(), 2 * sizeof(uint2), hipHostMallocDefault));
            HIPCK(hipEventCreate(sp.ev[0].put()));
            HIPCK(hipEventCreate(sp.ev[1].put()));
        }
        a.V = ((long long)p.voxel_mm * 65536 + 500) / 1000;
        for (int k = 0; k < 3; ++k) a.origin[k] = p.origin[k];
        a.split = p.split_normals;
        a.max_cells = p.max_cells;
        const char *e = std::getenv("SM_SIMPLIFY_NO_COMBINE");
        a.combine = (e && e[0] == '1') ? 0 : 1;
        uint64_t S = SIMP_MIN_SLOTS;
        while (S < 2 * std::min<uint64_t>(records, p.max_cells)) S <<= 1;
        if (S > (1ull << 31)) { g_err = std::string(who) + ": the table would need more than 2^31 slots"; return SM_E_CAPACITY; }
        HIPCK(hipMalloc((void **)table.put(), simplify_table_bytes((size_t)S)));
        uint8_t *b = table.get();
        auto take = [&](auto *&ptr, size_t planes, size_t width) { ptr = (std::remove_reference_t<decltype(ptr)>)b; b += planes * width * (size_t)S; };
        take(T.key, 1, 8); take(T.lo, 3, 4); take(T.init_min, 1, 4); take(T.first, 1, 4);
        uint8_t *zeros = b;
        take(T.SW, 1, 8); take(T.SP, 3, 8); take(T.SN, 3, 8); take(T.SC, 3, 8);
        take(T.n, 1, 4); take(T.hi, 3, 4); take(T.rmax, 1, 4); take(T.conf_max, 1, 4); take(T.time_max, 1, 4);
        T.mask = (uint32_t)(S - 1);
        T.tally = sp.d_tally;
        HIPCK(hipMemsetAsync(table.get(), 0xFF, (size_t)S * SIMP_ONES_BYTES, s->stream));
        HIPCK(hipMemsetAsync(zeros, 0, (size_t)S * SIMP_ZERO_BYTES, s->stream));
        HIPCK(hipMemsetAsync(sp.d_tally, 0, SIMP_TALLY_WORDS * 4, s->stream));
        return SM_OK;
    }
    // pass 1 of n <= CHUNK records
    void insert(const float4 *d_rec, uint32_t n, uint32_t gid0)
    {
        hipLaunchKernelGGL(k_simplify_insert, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, gid0, a, T);
        launches++;
        sp.stats.chunks++;
    }
    // pass 2 of n <= CHUNK records: the representatives at d_out + (rank - base) * 3, base = the first rank of this call (info non-null) or 0
    void emit(const float4 *d_rec, uint32_t n, uint32_t gid0, float4 *d_out, uint2 *d_info)
    {
        const unsigned nblk = (n + 255) / 256;
        hipLaunchKernelGGL(k_simplify_flag, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, gid0, a, T, sp.d_code.get(), sp.d_blk_cnt.get());
        hipLaunchKernelGGL(k_simplify_scan, dim3(1), dim3(1024), 0, s->stream, (const uint32_t *)sp.d_blk_cnt.get(), nblk, sp.d_blk_base.get(),
                           sp.d_tally.get(), d_info);
        hipLaunchKernelGGL(k_simplify_emit, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, a, T, (const uint32_t *)sp.d_code.get(),
                           (const uint32_t *)sp.d_blk_base.get(), (const uint2 *)d_info, d_out);
        launches += 3;
        sp.stats.chunks++;
    }
    // the tally, once the stream is idle; after pass 1 the sticky error word decides
    int tally(uint32_t out[SIMP_TALLY_WORDS])
    {
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(out, sp.d_tally, SIMP_TALLY_WORDS * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        if (out[SIMP_ERR] & 4u) { g_err = std::string(who) + ": internal: a key of pass 1 is missing in pass 2"; return SM_E_HIP; }
        if (out[SIMP_ERR]) {
            g_err = std::string(who) + ": more than max_cells = " + std::to_string(a.max_cells) + " distinct cells";
            return SM_E_CAPACITY;
        }
        return SM_OK;
    }
    // the time between ev[0] and ev[1] into the stats (the stream is idle)
    int mark(int i) { HIPCK(hipEventRecord(sp.ev[i], s->stream)); return SM_OK; }
    int add_marked()
    {
        float ms = 0.0f;
        HIPCK(hipEventSynchronize(sp.ev[1]));
        HIPCK(hipEventElapsedTime(&ms, sp.ev[0], sp.ev[1]));
        sp.stats.device_ms += ms;
        return SM_OK;
    }
    void fold_tally(const uint32_t t[SIMP_TALLY_WORDS])
    {
        sp.stats.cells_merged = t[SIMP_MERGED];
        sp.stats.loose = t[SIMP_N_LOOSE];
        sp.stats.largest_cell = std::max(t[SIMP_LARGEST], t[SIMP_CELLS] ? 1u : 0u);
        sp.stats.launches = launches;
    }
};

int ensure_out(Simplify &sp, int q, size_t records)
{
    if (records <= sp.out_cap[q]) return SM_OK;
    sp.out_cap[q] = 0;
    HIPCK(hipMalloc((void **)sp.d_out[q].put(), std::max<size_t>(records, 1) * 48));
    sp.out_cap[q] = records;
    return SM_OK;
}

}  // namespace

extern "C" {

int sm_default_simplify_params(sm_simplify_params *p)
{
    if (!p) { g_err = "sm_default_simplify_params: null argument"; return SM_E_ARG; }
    p->voxel_mm = 50;
    p->split_normals = 1;
    p->origin[0] = p->origin[1] = p->origin[2] = 0.0f;
    p->max_cells = 1u << 26;
    return SM_OK;
}

int sm_simplify(sm_ctx *s, const sm_simplify_params *p)
{
    const char *who = "sm_simplify";
    const double t_begin = now_ms();
    if (!s) { g_err = std::string(who) + ": null context"; return SM_E_ARG; }
    int rc;
    if ((rc = check_whole_map(s, who)) || (rc = check_params(p, who)) || (rc = check_not_mid_cull(s, who))) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = ensure_compact(s)) || (rc = pull_state(s))) return rc;      // (waits for frames in flight)
    const uint32_t cnt = s->h_state->count;
    Simplify &sp = s->simp;
    sp.stats = sm_simplify_stats_t{};
    sp.stats_valid = true;
    sp.stats.records_in = cnt;
    if (cnt == 0) { sp.stats.total_ms = (float)(now_ms() - t_begin); return SM_OK; }

    SimplifyJob job(s, who);
    if ((rc = ensure_export(s, (size_t)cnt * 48)) || (rc = ensure_out(sp, 0, cnt)) || (rc = job.open(cnt, *p))) return rc;
    const float4 *d_in = (const float4 *)s->d_export.get();
    export_aos(s, (float *)s->d_export.get(), 0u, cnt);
    if ((rc = job.mark(0))) return rc;
    for (uint32_t first = 0; first < cnt; first += CHUNK) job.insert(d_in + (size_t)first * 3, std::min(CHUNK, cnt - first), first);
    uint32_t t[SIMP_TALLY_WORDS];
    if ((rc = job.tally(t))) return rc;                  // (SM_E_CAPACITY: the model has only been read)
    for (uint32_t first = 0; first < cnt; first += CHUNK) {
        job.emit(d_in + (size_t)first * 3, std::min(CHUNK, cnt - first), first, sp.d_out[0], nullptr);
    }
    if ((rc = job.mark(1)) || (rc = job.tally(t)) || (rc = job.add_marked())) return rc;
    const uint32_t n_out = t[SIMP_RUN];
    job.fold_tally(t);
    sp.stats.records_out = n_out;

    // the model is the output's rows: what an upload of them leaves
    import_aos(s, (const float *)sp.d_out[0].get(), 0u, n_out);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(s->stream));
    if ((rc = publish_dense(s, n_out, 0))) return rc;
    if (sp.out_cap[0] > CHUNK) { sp.d_out[0] = Dev<float4>(); sp.out_cap[0] = 0; }      // (a model's worth of records: not kept)
    sp.stats.total_ms = (float)(now_ms() - t_begin);
    return SM_OK;
}

int sm_simplify_maps(sm_ctx *s, const sm_map_source *src, const sm_simplify_params *p, const char *out_path)
{
    const char *who = "sm_simplify_maps";
    const double t_begin = now_ms();
    if (!s || !src || !out_path) { g_err = std::string(who) + ": null context, source or output path"; return SM_E_ARG; }
    int rc;
    if ((rc = check_whole_map(s, who)) || (rc = check_params(p, who)) || (rc = check_map_source(src, who))) return rc;
    for (uint32_t i = 0; i < src->n_paths; ++i)
        if (strcmp(src->paths[i], out_path) == 0) { g_err = sm_mapfile::said(who, out_path, " is a source of the set: the output needs a path of its own"); return SM_E_ARG; }
    sm_mapset::ReadSet set;
    uint32_t cnt;
    if ((rc = maps_open(s, src, who, check_whole_map, set, cnt))) return rc;
    Simplify &sp = s->simp;
    sp.stats = sm_simplify_stats_t{};
    sp.stats_valid = true;
    const uint64_t total = set.file_total + cnt;
    sp.stats.records_in = total;
    int32_t start_id = 0, end_id = 0;                    // the header's frame range: the files' together
    for (size_t i = 0; i < set.files.size(); ++i) {
        start_id = i ? std::min(start_id, set.files[i].start_id) : set.files[i].start_id;
        end_id = i ? std::max(end_id, set.files[i].end_id) : set.files[i].end_id;
    }

    sm_mapfile::Writer w;                                // (a writer that goes away uncommitted removes its file)
    const std::string tmp = std::string(out_path) + ".simplify.tmp";
    if (total) {
        uint32_t largest_job = std::min(cnt, CHUNK);
        for (const sm_mapfile::Job &j : set.jobs) largest_job = std::max(largest_job, j.n);
        SimplifyJob job(s, who);
        if ((rc = maps_ensure_staging(s)) || (rc = ensure_out(sp, 0, largest_job)) || (rc = ensure_out(sp, 1, largest_job)) ||
            (rc = job.open(total, *p)))
            return rc;
        MapStaging &sg = s->staging;
        const float4 *d_model = nullptr;
        if (cnt) {
            if ((rc = ensure_export(s, (size_t)cnt * 48))) return rc;
            export_aos(s, (float *)s->d_export.get(), 0u, cnt);
            d_model = (const float4 *)s->d_export.get();
        }
        float copy_ms = 0.0f;
        MapStream in(s, who, src->paths, {&sp.stats.read_ms, &copy_ms, &sp.stats.device_ms});
        auto gid_of = [&](const sm_mapfile::Job &j) { return (uint32_t)(set.id_base[j.file] + j.first); };

        // ---- pass 1: the files, chunk by chunk, then the live model
        for (in.begin(set.jobs); in.more();) {
            MapStream::Chunk ck;
            if ((rc = in.next(ck))) return rc;
            job.insert(ck.d_rec, ck.job->n, gid_of(*ck.job));
            if ((rc = in.done(ck.q))) return rc;
            HIPCK(hipGetLastError());
        }
        if ((rc = in.fold(0)) || (rc = in.fold(1)) || (rc = job.mark(0))) return rc;
        for (uint32_t first = 0; first < cnt; first += CHUNK)
            job.insert(d_model + (size_t)first * 3, std::min(CHUNK, cnt - first), (uint32_t)set.file_total + first);
        uint32_t t[SIMP_TALLY_WORDS];
        if ((rc = job.mark(1)) || (rc = job.tally(t)) || (rc = job.add_marked())) return rc;   // (SM_E_CAPACITY: nothing is written)

        // ---- pass 2: the representatives of chunk c into the output while chunk c + 1 is on the device
        if (!w.open(tmp, sm_mapfile::Writer::UNKNOWN, start_id, end_id, who, g_err)) return SM_E_ARG;
        const auto enqueue = [&](MapStream::Chunk &ck) -> int {
            if (int e = in.next(ck)) return e;
            const int q = ck.q;
            job.emit(ck.d_rec, ck.job->n, gid_of(*ck.job), sp.d_out[q], sp.d_info.get() + q);
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpyAsync(sp.h_info.get() + q, sp.d_info.get() + q, sizeof(uint2), hipMemcpyDeviceToHost, s->stream));
            if (int e = in.done(q)) return e;
            return SM_OK;
        };
        const auto finish = [&](const MapStream::Chunk &ck) -> int {
            const int q = ck.q;
            if (int e = in.fold(q)) return e;            // (waits for the chunk's kernels and the copy of its count)
            const uint32_t m = sp.h_info.get()[q].y;
            if (m == 0) return SM_OK;
            // (the staging's host buffer q is free until the stream reads chunk c + 2 into it; the kernels that wrote d_out[q] are over)
            HIPCK(hipMemcpyAsync(sg.h_rec[q], sp.d_out[q], (size_t)m * 48, hipMemcpyDeviceToHost, sg.copy));
            HIPCK(hipStreamSynchronize(sg.copy));
            return w.append(sg.h_rec[q].get(), m, g_err) ? SM_OK : SM_E_ARG;
        };
        if ((rc = sm_mapset::stream_files(in, set.jobs, enqueue, finish))) return rc;
        for (uint32_t first = 0; first < cnt; first += CHUNK) {
            if ((rc = job.mark(0))) return rc;
            job.emit(d_model + (size_t)first * 3, std::min(CHUNK, cnt - first), (uint32_t)set.file_total + first, sp.d_out[0], sp.d_info.get());
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpyAsync(sp.h_info.get(), sp.d_info.get(), sizeof(uint2), hipMemcpyDeviceToHost, s->stream));
            if ((rc = job.mark(1)) || (rc = job.add_marked())) return rc;
            HIPCK(hipStreamSynchronize(s->stream));
            const uint32_t m = sp.h_info.get()[0].y;
            if (m == 0) continue;
            HIPCK(hipMemcpyAsync(sg.h_rec[0], sp.d_out[0], (size_t)m * 48, hipMemcpyDeviceToHost, s->stream));
            HIPCK(hipStreamSynchronize(s->stream));
            if (!w.append(sg.h_rec[0].get(), m, g_err)) return SM_E_ARG;
        }
        if ((rc = job.tally(t))) return rc;
        job.fold_tally(t);
        if (w.rows() != t[SIMP_RUN]) { g_err = std::string(who) + ": internal: rows written and ranks given differ"; return SM_E_HIP; }
    } else if (!w.open(tmp, sm_mapfile::Writer::UNKNOWN, start_id, end_id, who, g_err)) {
        return SM_E_ARG;
    }
    sp.stats.records_out = w.rows();
    if (!w.commit(g_err)) return SM_E_ARG;
    if (std::rename(tmp.c_str(), out_path) != 0) {
        std::remove(tmp.c_str());
        g_err = sm_mapfile::said(who, out_path, " saved err!!");
        return SM_E_ARG;
    }
    sp.stats.total_ms = (float)(now_ms() - t_begin);
    return SM_OK;
}

int sm_simplify_stats(sm_ctx *s, sm_simplify_stats_t *out)
{
    if (!s || !out) { g_err = "sm_simplify_stats: null argument"; return SM_E_ARG; }
    if (!s->simp.stats_valid) { g_err = "sm_simplify_stats: no sm_simplify / sm_simplify_maps call yet"; return SM_E_ARG; }
    *out = s->simp.stats;
    return SM_OK;
}

}  // extern "C"
