// sm_compare.hip -- change detection between two map sets (sm_compare_maps; DESIGN.md "4r. Change detection"): the reference set
// streamed once into a fine voxel table with one representative per key and a cover table of keys, then the query set streamed
// once, every record labelled against them and the records whose label is asked for written, in set order, to one map file.
// Kernels: sm_k_compare.h.
#include "sm_map_stream.h"
#include "sm_k_compare.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

constexpr uint32_t CHUNK = MapStaging::CHUNK;
constexpr size_t CMP_SUM_BYTES = 8 * 7;                  // per fine slot beside the key and the lookup record: SW, SP[3], SN[3]
enum { EV_CLR0 = 0, EV_CLR1, EV_REF0, EV_REF1, EV_QRY0, EV_QRY1 };     // pairs: add_marked(first)

int check_params(const sm_compare_params *p, bool writes, const char *who)
{
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (p->voxel_mm < 10 || p->voxel_mm > 10000) return bad("voxel_mm outside 10..10000");
    if (p->cover_shift < 1 || p->cover_shift > 6) return bad("cover_shift outside 1..6");
    if (!(p->reach_cells > 0.0f) || !std::isfinite(p->reach_cells)) return bad("reach_cells is not a positive number");
    if (p->plane_mm < 1 || p->plane_mm > 10000) return bad("plane_mm outside 1..10000");
    if (!(p->angle_thresh > 0.0f && p->angle_thresh < 90.0f)) return bad("angle_thresh outside (0, 90)");
    if (p->match_class != 0 && p->match_class != 1) return bad("match_class is 0 or 1");
    if (writes && (p->write_mask < 1 || p->write_mask > 15)) return bad("write_mask outside 1..15");
    if (p->max_cells == 0) return bad("max_cells is 0");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k])) return bad("non-finite origin");
    return SM_OK;
}

// what the call asks of its sets, without the device: the sources, no path in both, the output a path of its own, every header of both
int open_sets(const sm_map_source *query, const sm_map_source *reference, const char *out_path, const char *who, sm_mapset::ReadSet &qset,
              sm_mapset::ReadSet &rset)
{
    int rc;
    if ((rc = check_map_source(query, who)) || (rc = check_map_source(reference, who))) return rc;
    for (uint32_t i = 0; i < query->n_paths; ++i)
        for (uint32_t k = 0; k < reference->n_paths; ++k)
            if (strcmp(query->paths[i], reference->paths[k]) == 0) { g_err = sm_mapfile::said(who, query->paths[i], " is in both sets"); return SM_E_ARG; }
    for (const sm_map_source *src : {query, reference})
        for (uint32_t i = 0; out_path && i < src->n_paths; ++i)
            if (strcmp(src->paths[i], out_path) == 0) { g_err = sm_mapfile::said(who, out_path, " is a file of a set: the output needs a path of its own"); return SM_E_ARG; }
    if (!sm_mapset::open_read_set(query->paths, query->n_paths, CHUNK, who, qset, g_err)) return SM_E_ARG;
    if (!sm_mapset::open_read_set(reference->paths, reference->n_paths, CHUNK, who, rset, g_err)) return SM_E_ARG;
    return SM_OK;
}

int cmp_alloc(sm_ctx *s)
{
    Compare &cm = s->cmp;
    if (cm.d_tally) return SM_OK;
    Dev<uint8_t> label[2], keep;
    Dev<uint32_t> cnt, base, tally;
    Dev<uint2> info;
    int rc;
    if ((rc = dalloc(label[0], CHUNK)) || (rc = dalloc(label[1], CHUNK)) || (rc = dalloc(keep, CHUNK)) || (rc = dalloc(cnt, CHUNK / 256)) ||
        (rc = dalloc(base, CHUNK / 256)) || (rc = dalloc(info, 2)) || (rc = dalloc(tally, CMP_TALLY_WORDS)))
        return rc;
    HIPCK(hipHostMalloc((void **)cm.h_tally.put(), CMP_TALLY_WORDS * 4, hipHostMallocDefault));
    HIPCK(hipHostMalloc((void **)cm.h_info.put(), 2 * sizeof(uint2), hipHostMallocDefault));
    for (Host<uint8_t> &h : cm.h_label) HIPCK(hipHostMalloc((void **)h.put(), CHUNK, hipHostMallocDefault));
    for (Event &e : cm.ev) HIPCK(hipEventCreate(e.put()));
    cm.d_label[0] = std::move(label[0]); cm.d_label[1] = std::move(label[1]); cm.d_keep = std::move(keep);
    cm.d_blk_cnt = std::move(cnt); cm.d_blk_base = std::move(base); cm.d_info = std::move(info);
    cm.d_tally = std::move(tally);                       // last: it marks the set complete
    return SM_OK;
}

int ensure_out(Compare &cm, int q, size_t records)
{
    if (records <= cm.out_cap[q]) return SM_OK;
    cm.out_cap[q] = 0;
    HIPCK(hipMalloc((void **)cm.d_out[q].put(), std::max<size_t>(records, 1) * 48));
    cm.out_cap[q] = records;
    return SM_OK;
}

// One call's device side: both tables, the kernel arguments, the launches on the context's stream.
struct CompareJob {
    sm_ctx *s;
    Compare &cm;
    const char *who;
    const sm_compare_params &p;
    SimplifyArgs aF{}, aC{};
    SimplifyTable TF{}, TC{};
    RegCell *lut = nullptr;
    CmpParams cp{};
    Dev<uint8_t> tables;               // freed when the call ends: 104 bytes per slot
    bool writes = false;
    uint32_t launches = 0;

    CompareJob(sm_ctx *s_, const char *who_, const sm_compare_params &p_) : s(s_), cm(s_->cmp), who(who_), p(p_) {}

    int open(uint64_t reference_records, const float *pose16, bool writes_)
    {
        writes = writes_;
        int rc;
        if ((rc = cmp_alloc(s))) return rc;
        uint64_t S = SIMP_MIN_SLOTS;
        while (S < 2 * std::min<uint64_t>(reference_records, p.max_cells)) S <<= 1;
        if (S > (1ull << 31)) { g_err = std::string(who) + ": a table would need more than 2^31 slots"; return SM_E_CAPACITY; }
        HIPCK(hipMalloc((void **)tables.put(), (size_t)S * (sizeof(RegCell) + 8 + CMP_SUM_BYTES + 8)));
        uint8_t *b = tables.get();
        lut = (RegCell *)b;                              // (first: 32-byte aligned)
        b += (size_t)S * sizeof(RegCell);
        TF.key = (unsigned long long *)b;
        TF.SW = TF.key + S; TF.SP = TF.SW + S; TF.SN = TF.SP + 3 * S;
        TC.key = TF.SN + 3 * S;
        TF.mask = TC.mask = (uint32_t)(S - 1);
        TF.tally = cm.d_tally.get() + CMP_FINE;
        TC.tally = cm.d_tally.get() + CMP_COVER;
        const char *e = std::getenv("SM_SIMPLIFY_NO_COMBINE");
        aF.V = ((long long)p.voxel_mm * 65536 + 500) / 1000;
        aC.V = (((long long)p.voxel_mm << p.cover_shift) * 65536 + 500) / 1000;
        for (int k = 0; k < 3; ++k) aF.origin[k] = aC.origin[k] = p.origin[k];
        aF.split = 1;
        aC.split = 0;
        aF.max_cells = aC.max_cells = p.max_cells;
        aF.combine = aC.combine = (e && e[0] == '1') ? 0 : 1;
        if ((rc = mark(EV_CLR0))) return rc;             // the tables' initialisation is device time of theirs (table_ms)
        HIPCK(hipMemsetAsync(TF.key, 0xFF, (size_t)S * 8, s->stream));
        HIPCK(hipMemsetAsync(TF.SW, 0, (size_t)S * CMP_SUM_BYTES, s->stream));
        HIPCK(hipMemsetAsync(TC.key, 0xFF, (size_t)S * 8, s->stream));
        HIPCK(hipMemsetAsync(cm.d_tally, 0, CMP_TALLY_WORDS * 4, s->stream));
        if ((rc = mark(EV_CLR1))) return rc;

        cp.lut = lut;
        cp.cover = TC.key;
        cp.mask = TF.mask; cp.cmask = TC.mask;
        cp.V0 = aF.V; cp.V1 = aC.V;
        for (int k = 0; k < 3; ++k) cp.origin[k] = p.origin[k];
        cp.match_class = p.match_class;
        cp.write_mask = writes ? p.write_mask : 0u;
        for (int e16 = 0; e16 < 16; ++e16) cp.T[e16] = pose16 ? (double)pose16[e16] : (e16 % 5 == 0 ? 1.0 : 0.0);
        cp.reach = (double)p.reach_cells * ((double)aF.V * (1.0 / 65536.0));
        cp.cos_angle = std::cos((double)p.angle_thresh * (3.14159265358979323846 / 180.0));
        cp.plane = (double)p.plane_mm / 1000.0;
        return SM_OK;
    }
    // n <= CHUNK records of the reference into both tables
    void insert(const float4 *d_rec, uint32_t n)
    {
        hipLaunchKernelGGL(k_compare_insert, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, aF, TF, p.match_class, aC, TC);
        launches++;
        cm.stats.chunks++;
    }
    void finish()
    {
        hipLaunchKernelGGL(k_compare_finish, dim3(TF.mask / 256u + 1u), dim3(256), 0, s->stream, aF, TF, lut);
        launches++;
    }
    // n <= CHUNK records of the query: labels into d_label[q], and with an output the kept ones at d_out[q] + (rank - the chunk's first rank) * 3
    void classify(const float4 *d_rec, uint32_t n, int q)
    {
        const unsigned nblk = (n + 255) / 256;
        hipLaunchKernelGGL(k_compare_classify, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, cp, cm.d_label[q].get(), cm.d_keep.get(),
                           cm.d_blk_cnt.get(), cm.d_tally.get());
        launches++;
        if (writes) {
            hipLaunchKernelGGL(k_compare_scan, dim3(1), dim3(1024), 0, s->stream, (const uint32_t *)cm.d_blk_cnt.get(), nblk, cm.d_blk_base.get(),
                               cm.d_tally.get() + CMP_FINE, cm.d_info.get() + q);
            hipLaunchKernelGGL(k_compare_emit, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, (const uint8_t *)cm.d_keep.get(),
                               (const uint32_t *)cm.d_blk_base.get(), (const uint2 *)(cm.d_info.get() + q), cm.d_out[q].get());
            launches += 2;
        }
        cm.stats.chunks++;
    }
    // the tally, once the stream is idle
    int tally()
    {
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(cm.h_tally.get(), cm.d_tally.get(), CMP_TALLY_WORDS * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        return SM_OK;
    }
    int mark(int i) { HIPCK(hipEventRecord(cm.ev[i], s->stream)); return SM_OK; }
    int add_marked(int i, float *ms_sum)                 // (the stream is idle)
    {
        float ms = 0.0f;
        HIPCK(hipEventElapsedTime(&ms, cm.ev[i], cm.ev[i + 1]));
        *ms_sum += ms;
        return SM_OK;
    }
};

}  // namespace

extern "C" {

int sm_default_compare_params(sm_compare_params *p)
{
    if (!p) { g_err = "sm_default_compare_params: null argument"; return SM_E_ARG; }
    *p = sm_compare_params{};
    p->voxel_mm = 100;
    p->cover_shift = 3;
    p->reach_cells = 2.0f;
    p->plane_mm = 50;
    p->angle_thresh = 30.0f;
    p->match_class = 0;
    p->write_mask = 1u << SM_COMPARE_CHANGED;
    p->max_cells = 1u << 24;
    return SM_OK;
}

int sm_compare_maps(sm_ctx *s, const sm_map_source *query, const sm_map_source *reference, const float *pose16, const sm_compare_params *p,
                    uint8_t *labels, const char *out_path, sm_compare_info *info)
{
    const char *who = "sm_compare_maps";
    const double t_begin = now_ms();
    if (!s || !query || !reference || !p || !info) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    const bool writes = out_path != nullptr;
    int rc;
    if ((rc = check_whole_map(s, who)) || (rc = check_params(p, writes, who)) || (rc = check_not_mid_cull(s, who)) || (rc = check_pose(pose16, who)))
        return rc;
    sm_mapset::ReadSet qset, rset;
    if ((rc = open_sets(query, reference, out_path, who, qset, rset))) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = ensure_compact(s)) || (rc = pull_state(s))) return rc;      // (waits for frames in flight; count is the live surfels)
    const uint32_t model = s->h_state->count, qcnt = query->include_model ? model : 0u, rcnt = reference->include_model ? model : 0u;
    const uint64_t qtotal = qset.file_total + qcnt, rtotal = rset.file_total + rcnt;
    if (qtotal > 0x7FFFFFFFull || rtotal > 0x7FFFFFFFull) { g_err = std::string(who) + ": a set of more than 2^31 - 1 records"; return SM_E_CAPACITY; }

    Compare &cm = s->cmp;
    cm.stats = sm_compare_stats_t{};
    cm.stats_valid = true;
    sm_compare_info out{};
    out.query_records = qtotal;
    out.reference_records = rtotal;
    int32_t start_id = 0, end_id = 0;                    // the output header's frame range: the query files' together
    for (size_t i = 0; i < qset.files.size(); ++i) {
        start_id = i ? std::min(start_id, qset.files[i].start_id) : qset.files[i].start_id;
        end_id = i ? std::max(end_id, qset.files[i].end_id) : qset.files[i].end_id;
    }

    CompareJob job(s, who, *p);
    if ((rc = job.open(rtotal, pose16, writes))) return rc;
    if (writes) {
        uint32_t largest_job = std::min(qcnt, CHUNK);
        for (const sm_mapfile::Job &j : qset.jobs) largest_job = std::max(largest_job, j.n);
        if ((rc = ensure_out(cm, 0, largest_job)) || (rc = ensure_out(cm, 1, largest_job))) return rc;
    }
    const float4 *d_model = nullptr;
    if (qcnt || rcnt) {
        if ((rc = ensure_export(s, (size_t)model * 48))) return rc;
        export_aos(s, (float *)s->d_export.get(), 0u, model);
        d_model = (const float4 *)s->d_export.get();
    }
    if (qset.jobs.size() + rset.jobs.size() || (qcnt && writes))       // (the live model's kept records leave through its host buffer too)
        if ((rc = maps_ensure_staging(s))) return rc;
    MapStaging &sg = s->staging;
    float copy_ms = 0.0f;

    // ---- the reference: every chunk into both tables, then the representatives
    {
        MapStream in(s, who, reference->paths, {&cm.stats.read_ms, &copy_ms, &cm.stats.table_ms});
        for (in.begin(rset.jobs); in.more();) {
            MapStream::Chunk ck;
            if ((rc = in.next(ck))) return rc;
            job.insert(ck.d_rec, ck.job->n);
            if ((rc = in.done(ck.q))) return rc;
            HIPCK(hipGetLastError());
        }
        if ((rc = in.fold(0)) || (rc = in.fold(1))) return rc;
    }
    if ((rc = job.mark(EV_REF0))) return rc;
    for (uint32_t first = 0; first < rcnt; first += CHUNK) job.insert(d_model + (size_t)first * 3, std::min(CHUNK, rcnt - first));
    job.finish();
    if ((rc = job.mark(EV_REF1)) || (rc = job.tally())) return rc;
    if ((rc = job.add_marked(EV_CLR0, &cm.stats.table_ms)) || (rc = job.add_marked(EV_REF0, &cm.stats.table_ms))) return rc;
    const uint32_t *h = cm.h_tally.get();
    for (int t = 0; t < 2; ++t)
        if (h[(t ? CMP_COVER : CMP_FINE) + SIMP_ERR]) {  // (nothing has been written: the labels and the output follow)
            g_err = std::string(who) + ": more than max_cells = " + std::to_string(p->max_cells) + " keys in the " + (t ? "cover" : "fine") + " table";
            return SM_E_CAPACITY;
        }
    out.cells_fine = h[CMP_FINE + SIMP_CELLS];
    out.cells_cover = h[CMP_COVER + SIMP_CELLS];

    // ---- the query: the labels of chunk c, and what is kept of it, come back while chunk c + 1 is on the device
    sm_mapfile::Writer w;                                // (a writer that goes away uncommitted removes its file)
    const std::string tmp = writes ? std::string(out_path) + ".compare.tmp" : std::string();
    if (writes && !w.open(tmp, sm_mapfile::Writer::UNKNOWN, start_id, end_id, who, g_err)) return SM_E_ARG;
    // the chunk of n records in buffer q, ids gid0 ..: its kernels are over; on `stream`: the kept records through the staging's host
    // buffer q (free until chunk c + 2 is read into it), the labels through the pinned buffer q of this call's own
    const auto collect = [&](int q, uint32_t n, uint64_t gid0, hipStream_t stream) -> int {
        const double t0 = now_ms();
        const uint32_t m = writes ? cm.h_info.get()[q].y : 0u;
        if (m) HIPCK(hipMemcpyAsync(sg.h_rec[q], cm.d_out[q], (size_t)m * 48, hipMemcpyDeviceToHost, stream));
        if (labels) HIPCK(hipMemcpyAsync(cm.h_label[q], cm.d_label[q], n, hipMemcpyDeviceToHost, stream));
        if (m || labels) HIPCK(hipStreamSynchronize(stream));
        if (labels) memcpy(labels + gid0, cm.h_label[q].get(), n);
        const bool ok = !m || w.append(sg.h_rec[q].get(), m, g_err);
        cm.stats.write_ms += (float)(now_ms() - t0);
        return ok ? SM_OK : SM_E_ARG;
    };
    {
        MapStream in(s, who, query->paths, {&cm.stats.read_ms, &copy_ms, &cm.stats.classify_ms});
        const auto enqueue = [&](MapStream::Chunk &ck) -> int {
            if (int e = in.next(ck)) return e;
            const int q = ck.q;
            job.classify(ck.d_rec, ck.job->n, q);
            HIPCK(hipGetLastError());
            if (writes) HIPCK(hipMemcpyAsync(cm.h_info.get() + q, cm.d_info.get() + q, sizeof(uint2), hipMemcpyDeviceToHost, s->stream));
            return in.done(q);
        };
        const auto finish = [&](const MapStream::Chunk &ck) -> int {
            if (int e = in.fold(ck.q)) return e;         // (waits for the chunk's kernels and the copy of its count)
            return collect(ck.q, ck.job->n, qset.id_base[ck.job->file] + ck.job->first, sg.copy);
        };
        if ((rc = sm_mapset::stream_files(in, qset.jobs, enqueue, finish))) return rc;
    }
    for (uint32_t first = 0; first < qcnt; first += CHUNK) {
        const uint32_t n = std::min(CHUNK, qcnt - first);
        if ((rc = job.mark(EV_QRY0))) return rc;
        job.classify(d_model + (size_t)first * 3, n, 0);
        HIPCK(hipGetLastError());
        if (writes) HIPCK(hipMemcpyAsync(cm.h_info.get(), cm.d_info.get(), sizeof(uint2), hipMemcpyDeviceToHost, s->stream));
        if ((rc = job.mark(EV_QRY1))) return rc;
        HIPCK(hipStreamSynchronize(s->stream));
        if ((rc = job.add_marked(EV_QRY0, &cm.stats.classify_ms)) || (rc = collect(0, n, qset.file_total + first, s->stream))) return rc;
    }
    if ((rc = job.tally())) return rc;
    for (int l = 0; l < CMP_LABELS; ++l) out.counts[l] = h[CMP_COUNTS + l];
    if (writes) {
        if (w.rows() != h[CMP_FINE + SIMP_RUN]) { g_err = std::string(who) + ": internal: rows written and ranks given differ"; return SM_E_HIP; }
        out.written = w.rows();
        if (!w.commit(g_err)) return SM_E_ARG;
        if (std::rename(tmp.c_str(), out_path) != 0) {
            std::remove(tmp.c_str());
            g_err = sm_mapfile::said(who, out_path, " saved err!!");
            return SM_E_ARG;
        }
    }
    *info = out;
    cm.stats.launches = job.launches;
    cm.stats.total_ms = (float)(now_ms() - t_begin);
    return SM_OK;
}

int sm_compare_stats(sm_ctx *s, sm_compare_stats_t *out)
{
    if (!s || !out) { g_err = "sm_compare_stats: null argument"; return SM_E_ARG; }
    if (!s->cmp.stats_valid) { g_err = "sm_compare_stats: no sm_compare_maps call yet"; return SM_E_ARG; }
    *out = s->cmp.stats;
    return SM_OK;
}

}  // extern "C"
