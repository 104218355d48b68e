// sm_simplify.hip -- voxel-cell simplification (sm_simplify, sm_simplify_maps; DESIGN.md "4p. Simplification"): the records of
// the live model or of a map set merged per cell of a world grid, in two passes over the records.  A map set's files go through
// the context's chunk stream twice, the live model through the export scratch.  Kernels: sm_k_simplify.h; the grid, the table's
// size and the ranked output of pass 2: sm_voxel.h; the frame of the call on a set: sm_set_call.h.
#include "sm_set_call.h"
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
    const Event *ev;
    const char *who;
    SimplifyArgs a{};
    SimplifyTable T{};
    Dev<uint8_t> table;                // freed when the call ends: up to 136 bytes per record
    RankedOutput out;
    uint32_t launches = 0;

    SimplifyJob(sm_ctx *s_, const char *who_) : s(s_), sp(s_->simp), ev(s_->simp.scratch.ev), who(who_), out(s_, who_) {}

    // the scratch every call shares, the table for `records` records, everything initialised
    int open(uint64_t records, const sm_simplify_params &p)
    {
        int rc;
        if ((rc = sp.scratch.ensure(SIMP_TALLY_WORDS)) || (!sp.d_code && (rc = dalloc(sp.d_code, CHUNK)))) return rc;
        a = voxel_args(p.voxel_mm, 0, p.origin, p.split_normals, p.max_cells);
        uint64_t S;
        if ((rc = voxel_slots(records, p.max_cells, who, "the table", S))) return rc;
        HIPCK(hipMalloc((void **)table.put(), simplify_table_bytes((size_t)S)));
        uint8_t *b = table.get();
        auto take = [&](auto *&ptr, size_t planes, size_t width) { ptr = (std::remove_reference_t<decltype(ptr)>)b; b += planes * width * (size_t)S; };
        take(T.key, 1, 8); take(T.lo, 3, 4); take(T.init_min, 1, 4); take(T.first, 1, 4);
        uint8_t *zeros = b;
        take(T.SW, 1, 8); take(T.SP, 3, 8); take(T.SN, 3, 8); take(T.SC, 3, 8);
        take(T.n, 1, 4); take(T.hi, 3, 4); take(T.rmax, 1, 4); take(T.conf_max, 1, 4); take(T.time_max, 1, 4);
        T.mask = (uint32_t)(S - 1);
        T.tally = sp.scratch.d_tally;
        HIPCK(hipMemsetAsync(table.get(), 0xFF, (size_t)S * SIMP_ONES_BYTES, s->stream));
        HIPCK(hipMemsetAsync(zeros, 0, (size_t)S * SIMP_ZERO_BYTES, s->stream));
        return sp.scratch.clear(s->stream);
    }
    // pass 1 of n <= CHUNK records
    void insert(const float4 *d_rec, uint32_t n, uint32_t gid0)
    {
        hipLaunchKernelGGL(k_simplify_insert, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, gid0, a, T);
        launches++;
        sp.stats.chunks++;
    }
    // pass 2 of n <= CHUNK records: the representatives at out(q) + (rank - the chunk's first rank) * 3; q < 0: at out(0) + rank * 3
    void emit(const float4 *d_rec, uint32_t n, uint32_t gid0, int q)
    {
        const unsigned nblk = (n + 255) / 256;
        hipLaunchKernelGGL(k_simplify_flag, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, gid0, a, T, sp.d_code.get(), out.blk_cnt());
        launches++;
        out.scan(nblk, sp.scratch.d_tally.get(), q, launches);
        hipLaunchKernelGGL(k_simplify_emit, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, a, T, (const uint32_t *)sp.d_code.get(), out.blk_base(),
                           q < 0 ? nullptr : out.info(q), out.out(std::max(q, 0)));
        launches++;
        sp.stats.chunks++;
    }
    // the tally at h(), once the stream is idle; after pass 1 the sticky error word decides
    const uint32_t *h() const { return sp.scratch.h(); }
    int tally()
    {
        if (int rc = sp.scratch.read(s)) return rc;
        const uint32_t *t = h();
        if (t[SIMP_ERR] & 4u) { g_err = std::string(who) + ": internal: a key of pass 1 is missing in pass 2"; return SM_E_HIP; }
        return voxel_check_tally(t, a.max_cells, who, "distinct cells");
    }
    void fold_tally()
    {
        const uint32_t *t = h();
        sp.stats.cells_merged = t[SIMP_MERGED];
        sp.stats.loose = t[SIMP_N_LOOSE];
        sp.stats.largest_cell = std::max(t[SIMP_LARGEST], t[SIMP_CELLS] ? 1u : 0u);
        sp.stats.launches = launches;
    }
};

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
    if ((rc = ensure_export(s, (size_t)cnt * 48)) || (rc = job.out.ensure(0, cnt)) || (rc = job.open(cnt, *p))) return rc;
    const float4 *d_in = (const float4 *)s->d_export.get();
    export_aos(s, (float *)s->d_export.get(), 0u, cnt);
    if ((rc = mark(s, job.ev[0]))) return rc;
    for (uint32_t first = 0; first < cnt; first += CHUNK) job.insert(d_in + (size_t)first * 3, std::min(CHUNK, cnt - first), first);
    if ((rc = job.tally())) return rc;                   // (SM_E_CAPACITY: the model has only been read)
    for (uint32_t first = 0; first < cnt; first += CHUNK) job.emit(d_in + (size_t)first * 3, std::min(CHUNK, cnt - first), first, -1);
    if ((rc = mark(s, job.ev[1])) || (rc = job.tally()) || (rc = add_marked(job.ev, &sp.stats.device_ms))) return rc;
    const uint32_t n_out = job.h()[SIMP_RUN];
    job.fold_tally();
    sp.stats.records_out = n_out;

    // the model is the output's rows: what an upload of them leaves
    import_aos(s, (const float *)job.out.out(0), 0u, n_out);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(s->stream));
    if ((rc = publish_dense(s, n_out, 0))) return rc;
    RankScratch &rs = s->ranked;
    if (rs.out_cap[0] > CHUNK) { rs.d_out[0] = Dev<float4>(); rs.out_cap[0] = 0; }      // (a model's worth of records: not kept)
    sp.stats.total_ms = (float)(now_ms() - t_begin);
    return SM_OK;
}

int sm_simplify_maps(sm_ctx *s, const sm_map_source *src, const sm_simplify_params *p, const char *out_path)
{
    const char *who = "sm_simplify_maps";
    SetCall call(s, src, who);
    if (!s || !src || !out_path) { g_err = std::string(who) + ": null context, source or output path"; return SM_E_ARG; }
    int rc;
    if ((rc = call.open([&] { return check_params(p, who); }, {out_path}))) return rc;
    const sm_mapset::ReadSet &set = call.set;
    const uint32_t cnt = call.cnt;
    const uint64_t total = call.total;
    Simplify &sp = s->simp;
    sp.stats = sm_simplify_stats_t{};
    sp.stats_valid = true;
    sp.stats.records_in = total;

    SimplifyJob job(s, who);
    RankedOutput &out = job.out;
    if (total) {
        if ((rc = call.staging()) || (rc = job.open(total, *p)) || (rc = call.model())) return rc;
        const float4 *d_model = call.d_model;
        const MapStream::Tally times = {&sp.stats.read_ms, &call.copy_ms, &sp.stats.device_ms};

        // ---- pass 1: the files, chunk by chunk, then the live model
        if ((rc = maps_feed(s, who, set, src->paths, cnt, d_model, times, job.ev[0],
                            [&](const float4 *d_rec, uint32_t n, uint32_t gid0) { job.insert(d_rec, n, gid0); })))
            return rc;
        if ((rc = mark(s, job.ev[1])) || (rc = job.tally()) || (rc = add_marked(job.ev, &sp.stats.device_ms))) return rc;   // (SM_E_CAPACITY: nothing is written)

        // ---- pass 2: the representatives of chunk c into the output while chunk c + 1 is on the device
        if ((rc = out.open(out_path, ".simplify.tmp", set, cnt))) return rc;
        if ((rc = out.run(set, src->paths, cnt, d_model, times, job.ev,
                          [&](const float4 *d_rec, uint32_t n, uint64_t gid0, int q) { job.emit(d_rec, n, (uint32_t)gid0, q); },
                          [&](int q, uint32_t, uint64_t, hipStream_t stream) -> int {
                              uint32_t m;
                              if (int e = out.stage(q, stream, m)) return e;
                              if (m) HIPCK(hipStreamSynchronize(stream));
                              return out.write(q, m);
                          })))
            return rc;
        if ((rc = job.tally())) return rc;
        job.fold_tally();
    } else if ((rc = out.open(out_path, ".simplify.tmp", set, cnt))) {
        return rc;
    }
    if ((rc = out.commit(out_path, total ? job.h()[SIMP_RUN] : 0u, sp.stats.records_out))) return rc;
    sp.stats.total_ms = call.elapsed_ms();
    return SM_OK;
}

SM_STATS_GETTER(sm_simplify_stats, sm_simplify_stats_t, simp, "sm_simplify / sm_simplify_maps")

}  // extern "C"
