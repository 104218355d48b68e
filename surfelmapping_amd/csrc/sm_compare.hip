// sm_compare.hip -- change detection between two map sets (sm_compare_maps; DESIGN.md "4r. Change detection"): the reference set
// streamed once into a fine voxel table with one representative per key and a cover table of keys, then the query set streamed
// once, every record labelled against them and the records whose label is asked for written, in set order, to one map file.
// Kernels: sm_k_compare.h; the tables themselves and the ranked output: sm_voxel.h; the scratch, the export and the collect of a
// call: sm_set_call.h.
#include "sm_set_call.h"
#include "sm_k_compare.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

constexpr uint32_t CHUNK = MapStaging::CHUNK;
enum { EV_CLR0 = 0, EV_CLR1, EV_REF0, EV_REF1, EV_QRY0, EV_QRY1 };     // pairs of the scratch's events: add_marked(&ev[first])
static_assert(CMP_FINE == 0 && CMP_COVER == SIMP_TALLY_WORDS, "lut_open puts a table's tally words first and its cover's behind them");

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

// One call's device side: both tables, the kernel arguments, the launches on the context's stream.
struct CompareJob {
    sm_ctx *s;
    Compare &cm;
    const Event *ev;
    const char *who;
    const sm_compare_params &p;
    LookupTable t;                     // the fine table (split faces) with its cover table (no faces); tally words CMP_FINE, CMP_COVER
    CmpParams cp{};
    Dev<uint8_t> tables;               // freed when the call ends: 104 bytes per slot
    RankedOutput out;
    uint32_t launches = 0;

    CompareJob(sm_ctx *s_, const char *who_, const sm_compare_params &p_) : s(s_), cm(s_->cmp), ev(s_->cmp.scratch.ev), who(who_), p(p_), out(s_, who_) {}

    int open(uint64_t reference_records, const float *pose16, bool writes)
    {
        int rc;
        uint64_t S;
        if ((rc = cm.scratch.ensure(CMP_TALLY_WORDS)) || (rc = cm.label.ensure()) || (!cm.d_keep && (rc = dalloc(cm.d_keep, CHUNK)))) return rc;
        if ((rc = voxel_slots(reference_records, p.max_cells, who, "a table", S))) return rc;
        t.a = voxel_args(p.voxel_mm, 0, p.origin, 1, p.max_cells);
        t.ac = voxel_args(p.voxel_mm, p.cover_shift, p.origin, 0, p.max_cells);
        if ((rc = lut_open(tables, &t, 1, S, true, cm.scratch.d_tally.get()))) return rc;
        // the tables' initialisation is device time of theirs (table_ms)
        if ((rc = mark(s, ev[EV_CLR0])) || (rc = lut_clear(s, &t, 1)) || (rc = cm.scratch.clear(s->stream)) || (rc = mark(s, ev[EV_CLR1]))) return rc;

        cp.lut = t.lut;
        cp.cover = t.TC.key;
        cp.mask = t.T.mask; cp.cmask = t.TC.mask;
        cp.V0 = t.a.V; cp.V1 = t.ac.V;
        for (int k = 0; k < 3; ++k) cp.origin[k] = p.origin[k];
        cp.match_class = p.match_class;
        cp.write_mask = writes ? p.write_mask : 0u;
        for (int e16 = 0; e16 < 16; ++e16) cp.T[e16] = pose16 ? (double)pose16[e16] : (e16 % 5 == 0 ? 1.0 : 0.0);
        cp.reach = (double)p.reach_cells * ((double)t.a.V * (1.0 / 65536.0));
        cp.cos_angle = std::cos((double)p.angle_thresh * (3.14159265358979323846 / 180.0));
        cp.plane = (double)p.plane_mm / 1000.0;
        return SM_OK;
    }
    // n <= CHUNK records of the reference into both tables
    void insert(const float4 *d_rec, uint32_t n)
    {
        lut_insert(s, t, d_rec, n, p.match_class, launches);
        cm.stats.chunks++;
    }
    // n <= CHUNK records of the query: labels into d_label[q], and with an output the kept ones at out(q) + (rank - the chunk's first rank) * 3
    void classify(const float4 *d_rec, uint32_t n, int q)
    {
        const unsigned nblk = (n + 255) / 256;
        hipLaunchKernelGGL(k_compare_classify, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, cp, cm.label.d[q].get(), cm.d_keep.get(), out.blk_cnt(),
                           cm.scratch.d_tally.get());
        launches++;
        if (out.writes()) {
            out.scan(nblk, cm.scratch.d_tally.get() + CMP_FINE, q, launches);
            hipLaunchKernelGGL(k_compare_emit, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, (const uint8_t *)cm.d_keep.get(), out.blk_base(),
                               out.info(q), out.out(q));
            launches++;
        }
        cm.stats.chunks++;
    }
    // the tally, once the stream is idle
    int tally() { return cm.scratch.read(s); }
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
    if ((rc = check_sets(query, reference, who)) || (rc = check_own_path(query, out_path, who)) || (rc = check_own_path(reference, out_path, who))) return rc;
    if ((rc = open_sets(query, reference, who, qset, rset))) return rc;
    const sm_map_source *const srcs[2] = {query, reference};
    const sm_mapset::ReadSet *const sets[2] = {&qset, &rset};
    uint32_t live[2];
    if ((rc = maps_counts(s, who, 2, srcs, sets, live))) return rc;
    const uint32_t qcnt = live[0], rcnt = live[1];
    const uint64_t qtotal = qset.file_total + qcnt, rtotal = rset.file_total + rcnt;

    Compare &cm = s->cmp;
    cm.stats = sm_compare_stats_t{};
    cm.stats_valid = true;
    sm_compare_info out{};
    out.query_records = qtotal;
    out.reference_records = rtotal;

    CompareJob job(s, who, *p);
    RankedOutput &ro = job.out;
    const Event *ev = job.ev;
    const float4 *d_model;
    if ((rc = job.open(rtotal, pose16, writes)) || (rc = maps_export(s, std::max(qcnt, rcnt), d_model))) return rc;
    if (qset.jobs.size() + rset.jobs.size() || (qcnt && writes))       // (the live model's kept records leave through its host buffer too)
        if ((rc = maps_ensure_staging(s))) return rc;
    float copy_ms = 0.0f;

    // ---- the reference: every chunk into both tables, then the representatives
    if ((rc = maps_feed(s, who, rset, reference->paths, rcnt, d_model, {&cm.stats.read_ms, &copy_ms, &cm.stats.table_ms}, ev[EV_REF0],
                        [&](const float4 *d_rec, uint32_t n, uint32_t) { job.insert(d_rec, n); })))
        return rc;
    lut_finish(s, job.t, job.launches);
    if ((rc = mark(s, ev[EV_REF1])) || (rc = job.tally())) return rc;
    if ((rc = add_marked(&ev[EV_CLR0], &cm.stats.table_ms)) || (rc = add_marked(&ev[EV_REF0], &cm.stats.table_ms))) return rc;
    const uint32_t *h = cm.scratch.h();
    // (nothing has been written: the labels and the output follow)
    if ((rc = voxel_check_tally(h + CMP_FINE, p->max_cells, who, "keys in the fine table")) ||
        (rc = voxel_check_tally(h + CMP_COVER, p->max_cells, who, "keys in the cover table")))
        return rc;
    out.cells_fine = h[CMP_FINE + SIMP_CELLS];
    out.cells_cover = h[CMP_COVER + SIMP_CELLS];

    // ---- the query: the labels of chunk c, and what is kept of it, come back while chunk c + 1 is on the device
    // (without an output the scratch alone: the labelling counts per block either way)
    if ((rc = writes ? ro.open(out_path, ".compare.tmp", qset, qcnt) : ro.ensure(0, 0))) return rc;
    const auto collect = [&](int q, uint32_t n, uint64_t gid0, hipStream_t stream) {
        return collect_labelled(ro, cm.label, labels, q, n, gid0, stream, &cm.stats.write_ms);
    };
    if ((rc = ro.run(qset, query->paths, qcnt, d_model, {&cm.stats.read_ms, &copy_ms, &cm.stats.classify_ms}, &ev[EV_QRY0],
                     [&](const float4 *d_rec, uint32_t n, uint64_t, int q) { job.classify(d_rec, n, q); }, collect)))
        return rc;
    if ((rc = job.tally())) return rc;
    for (int l = 0; l < CMP_LABELS; ++l) out.counts[l] = h[CMP_COUNTS + l];
    if (writes && (rc = ro.commit(out_path, h[CMP_FINE + SIMP_RUN], out.written))) return rc;
    *info = out;
    cm.stats.launches = job.launches;
    cm.stats.total_ms = (float)(now_ms() - t_begin);
    return SM_OK;
}

SM_STATS_GETTER(sm_compare_stats, sm_compare_stats_t, cmp, "sm_compare_maps")

}  // extern "C"
