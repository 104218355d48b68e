// sm_segment.hip -- segmentation of a map set (sm_segment_maps; DESIGN.md "4t. Segmentation"): the set streamed once into a voxel
// table of nodes, the nodes united with their neighbours by a lock-free union-find over the table's slots, the trees flattened and
// the components summed at their roots; then the set streamed again, every record labelled with its component's number -- given in
// order of first appearance --, a row written per component and the records of the label kinds asked for written, in set order, to
// one map file.  Kernels: sm_k_segment.h; the grid, the table's size, the tally's verdict and the ranked output: sm_voxel.h.
#include "sm_voxel.h"
#include "sm_k_segment.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

constexpr uint32_t CHUNK = MapStaging::CHUNK;
enum { EV_CLR0 = 0, EV_CLR1, EV_INS0, EV_INS1, EV_LINK0, EV_LINK1, EV_LAB0, EV_LAB1 };       // pairs: add_marked(&ev[first])
static_assert(sizeof(SegRow) == sizeof(sm_segment_component), "a row leaves the device as it is");
static_assert(SEG_LOOSE == SM_SEGMENT_LOOSE && SEG_SMALL == SM_SEGMENT_SMALL && SEG_SKIPPED == SM_SEGMENT_SKIPPED, "the codes are the labels");

int check_params(const sm_segment_params *p, bool writes, const char *who)
{
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (p->voxel_mm < 10 || p->voxel_mm > 10000) return bad("voxel_mm outside 10..10000");
    if (p->connectivity != 6 && p->connectivity != 18 && p->connectivity != 26) return bad("connectivity is 6, 18 or 26");
    if (p->by_class != 0 && p->by_class != 1) return bad("by_class is 0 or 1");
    if (p->min_records == 0) return bad("min_records is 0");
    if (writes && (p->write_mask < 1 || p->write_mask > 15)) return bad("write_mask outside 1..15");
    if (p->max_cells == 0) return bad("max_cells is 0");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k])) return bad("non-finite origin");
    return SM_OK;
}

int seg_alloc(sm_ctx *s)
{
    Segment &sg = s->seg;
    if (sg.d_tally) return SM_OK;
    Dev<uint32_t> code, label[2], tally;
    int rc;
    if ((rc = dalloc(code, CHUNK)) || (rc = dalloc(label[0], CHUNK)) || (rc = dalloc(label[1], CHUNK)) || (rc = dalloc(tally, SEG_TALLY_WORDS))) return rc;
    HIPCK(hipHostMalloc((void **)sg.h_tally.put(), SEG_TALLY_WORDS * 4, hipHostMallocDefault));
    for (Host<uint32_t> &h : sg.h_label) HIPCK(hipHostMalloc((void **)h.put(), (size_t)CHUNK * 4, hipHostMallocDefault));
    for (Event &e : sg.ev) HIPCK(hipEventCreate(e.put()));
    sg.d_code = std::move(code); sg.d_label[0] = std::move(label[0]); sg.d_label[1] = std::move(label[1]);
    sg.d_tally = std::move(tally);                       // last: it marks the set complete
    return SM_OK;
}

// One call's device side: the table with its planes, the kernel arguments, the launches on the context's stream.
struct SegmentJob {
    sm_ctx *s;
    Segment &sg;
    const char *who;
    const sm_segment_params &p;
    SimplifyArgs a{};
    SegArgs sa{};
    SimplifyTable T{};                 // key, n and first only
    SegPlanes P{};
    Dev<uint8_t> table;                // freed when the call ends: SEG_SLOT_BYTES per slot
    Dev<SegRow> d_rows;
    uint32_t cap = 0;                  // rows at d_rows
    RankedOutput out;
    uint32_t launches = 0;

    SegmentJob(sm_ctx *s_, const char *who_, const sm_segment_params &p_) : s(s_), sg(s_->seg), who(who_), p(p_), out(s_, who_) {}

    uint32_t *tally() const { return sg.d_tally.get(); }

    int open(uint64_t records, bool writes)
    {
        int rc;
        uint64_t slots;
        if ((rc = seg_alloc(s)) || (rc = voxel_slots(records, p.max_cells, who, "the table", slots))) return rc;
        a = voxel_args(p.voxel_mm, 0, p.origin, 0, p.max_cells);
        for (int i = 0; i < 8; ++i) sa.class_mask[i] = p.class_mask[i];
        sa.by_class = p.by_class;
        sa.max_l1 = p.connectivity == 6 ? 1 : p.connectivity == 18 ? 2 : 3;
        sa.min_records = p.min_records;
        sa.write_mask = writes ? p.write_mask : 0u;
        const char *e = std::getenv("SM_SEGMENT_NO_COMBINE");
        sa.combine = (e && e[0] == '1') ? 0 : 1;
        // key | first, c_first, c_lo[3] (all ones) | c_sum[3], n, c_records, c_cells, c_hi[3] (zero) | parent, number
        const size_t S = (size_t)slots;
        if ((rc = dalloc(table, S * SEG_SLOT_BYTES))) return rc;
        uint8_t *b = table.get();
        T.key = (unsigned long long *)b;
        T.first = (uint32_t *)(b + S * 8);
        P.c_first = T.first + S; P.c_lo = P.c_first + S;
        P.c_sum = (unsigned long long *)(b + S * SEG_ONES_BYTES);
        T.n = (uint32_t *)(P.c_sum + 3 * S);
        P.c_records = T.n + S; P.c_cells = P.c_records + S; P.c_hi = P.c_cells + S;
        P.parent = P.c_hi + 3 * S; P.number = P.parent + S;
        T.mask = (uint32_t)(S - 1);
        T.tally = tally();
        // the table's initialisation is device time of its own (table_ms)
        if ((rc = mark(s, sg.ev[EV_CLR0]))) return rc;
        HIPCK(hipMemsetAsync(b, 0xFF, S * SEG_ONES_BYTES, s->stream));
        HIPCK(hipMemsetAsync(b + S * SEG_ONES_BYTES, 0, S * SEG_ZERO_BYTES, s->stream));
        HIPCK(hipMemsetAsync(tally(), 0, SEG_TALLY_WORDS * 4, s->stream));
        return mark(s, sg.ev[EV_CLR1]);
    }
    // reading 1 of n <= CHUNK records
    void insert(const float4 *d_rec, uint32_t n, uint32_t gid0)
    {
        hipLaunchKernelGGL(k_segment_insert, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, gid0, a, sa, T, P.parent);
        launches++;
        sg.stats.chunks++;
    }
    // the nodes united, the trees flattened, the components summed
    void link()
    {
        const dim3 grid(T.mask / 256u + 1u);
        hipLaunchKernelGGL(k_segment_link, grid, dim3(256), 0, s->stream, T, P.parent, sa.max_l1);
        hipLaunchKernelGGL(k_segment_flatten, grid, dim3(256), 0, s->stream, T, P.parent);
        hipLaunchKernelGGL(k_segment_reduce, grid, dim3(256), 0, s->stream, T, P, sa.combine);
        launches += 3;
    }
    // reading 2 of n <= CHUNK records: labels into d_label[q], the openers' rows, and with an output the kept records at out(q)
    void label(const float4 *d_rec, uint32_t n, uint32_t gid0, int q)
    {
        const unsigned nblk = (n + 255) / 256;
        const bool writes = out.writes();
        hipLaunchKernelGGL(k_segment_mark, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, gid0, a, sa, T, P, sg.d_code.get(), out.blk_cnt(0), out.blk_cnt(1));
        launches++;
        if (writes) out.scan(nblk, tally() + SEG_TABLE, q, launches, 0);
        out.scan(nblk, tally() + SEG_OPEN, -1, launches, 1);
        hipLaunchKernelGGL(k_segment_open, dim3(nblk), dim3(256), 0, s->stream, n, gid0, (const uint32_t *)sg.d_code.get(), T, P, sa.by_class, out.blk_base(1),
                           cap, d_rows.get());
        hipLaunchKernelGGL(k_segment_label, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, (const uint32_t *)sg.d_code.get(), (const uint32_t *)P.number,
                           sa.write_mask, sg.d_label[q].get(), out.blk_base(0), writes ? out.info(q) : nullptr, writes ? out.out(q) : nullptr);
        launches += 2;
        sg.stats.chunks++;
    }
    // the tally, once the stream is idle; SM_E_STALL if a device loop reached its bound
    int read_tally()
    {
        if (int rc = voxel_read_tally(s, tally(), sg.h_tally.get(), SEG_TALLY_WORDS)) return rc;
        if (sg.h_tally.get()[SIMP_ERR] & SEG_ERR_STALL) {
            g_err = std::string(who) + ": a union-find walk reached its bound of " + std::to_string((uint64_t)T.mask + 1u) + " steps";
            return SM_E_STALL;
        }
        return SM_OK;
    }
};

}  // namespace

extern "C" {

int sm_default_segment_params(sm_segment_params *p)
{
    if (!p) { g_err = "sm_default_segment_params: null argument"; return SM_E_ARG; }
    *p = sm_segment_params{};
    p->voxel_mm = 200;
    p->connectivity = 26;
    p->by_class = 1;
    for (uint32_t &w : p->class_mask) w = 0xFFFFFFFFu;
    p->min_records = 1;
    p->write_mask = 1;
    p->max_cells = 1u << 24;
    return SM_OK;
}

int sm_segment_maps(sm_ctx *s, const sm_map_source *src, const sm_segment_params *p, uint32_t *labels, sm_segment_component *components, uint32_t cap,
                    const char *out_path, sm_segment_info *info)
{
    const char *who = "sm_segment_maps";
    const double t_begin = now_ms();
    if (!s || !src || !p || !info) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if (!components && cap) { g_err = std::string(who) + ": no components to hold cap = " + std::to_string(cap) + " rows"; return SM_E_ARG; }
    const bool writes = out_path != nullptr;
    int rc;
    if ((rc = check_whole_map(s, who)) || (rc = check_params(p, writes, who)) || (rc = check_not_mid_cull(s, who)) || (rc = check_map_source(src, who)))
        return rc;
    for (uint32_t i = 0; writes && i < src->n_paths; ++i)                // the output needs a path of its own
        if (strcmp(src->paths[i], out_path) == 0) { g_err = sm_mapfile::said(who, out_path, " is a file of the set: the output needs a path of its own"); return SM_E_ARG; }
    sm_mapset::ReadSet set;
    uint32_t cnt;
    if ((rc = maps_open(s, src, who, check_whole_map, set, cnt))) return rc;
    const uint64_t total = set.file_total + cnt;

    Segment &sg = s->seg;
    sg.stats = sm_segment_stats_t{};
    sg.stats_valid = true;
    sm_segment_info got{};
    got.records = total;

    SegmentJob job(s, who, *p);
    RankedOutput &ro = job.out;
    if ((rc = job.open(total, writes))) return rc;
    const float4 *d_model = nullptr;
    if (cnt) {
        if ((rc = ensure_export(s, (size_t)cnt * 48))) return rc;
        export_aos(s, (float *)s->d_export.get(), 0u, cnt);
        d_model = (const float4 *)s->d_export.get();
    }
    if (!set.jobs.empty() || (cnt && writes))            // (the live model's kept records leave through the staging's host buffer too)
        if ((rc = maps_ensure_staging(s))) return rc;
    float copy_ms = 0.0f;

    // ---- reading 1: the nodes; then link, flatten, reduce
    if ((rc = maps_feed(s, who, set, src->paths, cnt, d_model, {&sg.stats.read_ms, &copy_ms, &sg.stats.table_ms}, sg.ev[EV_INS0],
                        [&](const float4 *d_rec, uint32_t n, uint32_t gid0) { job.insert(d_rec, n, gid0); })))
        return rc;
    sg.stats.readings = 1;
    if ((rc = mark(s, sg.ev[EV_INS1])) || (rc = job.read_tally())) return rc;
    if ((rc = add_marked(&sg.ev[EV_CLR0], &sg.stats.table_ms)) || (rc = add_marked(&sg.ev[EV_INS0], &sg.stats.table_ms))) return rc;
    const uint32_t *h = sg.h_tally.get();
    // (nothing has been written: the labels, the rows and the output follow)
    if ((rc = voxel_check_tally(h + SEG_TABLE, p->max_cells, who, "nodes"))) return rc;
    got.cells = h[SEG_TABLE + SIMP_CELLS];
    if ((rc = mark(s, sg.ev[EV_LINK0]))) return rc;
    job.link();
    if ((rc = mark(s, sg.ev[EV_LINK1])) || (rc = job.read_tally()) || (rc = add_marked(&sg.ev[EV_LINK0], &sg.stats.link_ms))) return rc;

    // ---- reading 2: the labels of chunk c, and what is kept of it, come back while chunk c + 1 is on the device
    job.cap = std::min(cap, got.cells);                  // (there are no more components than nodes)
    if (job.cap && (rc = dalloc(job.d_rows, job.cap))) return rc;
    if ((rc = writes ? ro.open(out_path, ".segment.tmp", set, cnt) : ro.ensure(0, 0))) return rc;
    const auto collect = [&](int q, uint32_t n, uint64_t gid0, hipStream_t stream) -> int {
        const double t0 = now_ms();
        uint32_t m;
        if (int e = ro.stage(q, stream, m)) return e;
        if (labels) HIPCK(hipMemcpyAsync(sg.h_label[q], sg.d_label[q], (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        if (m || labels) HIPCK(hipStreamSynchronize(stream));
        if (labels) memcpy(labels + gid0, sg.h_label[q].get(), (size_t)n * 4);
        const int e = ro.write(q, m);
        sg.stats.write_ms += (float)(now_ms() - t0);
        return e;
    };
    if ((rc = ro.run(set, src->paths, cnt, d_model, {&sg.stats.read_ms, &copy_ms, &sg.stats.label_ms}, &sg.ev[EV_LAB0],
                     [&](const float4 *d_rec, uint32_t n, uint64_t gid0, int q) { job.label(d_rec, n, (uint32_t)gid0, q); }, collect)))
        return rc;
    sg.stats.readings = 2;
    if ((rc = job.read_tally())) return rc;
    if (h[SIMP_ERR] & SEG_ERR_CHANGED) { g_err = std::string(who) + ": the set changed while it was read"; return SM_E_ARG; }
    for (int l = 0; l < SEG_KINDS; ++l) got.counts[l] = h[SEG_COUNTS + l];
    got.components = h[SEG_OPEN + SIMP_RUN];
    got.small_components = h[SEG_SMALL_COMPONENTS];
    got.largest = h[SEG_LARGEST];
    const uint32_t rows = std::min(job.cap, got.components);
    if (rows) {
        HIPCK(hipMemcpyAsync(components, job.d_rows.get(), (size_t)rows * sizeof(SegRow), hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
    }
    if (writes && (rc = ro.commit(out_path, h[SEG_TABLE + SIMP_RUN], got.written))) return rc;
    *info = got;
    sg.stats.launches = job.launches;
    sg.stats.total_ms = (float)(now_ms() - t_begin);
    return SM_OK;
}

int sm_segment_stats(sm_ctx *s, sm_segment_stats_t *out)
{
    if (!s || !out) { g_err = "sm_segment_stats: null argument"; return SM_E_ARG; }
    if (!s->seg.stats_valid) { g_err = "sm_segment_stats: no sm_segment_maps call yet"; return SM_E_ARG; }
    *out = s->seg.stats;
    return SM_OK;
}

}  // extern "C"
