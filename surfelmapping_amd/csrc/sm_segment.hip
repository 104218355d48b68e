// sm_segment.hip -- segmentation of a map set (sm_segment_maps; DESIGN.md "4t. Segmentation"): the set streamed once into a voxel
// table of nodes, the nodes united with their neighbours by a lock-free union-find over the table's slots, the trees flattened and
// the components summed at their roots; then the set streamed again, every record labelled with its component's number -- given in
// order of first appearance --, a row written per component and the records of the label kinds asked for written, in set order, to
// one map file.  Kernels: sm_k_segment.h; the grid, the table's size, the tally's verdict and the ranked output: sm_voxel.h; the
// call's frame: sm_set_call.h.
#include "sm_set_call.h"
#include "sm_k_segment.h"

using namespace sm;

namespace {

constexpr uint32_t CHUNK = MapStaging::CHUNK;
enum { EV_CLR0 = 0, EV_CLR1, EV_INS0, EV_INS1, EV_LINK0, EV_LINK1, EV_LAB0, EV_LAB1 };       // pairs of the scratch's events: add_marked(&ev[first])
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

// One call's device side: the table with its planes, the kernel arguments, the launches on the context's stream.
struct SegmentJob {
    sm_ctx *s;
    Segment &sg;
    const Event *ev;
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

    SegmentJob(sm_ctx *s_, const char *who_, const sm_segment_params &p_) : s(s_), sg(s_->seg), ev(s_->seg.scratch.ev), who(who_), p(p_), out(s_, who_) {}

    uint32_t *tally() const { return sg.scratch.d_tally.get(); }

    int open(uint64_t records, bool writes)
    {
        int rc;
        uint64_t slots;
        if ((rc = sg.scratch.ensure(SEG_TALLY_WORDS)) || (rc = sg.label.ensure()) || (!sg.d_code && (rc = dalloc(sg.d_code, CHUNK)))) return rc;
        if ((rc = voxel_slots(records, p.max_cells, who, "the table", slots))) return rc;
        a = voxel_args(p.voxel_mm, 0, p.origin, 0, p.max_cells);
        for (int i = 0; i < 8; ++i) sa.class_mask[i] = p.class_mask[i];
        sa.by_class = p.by_class;
        sa.max_l1 = p.connectivity == 6 ? 1 : p.connectivity == 18 ? 2 : 3;
        sa.min_records = p.min_records;
        sa.write_mask = writes ? p.write_mask : 0u;
        sa.combine = env_is_one("SM_SEGMENT_NO_COMBINE") ? 0 : 1;
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
        if ((rc = mark(s, ev[EV_CLR0]))) return rc;
        HIPCK(hipMemsetAsync(b, 0xFF, S * SEG_ONES_BYTES, s->stream));
        HIPCK(hipMemsetAsync(b + S * SEG_ONES_BYTES, 0, S * SEG_ZERO_BYTES, s->stream));
        if ((rc = sg.scratch.clear(s->stream))) return rc;
        return mark(s, ev[EV_CLR1]);
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
                           sa.write_mask, sg.label.d[q].get(), out.blk_base(0), writes ? out.info(q) : nullptr, writes ? out.out(q) : nullptr);
        launches += 2;
        sg.stats.chunks++;
    }
    // the tally, once the stream is idle; SM_E_STALL if a device loop reached its bound
    int read_tally()
    {
        if (int rc = sg.scratch.read(s)) return rc;
        if (sg.scratch.h()[SIMP_ERR] & SEG_ERR_STALL) {
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
    SetCall call(s, src, who);
    if (!s || !src || !p || !info) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if (!components && cap) { g_err = std::string(who) + ": no components to hold cap = " + std::to_string(cap) + " rows"; return SM_E_ARG; }
    const bool writes = out_path != nullptr;
    int rc;
    if ((rc = call.open([&] { return check_params(p, writes, who); }, {out_path}))) return rc;
    const sm_mapset::ReadSet &set = call.set;
    const uint32_t cnt = call.cnt;
    const uint64_t total = call.total;

    Segment &sg = s->seg;
    sg.stats = sm_segment_stats_t{};
    sg.stats_valid = true;
    sm_segment_info got{};
    got.records = total;

    SegmentJob job(s, who, *p);
    RankedOutput &ro = job.out;
    const Event *ev = job.ev;
    if ((rc = job.open(total, writes)) || (rc = call.model())) return rc;
    const float4 *d_model = call.d_model;
    if (!set.jobs.empty() || (cnt && writes))            // (the live model's kept records leave through the staging's host buffer too)
        if ((rc = call.staging())) return rc;
    float &copy_ms = call.copy_ms;

    // ---- reading 1: the nodes; then link, flatten, reduce
    if ((rc = maps_feed(s, who, set, src->paths, cnt, d_model, {&sg.stats.read_ms, &copy_ms, &sg.stats.table_ms}, ev[EV_INS0],
                        [&](const float4 *d_rec, uint32_t n, uint32_t gid0) { job.insert(d_rec, n, gid0); })))
        return rc;
    sg.stats.readings = 1;
    if ((rc = mark(s, ev[EV_INS1])) || (rc = job.read_tally())) return rc;
    if ((rc = add_marked(&ev[EV_CLR0], &sg.stats.table_ms)) || (rc = add_marked(&ev[EV_INS0], &sg.stats.table_ms))) return rc;
    const uint32_t *h = sg.scratch.h();
    // (nothing has been written: the labels, the rows and the output follow)
    if ((rc = voxel_check_tally(h + SEG_TABLE, p->max_cells, who, "nodes"))) return rc;
    got.cells = h[SEG_TABLE + SIMP_CELLS];
    if ((rc = mark(s, ev[EV_LINK0]))) return rc;
    job.link();
    if ((rc = mark(s, ev[EV_LINK1])) || (rc = job.read_tally()) || (rc = add_marked(&ev[EV_LINK0], &sg.stats.link_ms))) return rc;

    // ---- reading 2: the labels of chunk c, and what is kept of it, come back while chunk c + 1 is on the device
    job.cap = std::min(cap, got.cells);                  // (there are no more components than nodes)
    if (job.cap && (rc = dalloc(job.d_rows, job.cap))) return rc;
    if ((rc = writes ? ro.open(out_path, ".segment.tmp", set, cnt) : ro.ensure(0, 0))) return rc;
    const auto collect = [&](int q, uint32_t n, uint64_t gid0, hipStream_t stream) {
        return collect_labelled(ro, sg.label, labels, q, n, gid0, stream, &sg.stats.write_ms);
    };
    if ((rc = ro.run(set, src->paths, cnt, d_model, {&sg.stats.read_ms, &copy_ms, &sg.stats.label_ms}, &ev[EV_LAB0],
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
    sg.stats.total_ms = call.elapsed_ms();
    return SM_OK;
}

SM_STATS_GETTER(sm_segment_stats, sm_segment_stats_t, seg, "sm_segment_maps")

}  // extern "C"
