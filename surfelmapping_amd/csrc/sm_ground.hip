// sm_ground.hip -- a map set as a planner's ground map (sm_ground_maps; DESIGN.md "4v. Ground map"): the set streamed once for the
// lowest ground-like record of every cell of the window, the reference heights filled in from neighbouring cells, the set streamed
// again for the ground's sums and the obstacles, the planes and states finished per cell, the blocking cells' capped Euclidean
// distance transform, and every plane asked for back with one copy.  A file whose index box misses the window is read in neither
// reading.  Kernels: sm_k_ground.h; the call's frame: sm_set_call.h.  The accumulators and planes are allocated per call and freed
// when it ends.
#include "sm_set_call.h"
#include "sm_k_ground.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

enum { EV_CLR0 = 0, EV_CLR1, EV_MIN0, EV_MIN1, EV_FILL0, EV_FILL1, EV_ACC0, EV_ACC1, EV_STATE0, EV_STATE1, EV_CLEAR0, EV_CLEAR1, N_EV };
static_assert(N_EV == decltype(Ground::scratch)::N_EV, "the context holds the events of a call");
static_assert(GROUND_NONE == SM_GROUND_NONE && GROUND_UNKNOWN == SM_GROUND_UNKNOWN && GROUND_FREE == SM_GROUND_FREE &&
              GROUND_OBSTACLE == SM_GROUND_OBSTACLE && GROUND_STEP == SM_GROUND_STEP, "the states are the header's");

int q16(int64_t mm) { return (int)((mm * 65536 + 500) / 1000); }

int check_params(const sm_ground_params *p, const char *who)
{
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (p->cell_mm < 10 || p->cell_mm > 10000) return bad("cell_mm outside 10..10000");
    if (p->up < 0 || p->up > 5) return bad("up outside 0..5");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k])) return bad("non-finite origin");
    if (p->nu < 1 || p->nu > 8192) return bad("nu outside 1..8192");
    if (p->nv < 1 || p->nv > 8192) return bad("nv outside 1..8192");
    if ((int64_t)p->nu * p->nv > (1 << 24)) return bad("nu * nv above 2^24");
    if (p->min_up < 0 || p->min_up > 16384) return bad("min_up outside 0..16384");
    if (p->band_mm < 0 || p->band_mm > 10000) return bad("band_mm outside 0..10000");
    if (p->clear_lo_mm < 0 || p->clear_lo_mm >= p->clear_hi_mm) return bad("clear_lo_mm must be >= 0 and below clear_hi_mm");
    if (p->clear_hi_mm > 100000) return bad("clear_hi_mm above 100000");
    if (p->min_obstacle == 0) return bad("min_obstacle is 0");
    if (p->fill_cells < 0 || p->fill_cells > GROUND_MAX_FILL) return bad("fill_cells outside 0..16");
    if (p->step_mm < 0 || p->step_mm > 10000) return bad("step_mm outside 0..10000");
    if (p->reach_cells < 1 || p->reach_cells > GROUND_MAX_REACH) return bad("reach_cells outside 1..255");
    if (p->unknown_blocks != 0 && p->unknown_blocks != 1) return bad("unknown_blocks is 0 or 1");
    if (p->normal_sign != 1 && p->normal_sign != -1) return bad("normal_sign is +1 or -1");
    return SM_OK;
}

GroundArgs ground_args(const sm_ground_params &p)
{
    GroundArgs g{};
    g.C = q16(p.cell_mm);
    g.B = q16(p.band_mm); g.L = q16(p.clear_lo_mm); g.Hi = q16(p.clear_hi_mm); g.S = q16(p.step_mm);
    for (int k = 0; k < 3; ++k) g.origin[k] = p.origin[k];
    g.a = p.up >> 1;
    g.sgn = (p.up & 1) ? -1 : 1;
    g.nsgn = g.sgn * p.normal_sign;
    g.ua = g.a == 0 ? 1 : 0;
    g.va = g.a == 2 ? 1 : 2;
    g.nu = p.nu; g.nv = p.nv;
    g.min_up = p.min_up;
    for (int i = 0; i < 8; ++i) g.ground_mask[i] = p.ground_mask[i];
    g.min_obstacle = p.min_obstacle;
    g.fill = p.fill_cells;
    g.reach = p.reach_cells;
    g.unknown_blocks = p.unknown_blocks;
    g.step_on = p.step_mm > 0 ? 1 : 0;
    g.combine = env_is_one("SM_GROUND_NO_COMBINE") ? 0 : 1;
    return g;
}

// Can no record of a file with this index box lie in the window?  A record is in on a horizontal axis k iff 0 <= X[k] < n * C, X[k] =
// floor(((double)p - (double)origin) * 65536), which rises with p: the box's ends decide for every centre between them.  (A box
// with lo > hi holds no finite centre: every record of the file is loose.)
bool box_misses_window(const sm_mapset::FileIndex::Entry &e, const GroundArgs &g)
{
    const int axis[2] = {g.ua, g.va}, cells[2] = {g.nu, g.nv};
    for (int i = 0; i < 2; ++i) {
        const int k = axis[i];
        if (e.lo[k] > e.hi[k]) return true;
        const double extent = (double)((long long)cells[i] * g.C) / 65536.0;
        if ((double)e.hi[k] - (double)g.origin[k] < 0.0 || (double)e.lo[k] - (double)g.origin[k] >= extent) return true;
    }
    return false;
}

// One call's device side: the accumulators and the planes of N cells, the launches on the context's stream.
struct GroundJob {
    sm_ctx *s;
    Ground &gr;
    const Event *ev;
    GroundArgs g;
    size_t N;
    Dev<uint8_t> mem;                  // freed when the call ends
    GroundSums P{};
    int *Z = nullptr, *R = nullptr, *ground = nullptr;
    uint32_t *clear2 = nullptr;
    uint8_t *state = nullptr, *cls = nullptr, *gcol = nullptr, *bgr = nullptr;
    uint32_t launches = 0;
    sm_ground_stats_t stats{};         // this call's; the context's once the call has succeeded

    GroundJob(sm_ctx *s_, const GroundArgs &g_) : s(s_), gr(s_->ground), ev(s_->ground.scratch.ev), g(g_), N((size_t)g_.nu * g_.nv) {}

    uint32_t *tally() const { return gr.scratch.d_tally.get(); }

    int open()
    {
        int rc;
        // SW, SH, SC[3], best, n_obst, top (zero) | Z (no ground) | R, ground, clear2 | state, cls, gcol, bgr[3]
        if ((rc = gr.scratch.ensure(GROUND_TALLY_WORDS)) || (rc = dalloc(mem, N * (GROUND_ZERO_BYTES + 4 * 4 + 6)))) return rc;
        uint8_t *b = mem.get();
        P.SW = (unsigned long long *)b; P.SH = P.SW + N; P.SC = P.SH + N; P.best = P.SC + 3 * N;
        P.n_obst = (uint32_t *)(P.best + N);
        P.top = (int *)(P.n_obst + N);
        Z = P.top + N; R = Z + N; ground = R + N;
        clear2 = (uint32_t *)(ground + N);
        state = (uint8_t *)(clear2 + N); cls = state + N; gcol = cls + N; bgr = gcol + N;
        if ((rc = mark(s, ev[EV_CLR0]))) return rc;
        HIPCK(hipMemsetAsync(b, 0, N * GROUND_ZERO_BYTES, s->stream));
        HIPCK(hipMemsetAsync(Z, 0x7F, N * 4, s->stream));
        if ((rc = gr.scratch.clear(s->stream))) return rc;
        return mark(s, ev[EV_CLR1]);
    }
    void lowest(const float4 *d_rec, uint32_t n)
    {
        if (!n) return;
        hipLaunchKernelGGL(k_ground_min, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, g, Z);
        launches++;
        stats.chunks++;
    }
    void fill()
    {
        const dim3 grid((g.nu + GROUND_TILE - 1) / GROUND_TILE, (g.nv + GROUND_TILE - 1) / GROUND_TILE);
        hipLaunchKernelGGL(k_ground_fill, grid, dim3(256), 0, s->stream, g, (const int *)Z, R);
        launches++;
    }
    void accumulate(const float4 *d_rec, uint32_t n, uint32_t gid0)
    {
        if (!n) return;
        hipLaunchKernelGGL(k_ground_accum, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, gid0, g, (const int *)R, P, tally());
        launches++;
        stats.chunks++;
    }
    void finish()
    {
        const dim3 grid((unsigned)((N + 255) / 256));
        hipLaunchKernelGGL(k_ground_finish, grid, dim3(256), 0, s->stream, g, (const int *)Z, P, ground, cls, bgr);
        hipLaunchKernelGGL(k_ground_state, grid, dim3(256), 0, s->stream, g, (const int *)ground, (const uint32_t *)P.n_obst, state, tally());
        launches += 2;
    }
    void clearance()
    {
        hipLaunchKernelGGL(k_ground_columns, dim3((g.nu + 255) / 256), dim3(256), 0, s->stream, g, (const uint8_t *)state, gcol);
        hipLaunchKernelGGL(k_ground_rows, dim3((g.nu + 255) / 256, g.nv), dim3(256), 0, s->stream, g, (const uint8_t *)gcol, clear2);
        launches += 2;
    }
};

}  // namespace

extern "C" {

int sm_default_ground_params(sm_ground_params *p)
{
    if (!p) { g_err = "sm_default_ground_params: null argument"; return SM_E_ARG; }
    *p = sm_ground_params{};
    p->cell_mm = 100;
    p->up = 3;
    p->nu = p->nv = 256;
    p->min_up = 11585;
    for (uint32_t &w : p->ground_mask) w = 0xFFFFFFFFu;
    p->band_mm = 200;
    p->clear_lo_mm = 150;
    p->clear_hi_mm = 2000;
    p->min_obstacle = 2;
    p->fill_cells = 3;
    p->step_mm = 150;
    p->reach_cells = 32;
    p->unknown_blocks = 0;
    p->normal_sign = -1;
    return SM_OK;
}

int sm_ground_maps(sm_ctx *s, const sm_map_source *src, const sm_ground_params *p, int32_t *ground, int32_t *top, uint8_t *state, uint8_t *cls,
                   uint8_t *bgr, uint32_t *clear2, sm_ground_info *info)
{
    const char *who = "sm_ground_maps";
    SetCall call(s, src, who);
    if (!s || !src || !p || !info) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    int rc;
    if ((rc = call.open([&] { return check_params(p, who); }))) return rc;
    sm_mapset::ReadSet &set = call.set;
    const uint32_t cnt = call.cnt;
    const uint64_t total = call.total;

    GroundJob job(s, ground_args(*p));
    const GroundArgs &g = job.g;
    sm_ground_stats_t &st = job.stats;
    sm_ground_info got{};
    got.records = total;

    // ---- the files no record of which can lie in the window leave the chunk plan; their ids stay
    uint64_t skipped_records = 0;
    if (sm_mapset::FileIndex::lookups_on()) {
        std::vector<char> skip(src->n_paths, 0);
        for (uint32_t i = 0; i < src->n_paths; ++i) {
            sm_mapfile::Header now;
            const sm_mapset::FileIndex::Entry *e = s->index.valid(src->paths[i], now);
            if (e && box_misses_window(*e, g)) { skip[i] = 1; st.files_skipped++; skipped_records += set.files[i].count; }
        }
        if (st.files_skipped)
            set.jobs.erase(std::remove_if(set.jobs.begin(), set.jobs.end(), [&](const sm_mapfile::Job &j) { return skip[j.file] != 0; }), set.jobs.end());
    }

    Ground &gr = s->ground;
    const Event *ev = job.ev;
    if ((rc = job.open()) || (rc = call.model())) return rc;
    const float4 *d_model = call.d_model;
    if (!set.jobs.empty() && (rc = call.staging())) return rc;
    float &h2d_ms = call.copy_ms;

    // ---- reading 1: the lowest ground-like record of every cell; then the reference heights
    if ((rc = maps_feed(s, who, set, src->paths, cnt, d_model, {&st.read_ms, &h2d_ms, &st.ground_ms}, ev[EV_MIN0],
                        [&](const float4 *d_rec, uint32_t n, uint32_t) { job.lowest(d_rec, n); })))
        return rc;
    if ((rc = mark(s, ev[EV_MIN1])) || (rc = mark(s, ev[EV_FILL0]))) return rc;
    job.fill();
    if ((rc = mark(s, ev[EV_FILL1]))) return rc;
    HIPCK(hipGetLastError());
    if ((rc = add_marked(&ev[EV_CLR0], &st.ground_ms)) || (rc = add_marked(&ev[EV_MIN0], &st.ground_ms)) ||
        (rc = add_marked(&ev[EV_FILL0], &st.fill_ms)))
        return rc;

    // ---- reading 2: the ground's sums and the obstacles
    if ((rc = maps_feed(s, who, set, src->paths, cnt, d_model, {&st.read_ms, &h2d_ms, &st.accumulate_ms}, ev[EV_ACC0],
                        [&](const float4 *d_rec, uint32_t n, uint32_t gid0) { job.accumulate(d_rec, n, gid0); })))
        return rc;
    if ((rc = mark(s, ev[EV_ACC1])) || (rc = mark(s, ev[EV_STATE0]))) return rc;

    // ---- planes, states, clearance
    job.finish();
    if ((rc = mark(s, ev[EV_STATE1])) || (rc = mark(s, ev[EV_CLEAR0]))) return rc;
    if (clear2) job.clearance();
    if ((rc = mark(s, ev[EV_CLEAR1])) || (rc = gr.scratch.read(s))) return rc;
    if ((rc = add_marked(&ev[EV_ACC0], &st.accumulate_ms)) || (rc = add_marked(&ev[EV_STATE0], &st.state_ms)) ||
        (rc = add_marked(&ev[EV_CLEAR0], &st.clear_ms)))
        return rc;
    const uint32_t *h = gr.scratch.h();
    uint64_t seen = 0;
    for (int k = 0; k < GROUND_KINDS; ++k) { got.counts[k] = h[GROUND_COUNTS + k]; seen += got.counts[k]; }
    got.counts[GROUND_K_OUTSIDE] += skipped_records;
    if (seen + skipped_records != total) { g_err = std::string(who) + ": the set changed while it was read"; return SM_E_ARG; }
    for (int k = 0; k < GROUND_STATES; ++k) got.cells[k] = h[GROUND_CELLS + k];

    // ---- the planes asked for, one copy each (nothing has been written so far)
    const double t_copy = now_ms();
    const size_t N = job.N;
    const auto back = [&](void *dst, const void *d_src, size_t bytes) -> int {
        if (dst) HIPCK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, s->stream));
        return SM_OK;
    };
    if ((rc = back(ground, job.ground, N * 4)) || (rc = back(top, job.P.top, N * 4)) || (rc = back(state, job.state, N)) || (rc = back(cls, job.cls, N)) ||
        (rc = back(bgr, job.bgr, N * 3)) || (rc = back(clear2, job.clear2, N * 4)))
        return rc;
    HIPCK(hipStreamSynchronize(s->stream));
    st.copy_ms = (float)(now_ms() - t_copy);
    *info = got;
    st.launches = job.launches;
    st.total_ms = call.elapsed_ms();
    gr.stats = st;                                       // (a call that fails leaves the last one's)
    gr.stats_valid = true;
    return SM_OK;
}

SM_STATS_GETTER(sm_ground_stats, sm_ground_stats_t, ground, "sm_ground_maps")

}  // extern "C"
