// sm_register.hip -- registration of one map set against another (sm_register_maps, sm_register_debug; DESIGN.md "4q.
// Registration"): the target set streamed once into one voxel table per level, the source set streamed once into resident
// samples, then the iterations enqueued whole.  Kernels: sm_k_register.h; the tables themselves: sm_voxel.h; the scratch and the
// export of a call: sm_set_call.h.
#include "sm_set_call.h"
#include "sm_k_register.h"
#include "sm_pose.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

constexpr uint32_t REG_MAX_SAMPLES = 1u << 28;
constexpr size_t REG_TALLY_WORDS = REG_MAX_LEVELS * SIMP_TALLY_WORDS + 1;    // per level a table's, then the regular samples
enum { EV_TGT0 = 0, EV_TGT1, EV_SRC0, EV_SRC1, EV_IT0, EV_IT1, EV_CLR0, EV_CLR1 };   // pairs of the scratch's events: add_marked(&ev[first])

int check_params(const sm_register_params *p, const char *who)
{
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (!p) return bad("null params");
    if (p->voxel_mm < 10 || p->voxel_mm > 10000) return bad("voxel_mm outside 10..10000");
    if (p->levels < 1 || p->levels > SM_REGISTER_MAX_LEVELS) return bad("levels outside 1..4");
    if (p->max_iters < 1 || p->max_iters > SM_TRACK_MAX_ITERS) return bad("max_iters outside 1..100");
    if (p->min_inliers < 0) return bad("min_inliers is negative");
    if (!(p->angle_thresh > 0.0f && p->angle_thresh < 90.0f)) return bad("angle_thresh outside (0, 90)");
    if (!(p->reach_cells > 0.0f) || !std::isfinite(p->reach_cells)) return bad("reach_cells is not a positive number");
    if (p->max_samples < 1 || p->max_samples > REG_MAX_SAMPLES) return bad("max_samples outside 1..2^28");
    if (p->max_cells == 0) return bad("max_cells is 0");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k]) || !std::isfinite(p->pivot[k])) return bad("non-finite origin or pivot");
    return SM_OK;
}

// One call's device side: the tables of all levels, the samples, the kernel arguments.
struct RegisterJob {
    sm_ctx *s;
    Register &rg;
    const Event *ev;
    const char *who;
    const sm_register_params &p;
    LookupTable t[REG_MAX_LEVELS];
    Dev<uint8_t> tables;
    Dev<float4> pos, nrm;
    uint32_t stride = 1, n_samples = 0;
    uint32_t launches = 0;

    RegisterJob(sm_ctx *s_, const char *who_, const sm_register_params &p_) : s(s_), rg(s_->reg), ev(s_->reg.scratch.ev), who(who_), p(p_) {}
    uint32_t *regular() const { return rg.scratch.d_tally.get() + REG_MAX_LEVELS * SIMP_TALLY_WORDS; }

    int open(uint64_t target_records, uint64_t source_records)
    {
        stride = p.stride ? p.stride : (uint32_t)std::max<uint64_t>(1, (source_records + p.max_samples - 1) / p.max_samples);
        const uint64_t ns = (source_records + stride - 1) / stride;
        if (ns > REG_MAX_SAMPLES) { g_err = std::string(who) + ": more than 2^28 samples"; return SM_E_CAPACITY; }
        if (ns > p.max_samples) { g_err = std::string(who) + ": stride leaves more than max_samples samples"; return SM_E_ARG; }
        n_samples = (uint32_t)ns;
        int rc;
        // (beside the scratch a call keeps the partial sums, the state and its pinned mirror on its context)
        if ((rc = rg.scratch.ensure(REG_TALLY_WORDS)) || (!rg.d_part && (rc = dalloc(rg.d_part, (size_t)TRACK_NSYS * TRACK_MAX_PARTS))) ||
            (!rg.d_state && (rc = dalloc(rg.d_state, 1))))
            return rc;
        if (!rg.h_state) HIPCK(hipHostMalloc((void **)rg.h_state.put(), sizeof(RegState), hipHostMallocDefault));
        if ((rc = dalloc(pos, n_samples)) || (rc = dalloc(nrm, n_samples))) return rc;
        uint64_t S;
        if ((rc = voxel_slots(target_records, p.max_cells, who, "a table", S))) return rc;
        for (int l = 0; l < p.levels; ++l) t[l].a = voxel_args(p.voxel_mm, l, p.origin, 1, p.max_cells);
        if ((rc = lut_open(tables, t, p.levels, S, false, rg.scratch.d_tally.get()))) return rc;
        // the tables' initialisation is device time of theirs (table_ms)
        if ((rc = mark(s, ev[EV_CLR0])) || (rc = lut_clear(s, t, p.levels)) || (rc = rg.scratch.clear(s->stream))) return rc;
        return mark(s, ev[EV_CLR1]);
    }
    // n <= CHUNK records of the target into every level's table, the class taken as 0
    void insert(const float4 *d_rec, uint32_t n)
    {
        for (int l = 0; l < p.levels; ++l) lut_insert(s, t[l], d_rec, n, 0, launches);
        rg.stats.chunks++;
    }
    void finish()
    {
        for (int l = 0; l < p.levels; ++l) lut_finish(s, t[l], launches);
    }
    // n <= CHUNK records of the source with ids gid0 ..
    void gather(const float4 *d_rec, uint32_t n, uint32_t gid0)
    {
        hipLaunchKernelGGL(k_register_gather, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, gid0, stride, pos.get(), nrm.get(), regular());
        launches++;
        rg.stats.chunks++;
    }
    RegParams params() const
    {
        RegParams rp{};
        for (int l = 0; l < p.levels; ++l) {
            rp.lv[l].lut = t[l].lut;
            rp.lv[l].mask = t[l].T.mask;
            rp.lv[l].V = t[l].a.V;
            rp.lv[l].reach = (double)p.reach_cells * ((double)t[l].a.V * (1.0 / 65536.0));
        }
        rp.levels = p.levels;
        for (int k = 0; k < 3; ++k) { rp.origin[k] = p.origin[k]; rp.pivot[k] = (double)p.pivot[k]; }
        rp.cos_angle = std::cos((double)p.angle_thresh * (3.14159265358979323846 / 180.0));
        rp.n_samples = n_samples;
        rp.nb = (int)std::min<long>(TRACK_MAX_PARTS, std::max<long>(1, ((long)n_samples + TRACK_BLOCK * 4 - 1) / (TRACK_BLOCK * 4)));
        rp.min_inliers = (uint32_t)p.min_inliers;
        rp.max_iters = p.max_iters;
        rp.degenerate_bound = SM_TRACK_DEGENERATE_BOUND;
        return rp;
    }
    void iteration(const RegParams &rp, int sum_only)
    {
        hipLaunchKernelGGL(k_register_reduce, dim3(rp.nb), dim3(TRACK_BLOCK), 0, s->stream, rp, (const float4 *)pos.get(), (const float4 *)nrm.get(),
                           (const RegState *)rg.d_state.get(), rg.d_part.get());
        hipLaunchKernelGGL(k_register_solve, dim3(1), dim3(256), 0, s->stream, rp, (const double *)rg.d_part.get(), rg.d_state.get(), sum_only);
        launches += 2;
    }
};

// Both entry points.  level < 0: sm_register_maps (pose16 the guess, null = identity); else sm_register_debug (pose16 the pose of
// the one system on `level`).
int register_run(sm_ctx *s, const sm_map_source *source, const sm_map_source *target, const float *pose16, int32_t level,
                 const sm_register_params *p, float *pose16_out, sm_register_info *info, double *sys29, uint32_t *n_samples_out, const char *who)
{
    const double t_begin = now_ms();
    const bool debug = level >= 0;
    int rc;
    if ((rc = check_whole_map(s, who)) || (rc = check_params(p, who)) || (rc = check_not_mid_cull(s, who)) || (rc = check_pose(pose16, who))) return rc;
    if (debug && level >= p->levels) { g_err = std::string(who) + ": level outside 0 .. levels - 1"; return SM_E_ARG; }
    sm_mapset::ReadSet sset, tset;
    if ((rc = check_sets(source, target, who)) || (rc = open_sets(source, target, who, sset, tset))) return rc;
    const sm_map_source *const srcs[2] = {source, target};
    const sm_mapset::ReadSet *const sets[2] = {&sset, &tset};
    uint32_t live[2];
    if ((rc = maps_counts(s, who, 2, srcs, sets, live))) return rc;
    const uint32_t scnt = live[0], tcnt = live[1];
    const uint64_t stotal = sset.file_total + scnt, ttotal = tset.file_total + tcnt;

    Register &rg = s->reg;
    rg.stats = sm_register_stats_t{};
    rg.stats_valid = true;
    rg.stats.source_records = stotal;
    rg.stats.target_records = ttotal;
    float guess[16];
    if (pose16) memcpy(guess, pose16, 64);
    else sm_pose::identity(guess);
    sm_register_info out{};
    out.status = SM_REGISTER_OK;

    RegisterJob job(s, who, *p);
    if ((rc = job.open(ttotal, stotal))) return rc;
    out.stride = job.stride;
    if (n_samples_out) *n_samples_out = job.n_samples;
    const Event *ev = job.ev;
    const float4 *d_model;
    if ((rc = maps_export(s, std::max(scnt, tcnt), d_model))) return rc;
    if (sset.jobs.size() + tset.jobs.size())
        if ((rc = maps_ensure_staging(s))) return rc;
    float copy_ms = 0.0f;
    const MapStream::Tally times = {&rg.stats.read_ms, &copy_ms, &rg.stats.table_ms};
    // ---- the target: every chunk into every level's table, then the representatives
    if ((rc = maps_feed(s, who, tset, target->paths, tcnt, d_model, times, ev[EV_TGT0],
                        [&](const float4 *d_rec, uint32_t n, uint32_t) { job.insert(d_rec, n); })))
        return rc;
    job.finish();
    if ((rc = mark(s, ev[EV_TGT1]))) return rc;
    // ---- the source: the samples to their places
    if ((rc = maps_feed(s, who, sset, source->paths, scnt, d_model, times, ev[EV_SRC0],
                        [&](const float4 *d_rec, uint32_t n, uint32_t gid0) { job.gather(d_rec, n, gid0); })))
        return rc;
    if ((rc = mark(s, ev[EV_SRC1])) || (rc = rg.scratch.read(s))) return rc;
    for (int pair : {EV_CLR0, EV_TGT0, EV_SRC0})
        if ((rc = add_marked(&ev[pair], &rg.stats.table_ms))) return rc;
    const uint32_t *h = rg.scratch.h();
    for (int l = 0; l < p->levels; ++l) {
        if ((rc = voxel_check_tally(h + l * SIMP_TALLY_WORDS, p->max_cells, who, "keys at level " + std::to_string(l)))) return rc;
        out.cells[l] = h[l * SIMP_TALLY_WORDS + SIMP_CELLS];
        if (out.cells[l] == 0) out.status = SM_REGISTER_NO_TARGET;
    }
    out.samples = h[REG_MAX_LEVELS * SIMP_TALLY_WORDS];
    if (out.status == SM_REGISTER_OK && out.samples == 0) out.status = SM_REGISTER_NO_SOURCE;

    RegState &hs = *rg.h_state;
    memset(&hs, 0, sizeof hs);
    if (out.status == SM_REGISTER_OK || debug) {
        // ---- the iterations, enqueued whole; the one wait follows the last
        const RegParams rp = job.params();
        for (int e = 0; e < 16; ++e) hs.T[e] = hs.guess[e] = (double)guess[e];
        if (!debug) sm_pose::orthonormalize_d(hs.T);
        hs.level = debug ? level : p->levels - 1;
        HIPCK(hipMemcpyAsync(rg.d_state.get(), &hs, sizeof hs, hipMemcpyHostToDevice, s->stream));
        if ((rc = mark(s, ev[EV_IT0]))) return rc;
        if (debug) job.iteration(rp, 1);
        else
            for (int i = 0; i < p->levels * p->max_iters; ++i) job.iteration(rp, 0);
        HIPCK(hipGetLastError());
        if ((rc = mark(s, ev[EV_IT1]))) return rc;
        HIPCK(hipMemcpyAsync(&hs, rg.d_state.get(), sizeof hs, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        if ((rc = add_marked(&ev[EV_IT0], &rg.stats.iterate_ms))) return rc;
    }
    if (debug) {
        for (int e = 0; e < TRACK_NSYS; ++e) sys29[e] = hs.sys[e];
    } else {
        if (out.status == SM_REGISTER_OK) {
            out.status = hs.status;
            for (int l = 0; l < REG_MAX_LEVELS; ++l) out.iterations[l] = hs.iters[l];
            out.inliers = hs.inliers;
            out.rmse = (float)hs.rmse;
            out.pivot_ratio = (float)hs.pivot_ratio;
        }
        for (int e = 0; e < 16; ++e) pose16_out[e] = out.status == SM_REGISTER_OK ? (float)hs.T[e] : guess[e];
        *info = out;
    }
    rg.stats.launches = job.launches;
    rg.stats.total_ms = (float)(now_ms() - t_begin);
    return SM_OK;
}

}  // namespace

extern "C" {

int sm_default_register_params(sm_register_params *p)
{
    if (!p) { g_err = "sm_default_register_params: null argument"; return SM_E_ARG; }
    *p = sm_register_params{};
    p->voxel_mm = 200;
    p->levels = 3;
    p->max_iters = 20;
    p->min_inliers = 1000;
    p->angle_thresh = 30.0f;
    p->reach_cells = 1.0f;
    p->stride = 0;
    p->max_samples = 1u << 22;
    p->max_cells = 1u << 24;
    return SM_OK;
}

int sm_register_maps(sm_ctx *s, const sm_map_source *source, const sm_map_source *target, const float *guess16, const sm_register_params *p,
                     float *pose16_out, sm_register_info *info)
{
    const char *who = "sm_register_maps";
    if (!s || !source || !target || !p || !pose16_out || !info) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    return register_run(s, source, target, guess16, -1, p, pose16_out, info, nullptr, nullptr, who);
}

int sm_register_debug(sm_ctx *s, const sm_map_source *source, const sm_map_source *target, const float *pose16_eval, int32_t level,
                      const sm_register_params *p, double *sys29, uint32_t *n_samples)
{
    const char *who = "sm_register_debug";
    if (!s || !source || !target || !pose16_eval || !p || !sys29 || !n_samples) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if (level < 0) { g_err = std::string(who) + ": level outside 0 .. levels - 1"; return SM_E_ARG; }
    return register_run(s, source, target, pose16_eval, level, p, nullptr, nullptr, sys29, n_samples, who);
}

SM_STATS_GETTER(sm_register_stats, sm_register_stats_t, reg, "sm_register_maps / sm_register_debug")

}  // extern "C"
