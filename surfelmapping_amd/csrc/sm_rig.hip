// sm_rig.hip -- a rig of cameras, one per rank, consolidated into a single GlobalModel (sm_rig_*).
#include "sm_ctx.h"

using namespace sm;

namespace sm {

// first surfel (position in the compacted model) created after time stamp t0: the model is kept in creation order, so the
// surfels a rig rank has not yet contributed to the single GlobalModel are the suffix from there on (sm_rig_consolidate_step)
__global__ __launch_bounds__(256) void k_first_newer(Model M, const DevState *__restrict__ st, float t0, uint32_t *__restrict__ out)
{
    const uint32_t N = st->count;
    const float *__restrict__ it = M.s[st->cur].init_time;
    uint32_t best = 0xFFFFFFFFu;
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < N; k += gridDim.x * 256u)
        if (it[k] > t0) { best = k; break; }               // (k ascending per thread: its first hit is its smallest)
    best = 0xFFFFFFFFu - wave_max_u32(0xFFFFFFFFu - best);
    if ((threadIdx.x & 63) == 0 && best != 0xFFFFFFFFu) atomicMin(out, best);
}

}  // namespace sm

extern "C" {

// ---- BASELINE configs[4]: a rig of `world` cameras, one per rank, consolidated into a single GlobalModel ----
// Frames go through the ordinary entry points (no collective).  sm_rig_consolidate is the definition of DESIGN.md 6 --
// union in rank order, cleanPoints against every camera's latest view in rank order -- entirely on the device: the views,
// the slice sizes, the per-view conflict totals and the cleaned slices cross the ranks through the installed collective
// (RCCL's all-reduce, or a callback); an all-gather is the sum of buffers that are zero outside the sender's part.

int sm_rig_configure(sm_ctx *s, int rank, int world)
{
    if (!s || world < 1 || rank < 0 || rank >= world) return SM_E_ARG;
    if (s->ss_on) { g_err = "sm_rig_configure: the context is configured for sharding"; return SM_E_ARG; }
    s->rig_on = true; s->ss_rank = rank; s->ss_world = world;
    s->aloop.on = false;                                  // (sm_set_auto_loop: a rank holds only its own surfels)
    return SM_OK;
}

namespace {
// The exchanges of a rig consolidation.  Every rank contributes a row of four words -- live surfels of its slice, conflicts of
// the view at hand, a status word, a spare -- through an all-gather, so that (a) all ranks see all counts and (b) a rank whose
// LOCAL step failed says so in the very exchange the others are waiting in: everybody then leaves together with an error
// instead of one rank returning early and the rest blocking inside RCCL.
struct RigXchg {
    sm_ctx *s; int W, r;
    Dev<unsigned long long> d_cnt;                 // [W][4]
    std::vector<unsigned long long> h;
    RigXchg(sm_ctx *s_, int W_, int r_) : s(s_), W(W_), r(r_), h((size_t)W_ * 4) {}
    // returns 0, this rank's own failure code, or SM_E_HIP when another rank failed
    int run(unsigned long long count, unsigned long long conflicts, int status)
    {
        unsigned long long row[4] = {count, conflicts, (unsigned long long)(long long)status, 0ull};
        if (hipMemcpyAsync(d_cnt + (size_t)r * 4, row, 32, hipMemcpyHostToDevice, s->stream) != hipSuccess) return SM_E_HIP;
        int rc = ss_collective(s, d_cnt + (size_t)r * 4, d_cnt, 4, SM_COLL_GATHER);
        if (rc) return rc;
        if (hipMemcpyAsync(h.data(), d_cnt, 32 * (size_t)W, hipMemcpyDeviceToHost, s->stream) != hipSuccess) return SM_E_HIP;
        if (hipStreamSynchronize(s->stream) != hipSuccess) return SM_E_HIP;
        if (status) return status;
        for (int q = 0; q < W; ++q)
            if (h[(size_t)q * 4 + 2]) { g_err = "sm_rig_consolidate: rank " + std::to_string(q) + " failed (code " + std::to_string((long long)h[(size_t)q * 4 + 2]) + "); all ranks abandon the consolidation"; return SM_E_HIP; }
        return SM_OK;
    }
    unsigned long long count(int q) const { return h[(size_t)q * 4]; }
    unsigned long long conflicts(int q) const { return h[(size_t)q * 4 + 1]; }
};
}  // namespace

// The single GlobalModel DURING a run ("all-gather of per-GPU new-surfel lists into the single GlobalModel, followed by
// one conflict pass of every camera's depth against the union").  One step, collective:
//   1. every rank's NEW surfels -- created since its previous step, still alive, in creation order (the model is kept in creation
//      order, so they are a suffix of the compacted model) -- are all-gathered and appended to `global` in rank order
//      (GlobalModel::concatenate's order for W append lists), on every rank;
//   2. the cameras' latest views are all-gathered and `global` is cleaned against each of them in rank order with
//      SurfelMapping::cleanPoints (src/SurfelMapping.cpp:496-532) -- replicated: every rank holds the same GlobalModel, so the W*H
//      conflict cap and the id-0 rule need no exchange, and the work runs on `global`'s own stream, next to the camera's frames.
// The camera's own slice is not touched (its fusion goes on as if alone); what an older surfel of it becomes later -- fused
// updates, its own culls -- reaches `global` only through the views' conflict tests.  sm_rig_consolidate above is the exact
// end-of-run union; this is the incremental model, defined by the same reference operations (tests/test_rig.py states it on
// oracles).
int sm_rig_consolidate_step(sm_ctx *s, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16, sm_ctx *global,
                            uint32_t *new_surfels, uint32_t *global_count)
{
    if (!s || !depth_mm || !semantic || !pose16 || !global || !s->rig_on) { g_err = "sm_rig_consolidate_step: bad argument (sm_rig_configure first)"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (hip_runtime_conflict("sm_rig_consolidate_step")) return SM_E_HIP;
    const int W = s->ss_world, r = s->ss_rank;
    const size_t P = (size_t)s->P;
    const size_t off_sem = 2 * P, off_pose = (3 * P + 7) / 8 * 8, row = off_pose + 64;
    Dev<uint8_t> d_views;
    Dev<float> d_lists;
    Dev<uint32_t> d_first;
    RigXchg x(s, W, r);
    HIPCK(hipMalloc(x.d_cnt.put(), 32 * (size_t)W));
    // ---- local: compact (slots become positions), find the first surfel newer than the previous step, stage the view
    int st = ensure_compact(s);
    if (!st) st = pull_state(s);
    uint32_t cnt = 0, first = 0;
    if (!st) {
        cnt = s->h_state->count;
        first = cnt;
        if (hipMalloc(d_first.put(), 4) != hipSuccess || hipMemsetAsync(d_first, 0xFF, 4, s->stream) != hipSuccess) st = SM_E_HIP;
        if (!st && cnt) {
            hipLaunchKernelGGL(k_first_newer, dim3(std::min<uint32_t>((cnt + 255u) / 256u, 1024u)), dim3(256), 0, s->stream, s->M, s->d_state, s->rig_last_time, d_first);
            uint32_t f = 0xFFFFFFFFu;
            if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&f, d_first, 4, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
                hipStreamSynchronize(s->stream) != hipSuccess) st = SM_E_HIP;
            else first = std::min(f, cnt);
        }
    }
    const uint32_t n_new = st ? 0u : cnt - first;
    if (!st && hipMalloc(d_views.put(), row * (size_t)W) != hipSuccess) { g_err = "sm_rig_consolidate_step: out of device memory for the views"; st = SM_E_HIP; }
    if (!st && (hipMemsetAsync(d_views + row * r, 0, row, s->stream) != hipSuccess ||
                hipMemcpyAsync(d_views + row * r, depth_mm, 2 * P, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
                hipMemcpyAsync(d_views + row * r + off_sem, semantic, P, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
                hipMemcpyAsync(d_views + row * r + off_pose, pose16, 64, hipMemcpyHostToDevice, s->stream) != hipSuccess)) st = SM_E_HIP;
    int rc = x.run(n_new, 0ull, st);
    if (rc) return rc;
    // ---- 1. the new-surfel lists, all-gathered (padded to the longest) and appended to `global` in rank order
    unsigned long long T = 0, maxn = 0;
    std::vector<unsigned long long> nn((size_t)W);
    for (int q = 0; q < W; ++q) { nn[(size_t)q] = x.count(q); T += nn[(size_t)q]; maxn = std::max(maxn, nn[(size_t)q]); }
    if (new_surfels) *new_surfels = (uint32_t)T;
    st = SM_OK;
    if (T && hipMalloc(d_lists.put(), (size_t)maxn * 48 * (size_t)W) != hipSuccess) { g_err = "sm_rig_consolidate_step: out of device memory for the lists"; st = SM_E_HIP; }
    if ((rc = x.run(n_new, 0ull, st))) return rc;
    if (T) {
        if (n_new) export_aos(s, d_lists + (size_t)r * maxn * 12, first, n_new);
        if (hipGetLastError() != hipSuccess) return SM_E_HIP;
        if ((rc = ss_collective(s, d_lists + (size_t)r * maxn * 12, d_lists, (size_t)maxn * 6, SM_COLL_GATHER))) return rc;
    }
    if ((rc = ss_collective(s, d_views + row * r, d_views, row / 8, SM_COLL_GATHER))) return rc;
    std::vector<float> poses((size_t)W * 16);
    for (int v = 0; v < W; ++v)
        if (hipMemcpyAsync(&poses[(size_t)v * 16], d_views + row * v + off_pose, 64, hipMemcpyDeviceToHost, s->stream) != hipSuccess) return SM_E_HIP;
    if (hipStreamSynchronize(s->stream) != hipSuccess) return SM_E_HIP;
    for (int q = 0; q < W; ++q)
        if (nn[(size_t)q] && (rc = sm_append_model_aos_device(global, d_lists + (size_t)q * maxn * 12, (uint32_t)nn[(size_t)q]))) return rc;
    // ---- 2. the union cleaned against every camera's latest view, in rank order (the same work on every rank)
    for (int v = 0; v < W; ++v)
        if ((rc = clean_points_device(global, reinterpret_cast<const uint16_t *>(d_views + row * v), d_views + row * v + off_sem,
                                      &poses[(size_t)v * 16], 1))) return rc;
    if (global_count) *global_count = global->counts.count;
    s->rig_last_time = (float)(s->tick - 1);           // every surfel created so far carries a time stamp <= tick - 1
    return SM_OK;
}

int sm_rig_consolidate(sm_ctx *s, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16, sm_ctx *global,
                       uint32_t *view_conflicts, uint32_t *total_out)
{
    if (!s || !depth_mm || !semantic || !pose16 || !global || !s->rig_on) { g_err = "sm_rig_consolidate: bad argument (sm_rig_configure first)"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (hip_runtime_conflict("sm_rig_consolidate")) return SM_E_HIP;
    const int W = s->ss_world, r = s->ss_rank;
    const size_t P = (size_t)s->P;
    const size_t off_sem = 2 * P, off_pose = (3 * P + 7) / 8 * 8, row = off_pose + 64;        // bytes of one view (a multiple of 8)
    Dev<uint8_t> d_views;
    Dev<float> d_union;
    RigXchg x(s, W, r);
    // the exchange buffer first: without it this rank cannot even tell the others that it failed
    HIPCK(hipMalloc(x.d_cnt.put(), 32 * (size_t)W));
    // ---- local, fallible: settle the stream's pending work, stage this camera's latest view
    int st = finalize_if_pending(s);
    if (!st) st = pull_state(s);
    if (!st && hipMalloc(d_views.put(), row * (size_t)W) != hipSuccess) { g_err = "sm_rig_consolidate: out of device memory for the views"; st = SM_E_HIP; }
    if (!st && (hipMemsetAsync(d_views + row * r, 0, row, s->stream) != hipSuccess ||
                hipMemcpyAsync(d_views + row * r, depth_mm, 2 * P, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
                hipMemcpyAsync(d_views + row * r + off_sem, semantic, P, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
                hipMemcpyAsync(d_views + row * r + off_pose, pose16, 64, hipMemcpyHostToDevice, s->stream) != hipSuccess)) {
        g_err = "sm_rig_consolidate: staging the view failed"; st = SM_E_HIP;
    }
    int rc = x.run(st ? 0ull : s->counts.count, 0ull, st);
    if (rc) return rc;
    // ---- 1. every rank learns every camera's latest view: all-gather, in place (3 bytes per pixel and camera)
    if ((rc = ss_collective(s, d_views + row * r, d_views, row / 8, SM_COLL_GATHER))) return rc;
    std::vector<float> poses((size_t)W * 16);
    st = SM_OK;
    for (int v = 0; v < W && !st; ++v)
        if (hipMemcpyAsync(&poses[(size_t)v * 16], d_views + row * v + off_pose, 64, hipMemcpyDeviceToHost, s->stream) != hipSuccess) st = SM_E_HIP;
    if (!st && hipStreamSynchronize(s->stream) != hipSuccess) st = SM_E_HIP;
    // ---- 2. the union cleaned against every view, in rank order: each rank cleans ITS slice (the test is per surfel and view)
    for (int v = 0; v < W; ++v) {
        int first = -1;
        for (int q = 0; q < W && first < 0; ++q) if (x.count(q) > 0) first = q;
        unsigned long long view_total = 0;
        bool hook_ran = false;
        // Between the conflict test and the cull the ranks exchange their conflict counts: at most W*H conflicts take effect per
        // view, in the surfel order of the UNION (src/GlobalModel.cpp:54-57) -- slices are concatenated in rank order, so this
        // rank's share is what the lower ranks left of the W*H, and "the first `share` conflicts of my slice" is exactly the rule
        // the single-model cull applies with that cap.
        const std::function<long long(uint32_t)> hook = [&](uint32_t local) -> long long {
            hook_ran = true;
            const int e = x.run(s->counts.count, local, SM_OK);
            if (e) return e;
            unsigned long long before = 0;
            for (int q = 0; q < W; ++q) { if (q < r) before += x.conflicts(q); view_total += x.conflicts(q); }
            if (!s->cfg.conflict_cap) return 0xFFFFFFFFll;
            return before >= (unsigned long long)s->P ? 0ll : (long long)std::min<unsigned long long>(local, (unsigned long long)s->P - before);
        };
        // surfel id 0 never conflicts (conflict.geom:15): the exemption belongs to the rank that holds the union's first surfel
        const int cl = st ? st : clean_points_device(s, reinterpret_cast<const uint16_t *>(d_views + row * v), d_views + row * v + off_sem,
                                                     &poses[(size_t)v * 16], first == r ? 1 : 0, &hook);
        // every rank makes both exchanges of a view whatever happened to it locally: a failure travels in the status word
        if (!hook_ran) (void)x.run(0ull, 0ull, cl ? cl : SM_E_HIP);
        if ((rc = x.run(s->counts.count, 0ull, cl))) return rc;              // the slices' sizes after this view
        if (view_conflicts) view_conflicts[v] = (uint32_t)(s->cfg.conflict_cap ? std::min<unsigned long long>(view_total, (unsigned long long)s->P) : view_total);
    }
    // ---- 3. the cleaned slices, all-gathered (padded to the largest) and appended in rank order to `global` on every rank
    unsigned long long T = 0, maxcnt = 0;
    std::vector<unsigned long long> cnt((size_t)W);
    for (int q = 0; q < W; ++q) { cnt[(size_t)q] = x.count(q); T += cnt[(size_t)q]; maxcnt = std::max(maxcnt, cnt[(size_t)q]); }
    if (total_out) *total_out = (uint32_t)T;
    d_views = {};
    st = SM_OK;
    if (T && hipMalloc(d_union.put(), (size_t)maxcnt * 48 * (size_t)W) != hipSuccess) { g_err = "sm_rig_consolidate: out of device memory for the union"; st = SM_E_HIP; }
    if (!st) st = ensure_compact(s);
    if (!st) st = pull_state(s);
    if ((rc = x.run(cnt[(size_t)r], 0ull, st))) return rc;
    if (T == 0) return SM_OK;
    const uint32_t own = s->h_state->count;
    if (own) export_aos(s, d_union + (size_t)r * maxcnt * 12, 0u, own);
    if (hipGetLastError() != hipSuccess) { g_err = "sm_rig_consolidate: export kernel launch failed"; return SM_E_HIP; }   // (the others' all-gather then fails or stalls: a launch failure is not recoverable)
    if ((rc = ss_collective(s, d_union + (size_t)r * maxcnt * 12, d_union, (size_t)maxcnt * 6, SM_COLL_GATHER))) return rc;
    if (hipStreamSynchronize(s->stream) != hipSuccess) return SM_E_HIP;
    for (int q = 0; q < W; ++q)
        if (cnt[(size_t)q] && (rc = sm_append_model_aos_device(global, d_union + (size_t)q * maxcnt * 12, (uint32_t)cnt[(size_t)q]))) return rc;
    return SM_OK;
}

}  // extern "C"
