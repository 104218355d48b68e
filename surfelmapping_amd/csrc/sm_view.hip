// sm_view.hip -- the model view: GlobalModel::renderModel's discs or points into an RGBA image (sm_render_model*).
// Kernels: sm_k_view.h.
#include "sm_ctx.h"
#include "sm_k_view.h"

using namespace sm;

int sm_impl::check_model_view(const sm_model_view *v, const char *fn)
{
    if (!v) { g_err = std::string(fn) + ": null view"; return SM_E_ARG; }
    if (v->width <= 0 || v->height <= 0 || (uint64_t)v->width * (uint64_t)v->height > (1u << 28)) {
        g_err = std::string(fn) + ": width and height must be positive, w*h at most 2^28"; return SM_E_ARG;
    }
    if (v->color_type < 0 || v->color_type > 3) { g_err = std::string(fn) + ": color_type is 0..3"; return SM_E_ARG; }
    return SM_OK;
}

void sm_impl::model_view_params(const sm_model_view *v, ViewParams &vp, ViewShade &vs)
{
    memcpy(vp.mvp, v->mvp, 64);
    memcpy(vp.mvinv, v->mv_inv, 64);
    vp.threshold = v->threshold;
    vp.unstable = v->draw_unstable ? 1 : 0;
    vp.points = v->draw_points ? 1 : 0;
    vp.w = v->width; vp.h = v->height;
    vp.fp_lane = 64;                                              // tuning constant: DESIGN.md "Model view" has the sweep
    if (const char *e = std::getenv("SM_RENDER_MODEL_LANE_PX")) vp.fp_lane = (uint32_t)std::max(0, std::atoi(e));
    vs.color_type = v->color_type;
    vs.window = (v->draw_window && !v->draw_points) ? 1 : 0;      // draw_feedback.vert has no window
    vs.time = v->time; vs.time_delta = v->time_delta;
    vs.clear = (uint32_t)v->clear_rgba[0] | ((uint32_t)v->clear_rgba[1] << 8) | ((uint32_t)v->clear_rgba[2] << 16) |
               ((uint32_t)v->clear_rgba[3] << 24);
}

int sm_impl::view_splat_model(sm_ctx *s, const ViewParams &vp, uint64_t *key, uint32_t *d_ovf_n, uint32_t *d_ovf, uint32_t id_base,
                              const Event *timing)
{
    const uint32_t cnt = s->h_state->count;
    HIPCK(hipMemsetAsync(d_ovf_n, 0, 4, s->stream));
    if (timing) HIPCK(hipEventRecord(timing[0], s->stream));
    if (cnt) hipLaunchKernelGGL(k_view_splat, dim3((cnt + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, vp, key, d_ovf_n, d_ovf, id_base);
    if (timing) HIPCK(hipEventRecord(timing[1], s->stream));
    if (cnt && !vp.points)
        hipLaunchKernelGGL(k_view_overflow, dim3(VIEW_OVF_BLOCKS), dim3(256), 0, s->stream, s->M, s->d_state, vp, key, d_ovf_n, d_ovf, id_base);
    if (timing) HIPCK(hipEventRecord(timing[2], s->stream));
    return SM_OK;
}

namespace {
// GlobalModel::renderModel (src/GlobalModel.cpp:683-758) into device memory (sm_k_view.h): keys [8 w h] | overflow length
// [256] | overflow list [4 count] in the export scratch; with `stage` (the host path) the images follow there too -- rgba,
// depth, id, w*h*4 bytes each -- and *stage points at them.  Changes neither the model nor the frame state; the forced
// compaction of ensure_compact is the one every read-back does.
int render_model_enqueue(sm_ctx *s, const sm_model_view *v, const char *fn, uint8_t **stage, uint8_t *d_rgba, float *d_depth,
                         int32_t *d_id)
{
    // (the view is checked before the context, so that each rule can be exercised without a device)
    if (int rc = check_model_view(v, fn)) return rc;
    if (!d_rgba && !stage) { g_err = std::string(fn) + ": null rgba"; return SM_E_ARG; }
    if (!s) { g_err = std::string(fn) + ": null context"; return SM_E_ARG; }
    if (!stage && (((uintptr_t)d_rgba | (uintptr_t)d_depth | (uintptr_t)d_id) & 3u)) {
        g_err = std::string(fn) + ": outputs must be 4-byte aligned"; return SM_E_ARG;
    }
    if (s->ss_on) { g_err = std::string(fn) + ": a sharded context holds only its rank's surfels; rendering the union is not supported"; return SM_E_UNSUPPORTED; }
    if (int rc = check_not_mid_cull(s, fn)) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = ensure_compact(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;                          // (waits for frames in flight; count is the live surfels)
    const uint32_t cnt = s->h_state->count;
    const size_t npix = (size_t)v->width * v->height;
    const size_t ovf_off = npix * 8, list_off = ovf_off + 256, extra_off = list_off + (((size_t)cnt * 4 + 255) & ~(size_t)255);
    if ((rc = ensure_export(s, extra_off + (stage ? npix * 12 : 0)))) return rc;
    uint8_t *base = (uint8_t *)s->d_export.get();
    uint64_t *d_key = (uint64_t *)base;
    uint32_t *d_ovf_n = (uint32_t *)(base + ovf_off), *d_ovf = (uint32_t *)(base + list_off);
    if (stage) {
        *stage = base + extra_off;
        d_rgba = *stage;
        if (d_depth) d_depth = (float *)(*stage + npix * 4);
        if (d_id) d_id = (int32_t *)(*stage + npix * 8);
    }
    ViewParams vp;
    ViewShade vs;
    model_view_params(v, vp, vs);
    const char *te = std::getenv("SM_RENDER_MODEL_TIMING");
    s->rm.timed = te && te[0] == '1';
    if (s->rm.timed && !s->rm.ev[0]) {
        Event ev[4];
        for (Event &e : ev) HIPCK(hipEventCreate(e.put()));
        std::move(std::begin(ev), std::end(ev), s->rm.ev);
    }
    const unsigned pblocks = (unsigned)((npix + 255) / 256);
    fill_keys(s, d_key, npix);
    if ((rc = view_splat_model(s, vp, d_key, d_ovf_n, d_ovf, 0u, s->rm.timed ? s->rm.ev : nullptr))) return rc;
    hipLaunchKernelGGL(k_view_resolve, dim3(pblocks), dim3(256), 0, s->stream, s->M, s->d_state, vs, d_key, (int)npix,
                       (uint32_t *)d_rgba, d_depth, d_id);
    if (s->rm.timed) HIPCK(hipEventRecord(s->rm.ev[3], s->stream));
    HIPCK(hipGetLastError());
    s->rm.ovf_off = ovf_off;
    s->rm.ovf_valid = true;
    return SM_OK;
}
}  // namespace

extern "C" {

int sm_render_model(sm_ctx *s, const sm_model_view *v, uint8_t *rgba, float *depth, int32_t *id)
{
    uint8_t *stage = nullptr;
    // (rgba / depth / id only say which images are wanted: the staging area receives them)
    int rc = render_model_enqueue(s, v, "sm_render_model", rgba ? &stage : nullptr, nullptr, depth, id);
    if (rc) return rc;
    const size_t npix = (size_t)v->width * v->height;
    HIPCK(hipMemcpyAsync(rgba, stage, npix * 4, hipMemcpyDeviceToHost, s->stream));
    if (depth) HIPCK(hipMemcpyAsync(depth, stage + npix * 4, npix * 4, hipMemcpyDeviceToHost, s->stream));
    if (id) HIPCK(hipMemcpyAsync(id, stage + npix * 8, npix * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

int sm_render_model_device(sm_ctx *s, const sm_model_view *v, uint8_t *d_rgba, float *d_depth, int32_t *d_id)
{
    return render_model_enqueue(s, v, "sm_render_model_device", nullptr, d_rgba, d_depth, d_id);
}

// Diagnostic, deliberately not part of include/sm_c_api.h (tools/render_model_probe.py, tests/test_render_model.py): waits
// for the context's stream; `overflow` = surfels the last sm_render_model* call rasterised on the overflow path (the count
// lives in the export scratch: SM_E_ARG if another read-back has reused it since), `ms3` = its splat / overflow / resolve
// kernel times when SM_RENDER_MODEL_TIMING=1 was set for that call, else -1.
int sm_debug_render_model_stats(sm_ctx *s, uint32_t *overflow, float *ms3)
{
    if (!s) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipStreamSynchronize(s->stream));
    if (!s->rm.ovf_valid) { g_err = "sm_debug_render_model_stats: no model view since the last reuse of the export scratch"; return SM_E_ARG; }
    if (overflow) HIPCK(hipMemcpy(overflow, (uint8_t *)s->d_export.get() + s->rm.ovf_off, 4, hipMemcpyDeviceToHost));
    if (ms3)
        for (int i = 0; i < 3; ++i) {
            ms3[i] = -1.0f;
            if (s->rm.timed) HIPCK(hipEventElapsedTime(&ms3[i], s->rm.ev[i], s->rm.ev[i + 1]));
        }
    return SM_OK;
}

}  // extern "C"
