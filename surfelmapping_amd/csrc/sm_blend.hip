// sm_blend.hip -- blended novel views (DESIGN.md "4o. Blended views"): the accumulation of the visible layer's fragments over a
// finished key map and its normalisation, as a stage of the two render paths (sm_model_io.hip, sm_render_maps.hip); the entry points
// sm_render_image_blend and sm_render_image_maps_blend, the stage's scratch and its tally (sm_blend_stats).  Kernels: sm_k_blend.h.
#include "sm_ctx.h"
#include "sm_k_blend.h"

using namespace sm;

int sm_impl::check_blend_params(const sm_blend_params *p, const char *who)
{
    if (!p) return SM_OK;
    const char *why = (p->depth_tol_256 < 0 || p->depth_tol_256 > 255) ? "depth_tol_256 is outside 0..255"
                    : (p->falloff < 0 || p->falloff > 2) ? "falloff is outside 0..2" : nullptr;
    if (why) { g_err = std::string(who) + ": " + why; return SM_E_ARG; }
    return SM_OK;
}

void sm_impl::blend_begin(sm_ctx *s)
{
    s->blend.stats = sm_blend_stats_t{};
    s->blend.stats_valid = true;
}

int sm_impl::blend_clear(sm_ctx *s, size_t pixels)
{
    Blend &b = s->blend;
    const size_t need = ((size_t)BLEND_TALLY_WORDS + pixels * 4) * sizeof(blend_u64);
    if (need > b.bytes) {
        HIPCK(hipStreamSynchronize(s->stream));
        b.bytes = 0;
        HIPCK(hipMalloc((void **)b.d_scratch.put(), need));
        b.bytes = need;
    }
    HIPCK(hipMemsetAsync(b.d_scratch, 0, need, s->stream));
    return SM_OK;
}

int sm_impl::blend_mark(sm_ctx *s)
{
    Blend &b = s->blend;
    if (!b.ev[1]) { HIPCK(hipEventCreate(b.ev[0].put())); HIPCK(hipEventCreate(b.ev[1].put())); }
    HIPCK(hipEventRecord(b.ev[0], s->stream));
    return SM_OK;
}

void sm_impl::blend_accum_model(sm_ctx *s, const sm_blend_params &p, const RenderParams &rp, const uint64_t *d_key, size_t acc_pixel)
{
    const uint32_t cnt = s->h_state->count;
    if (!cnt) return;
    blend_u64 *tally = s->blend.d_scratch, *acc = tally + BLEND_TALLY_WORDS + acc_pixel * 4;
    hipLaunchKernelGGL(k_blend_accum, dim3((cnt + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, rp, d_key, acc,
                       256u + (uint32_t)p.depth_tol_256, p.falloff, tally);
    s->blend.stats.launches++;
}

void sm_impl::blend_accum_chunk(sm_ctx *s, const sm_blend_params &p, uint32_t n, const RenderParams *d_rps, const uint64_t *d_key,
                                size_t npix, uint32_t views, int cull)
{
    blend_u64 *tally = s->blend.d_scratch, *acc = tally + BLEND_TALLY_WORDS;
    const MapStaging &st = s->staging;
    const MapsSoA chunk{st.d_pos_conf, st.d_norm_rad, st.d_color, st.d_time};
    hipLaunchKernelGGL(k_maps_blend_accum, dim3((n + MAPS_BLOCK - 1) / MAPS_BLOCK, views), dim3(256), 0, s->stream, chunk, n,
                       (const float4 *)st.d_box.get(), d_rps, d_key, npix, cull, acc, 256u + (uint32_t)p.depth_tol_256, p.falloff, tally);
    s->blend.stats.launches++;
}

int sm_impl::blend_normalise(sm_ctx *s, const uint64_t *d_key, size_t npix, uint32_t views, uint8_t *d_bgr, const uint8_t *d_sem)
{
    blend_u64 *tally = s->blend.d_scratch;
    hipLaunchKernelGGL(k_blend_normalise, dim3((unsigned)((npix + 255) / 256), views), dim3(256), 0, s->stream, d_key, npix,
                       tally + BLEND_TALLY_WORDS, d_bgr, d_sem, tally);
    s->blend.stats.launches++;
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(s->blend.ev[1], s->stream));
    return SM_OK;
}

void sm_impl::blend_add_ms(sm_ctx *s, float ms) { s->blend.stats.device_ms += ms; }

int sm_impl::blend_fold(sm_ctx *s)
{
    Blend &b = s->blend;
    blend_u64 t[3];
    HIPCK(hipMemcpyAsync(t, b.d_scratch, sizeof(t), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    b.stats.contributions += t[0]; b.stats.drawn += t[1]; b.stats.changed += t[2];
    float ms = 0.0f;
    HIPCK(hipEventElapsedTime(&ms, b.ev[0], b.ev[1]));
    b.stats.device_ms += ms;
    return SM_OK;
}

extern "C" {

int sm_default_blend_params(sm_blend_params *p)
{
    if (!p) { g_err = "sm_default_blend_params: null argument"; return SM_E_ARG; }
    p->depth_tol_256 = 13;
    p->falloff = 2;
    return SM_OK;
}

int sm_render_image_blend(sm_ctx *s, const float *view16, int w, int h, float fx, float fy, float cx, float cy, const sm_blend_params *blend,
                          const sm_fill_params *fill, uint8_t *bgr_out, uint8_t *sem_out, uint16_t *depth_mm_out)
{
    const char *who = "sm_render_image_blend";
    if (!blend) return sm_render_image_ex(s, view16, w, h, fx, fy, cx, cy, fill, bgr_out, sem_out, depth_mm_out);
    if (!s) { g_err = std::string(who) + ": null context"; return SM_E_ARG; }
    int rc;
    if ((rc = check_whole_map(s, who)) || (rc = check_blend_params(blend, who)) || (rc = check_fill_params(fill, who))) return rc;
    return render_image(s, view16, w, h, fx, fy, cx, cy, blend, fill, bgr_out, sem_out, depth_mm_out, who);
}

int sm_render_image_maps_blend(sm_ctx *s, const sm_map_source *src, const float *views16, uint32_t n_views, int w, int h, float fx, float fy,
                               float cx, float cy, const sm_blend_params *blend, const sm_fill_params *fill, uint8_t *bgr_out,
                               uint8_t *sem_out, uint16_t *depth_mm_out)
{
    const char *fn = "sm_render_image_maps_blend";
    if (!blend) return sm_render_image_maps_ex(s, src, views16, n_views, w, h, fx, fy, cx, cy, fill, bgr_out, sem_out, depth_mm_out);
    int rc;
    if (s && (rc = check_whole_map(s, fn))) return rc;
    if ((rc = check_blend_params(blend, fn)) || (rc = check_fill_params(fill, fn))) return rc;
    return render_image_maps(s, src, views16, n_views, w, h, fx, fy, cx, cy, blend, fill, bgr_out, sem_out, depth_mm_out, fn);
}

int sm_blend_stats(sm_ctx *s, sm_blend_stats_t *out)
{
    if (!s || !out) { g_err = "sm_blend_stats: null argument"; return SM_E_ARG; }
    if (!s->blend.stats_valid) { g_err = "sm_blend_stats: no blended call yet"; return SM_E_ARG; }
    *out = s->blend.stats;
    return SM_OK;
}

}  // extern "C"
