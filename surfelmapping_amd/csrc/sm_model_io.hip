// sm_model_io.hip -- the model and the frame's textures in and out of the core: AoS download / upload, map files, the index
// map, the raw feedback cloud, depth textures, the novel-view renderer (sm_render_image, sm_render_image_ex and the view behind sm_render_image_blend), caller device buffers, and the
// device-side export / append of sharded and rig runs.  Kernels: sm_k_io.h.
#include "sm_ctx.h"
#include "sm_k_io.h"
#include "sm_mapfile.h"

using namespace sm;

void sm_impl::export_aos(sm_ctx *s, float *dst12, uint32_t first, uint32_t n)
{
    hipLaunchKernelGGL(k_export_aos, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, dst12, first, n);
}

void sm_impl::import_aos(sm_ctx *s, const float *d_src12, uint32_t first, uint32_t n)
{
    if (n) hipLaunchKernelGGL(k_import_aos, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, d_src12, first, n);
}

void sm_impl::render_splat_model(sm_ctx *s, const RenderParams &rp, uint64_t *key, uint32_t id_base)
{
    const uint32_t cnt = s->h_state->count;
    if (cnt) hipLaunchKernelGGL(k_render_splat, dim3((cnt + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, rp, key, id_base);
}

// sm_render_image, and with fill or depth_mm_out what sm_render_image_ex adds to it: the view's depth plane from its keys, the
// completion of the three planes in place (sm_fill.hip) between the resolve and the copies; with blend what sm_render_image_blend
// adds: the colours of the visible layer blended over the resolve's (sm_blend.hip), ahead of the completion
int sm_impl::render_image(sm_ctx *s, const float *view16, int w, int h, float fx, float fy, float cx, float cy, const sm_blend_params *blend,
                          const sm_fill_params *fill, uint8_t *bgr_out, uint8_t *sem_out, uint16_t *depth_mm_out, const char *who)
{
    if (!s || !view16 || w <= 0 || h <= 0 || (uint64_t)w * h > (1u << 28) || !bgr_out || !sem_out) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    if (int rc = check_not_mid_cull(s, who)) return rc;
    int rc = ensure_compact(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;
    const size_t npix = (size_t)w * h;
    const bool depth = fill || depth_mm_out;
    if ((rc = ensure_export(s, npix * (depth ? 14 : 12)))) return rc;            // [keys u64 | bgr | sem | depth_mm u16]
    uint64_t *d_key = (uint64_t *)s->d_export.get();
    uint8_t *d_bgr = (uint8_t *)s->d_export.get() + npix * 8, *d_sem = d_bgr + npix * 3;
    uint16_t *d_depth = (uint16_t *)(d_sem + npix);
    RenderParams rp;
    invert4(view16, rp.t_inv);
    rp.fx = fx; rp.fy = fy; rp.cx = cx; rp.cy = cy; rp.cols = (float)w; rp.rows = (float)h; rp.w = w; rp.h = h;
    fill_keys(s, d_key, npix);
    render_splat_model(s, rp, d_key, 0u);
    hipLaunchKernelGGL(k_render_resolve, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s->stream, s->M, s->d_state, d_key,
                       (int)npix, d_bgr, d_sem);
    HIPCK(hipGetLastError());
    if (blend) {
        blend_begin(s);
        if ((rc = blend_mark(s)) || (rc = blend_clear(s, npix))) return rc;
        blend_accum_model(s, *blend, rp, d_key, 0);
        if ((rc = blend_normalise(s, d_key, npix, 1u, d_bgr, d_sem))) return rc;
    }
    if (depth) fill_key_depth(s, d_key, npix, d_depth);
    if (fill) {
        fill_begin(s);
        if ((rc = fill_enqueue(s, *fill, w, h, 1u, d_bgr, d_sem, d_depth))) return rc;
    }
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(bgr_out, d_bgr, npix * 3, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(sem_out, d_sem, npix, hipMemcpyDeviceToHost, s->stream));
    if (depth_mm_out) HIPCK(hipMemcpyAsync(depth_mm_out, d_depth, npix * 2, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    if (blend && (rc = blend_fold(s))) return rc;
    return fill ? fill_fold(s) : SM_OK;
}

extern "C" {

int sm_download_model_aos(sm_ctx *s, float *dst12, uint32_t cap, uint32_t *n)
{
    if (!s || !n) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = ensure_compact(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;
    const uint32_t cnt = s->pending_cull ? s->count_before_cull : s->h_state->count;
    *n = cnt;
    if (!dst12) return SM_OK;
    if (cap < cnt) { g_err = "sm_download_model_aos: destination too small"; return SM_E_CAPACITY; }
    if (int rc = check_not_mid_cull(s, "sm_download_model_aos")) return rc;
    const uint32_t CH = 1u << 22;                // 4 Mi surfels (192 MiB) per staging chunk
    if ((rc = ensure_export(s, (size_t)std::min(cnt, CH) * 48))) return rc;
    return drain_export(s, cnt, CH, dst12, 12, [s](float *d, uint32_t first, uint32_t m) { export_aos(s, d, first, m); }, no_hook);
}

int sm_upload_model_aos(sm_ctx *s, const float *src12, uint32_t n)
{
    if (!s || (!src12 && n)) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    if (n > s->cap) { g_err = "sm_upload_model_aos: exceeds MAX_VERTICES"; return SM_E_CAPACITY; }
    int rc = ensure_compact(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;
    const uint32_t CH = 1u << 22;
    if (n && (rc = ensure_export(s, (size_t)std::min(n, CH) * 48))) return rc;
    for (uint32_t first = 0; first < n; first += CH) {
        const uint32_t m = std::min(CH, n - first);
        HIPCK(hipMemcpyAsync(s->d_export, src12 + (size_t)first * 12, (size_t)m * 48, hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(k_import_aos, dim3((m + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, (const float *)s->d_export.get(), first, m);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(s->stream));
    }
    s->pending_cull = false;
    return publish_dense(s, n, 0);
}

// (a call that fails leaves no file at `path`, not a truncated one)
int sm_save_map(sm_ctx *s, const char *path, int32_t start_id, int32_t end_id)
{
    if (!s || !path) return SM_E_ARG;
    uint32_t n = 0;
    int rc = sm_download_model_aos(s, nullptr, 0, &n);
    if (rc) return rc;
    std::vector<float> buf((size_t)n * 12);
    if ((rc = sm_download_model_aos(s, buf.data(), n, &n))) return rc;
    sm_mapfile::Writer w;
    return w.open(path, n, start_id, end_id, nullptr, g_err) && w.append(buf.data(), n, g_err) && w.commit(g_err) ? SM_OK : SM_E_ARG;
}

int sm_load_map(sm_ctx *s, const char *path, int32_t *start_id, int32_t *end_id)
{
    if (!s || !path) return SM_E_ARG;
    sm_mapfile::Header h;
    sm_mapfile::File f = sm_mapfile::open_checked(path, nullptr, h, g_err, true);
    if (!f) return SM_E_ARG;
    if (h.count > s->cap) { g_err = "map larger than MAX_VERTICES"; return SM_E_CAPACITY; }
    std::vector<float> buf((size_t)h.count * 12);
    if (!sm_mapfile::read_rows(f.get(), buf.data(), h.count)) { g_err = std::string(path) + " read err!!"; return SM_E_ARG; }
    if (start_id) *start_id = h.start_id;
    if (end_id) *end_id = h.end_id;
    return sm_upload_model_aos(s, buf.data(), h.count);
}

int sm_download_index_map(sm_ctx *s, int32_t *id, float *vert_conf4, float *color_time4, float *norm_rad4)
{
    if (!s) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    const size_t P = (size_t)s->P;
    int rc = ensure_compact(s);
    if (rc) return rc;
    if ((rc = ensure_export(s, P * 52))) return rc;
    char *base = (char *)s->d_export.get();
    int32_t *d_id = (int32_t *)(base + P * 48);
    float4 *d_vc = (float4 *)base, *d_ct = (float4 *)(base + P * 16), *d_nr = (float4 *)(base + P * 32);
    FrameParams fp = make_params(s, s->curr_pose);
    hipLaunchKernelGGL(k_export_index, dim3((s->P + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, fp, s->keyT(), d_id, d_vc, d_ct, d_nr);
    HIPCK(hipGetLastError());
    if (id) HIPCK(hipMemcpyAsync(id, d_id, P * 4, hipMemcpyDeviceToHost, s->stream));
    if (vert_conf4) HIPCK(hipMemcpyAsync(vert_conf4, d_vc, P * 16, hipMemcpyDeviceToHost, s->stream));
    if (color_time4) HIPCK(hipMemcpyAsync(color_time4, d_ct, P * 16, hipMemcpyDeviceToHost, s->stream));
    if (norm_rad4) HIPCK(hipMemcpyAsync(norm_rad4, d_nr, P * 16, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

int sm_download_raw_cloud(sm_ctx *s, float *dst12, uint32_t cap, uint32_t *n)
{
    if (!s || !n) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    *n = 0;
    if (!s->raw_valid) return SM_OK;                     // nothing computed yet (the reference's buffer is empty before the 2nd frame)
    const size_t P = (size_t)s->P;
    int rc = ensure_export(s, P * 49);
    if (rc) return rc;
    float4 *d_rec = (float4 *)s->d_export.get();
    uint8_t *d_flag = (uint8_t *)s->d_export.get() + P * 48;
    FrameParams fp = make_params(s, s->curr_pose);
    fp.init_mode = 1;
    fp.time = s->raw_tick;
    hipLaunchKernelGGL(k_raw_cloud, dim3((s->P + 255) / 256), dim3(256), 0, s->stream, fp, s->cur().depthT, s->cur().rgbsT, s->d_xs, s->d_ys, d_rec, d_flag);
    HIPCK(hipGetLastError());
    std::vector<uint8_t> flag(P);
    HIPCK(hipMemcpyAsync(flag.data(), d_flag, P, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    uint32_t cnt = 0;
    for (size_t q = 0; q < P; ++q) cnt += flag[q];
    *n = cnt;
    if (!dst12) return SM_OK;
    if (cap < cnt) { g_err = "sm_download_raw_cloud: destination too small"; return SM_E_CAPACITY; }
    std::vector<float> rec(P * 12);
    HIPCK(hipMemcpyAsync(rec.data(), d_rec, P * 48, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    uint32_t w = 0;
    for (size_t q = 0; q < P; ++q)                       // q = i * H + j: the feedback buffer's vertex order
        if (flag[q]) { memcpy(dst12 + (size_t)w * 12, rec.data() + q * 12, 48); ++w; }
    return SM_OK;
}

int sm_download_depth(sm_ctx *s, int which, float *dst)
{
    if (!s || !dst) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    const bool alias = s->cfg.preprocess == 0;
    // preprocess == 1: after every processFrame LAST == DEPTH_FILTERED (src/SurfelMapping.cpp:244); the two
    // buffers are swapped instead of copied, so both names read d_lastT.
    const float *depthT = s->cur().depthT;
    const float *src = which == SM_TEX_DEPTH_METRIC ? depthT : which == SM_TEX_DEPTH_FILTERED ? (alias ? depthT : s->d_lastT)
                     : which == SM_TEX_LAST ? (alias ? depthT : s->d_lastT) : nullptr;
    if (!src) return SM_E_ARG;
    int rc = ensure_export(s, (size_t)s->P * 4);
    if (rc) return rc;
    hipLaunchKernelGGL(k_untranspose_f32, dim3((s->P + 255) / 256), dim3(256), 0, s->stream, src, (float *)s->d_export.get(), s->W, s->H);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(dst, s->d_export, (size_t)s->P * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

int sm_render_image(sm_ctx *s, const float *view16, int w, int h, float fx, float fy, float cx, float cy, uint8_t *bgr_out,
                    uint8_t *sem_out)
{
    return render_image(s, view16, w, h, fx, fy, cx, cy, nullptr, nullptr, bgr_out, sem_out, nullptr, "sm_render_image");
}

int sm_render_image_ex(sm_ctx *s, const float *view16, int w, int h, float fx, float fy, float cx, float cy, const sm_fill_params *fill,
                       uint8_t *bgr_out, uint8_t *sem_out, uint16_t *depth_mm_out)
{
    const char *who = "sm_render_image_ex";
    if (!s) { g_err = std::string(who) + ": null context"; return SM_E_ARG; }
    if (int rc = check_whole_map(s, who)) return rc;
    if (int rc = check_fill_params(fill, who)) return rc;
    return render_image(s, view16, w, h, fx, fy, cx, cy, nullptr, fill, bgr_out, sem_out, depth_mm_out, who);
}

void *sm_device_alloc(sm_ctx *s, size_t bytes)
{
    if (!s) return nullptr;
    if (hipSetDevice(s->cfg.device) != hipSuccess) return nullptr;
    Dev<void> p;
    if (hipMalloc(p.put(), std::max<size_t>(bytes, 1)) != hipSuccess) { g_err = "sm_device_alloc: hipMalloc failed"; return nullptr; }
    s->user_allocs.push_back(std::move(p));
    return s->user_allocs.back();
}

int sm_device_free(sm_ctx *s, void *p)
{
    if (!s || !p) return SM_E_ARG;
    auto it = std::find(s->user_allocs.begin(), s->user_allocs.end(), p);
    if (it == s->user_allocs.end()) return SM_E_ARG;
    (void)it->release();
    s->user_allocs.erase(it);
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipStreamSynchronize(s->stream));
    HIPCK(hipFree(p));
    return SM_OK;
}

int sm_device_upload(sm_ctx *s, void *dst_device, const void *src_host, size_t bytes)
{
    if (!s || !dst_device || !src_host) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipMemcpyAsync(dst_device, src_host, bytes, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

int sm_export_model_device(sm_ctx *s, void **d_aos, uint32_t *n)
{
    if (!s || !d_aos || !n) return SM_E_ARG;
    if (hip_runtime_conflict("sm_export_model_device")) return SM_E_HIP;     // the pointer goes to foreign code (RCCL)
    HIPCK(hipSetDevice(s->cfg.device));
    if (int rc = check_not_mid_cull(s, "sm_export_model_device")) return rc;
    int rc = ensure_compact(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;
    const uint32_t cnt = s->h_state->count;
    if ((rc = ensure_export(s, (size_t)std::max(cnt, 1u) * 48))) return rc;
    if (cnt) {
        export_aos(s, (float *)s->d_export.get(), 0u, cnt);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(s->stream));
    }
    *d_aos = s->d_export;
    *n = cnt;
    return SM_OK;
}

int sm_append_model_aos_device(sm_ctx *s, const float *d_src12, uint32_t n)
{
    if (!s || (!d_src12 && n)) return SM_E_ARG;
    if (hip_runtime_conflict("sm_append_model_aos_device")) return SM_E_HIP;
    HIPCK(hipSetDevice(s->cfg.device));
    if (int rc = check_not_mid_cull(s, "sm_append_model_aos_device")) return rc;
    int rc = ensure_compact(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;
    const uint32_t cnt = s->h_state->count;
    if ((uint64_t)cnt + n > s->cap) { g_err = "sm_append_model_aos_device: exceeds MAX_VERTICES"; return SM_E_CAPACITY; }
    if (n) {
        hipLaunchKernelGGL(k_import_aos, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, d_src12, cnt, n);
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(s->stream));
    }
    s->h_state->count = cnt + n;
    s->h_state->offset = cnt;
    if ((rc = push_state(s))) return rc;
    if ((rc = rebuild_bounds(s, cnt, cnt + n))) return rc;
    return pull_state(s);
}

int sm_device_download(sm_ctx *s, void *dst_host, const void *src_device, size_t bytes)
{
    if (!s || !dst_host || !src_device) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipMemcpyAsync(dst_host, src_device, bytes, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

}  // extern "C"
