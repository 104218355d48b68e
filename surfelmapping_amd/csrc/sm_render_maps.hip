// sm_render_maps.hip -- views of a map set (sm_render_image_maps, its _ex form and the views behind its _blend form, sm_render_model_maps; DESIGN.md "4f. Views of a map set"): map files streamed through the two
// renderers in chunks, the live model last; for every source that streams map files, the context's MapStaging: its allocation and intake kernel.  Kernels: sm_k_render_maps.h.
#include "sm_map_stream.h"
#include "sm_k_render_maps.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

// what differs between the two renderers
struct Mode {
    bool image;
    int w, h;
    uint32_t n_views;
    const void *params; size_t param_size;               // RenderParams / ViewParams per view
    const ViewShade *shade;                              // model view only
    // host outputs, per view npix * 3 | npix (image) or npix * 4 each (view: depth and id may be null)
    uint8_t *out0; uint8_t *out1; uint8_t *out2;
    // image only (sm_render_image_maps_ex): the completion of every batch's planes (null: none), the depth plane (null: not wanted)
    const sm_fill_params *fill;
    uint16_t *out_depth;
    // image only (sm_render_image_maps_blend): the colours of the visible layer blended (null: the nearest surfel's), which takes a
    // second pass over the files per batch
    const sm_blend_params *blend;
    // image only (sm_render_image_scene): the actors drawn after every static source (null: none)
    ScenePlan *scene;
};

int render_maps(sm_ctx *s, const sm_map_source *src, const char *fn, const Mode &md)
{
    const double t_begin = now_ms();
    sm_mapset::ReadSet set;
    uint32_t cnt;
    int rc = maps_open(s, src, fn, [](const sm_ctx *c, const char *who) -> int {
        if (c->ss_on) { g_err = std::string(who) + ": a sharded context holds only its rank's surfels; rendering the union is not supported"; return SM_E_UNSUPPORTED; }
        return SM_OK;
    }, set, cnt);
    if (rc) return rc;
    const uint64_t file_total = set.file_total;
    const MapStaging &st = s->staging;
    RenderMaps &rm = s->maps;
    rm.stats = sm_maps_stats{};
    rm.stats_valid = true;
    if (md.scene && (rc = scene_load(s, *md.scene, file_total + cnt, md.n_views != 0, fn))) return rc;
    if (md.n_views == 0) { rm.stats.total_ms = (float)(now_ms() - t_begin); return SM_OK; }
    if (file_total && (rc = maps_ensure_staging(s))) return rc;

    const size_t npix = (size_t)md.w * md.h;
    int cull;
    // the key budget bounds what a view of the batch holds beside its keys too: the depth plane, the completion's pyramid and the
    // blend's four 64-bit sums per pixel
    const bool depth16 = md.fill || md.out_depth;
    const size_t extra = (depth16 ? npix * 2 : 0) + (md.fill ? fill_scratch_bytes(*md.fill, md.w, md.h, 1) : 0) + (md.blend ? npix * 32 : 0);
    const uint32_t B = maps_batch(md.n_views, npix + (extra + 7) / 8, "SM_RENDER_MAPS_KEY_MB", "SM_RENDER_MAPS_NO_CULL", &cull);
    if (md.fill) fill_begin(s);
    if (md.blend) blend_begin(s);
    const unsigned pblocks = (unsigned)((npix + 255) / 256);

    // per-view parameters | shading | skipped counters | hit flags
    const size_t V = md.n_views;
    const size_t off_shade = (V * md.param_size + 15) & ~(size_t)15, off_skip = off_shade + V * sizeof(ViewShade), off_hit = off_skip + V * 4,
                 par_bytes = off_hit + V;
    if (par_bytes > rm.par_bytes) {
        rm.par_bytes = 0;
        HIPCK(hipMalloc((void **)rm.d_par.put(), par_bytes));
        rm.par_bytes = par_bytes;
    }
    uint8_t *d_par = rm.d_par;
    uint32_t *d_skip = (uint32_t *)(d_par + off_skip);
    uint8_t *d_hit = d_par + off_hit;
    HIPCK(hipMemcpyAsync(d_par, md.params, V * md.param_size, hipMemcpyHostToDevice, s->stream));
    if (!md.image) HIPCK(hipMemcpyAsync(d_par + off_shade, md.shade, V * sizeof(ViewShade), hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemsetAsync(d_skip, 0, V * 4, s->stream));

    // export scratch: keys | output planes of one batch | (model view + live model) overflow length and list
    const size_t out_px = md.image ? (depth16 ? 6 : 4) : 12;
    const size_t off_out = (size_t)B * npix * 8, off_ovf = off_out + (((size_t)B * npix * out_px + 255) & ~(size_t)255);
    if ((rc = ensure_export(s, off_ovf + ((!md.image && cnt) ? 256 + (size_t)cnt * 4 : 0)))) return rc;
    uint8_t *base = (uint8_t *)s->d_export.get();
    uint64_t *d_key = (uint64_t *)base;
    uint8_t *d_out = base + off_out;
    uint32_t *d_ovf_n = (uint32_t *)(base + off_ovf), *d_ovf = (uint32_t *)(base + off_ovf + 256);

    if (cnt && !rm.ev[1]) { HIPCK(hipEventCreate(rm.ev[0].put())); HIPCK(hipEventCreate(rm.ev[1].put())); }
    const MapsSoA chunk = planes(st);
    const SurfelSet cur = s->M.s[s->h_state->cur];
    const MapsSoA live{cur.pos_conf, cur.norm_rad, cur.color, cur.time};
    MapStream in(s, fn, src->paths, {&rm.stats.read_ms, &rm.stats.copy_ms, &rm.stats.device_ms});

    for (uint32_t v0 = 0; v0 < md.n_views; v0 += B) {
        const uint32_t b = std::min(B, md.n_views - v0);
        const size_t bp = (size_t)b * npix;
        rm.stats.passes++;
        // this batch's planes
        uint8_t *d_bgr = d_out, *d_sem = d_out + bp * 3;
        uint16_t *d_depth16 = (uint16_t *)(d_out + bp * 4);
        uint32_t *d_rgba = (uint32_t *)d_out;
        float *d_depth = (float *)(d_out + bp * 4);
        int32_t *d_id = (int32_t *)(d_out + bp * 8);
        const RenderParams *d_rp = (const RenderParams *)d_par + v0;
        const ViewParams *d_vp = (const ViewParams *)d_par + v0;
        const ViewShade *d_vs = (const ViewShade *)(d_par + off_shade) + v0;
        auto resolve = [&](const MapsSoA &from, uint32_t id_base, uint32_t n) {
            if (md.image)
                hipLaunchKernelGGL(k_maps_resolve_image, dim3(pblocks, b), dim3(256), 0, s->stream, from, id_base, n, d_key, npix, d_hit + v0, d_bgr, d_sem);
            else
                hipLaunchKernelGGL(k_maps_resolve_view, dim3(pblocks, b), dim3(256), 0, s->stream, from, id_base, n, d_vs, d_key, npix, d_hit + v0,
                                   d_rgba, d_depth, d_id);
        };
        fill_keys(s, d_key, bp);

        // ---- one pass over the files, chunk by chunk: the host reads chunk c + 1 while the copy and the kernels of chunk c run;
        // launch(chunk's id base, records, blocks) enqueues what the pass does with the chunk in the staging's planes
        auto pass = [&](auto &&launch) -> int {
            for (in.begin(set.jobs); in.more();) {
                MapStream::Chunk ck;
                if (int e = in.next(ck)) return e;
                const uint32_t n = ck.job->n;
                const unsigned nblk = (n + MAPS_BLOCK - 1) / MAPS_BLOCK;
                maps_intake(s, ck.d_rec, n);
                if (int e = launch((uint32_t)(set.id_base[ck.job->file] + ck.job->first), n, nblk)) return e;
                if (int e = in.done(ck.q)) return e;
                HIPCK(hipGetLastError());
                rm.stats.surfels_read += n;
                rm.stats.chunks++;
                if (cull) rm.stats.pairs_tested += (uint64_t)nblk * b;
            }
            if (int e = in.fold(0)) return e;
            return in.fold(1);
        };
        rc = pass([&](uint32_t gid, uint32_t n, unsigned nblk) -> int {
            HIPCK(hipMemsetAsync(d_hit + v0, 0, b, s->stream));
            if (md.image)
                hipLaunchKernelGGL(k_maps_splat_image, dim3(nblk, b), dim3(256), 0, s->stream, chunk, n, gid, (const float4 *)st.d_box.get(), d_rp,
                                   d_key, npix, cull, d_skip + v0, d_hit + v0);
            else
                hipLaunchKernelGGL(k_maps_splat_view, dim3(nblk, b), dim3(256), 0, s->stream, chunk, n, gid, (const float4 *)st.d_box.get(), d_vp,
                                   d_key, npix, cull, d_skip + v0, d_hit + v0);
            resolve(chunk, gid, n);
            return SM_OK;
        });
        if (rc) return rc;

        // ---- the live model, by the resident kernels with an id base
        if (cnt) {
            HIPCK(hipEventRecord(rm.ev[0], s->stream));
            for (uint32_t i = 0; i < b; ++i) {
                uint64_t *kv = d_key + (size_t)i * npix;
                if (md.image) render_splat_model(s, ((const RenderParams *)md.params)[v0 + i], kv, (uint32_t)file_total);
                else if ((rc = view_splat_model(s, ((const ViewParams *)md.params)[v0 + i], kv, d_ovf_n, d_ovf, (uint32_t)file_total))) return rc;
            }
            HIPCK(hipMemsetAsync(d_hit + v0, 1, b, s->stream));
            resolve(live, (uint32_t)file_total, cnt);
            HIPCK(hipEventRecord(rm.ev[1], s->stream));
            HIPCK(hipGetLastError());
            float ms = 0.0f;
            HIPCK(hipEventSynchronize(rm.ev[1]));
            HIPCK(hipEventElapsedTime(&ms, rm.ev[0], rm.ev[1]));
            rm.stats.device_ms += ms;
        }

        // ---- the scene's actors, under this batch's poses
        if (md.scene && (rc = scene_draw_image(s, *md.scene, d_rp, v0, b, d_key, npix, d_bgr, d_sem))) return rc;

        // ---- pixels nobody won, then the batch's planes to the caller
        if (md.image) hipLaunchKernelGGL(k_maps_finish_image, dim3((unsigned)((bp + 255) / 256)), dim3(256), 0, s->stream, d_key, bp, d_bgr, d_sem);
        else hipLaunchKernelGGL(k_maps_finish_view, dim3(pblocks, b), dim3(256), 0, s->stream, d_vs, d_key, npix, d_rgba, d_depth, d_id);
        HIPCK(hipGetLastError());

        // ---- blended: the key map is whole, so every source is walked again, now adding the visible layer's fragments
        if (md.blend) {
            if ((rc = blend_clear(s, bp))) return rc;
            const float ms0 = rm.stats.device_ms;
            if ((rc = pass([&](uint32_t, uint32_t n, unsigned) -> int { blend_accum_chunk(s, *md.blend, n, d_rp, d_key, npix, b, cull); return SM_OK; })))
                return rc;
            blend_add_ms(s, rm.stats.device_ms - ms0);
            if ((rc = blend_mark(s))) return rc;
            if (cnt)
                for (uint32_t i = 0; i < b; ++i)
                    blend_accum_model(s, *md.blend, ((const RenderParams *)md.params)[v0 + i], d_key + (size_t)i * npix, (size_t)i * npix);
            if ((rc = blend_normalise(s, d_key, npix, b, d_bgr, d_sem))) return rc;
        }
        if (depth16) fill_key_depth(s, d_key, bp, d_depth16);
        if (md.fill && (rc = fill_enqueue(s, *md.fill, md.w, md.h, b, d_bgr, d_sem, d_depth16))) return rc;
        const size_t vp0 = (size_t)v0 * npix;
        if (md.image) {
            if (md.out_depth) HIPCK(hipMemcpyAsync(md.out_depth + vp0, d_depth16, bp * 2, hipMemcpyDeviceToHost, s->stream));
            HIPCK(hipMemcpyAsync(md.out0 + vp0 * 3, d_bgr, bp * 3, hipMemcpyDeviceToHost, s->stream));
            HIPCK(hipMemcpyAsync(md.out1 + vp0, d_sem, bp, hipMemcpyDeviceToHost, s->stream));
        } else {
            HIPCK(hipMemcpyAsync(md.out0 + vp0 * 4, d_rgba, bp * 4, hipMemcpyDeviceToHost, s->stream));
            if (md.out1) HIPCK(hipMemcpyAsync(md.out1 + vp0 * 4, d_depth, bp * 4, hipMemcpyDeviceToHost, s->stream));
            if (md.out2) HIPCK(hipMemcpyAsync(md.out2 + vp0 * 4, d_id, bp * 4, hipMemcpyDeviceToHost, s->stream));
        }
        HIPCK(hipStreamSynchronize(s->stream));
        if (md.blend && (rc = blend_fold(s))) return rc;
        if (md.fill && (rc = fill_fold(s))) return rc;
        if (md.scene && (rc = scene_fold(s))) return rc;
    }
    std::vector<uint32_t> skipped(V);
    HIPCK(hipMemcpy(skipped.data(), d_skip, V * 4, hipMemcpyDeviceToHost));
    for (uint32_t x : skipped) rm.stats.pairs_skipped += x;
    rm.stats.total_ms = (float)(now_ms() - t_begin);
    return md.scene ? scene_end(s, *md.scene) : SM_OK;
}

}  // namespace

int sm_impl::maps_ensure_staging(sm_ctx *s)
{
    MapStaging &st = s->staging;
    if (st.copy) return SM_OK;
    Stream copy;
    HIPCK(hipStreamCreateWithFlags(copy.put(), hipStreamNonBlocking));
    const size_t N = MapStaging::CHUNK;
    for (int b = 0; b < 2; ++b) {
        HIPCK(hipHostMalloc((void **)st.h_rec[b].put(), N * sm_mapfile::RECORD_BYTES, hipHostMallocDefault));
        HIPCK(hipMalloc(st.d_rec[b].put(), N * sm_mapfile::RECORD_BYTES));
        for (Event *e : {&st.ev_copy0[b], &st.ev_copied[b], &st.ev_k0[b], &st.ev_k1[b]}) HIPCK(hipEventCreate(e->put()));
    }
    int rc;
    if ((rc = dalloc(st.d_pos_conf, N)) || (rc = dalloc(st.d_norm_rad, N)) || (rc = dalloc(st.d_color, N)) || (rc = dalloc(st.d_time, N)) ||
        (rc = dalloc(st.d_box, 2 * (N / MAPS_BLOCK))))
        return rc;
    st.copy = std::move(copy);                           // last: the staging is whole or absent
    return SM_OK;
}

void sm_impl::maps_intake(sm_ctx *s, const float4 *d_rec, uint32_t n)
{
    maps_intake_to(s, d_rec, n, planes(s->staging), s->staging.d_box.get());
}

void sm_impl::maps_intake_to(sm_ctx *s, const float4 *d_rec, uint32_t n, const MapsSoA &out, float4 *d_box)
{
    hipLaunchKernelGGL(k_maps_intake, dim3((n + MAPS_BLOCK - 1) / MAPS_BLOCK), dim3(256), 0, s->stream, d_rec, n, out, d_box);
}

// sm_render_image_maps (fn) and, with fill or depth_mm_out, what sm_render_image_maps_ex adds to it; with blend, sm_render_image_maps_blend
int sm_impl::render_image_maps(sm_ctx *s, const sm_map_source *src, const float *views16, uint32_t n_views, int w, int h, float fx, float fy,
                               float cx, float cy, const sm_blend_params *blend, const sm_fill_params *fill, uint8_t *bgr_out,
                               uint8_t *sem_out, uint16_t *depth_mm_out, const char *fn, ScenePlan *scene)
{
    if (!s || !src) { g_err = std::string(fn) + ": null context or source"; return SM_E_ARG; }
    if (n_views && (!views16 || !bgr_out || !sem_out)) { g_err = std::string(fn) + ": null views or outputs"; return SM_E_ARG; }
    if (w <= 0 || h <= 0 || (uint64_t)w * h > (1u << 28)) { g_err = std::string(fn) + ": width and height must be positive, w*h at most 2^28"; return SM_E_ARG; }
    std::vector<RenderParams> rps(n_views);
    for (uint32_t i = 0; i < n_views; ++i) {
        RenderParams &rp = rps[i];
        invert4(views16 + (size_t)i * 16, rp.t_inv);
        rp.fx = fx; rp.fy = fy; rp.cx = cx; rp.cy = cy; rp.cols = (float)w; rp.rows = (float)h; rp.w = w; rp.h = h;
    }
    Mode md{};
    md.image = true; md.w = w; md.h = h; md.n_views = n_views;
    md.params = rps.data(); md.param_size = sizeof(RenderParams);
    md.out0 = bgr_out; md.out1 = sem_out;
    md.fill = fill; md.out_depth = depth_mm_out; md.blend = blend; md.scene = scene;
    return render_maps(s, src, fn, md);
}

extern "C" {

int sm_render_image_maps(sm_ctx *s, const sm_map_source *src, const float *views16, uint32_t n_views, int w, int h, float fx, float fy,
                         float cx, float cy, uint8_t *bgr_out, uint8_t *sem_out)
{
    return render_image_maps(s, src, views16, n_views, w, h, fx, fy, cx, cy, nullptr, nullptr, bgr_out, sem_out, nullptr, "sm_render_image_maps");
}

int sm_render_image_maps_ex(sm_ctx *s, const sm_map_source *src, const float *views16, uint32_t n_views, int w, int h, float fx, float fy,
                            float cx, float cy, const sm_fill_params *fill, uint8_t *bgr_out, uint8_t *sem_out, uint16_t *depth_mm_out)
{
    const char *fn = "sm_render_image_maps_ex";
    if (s)
        if (int rc = check_whole_map(s, fn)) return rc;
    if (int rc = check_fill_params(fill, fn)) return rc;
    return render_image_maps(s, src, views16, n_views, w, h, fx, fy, cx, cy, nullptr, fill, bgr_out, sem_out, depth_mm_out, fn);
}

int sm_render_model_maps(sm_ctx *s, const sm_map_source *src, const sm_model_view *views, uint32_t n_views, uint8_t *rgba, float *depth,
                         int32_t *id)
{
    const char *fn = "sm_render_model_maps";
    if (!s || !src) { g_err = std::string(fn) + ": null context or source"; return SM_E_ARG; }
    if (n_views && (!views || !rgba)) { g_err = std::string(fn) + ": null views or rgba"; return SM_E_ARG; }
    std::vector<ViewParams> vps(n_views);
    std::vector<ViewShade> vss(n_views);
    for (uint32_t i = 0; i < n_views; ++i) {
        if (int rc = check_model_view(&views[i], fn)) return rc;
        if (views[i].width != views[0].width || views[i].height != views[0].height) {
            g_err = std::string(fn) + ": all views of a call have one width x height"; return SM_E_ARG;
        }
        model_view_params(&views[i], vps[i], vss[i]);
    }
    Mode md{};
    md.image = false; md.n_views = n_views;
    md.w = n_views ? views[0].width : 1; md.h = n_views ? views[0].height : 1;
    md.params = vps.data(); md.param_size = sizeof(ViewParams);
    md.shade = vss.data();
    md.out0 = rgba; md.out1 = (uint8_t *)depth; md.out2 = (uint8_t *)id;
    return render_maps(s, src, fn, md);
}

int sm_render_maps_stats(sm_ctx *s, sm_maps_stats *out)
{
    if (!s || !out) return SM_E_ARG;
    if (!s->maps.stats_valid) { g_err = "sm_render_maps_stats: no sm_render_image_maps / sm_render_model_maps call yet"; return SM_E_ARG; }
    *out = s->maps.stats;
    return SM_OK;
}

}  // extern "C"
