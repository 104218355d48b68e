// sm_fill.hip -- hole filling of novel views (DESIGN.md "4n. Hole filling"): the depth of a view from its keys, the depth-aware
// push-pull completion of a batch of images in place (sm_fill_image*; the stage of sm_render_image_ex and sm_render_image_maps_ex),
// its pyramid scratch and its tally (sm_fill_stats).  Kernels: sm_k_fill.h.
#include "sm_ctx.h"
#include "sm_k_fill.h"

using namespace sm;

namespace {

// where everything lies in the pyramid scratch for n images of w x h
struct FillPlan {
    int lw[FILL_MAX_LEVELS + 1], lh[FILL_MAX_LEVELS + 1];
    size_t off_rec[FILL_MAX_LEVELS + 1], off_cnt5, off_pull, off_push, total;
    size_t tiles;                                        // 32 x 32 tiles of one image
};

FillPlan make_plan(int levels, int w, int h, size_t n)
{
    FillPlan pl{};
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    pl.lw[0] = w; pl.lh[0] = h;
    size_t off = up(n * (size_t)w * h);                  // the level-0 validity plane comes first
    for (int l = 1; l <= FILL_MAX_LEVELS; ++l) {
        pl.lw[l] = (pl.lw[l - 1] + 1) / 2; pl.lh[l] = (pl.lh[l - 1] + 1) / 2;
        pl.off_rec[l] = off;
        if (l <= levels) off += up(n * (size_t)pl.lw[l] * pl.lh[l] * sizeof(uint2));
    }
    pl.off_cnt5 = off;
    if (levels > FILL_LDS_LEVELS) off += up(n * (size_t)pl.lw[FILL_LDS_LEVELS] * pl.lh[FILL_LDS_LEVELS] * 4);
    pl.tiles = (size_t)((w + FILL_TILE - 1) / FILL_TILE) * (size_t)((h + FILL_TILE - 1) / FILL_TILE);
    pl.off_pull = off; off += up(n * pl.tiles * sizeof(uint2));
    pl.off_push = off; off += up(n * pl.tiles * sizeof(uint2));
    pl.total = off;
    return pl;
}

// what sm_fill_image* ask of their arguments
int fill_check(sm_ctx *s, const sm_fill_params *p, int w, int h, const void *bgr, const void *sem, const void *depth, const char *who)
{
    if (!s || !p || !bgr || !sem) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if (w <= 0 || h <= 0 || (uint64_t)w * h > (1u << 28)) { g_err = std::string(who) + ": width and height must be positive, w*h at most 2^28"; return SM_E_ARG; }
    if ((uintptr_t)depth & 1u) { g_err = std::string(who) + ": misaligned depth_mm"; return SM_E_ARG; }
    return check_fill_params(p, who);
}

}  // namespace

int sm_impl::check_fill_params(const sm_fill_params *p, const char *who)
{
    if (!p) return SM_OK;
    const char *why = (p->levels < 0 || p->levels > FILL_MAX_LEVELS) ? "levels is outside 0..8"
                    : (p->depth_tol_256 < 0 || p->depth_tol_256 > 255) ? "depth_tol_256 is outside 0..255"
                    : (p->through_count < 0 || p->through_count > 8) ? "through_count is outside 0..8"
                    : (p->prefer_far < 0 || p->prefer_far > 1) ? "prefer_far is not 0 or 1"
                    : (p->min_cover_256 < 0 || p->min_cover_256 > 256) ? "min_cover_256 is outside 0..256" : nullptr;
    if (why) { g_err = std::string(who) + ": " + why; return SM_E_ARG; }
    return SM_OK;
}

size_t sm_impl::fill_scratch_bytes(const sm_fill_params &p, int w, int h, size_t n) { return make_plan(p.levels, w, h, n).total; }

void sm_impl::fill_key_depth(sm_ctx *s, const uint64_t *key, size_t total, uint16_t *d_depth)
{
    hipLaunchKernelGGL(k_fill_key_depth, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s->stream, key, total, d_depth);
}

void sm_impl::fill_begin(sm_ctx *s)
{
    s->fill.stats = sm_fill_stats_t{};
    s->fill.stats_valid = true;
    s->fill.pending = false;
}

int sm_impl::fill_enqueue(sm_ctx *s, const sm_fill_params &p, int w, int h, uint32_t n, uint8_t *d_bgr, uint8_t *d_sem, uint16_t *d_depth)
{
    Fill &f = s->fill;
    if (!n) return SM_OK;
    if (f.pending)
        if (int rc = fill_fold(s)) return rc;
    const FillPlan pl = make_plan(p.levels, w, h, n);
    if (pl.total > f.bytes) {
        HIPCK(hipStreamSynchronize(s->stream));          // an enqueued stage still uses the old scratch
        f.bytes = 0;
        HIPCK(hipMalloc((void **)f.d_scratch.put(), pl.total));
        f.bytes = pl.total;
    }
    if (!f.ev[1]) { HIPCK(hipEventCreate(f.ev[0].put())); HIPCK(hipEventCreate(f.ev[1].put())); }
    uint8_t *base = f.d_scratch;
    FillArgs a{};
    a.bgr = d_bgr; a.sem = d_sem; a.depth = d_depth;
    a.v0 = base;
    for (int l = 1; l <= p.levels; ++l) a.rec[l] = (uint2 *)(base + pl.off_rec[l]);
    a.cnt5 = (uint32_t *)(base + pl.off_cnt5);
    a.part_pull = (uint2 *)(base + pl.off_pull); a.part_push = (uint2 *)(base + pl.off_push);
    a.w = w; a.h = h; a.n = n;
    for (int l = 0; l <= FILL_MAX_LEVELS; ++l) { a.lw[l] = pl.lw[l]; a.lh[l] = pl.lh[l]; }
    a.levels = p.levels; a.tol = p.depth_tol_256; a.through = p.through_count; a.prefer_far = p.prefer_far; a.cover = p.min_cover_256;
    const unsigned gy = (unsigned)std::min<uint32_t>(n, 65535u);
    auto tiles_of = [](int cw, int ch, int t) { return (unsigned)((size_t)((cw + t - 1) / t) * (size_t)((ch + t - 1) / t)); };

    HIPCK(hipEventRecord(f.ev[0], s->stream));
    hipLaunchKernelGGL(k_fill_pull, dim3((unsigned)pl.tiles, gy), dim3(256), 0, s->stream, a);
    f.stats.launches++;
    if (p.levels > FILL_LDS_LEVELS) {
        hipLaunchKernelGGL(k_fill_pull_top, dim3(tiles_of(pl.lw[FILL_LDS_LEVELS], pl.lh[FILL_LDS_LEVELS], FILL_TOP_TILE), gy), dim3(64), 0, s->stream, a);
        f.stats.launches++;
    }
    for (int l = p.levels - 1; l >= 1; --l) {
        hipLaunchKernelGGL(k_fill_push<false>, dim3(tiles_of(pl.lw[l], pl.lh[l], FILL_TILE), gy), dim3(256), 0, s->stream, a, l);
        f.stats.launches++;
    }
    // level 0: the images in their final layout (levels == 0: the pixels step 0 removed become zeros)
    hipLaunchKernelGGL(k_fill_push<true>, dim3((unsigned)pl.tiles, gy), dim3(256), 0, s->stream, a, 0);
    f.stats.launches++;
    HIPCK(hipGetLastError());
    HIPCK(hipEventRecord(f.ev[1], s->stream));
    f.off_pull = pl.off_pull; f.off_push = pl.off_push;
    f.n_pull = f.n_push = (size_t)n * pl.tiles;
    f.pending = true;
    return SM_OK;
}

int sm_impl::fill_fold(sm_ctx *s)
{
    Fill &f = s->fill;
    if (!f.pending) return SM_OK;
    f.pending = false;
    std::vector<uint2> part(f.n_pull + f.n_push);
    HIPCK(hipMemcpyAsync(part.data(), f.d_scratch.get() + f.off_pull, f.n_pull * sizeof(uint2), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(part.data() + f.n_pull, f.d_scratch.get() + f.off_push, f.n_push * sizeof(uint2), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    for (size_t i = 0; i < f.n_pull; ++i) { f.stats.valid += part[i].x; f.stats.seen_through += part[i].y; }
    for (size_t i = f.n_pull; i < part.size(); ++i) { f.stats.filled += part[i].x; f.stats.left_empty += part[i].y; }
    float ms = 0.0f;
    HIPCK(hipEventElapsedTime(&ms, f.ev[0], f.ev[1]));
    f.stats.device_ms += ms;
    return SM_OK;
}

extern "C" {

int sm_default_fill_params(sm_fill_params *p)
{
    if (!p) { g_err = "sm_default_fill_params: null argument"; return SM_E_ARG; }
    p->levels = 3;
    p->depth_tol_256 = 13;
    p->through_count = 6;
    p->prefer_far = 1;
    p->min_cover_256 = 64;
    return SM_OK;
}

int sm_fill_image_device(sm_ctx *s, const sm_fill_params *p, int w, int h, uint32_t n, uint8_t *d_bgr, uint8_t *d_sem, uint16_t *d_depth_mm)
{
    if (int rc = fill_check(s, p, w, h, d_bgr, d_sem, d_depth_mm, "sm_fill_image_device")) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    fill_begin(s);
    return fill_enqueue(s, *p, w, h, n, d_bgr, d_sem, d_depth_mm);
}

int sm_fill_image(sm_ctx *s, const sm_fill_params *p, int w, int h, uint32_t n, uint8_t *bgr, uint8_t *sem, uint16_t *depth_mm)
{
    if (int rc = fill_check(s, p, w, h, bgr, sem, depth_mm, "sm_fill_image")) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    fill_begin(s);
    if (!n) return SM_OK;
    Fill &f = s->fill;
    const size_t N = (size_t)n * (size_t)w * h, need = N * 6;              // bgr | sem | depth_mm
    if (need > f.img_bytes) {
        HIPCK(hipStreamSynchronize(s->stream));
        f.img_bytes = 0;
        HIPCK(hipMalloc((void **)f.d_img.put(), need));
        f.img_bytes = need;
    }
    uint8_t *d_bgr = f.d_img, *d_sem = d_bgr + N * 3;
    uint16_t *d_depth = depth_mm ? (uint16_t *)(d_bgr + N * 4) : nullptr;
    HIPCK(hipMemcpyAsync(d_bgr, bgr, N * 3, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(d_sem, sem, N, hipMemcpyHostToDevice, s->stream));
    if (depth_mm) HIPCK(hipMemcpyAsync(d_depth, depth_mm, N * 2, hipMemcpyHostToDevice, s->stream));
    if (int rc = fill_enqueue(s, *p, w, h, n, d_bgr, d_sem, d_depth)) return rc;
    HIPCK(hipMemcpyAsync(bgr, d_bgr, N * 3, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(sem, d_sem, N, hipMemcpyDeviceToHost, s->stream));
    if (depth_mm) HIPCK(hipMemcpyAsync(depth_mm, d_depth, N * 2, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return fill_fold(s);
}

int sm_fill_stats(sm_ctx *s, sm_fill_stats_t *out)
{
    if (!s || !out) { g_err = "sm_fill_stats: null argument"; return SM_E_ARG; }
    if (!s->fill.stats_valid) { g_err = "sm_fill_stats: no call that filled yet"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (int rc = fill_fold(s)) return rc;
    *out = s->fill.stats;
    return SM_OK;
}

}  // extern "C"
