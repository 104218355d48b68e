// sm_lidar_depth.hip -- lidar depth (DESIGN.md "4z. Lidar depth"): the planes of a context that turns scans into depth images
// (sm_set_lidar_depth), the depth image of a scan from host or device memory (sm_lidar_depth*), and the last call's tally
// (sm_lidar_depth_stats).  Kernels: sm_k_lidar_depth.h.
#include "sm_ctx.h"
#include "sm_k_lidar_depth.h"

#include <cstdlib>

using namespace sm;

namespace {

// what every entry point with a context asks first; stage: the context must have it
int ld_check(sm_ctx *s, bool stage, const char *who)
{
    if (!s) { g_err = std::string(who) + ": null context"; return SM_E_ARG; }
    if (int rc = check_whole_map(s, who)) return rc;
    if (int rc = check_not_mid_cull(s, who)) return rc;
    if (stage && !s->ldepth.on) { g_err = std::string(who) + ": the context has no lidar depth (sm_set_lidar_depth)"; return SM_E_ARG; }
    return SM_OK;
}

const char *check_params(const sm_lidar_depth_params &p)
{
    if (!std::isfinite(p.min_z) || !std::isfinite(p.max_z) || !(p.min_z > 0.0f) || !(p.min_z <= p.max_z) || !(p.max_z <= 65.535f))
        return "min_z and max_z must be finite with 0 < min_z <= max_z <= 65.535";
    if (p.stages < 0 || p.stages > 127) return "stages is outside 0..127";
    if (p.large < 3 || p.large > 31 || !(p.large & 1)) return "large is not odd in 3..31";
    if (p.tol_256 < 0 || p.tol_256 > 255) return "tol_256 is outside 0..255";
    return nullptr;
}

int ld_check_call(sm_ctx *s, const float *points, uint32_t n, const float *T16, const void *depth, const void *sparse, const void *index, const char *who)
{
    if (int rc = ld_check(s, true, who)) return rc;
    if (n > SM_LIDAR_DEPTH_MAX_POINTS) { g_err = std::string(who) + ": more than SM_LIDAR_DEPTH_MAX_POINTS points"; return SM_E_ARG; }
    if (n && !points) { g_err = std::string(who) + ": null points"; return SM_E_ARG; }
    if (!T16) { g_err = std::string(who) + ": null transform"; return SM_E_ARG; }
    if ((((uintptr_t)depth | (uintptr_t)sparse) & 1u) || ((uintptr_t)index & 3u)) { g_err = std::string(who) + ": misaligned output"; return SM_E_ARG; }
    return SM_OK;
}

// the tallies and times of the enqueued call into `stats`
int ld_fold(sm_ctx *s)
{
    LidarDepth &d = s->ldepth;
    if (!d.pending) return SM_OK;
    d.pending = false;
    const size_t rest = d.unfused ? 8 : d.tiles * 6;
    std::vector<uint32_t> part(d.blocks_project + rest);
    uint32_t *tail = part.data() + d.blocks_project;
    HIPCK(hipMemcpyAsync(part.data(), d.d_part, (size_t)d.blocks_project * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(tail, d.d_part.get() + d.part_project, rest * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    for (uint32_t b = 0; b < d.blocks_project; ++b) d.stats.landed += part[b];
    if (d.unfused) {
        d.stats.measured = tail[LDU_T_MEASURED]; d.stats.filled_small = tail[LDU_T_SMALL]; d.stats.filled_top = tail[LDU_T_TOP];
        d.stats.filled_large = tail[LDU_T_LARGE]; d.stats.left_empty = tail[LDU_T_EMPTY];
    } else {
        const uint32_t *finish = tail, *chain = tail + d.tiles * 4;
        for (size_t t = 0; t < d.tiles; ++t) {
            d.stats.measured += chain[2 * t]; d.stats.filled_small += chain[2 * t + 1];
            d.stats.filled_top += finish[4 * t]; d.stats.filled_large += finish[4 * t + 1]; d.stats.left_empty += finish[4 * t + 2];
        }
    }
    HIPCK(hipEventElapsedTime(&d.stats.device_ms, d.ev[0], d.ev[d.n_slots]));
    if (d.timed)
        for (int k = 0, last = 0; k < d.n_slots; ++k)
            if (d.ran[k]) { HIPCK(hipEventElapsedTime(&d.stats.launch_ms[k], d.ev[last], d.ev[k + 1])); last = k + 1; }
    return SM_OK;
}

// after launch `slot` of a call: its event (the last slot's always: device_ms ends there), its place in the tally
int ld_launched(sm_ctx *s, int slot)
{
    LidarDepth &d = s->ldepth;
    d.ran[slot] = true;
    d.stats.launches++;
    if (d.timed || slot == d.n_slots - 1) HIPCK(hipEventRecord(d.ev[slot + 1], s->stream));
    return SM_OK;
}

// the four launches
int ld_fused(sm_ctx *s, const LdArgs &a)
{
    LidarDepth &d = s->ldepth;
    int rc;
    hipLaunchKernelGGL(k_ld_chain, dim3((unsigned)d.tiles), dim3(LD_THREADS), 0, s->stream, a);
    if ((rc = ld_launched(s, 1))) return rc;
    if (a.stages & LD_FILL_LARGE) {
        hipLaunchKernelGGL(k_ld_rowmax, dim3((unsigned)((a.W + LD_ROW - 1) / LD_ROW), (unsigned)a.H), dim3(LD_ROW), 0, s->stream, a);
        if ((rc = ld_launched(s, 2))) return rc;
    }
    hipLaunchKernelGGL(k_ld_finish, dim3((unsigned)d.tiles), dim3(LD_THREADS), 0, s->stream, a);
    return ld_launched(s, 3);
}

// every step a launch of its own (SM_LIDAR_DEPTH_UNFUSED=1)
int ld_unfused(sm_ctx *s, const LdArgs &a)
{
    LidarDepth &d = s->ldepth;
    int rc;
    uint32_t *tally = d.d_part.get() + d.part_project;
    uint16_t *cur = d.d_v, *nxt = d.d_tmp;
    const dim3 grid((unsigned)(((size_t)a.W * a.H + 255) / 256)), block(256);
    HIPCK(hipMemsetAsync(tally, 0, 32, s->stream));
    hipLaunchKernelGGL(k_ld_u_init, grid, block, 0, s->stream, a, cur, tally);
    if ((rc = ld_launched(s, 1))) return rc;
#define LD_STEP(S, slot)                                                                          \
    do {                                                                                          \
        hipLaunchKernelGGL(k_ld_u_step<S>, grid, block, 0, s->stream, a, (const uint16_t *)cur, nxt, tally); \
        if ((rc = ld_launched(s, slot))) return rc;                                               \
        std::swap(cur, nxt);                                                                      \
    } while (0)
    if (a.stages & LD_DILATE) LD_STEP(LDU_DILATE, 2);
    if (a.stages & LD_CLOSE) { LD_STEP(LDU_MAX5, 3); LD_STEP(LDU_MIN5, 4); }
    if (a.stages & LD_FILL_SMALL) LD_STEP(LDU_FILL7, 5);
    if (a.stages & LD_EXTEND_TOP) {
        hipLaunchKernelGGL(k_ld_u_top, dim3((unsigned)((a.W + 63) / 64)), dim3(64, 16), 0, s->stream, a, (const uint16_t *)cur, nxt, tally);
        if ((rc = ld_launched(s, 6))) return rc;
        std::swap(cur, nxt);
    }
    if (a.stages & LD_FILL_LARGE) {
        hipLaunchKernelGGL(k_ld_u_step<LDU_ROWMAX>, grid, block, 0, s->stream, a, (const uint16_t *)cur, a.rowmax, tally);
        if ((rc = ld_launched(s, 7))) return rc;
        LD_STEP(LDU_COLMAX, 8);
    }
    if (a.stages & LD_MEDIAN) LD_STEP(LDU_MEDIAN, 9);
    if (a.stages & LD_SMOOTH) LD_STEP(LDU_SMOOTH, 10);
#undef LD_STEP
    hipLaunchKernelGGL(k_ld_u_step<LDU_OUT>, grid, block, 0, s->stream, a, (const uint16_t *)cur, nxt, tally);
    return ld_launched(s, 11);
}

// the whole chain for a scan on the device, enqueued on the context's stream
int ld_device(sm_ctx *s, const float *d_points, uint32_t n, const float *T16, uint16_t *d_depth, uint16_t *d_sparse, int32_t *d_index)
{
    LidarDepth &d = s->ldepth;
    int rc;
    // A call that nobody asked the tally of is not folded: this call's parts and events replace it, in stream order, and the
    // host waits for nothing.
    d.pending = false;
    const int W = s->W, H = s->H;
    d.stats = sm_lidar_depth_stats_t{};
    d.stats.points = n;
    for (float &ms : d.stats.launch_ms) ms = -1.0f;
    for (bool &r : d.ran) r = false;
    d.n_slots = d.unfused ? LidarDepth::MAX_LAUNCHES : 4;

    LdProjectArgs pa{};
    pa.points = (const float4 *)d_points; pa.n = n;
    for (int i = 0; i < 12; ++i) pa.T[i] = T16[i];
    pa.fx = s->cfg.fx; pa.fy = s->cfg.fy; pa.cx = s->cfg.cx; pa.cy = s->cfg.cy;
    pa.min_z = d.p.min_z; pa.max_z = d.p.max_z;
    pa.W = W; pa.H = H;
    pa.key = d.d_key; pa.top = d.d_top; pa.part = d.d_part;
    LdArgs a{};
    a.key = d.d_key; a.v = d.d_v; a.rowmax = d.d_rowmax; a.top = d.d_top;
    a.depth = d_depth; a.sparse = d_sparse; a.index = d_index;
    a.part_finish = (uint4 *)(d.d_part.get() + d.part_project);
    a.part_chain = (uint2 *)(d.d_part.get() + d.part_project + d.tiles * 4);
    a.W = W; a.H = H; a.tiles_x = (W + LD_TILE - 1) / LD_TILE;
    a.stages = d.p.stages; a.R = d.p.large / 2; a.tol = d.p.tol_256;

    d.blocks_project = (std::max<uint32_t>(n, (uint32_t)W) + 255u) / 256u;
    HIPCK(hipEventRecord(d.ev[0], s->stream));
    hipLaunchKernelGGL(k_ld_project, dim3(d.blocks_project), dim3(256), 0, s->stream, pa);
    if ((rc = ld_launched(s, 0))) return rc;
    if ((rc = d.unfused ? ld_unfused(s, a) : ld_fused(s, a))) return rc;
    HIPCK(hipGetLastError());
    d.stats_valid = true;
    d.pending = true;
    return SM_OK;
}

}  // namespace

extern "C" {

int sm_default_lidar_depth_params(const sm_config *c, sm_lidar_depth_params *p)
{
    if (!c || !p) { g_err = "sm_default_lidar_depth_params: null argument"; return SM_E_ARG; }
    p->min_z = 0.5f;
    p->max_z = 65.0f;
    p->stages = 127;
    p->large = 31;
    p->tol_256 = 13;
    return SM_OK;
}

int sm_set_lidar_depth(sm_ctx *s, const sm_lidar_depth_params *p)
{
    const char *who = "sm_set_lidar_depth";
    int rc;
    if ((rc = ld_check(s, false, who))) return rc;
    if (p)
        if (const char *why = check_params(*p)) { g_err = std::string(who) + ": " + why; return SM_E_ARG; }
    if (p && s->H > 65535) { g_err = std::string(who) + ": images higher than 65535 rows"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (s->ldepth.on) HIPCK(hipStreamSynchronize(s->stream));       // an enqueued call still uses the planes
    s->ldepth = LidarDepth();
    if (!p) return SM_OK;
    LidarDepth d;
    d.p = *p;
    const size_t P = (size_t)s->P;
    d.tiles = (size_t)((s->W + LD_TILE - 1) / LD_TILE) * (size_t)((s->H + LD_TILE - 1) / LD_TILE);
    d.part_project = (std::max<size_t>(SM_LIDAR_DEPTH_MAX_POINTS, (size_t)s->W) + 255) / 256;
    if ((rc = dalloc(d.d_key, P)) || (rc = dalloc(d.d_v, P)) || (rc = dalloc(d.d_rowmax, P)) || (rc = dalloc(d.d_top, (size_t)s->W)) ||
        (rc = dalloc(d.d_part, d.part_project + std::max<size_t>(d.tiles * 6, 8))) || (rc = dalloc(d.d_depth, P)) || (rc = dalloc(d.d_sparse, P)) ||
        (rc = dalloc(d.d_index, P))) {
        (void)hipGetLastError();                         // (the failed allocation's error is reported, not left behind)
        return rc;
    }
    fill_keys(s, d.d_key, P);                            // every call leaves them as it found them
    HIPCK(hipGetLastError());
    const char *te = std::getenv("SM_LIDAR_DEPTH_TIMING"), *ue = std::getenv("SM_LIDAR_DEPTH_UNFUSED");
    d.timed = te && te[0] == '1';
    d.unfused = ue && ue[0] == '1';
    if (d.unfused && (rc = dalloc(d.d_tmp, P))) { (void)hipGetLastError(); return rc; }
    for (Event &e : d.ev) HIPCK(hipEventCreate(e.put()));
    HIPCK(hipStreamSynchronize(s->stream));
    d.on = true;
    s->ldepth = std::move(d);
    return SM_OK;
}

int sm_lidar_depth_device(sm_ctx *s, const float *d_points4, uint32_t n, const float *T16, uint16_t *d_depth_mm_out, uint16_t *d_sparse_mm_out,
                          int32_t *d_index_out)
{
    const char *who = "sm_lidar_depth_device";
    if (int rc = ld_check_call(s, d_points4, n, T16, d_depth_mm_out, d_sparse_mm_out, d_index_out, who)) return rc;
    if ((uintptr_t)d_points4 & 15u) { g_err = std::string(who) + ": misaligned points"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    return ld_device(s, d_points4, n, T16, d_depth_mm_out, d_sparse_mm_out, d_index_out);
}

int sm_lidar_depth(sm_ctx *s, const float *points4, uint32_t n, const float *T16, uint16_t *depth_mm_out, uint16_t *sparse_mm_out, int32_t *index_out)
{
    const char *who = "sm_lidar_depth";
    int rc;
    if ((rc = ld_check_call(s, points4, n, T16, depth_mm_out, sparse_mm_out, index_out, who))) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    LidarDepth &d = s->ldepth;
    const size_t P = (size_t)s->P;
    if (n > d.points_cap) {
        HIPCK(hipStreamSynchronize(s->stream));          // an enqueued call still reads the old copy
        d.points_cap = 0;
        if ((rc = dalloc(d.d_points, (size_t)n))) return rc;
        d.points_cap = n;
    }
    if (n) HIPCK(hipMemcpyAsync(d.d_points, points4, (size_t)n * 16, hipMemcpyHostToDevice, s->stream));
    if ((rc = ld_device(s, (const float *)d.d_points.get(), n, T16, depth_mm_out ? d.d_depth.get() : nullptr,
                        sparse_mm_out ? d.d_sparse.get() : nullptr, index_out ? d.d_index.get() : nullptr)))
        return rc;
    if (depth_mm_out) HIPCK(hipMemcpyAsync(depth_mm_out, d.d_depth, P * 2, hipMemcpyDeviceToHost, s->stream));
    if (sparse_mm_out) HIPCK(hipMemcpyAsync(sparse_mm_out, d.d_sparse, P * 2, hipMemcpyDeviceToHost, s->stream));
    if (index_out) HIPCK(hipMemcpyAsync(index_out, d.d_index, P * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

int sm_lidar_depth_stats(sm_ctx *s, sm_lidar_depth_stats_t *out)
{
    const char *who = "sm_lidar_depth_stats";
    if (int rc = ld_check(s, true, who)) return rc;
    if (!out) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if (!s->ldepth.stats_valid) { g_err = std::string(who) + ": no call yet"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (int rc = ld_fold(s)) return rc;
    *out = s->ldepth.stats;
    return SM_OK;
}

}  // extern "C"
