// sm_k_track_rgb.h -- the colour term of the tracker: photometric + geometric Gauss-Newton over a luminance pyramid, coarse to
// fine (sm_track_frame_rgb; DESIGN.md "4d. Tracking", "colour term").  Included by sm_track.hip only, after sm_k_track.h, whose
// prediction, vertex stage, pair rule, partial sums, LDLT and step it uses unchanged.
//
// One tracked frame, after sm_track_frame's prediction (k_track_splat, k_track_resolve):
//   k_track_luma_pyr  the frame's luminance and its 2x2-mean pyramid, one 32x32 tile per workgroup: level 0 from the rgb bytes,
//                     every further level from the tile's previous level in LDS (32 = 2^5 covers the six levels allowed).
//   k_track_gather    slot map -> dense float4 plane (surfel centre, luminance of its colour word; w < 0: no surfel).
//   then per level l = levels-1 .. 0, at stride pixel_stride * 2^l:  k_track_vertex, and iters[l] times
//   k_track_rgb_icp   k_track_reduce's body on that grid                                  -> 29 partials per workgroup
//   k_track_rgb_photo the photometric samples of the same grid of the prediction          -> 29 partials per workgroup, unweighted
//   k_track_rgb_solve fixed-order sums of both, A = A_icp + lambda A_rgb in double, k_track_solve's step, the level schedule.
// Every per-iteration launch names its level; it is a no-op unless the device-side state is at that level and not done, so a
// level that converges early skips its remaining launches and the host still waits once.

#pragma once

#include "sm_k_track.h"

namespace sm {

constexpr int TRACK_RGB_LEVELS = 6;
constexpr int TRACK_RGB_TILE = 32;       // 2^(TRACK_RGB_LEVELS - 1): one tile holds one pixel of the coarsest level

struct TrackRgbParams {
    int levels;
    int iters[TRACK_RGB_LEVELS];
    int lw[TRACK_RGB_LEVELS], lh[TRACK_RGB_LEVELS];   // level sizes: floor(W / 2^l), floor(H / 2^l)
    int off[TRACK_RGB_LEVELS];                         // first float of level l in the pyramid buffer
    float max_residual;
    double lambda;
};

struct TrackRgbState {
    double sys_icp[32], sys_rgb[32];     // the two terms of the last system (TRACK_NSYS used), rgb unweighted
    double rgb_rmse;
    int32_t level, level_it;             // the level being solved, systems solved at it so far
    uint32_t rgb_inliers;
    int32_t pad;
    int32_t level_iterations[TRACK_RGB_LEVELS];
};

// Y = ((0.299 R + 0.587 G) + 0.114 B) / 255 of 8-bit channels
__device__ __forceinline__ float track_luma(uint32_t r, uint32_t g, uint32_t b)
{
    return ((0.299f * (float)r + 0.587f * (float)g) + 0.114f * (float)b) / 255.0f;
}

// grid (ceil(W / 32), ceil(H / 32)), 256 threads.  Level l+1 pixel (x, y) = mean of level l's (2x, 2y) .. (2x+1, 2y+1), kept iff
// it lies inside floor(W / 2^(l+1)) x floor(H / 2^(l+1)): then all its level-0 pixels are inside the image and inside this tile.
__global__ __launch_bounds__(256) void k_track_luma_pyr(const uint8_t *__restrict__ rgb, int W, int H, TrackRgbParams rp,
                                                        float *__restrict__ pyr)
{
    __shared__ float s_a[TRACK_RGB_TILE * TRACK_RGB_TILE];
    __shared__ float s_b[TRACK_RGB_TILE * TRACK_RGB_TILE / 4];
    const int tx0 = blockIdx.x * TRACK_RGB_TILE, ty0 = blockIdx.y * TRACK_RGB_TILE;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = threadIdx.x + k * 256;
        const int gx = tx0 + (q & 31), gy = ty0 + (q >> 5);
        float y = 0.0f;
        if (gx < W && gy < H) {
            const uint8_t *c = rgb + ((size_t)gy * W + gx) * 3;
            y = track_luma(c[0], c[1], c[2]);
            pyr[(size_t)gy * W + gx] = y;
        }
        s_a[q] = y;
    }
    __syncthreads();
    float *src = s_a, *dst = s_b;
    int n = TRACK_RGB_TILE;
    for (int l = 1; l < rp.levels; ++l) {
        n >>= 1;
        for (int q = threadIdx.x; q < n * n; q += 256) {
            const int lx = q % n, ly = q / n;
            const float *t = src + (2 * ly) * (2 * n) + 2 * lx;
            const float v = ((t[0] + t[1]) + (t[2 * n] + t[2 * n + 1])) * 0.25f;
            const int gx = (tx0 >> l) + lx, gy = (ty0 >> l) + ly;
            if (gx < rp.lw[l] && gy < rp.lh[l]) pyr[(size_t)rp.off[l] + (size_t)gy * rp.lw[l] + gx] = v;
            dst[q] = v;
        }
        __syncthreads();
        float *x = src; src = dst; dst = x;
    }
}

__global__ __launch_bounds__(256) void k_track_gather(Model M, const DevState *__restrict__ st, const int32_t *__restrict__ pred,
                                                      int npix, float4 *__restrict__ plane)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int32_t s = pred[p];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    if (s >= 0) {
        const SurfelSet cur = M.s[st->cur];
        const float4 pc = cur.pos_conf[s];
        const uint32_t c = cur.color[s];
        o = make_float4(pc.x, pc.y, pc.z, track_luma((c >> 16) & 0xFFu, (c >> 8) & 0xFFu, c & 0xFFu));
    }
    plane[p] = o;
}

__device__ __forceinline__ bool track_rgb_active(const TrackState *__restrict__ ts, const TrackRgbState *__restrict__ rs, int level)
{
    return !ts->done && rs->level == level;
}

// the geometric term of level `level`: tp is that level's grid (stride pixel_stride * 2^level), vmap / nmap its vertex stage
__global__ __launch_bounds__(TRACK_BLOCK) void k_track_rgb_icp(Model M, const DevState *__restrict__ st, TrackParams tp, int level,
                                                               const float4 *__restrict__ vmap, const float4 *__restrict__ nmap,
                                                               const int32_t *__restrict__ pred, const TrackState *__restrict__ ts,
                                                               const TrackRgbState *__restrict__ rs, double *__restrict__ part)
{
    if (!track_rgb_active(ts, rs, level)) return;
    __shared__ double s_w[TRACK_BLOCK / 64][TRACK_NSYS];
    track_reduce_body(M, st, tp, vmap, nmap, pred, ts, part, s_w);
}

// photometric sample of prediction pixel (i, j) under the pose `m`: the surfel there (pm: centre, luminance) projected into the
// current frame, gated by the frame's depth, sampled bilinearly in level image `img` (lw x lh, 1 / 2^level = inv_s)
__device__ __forceinline__ bool track_rgb_sample(const float4 pm, const float *m, const TrackParams &tp, const uint16_t *__restrict__ mm,
                                                 const float *__restrict__ img, int lw, int lh, float inv_s, float max_residual,
                                                 float *J, float &r)
{
    if (pm.w < 0.0f) return false;
    const float dx = pm.x - m[12], dy = pm.y - m[13], dz = pm.z - m[14];
    const float cx = (m[0] * dx + m[1] * dy) + m[2] * dz;     // R^T (p - t)
    const float cy = (m[4] * dx + m[5] * dy) + m[6] * dz;
    const float cz = (m[8] * dx + m[9] * dy) + m[10] * dz;
    if (!(cz > 0.0f)) return false;
    const float x = (tp.fx * cx) / cz + tp.cx, y = (tp.fy * cy) / cz + tp.cy;
    if (!(x >= 0.0f && x < (float)tp.W && y >= 0.0f && y < (float)tp.H)) return false;
    const float D = track_depth(mm, (int)x, (int)y, tp);
    if (D == 0.0f || !(fabsf(D - cz) <= tp.dist)) return false;
    const float u = x * inv_s - 0.5f, v = y * inv_s - 0.5f;
    const float fu = floorf(u), fv = floorf(v);
    if (!(fu >= 0.0f && fu < (float)(lw - 1) && fv >= 0.0f && fv < (float)(lh - 1))) return false;
    const float a = u - fu, b = v - fv;
    const float *t = img + (size_t)(int)fv * lw + (int)fu;
    const float i00 = t[0], i10 = t[1], i01 = t[lw], i11 = t[lw + 1];
    const float d0 = i10 - i00, d1 = i11 - i01;
    const float top = i00 + a * d0, bot = i01 + a * d1;
    const float dv = bot - top;
    r = (top + b * dv) - pm.w;
    if (!(fabsf(r) < max_residual)) return false;
    const float gx = (d0 + b * (d1 - d0)) * inv_s, gy = dv * inv_s;
    const float ga = (gx * tp.fx) / cz, gb = (gy * tp.fy) / cz;
    const float gc = -((ga * cx + gb * cy) / cz);
    const float3 gw = rot3(m, ga, gb, gc);
    const float3 pg = cross3(make_float3(pm.x, pm.y, pm.z), gw);
    J[0] = -gw.x; J[1] = -gw.y; J[2] = -gw.z; J[3] = -pg.x; J[4] = -pg.y; J[5] = -pg.z;
    return true;
}

// the photometric term of level `level`, unweighted; the same fixed lane -> grid point map as the geometric reduction
__global__ __launch_bounds__(TRACK_BLOCK) void k_track_rgb_photo(TrackParams tp, TrackRgbParams rp, int level,
                                                                 const uint16_t *__restrict__ mm, const float4 *__restrict__ plane,
                                                                 const float *__restrict__ pyr, const TrackState *__restrict__ ts,
                                                                 const TrackRgbState *__restrict__ rs, double *__restrict__ part)
{
    if (!track_rgb_active(ts, rs, level)) return;
    __shared__ double s_w[TRACK_BLOCK / 64][TRACK_NSYS];
    float m[16];
    track_pose_f(ts, m);
    const float *img = pyr + rp.off[level];
    const int lw = rp.lw[level], lh = rp.lh[level];
    const float inv_s = 1.0f / (float)(1 << level);
    double acc[TRACK_NSYS];
#pragma unroll
    for (int e = 0; e < TRACK_NSYS; ++e) acc[e] = 0.0;
    const int step = tp.nb * TRACK_BLOCK;
    for (int idx = blockIdx.x * TRACK_BLOCK + threadIdx.x; idx < tp.n; idx += step) {
        const int gj = idx / tp.ni;
        const int i = (idx - gj * tp.ni) * tp.stride, j = gj * tp.stride;
        float J[6], r;
        if (!track_rgb_sample(plane[(size_t)j * tp.W + i], m, tp, mm, img, lw, lh, inv_s, rp.max_residual, J, r)) continue;
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[e++] += (double)(J[a] * J[b]);
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] += (double)(J[a] * r);
        acc[27] += (double)(r * r);
        acc[28] += 1.0;
    }
    track_block_sum(acc, s_w, tp.nb, part);
}

// one workgroup.  sum_only: the sums only (sm_track_rgb_debug).  ts->sys receives the joint system: values 0..27 are
// icp + lambda * rgb, value 28 the geometric inlier count
__global__ __launch_bounds__(256) void k_track_rgb_solve(TrackParams tp, TrackRgbParams rp, int level, const double *__restrict__ part_icp,
                                                         const double *__restrict__ part_rgb, TrackState *__restrict__ ts,
                                                         TrackRgbState *__restrict__ rs, int sum_only)
{
    if (!track_rgb_active(ts, rs, level)) return;
    __shared__ double s_p[TRACK_NSYS][8];
    double si[TRACK_NSYS], sr[TRACK_NSYS];
    track_sum_parts(part_icp, tp.nb, s_p, si);
    __syncthreads();
    track_sum_parts(part_rgb, tp.nb, s_p, sr);
    if (threadIdx.x != 0) return;
    double sys[TRACK_NSYS];
    for (int e = 0; e < TRACK_NSYS; ++e) {
        rs->sys_icp[e] = si[e];
        rs->sys_rgb[e] = sr[e];
        sys[e] = (e == 28 || rp.lambda == 0.0) ? si[e] : si[e] + rp.lambda * sr[e];
        ts->sys[e] = sys[e];
    }
    if (sum_only) return;
    const double cnt = si[28];
    ts->iterations += 1;
    rs->level_iterations[level] += 1;
    rs->level_it += 1;
    ts->inliers = (uint32_t)cnt;
    ts->rmse = cnt > 0.0 ? sqrt(si[27] / cnt) : 0.0;
    rs->rgb_inliers = (uint32_t)sr[28];
    rs->rgb_rmse = sr[28] > 0.0 ? sqrt(sr[27] / sr[28]) : 0.0;
    if (ts->iterations == 1 && ts->in_view == 0u) { track_fail(ts, TRACK_NO_MODEL); return; }
    // (a grid of stride 2^level has 4^-level of the samples)
    if (cnt * (double)(1 << (2 * level)) < (double)tp.min_inliers || cnt < 6.0) { track_fail(ts, TRACK_LOST); return; }
    double A[6][6], b[6];
    track_unpack(sys, A, b);
    ts->pivot_ratio = track_pivot_ratio(A, tp.c);
    const bool degenerate = !(ts->pivot_ratio >= tp.degenerate_bound);
    if (!track_step(A, b, ts)) { track_fail(ts, TRACK_DEGENERATE); return; }
    const bool converged = ts->step_rot < 1e-6 && ts->step_trans < 1e-6;
    if (!(converged || rs->level_it >= rp.iters[level])) return;
    // the level ends: the next finer one, or the frame (DEGENERATE is judged on this, the last level-0 system)
    if (level > 0) { rs->level = level - 1; rs->level_it = 0; return; }
    if (degenerate) { track_fail(ts, TRACK_DEGENERATE); return; }
    ts->done = 1;
}

}  // namespace sm
