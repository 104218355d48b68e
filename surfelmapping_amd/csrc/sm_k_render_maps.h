// sm_k_render_maps.h -- views of a map set (DESIGN.md "4f. Views of a map set"): the renderers of sm_k_io.h / sm_k_view.h over
// chunks of map-file records instead of the resident model.  Included by sm_render_maps.hip only.
//   k_maps_intake        48-byte records -> chunk-local SoA planes (the layout of SurfelSet) + one box per 256 records
//   k_maps_splat_image   grid (blocks of the chunk, views of the batch): box test, then render_surfel per record
//   k_maps_splat_view    the same for the model view: view_surfel per record, large discs by the record's wave
//   k_maps_resolve_*     per pixel of the views the chunk touched: a key whose id lies in the chunk is shaded from its row
//   k_maps_finish_*      after the last source: pixels nobody won take the clear values
// Every per-surfel and per-pixel rule is sm_k_draw.h's, shared with the resident kernels: a record drawn here sets the key
// bits it would set as slot `id` of a model holding the whole set, and the keys are merged by the same atomicMin.
// The chunk's planes and the box layout are in sm_k_maps_box.h, shared with the lidar sweeps (sm_k_lidar.h).
#pragma once

#include "sm_device.h"
#include "sm_k_draw.h"
#include "sm_k_maps_box.h"

namespace sm {

// The disc's reach from its centre.  Its four vertices are c +- x, c +- y with |x| = |u| * r' * 1.41421356, |u| = 1 up to a few
// ulps (u is normalised), r' <= |r|, and y = d x x, so |y| <= |d| |x| (1 + a few ulps); 1e-4 covers the roundings (those of
// |d| = sqrt(d . d) included) many times over.  What d is decides the reach:
//   novel view (render_surfel): d is the rotated normal NORMALISED, or (0, 0, 1): |d| = 1, whatever the file and the pose hold
//   model view (view_disc):     d is the STORED normal as it is (near branch) or column 2 of the view's mv_inv as it is (far
//                               branch); both are caller input and need not be unit vectors.  So the reach is
//                               1.41421356 * |r| * max(1, |n|) resp. 1.41421356 * |r| * max(1, |mv_inv col 2|); a block may
//                               hold discs of both branches, so the larger bound of the two is taken.
__device__ __forceinline__ float maps_reach(float rmax) { return (1.41421356f * rmax) * 1.0001f; }
__device__ __forceinline__ float maps_reach_view(const MapsBox &b, float la /* |mv_inv col 2| */)
{
    return maps_reach(fmaxf(b.rnorm, b.rmax * fmaxf(1.0f, la)));
}

// ---------------------------------------------------------------------------------------------
// The box tests.  True = no record of the block can set a key in this view.  Conservative by construction:
//
// (1) A block with a record whose centre, radius or normal is not finite (rnorm = +inf, set by k_maps_intake) and a box with a
//     non-finite bound are not tested at all: maps_box_finite comes first.  (fminf / fmaxf skip a NaN, so the box of such a
//     block bounds its finite records only -- that is why the intake's flag, not the box, protects it.)  A model view whose
//     mv_inv column 2 has no finite length is not tested either.  Every comparison that reports "outside" is strict and false on a
//     NaN; an overflow of an intermediate gives +inf on the left-hand side (every term added to the corner maximum is >= 0).
//     A view with a NaN in it draws nothing whatever is tested: no vertex passes Z > 0 resp. w > 0.
// (2) A drawn record's centre c lies in [lo, hi], all four vertices v = c + d, |d| <= R = maps_reach(rmax) (novel view) resp.
//     maps_reach_view (model view; unit normals and a rigid mv_inv are NOT assumed, see above), pass the
//     renderer's vertex test (novel view: Z > 0; model view: clip w > 0), and a pixel is set only inside the vertices' pixel box
//     clipped to the image.  So a record draws nothing if all its vertices are on the outer side of one image side.
// (3) "Outer side" is a linear form f with f(v) < 0 (below).  f(v) <= max over the 8 box corners of f + |grad f| * R, because f
//     is affine and c is a convex combination of the corners.  What floating point adds is bounded by `slack`: every float
//     evaluation of an affine row sum(a_j p_j) + t errs by at most 3 ulps of A = sum|a_j p_j| + |t| (< 2e-7 A); the tests charge
//     4e-6 A (model view: the per-vertex clip rows) or move the centre by 4E, E = 1e-6 * the largest A of xform3 (novel view: the
//     camera-space centre and corners, each within sqrt(3) * 2e-7 A of its true value).
// (4) The image sides are moved out by 2 pixels + 1e-4 of the image terms (mp below), which covers the roundings between the
//     vertex's clip / camera coordinates and its fixed-point window position (relative 1e-6 of terms bounded by the view's
//     |cx| + cols resp. width), and the half pixel between a vertex and the pixel centres it can cover.
// tests/test_render_maps.py restates both tests in numpy and checks (2)-(4) against the per-surfel rules on random blocks.
// ---------------------------------------------------------------------------------------------

// novel view: 1 < z < 200 (draw_image_adaptive.geom:41) and the four image sides, in camera space
__device__ __forceinline__ bool maps_box_outside_image(const MapsBox &b, const RenderParams &rp)
{
    if (!maps_box_finite(b)) return false;
    const float *m = rp.t_inv;
    const float R = maps_reach(b.rmax);
    const float mpx = 2.0f + 1.0e-4f * (fabsf(rp.cx) + rp.cols), mpy = 2.0f + 1.0e-4f * (fabsf(rp.cy) + rp.rows);
    // f < 0: left of x = -mp, right of x = cols + mp, above y = -mp, below y = rows + mp (for Z > 0)
    const float cl = rp.cx + mpx, cr = (rp.cols + mpx) - rp.cx, ct = rp.cy + mpy, cb = (rp.rows + mpy) - rp.cy;
    float zmin = 3.0e38f, zmax = -3.0e38f, mag = 0.0f;
    float fl = -3.0e38f, fr = -3.0e38f, ft = -3.0e38f, fb = -3.0e38f, al = 0.0f, ar = 0.0f, at = 0.0f, ab = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float x = (c & 1) ? b.hx : b.lx, y = (c & 2) ? b.hy : b.ly, z = (c & 4) ? b.hz : b.lz;
        const float3 p = xform3(m, x, y, z);
        const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
        mag = fmaxf(mag, fmaxf(((fabsf(m[0]) * ax + fabsf(m[4]) * ay) + fabsf(m[8]) * az) + fabsf(m[12]),
                           fmaxf(((fabsf(m[1]) * ax + fabsf(m[5]) * ay) + fabsf(m[9]) * az) + fabsf(m[13]),
                                 ((fabsf(m[2]) * ax + fabsf(m[6]) * ay) + fabsf(m[10]) * az) + fabsf(m[14]))));
        zmin = fminf(zmin, p.z); zmax = fmaxf(zmax, p.z);
        fl = fmaxf(fl, rp.fx * p.x + cl * p.z);  al = fmaxf(al, fabsf(rp.fx * p.x) + fabsf(cl * p.z));
        fr = fmaxf(fr, cr * p.z - rp.fx * p.x);  ar = fmaxf(ar, fabsf(rp.fx * p.x) + fabsf(cr * p.z));
        ft = fmaxf(ft, rp.fy * p.y + ct * p.z);  at = fmaxf(at, fabsf(rp.fy * p.y) + fabsf(ct * p.z));
        fb = fmaxf(fb, cb * p.z - rp.fy * p.y);  ab = fmaxf(ab, fabsf(rp.fy * p.y) + fabsf(cb * p.z));
    }
    const float E4 = 4.0e-6f * mag, Rc = (R + E4) * 1.0001f;
    if (zmax + E4 < 1.0f) return true;                                      // every centre fails ph.z > 1
    if (zmin - E4 > 200.0f) return true;                                    // ... or ph.z < maxDepth
    const float gx = sqrtf(rp.fx * rp.fx + fmaxf(cl * cl, cr * cr)) * 1.0001f, gy = sqrtf(rp.fy * rp.fy + fmaxf(ct * ct, cb * cb)) * 1.0001f;
    if (fl + (gx * Rc + 4.0e-6f * al) < 0.0f) return true;
    if (fr + (gx * Rc + 4.0e-6f * ar) < 0.0f) return true;
    if (ft + (gy * Rc + 4.0e-6f * at) < 0.0f) return true;
    if (fb + (gy * Rc + 4.0e-6f * ab) < 0.0f) return true;
    return false;
}

// one clip-space form over the box: f(p) = (row_a + s * row_w) . (p, 1), its largest value over the corners plus everything (3)
// charges; `sgn` -1 turns row_a round (the right / top sides)
__device__ __forceinline__ float maps_clip_form(const MapsBox &b, const float *m, int row, float sgn, float s, float R)
{
    const float ax = sgn * m[row] + s * m[3], ay = sgn * m[row + 4] + s * m[7], az = sgn * m[row + 8] + s * m[11],
                at = sgn * m[row + 12] + s * m[15];
    // |a_j| of the two rows apart: the per-vertex evaluation rounds them apart
    const float qx = fabsf(m[row]) + s * fabsf(m[3]), qy = fabsf(m[row + 4]) + s * fabsf(m[7]), qz = fabsf(m[row + 8]) + s * fabsf(m[11]),
                qt = fabsf(m[row + 12]) + s * fabsf(m[15]);
    float f = -3.0e38f, A = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float x = (c & 1) ? b.hx : b.lx, y = (c & 2) ? b.hy : b.ly, z = (c & 4) ? b.hz : b.lz;
        f = fmaxf(f, ((ax * x + ay * y) + az * z) + at);
        A = fmaxf(A, ((qx * fabsf(x) + qy * fabsf(y)) + qz * fabsf(z)) + qt);
    }
    const float g = sqrtf((ax * ax + ay * ay) + az * az) * 1.0001f, q = sqrtf((qx * qx + qy * qy) + qz * qz);
    return f + (g * R + 4.0e-6f * (A + q * R));
}

// model view, discs and points alike: clip w > 0 and the four side planes, in world space (the box's own)
__device__ __forceinline__ bool maps_box_outside_view(const MapsBox &b, const ViewParams &vp)
{
    if (!maps_box_finite(b)) return false;
    const float la = sqrtf((vp.mvinv[8] * vp.mvinv[8] + vp.mvinv[9] * vp.mvinv[9]) + vp.mvinv[10] * vp.mvinv[10]);
    if (!(la - la == 0.0f)) return false;                                   // no finite bound on the far branch's y
    const float R = maps_reach_view(b, la);
    // xw = ((x/w) * 0.5 + 0.5) * W < -mp  <=>  x + (1 + 2 mp / W) w < 0  (w > 0)
    const float sx = 1.0f + 2.0f * (2.0f + 1.0e-4f * (float)vp.w) / (float)vp.w, sy = 1.0f + 2.0f * (2.0f + 1.0e-4f * (float)vp.h) / (float)vp.h;
    if (maps_clip_form(b, vp.mvp, 3, 0.0f, 1.0f, R) < 0.0f) return true;   // every vertex has w < 0 (row_w alone)
    if (maps_clip_form(b, vp.mvp, 0, 1.0f, sx, R) < 0.0f) return true;     // left
    if (maps_clip_form(b, vp.mvp, 0, -1.0f, sx, R) < 0.0f) return true;    // right
    if (maps_clip_form(b, vp.mvp, 1, 1.0f, sy, R) < 0.0f) return true;     // bottom
    if (maps_clip_form(b, vp.mvp, 1, -1.0f, sy, R) < 0.0f) return true;    // top
    return false;
}

// ---------------------------------------------------------------------------------------------
// Chunk intake: k_retire_gather in reverse.  A workgroup's 256 records are 768 consecutive float4s: read by consecutive lanes,
// laid out in LDS as they lie in memory, then each lane takes its own record out of LDS (12 KiB) and writes one element of every
// plane -- consecutive lanes on consecutive addresses both ways, no lane walks memory with the record's 48-byte stride.
// The box in the same pass: wave reductions (shuffles), then LDS across the four waves.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float maps_wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float maps_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(256) void k_maps_intake(const float4 *__restrict__ rec, uint32_t n, MapsSoA out, float4 *__restrict__ box)
{
    __shared__ float4 s_rec[MAPS_BLOCK * 3];             // 12 KiB
    __shared__ float s_red[4][9];
    const uint32_t first = blockIdx.x * (uint32_t)MAPS_BLOCK;
    const uint32_t m = min((uint32_t)MAPS_BLOCK, n - first);                // records of this block (>= 1: the grid is ceil(n / 256))
    const float4 *src = rec + (size_t)first * 3;
    for (uint32_t i = threadIdx.x; i < m * 3u; i += 256u) s_rec[i] = src[i];
    __syncthreads();
    const bool have = threadIdx.x < m;
    float4 pc = make_float4(0, 0, 0, 0), ct = pc, nr = pc;
    if (have) {
        pc = s_rec[threadIdx.x * 3 + 0]; ct = s_rec[threadIdx.x * 3 + 1]; nr = s_rec[threadIdx.x * 3 + 2];
        const uint32_t k = first + threadIdx.x;
        out.pos_conf[k] = pc;
        out.norm_rad[k] = nr;
        out.color[k] = __float_as_uint(ct.x);
        out.time[k] = ct.w;
    }
    const float INF = __uint_as_float(0x7F800000u);
    const float ra = fabsf(nr.w);
    const float ln = sqrtf((nr.x * nr.x + nr.y * nr.y) + nr.z * nr.z);     // (+inf / NaN if the normal is, or its square overflows)
    const float rn = ra * fmaxf(1.0f, ln);                                  // (fmaxf skips a NaN: ln is tested itself)
    const bool bad = have && !((pc.x - pc.x == 0.0f) && (pc.y - pc.y == 0.0f) && (pc.z - pc.z == 0.0f) && (ln - ln == 0.0f) && (rn - rn == 0.0f));
    const float lx = maps_wave_min(have ? pc.x : INF), ly = maps_wave_min(have ? pc.y : INF), lz = maps_wave_min(have ? pc.z : INF);
    const float hx = maps_wave_max(have ? pc.x : -INF), hy = maps_wave_max(have ? pc.y : -INF), hz = maps_wave_max(have ? pc.z : -INF);
    const float rm = maps_wave_max(have ? ra : 0.0f), rnm = maps_wave_max(have ? rn : 0.0f);
    const bool wbad = __ballot(bad) != 0ull;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = lx; s_red[wave][1] = ly; s_red[wave][2] = lz; s_red[wave][3] = rm;
        s_red[wave][4] = hx; s_red[wave][5] = hy; s_red[wave][6] = hz; s_red[wave][7] = wbad ? 1.0f : 0.0f; s_red[wave][8] = rnm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float4 lo, hi;
        lo.x = fminf(fminf(s_red[0][0], s_red[1][0]), fminf(s_red[2][0], s_red[3][0]));
        lo.y = fminf(fminf(s_red[0][1], s_red[1][1]), fminf(s_red[2][1], s_red[3][1]));
        lo.z = fminf(fminf(s_red[0][2], s_red[1][2]), fminf(s_red[2][2], s_red[3][2]));
        lo.w = fmaxf(fmaxf(s_red[0][3], s_red[1][3]), fmaxf(s_red[2][3], s_red[3][3]));
        hi.x = fmaxf(fmaxf(s_red[0][4], s_red[1][4]), fmaxf(s_red[2][4], s_red[3][4]));
        hi.y = fmaxf(fmaxf(s_red[0][5], s_red[1][5]), fmaxf(s_red[2][5], s_red[3][5]));
        hi.z = fmaxf(fmaxf(s_red[0][6], s_red[1][6]), fmaxf(s_red[2][6], s_red[3][6]));
        const bool any = (s_red[0][7] + s_red[1][7]) + (s_red[2][7] + s_red[3][7]) != 0.0f;
        hi.w = any ? INF : fmaxf(fmaxf(s_red[0][8], s_red[1][8]), fmaxf(s_red[2][8], s_red[3][8]));
        box[2 * (size_t)blockIdx.x] = lo;
        box[2 * (size_t)blockIdx.x + 1] = hi;
    }
}

// ---------------------------------------------------------------------------------------------
// Batched splat: workgroup (b, v) draws block b of the chunk into view v's key plane, or leaves before loading a record.
// skipped[v]: workgroups that left (one atomic each, one address per view); hit[v] = 1: view v was drawn into by this chunk.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_maps_splat_image(MapsSoA c, uint32_t n, uint32_t id_base, const float4 *__restrict__ box,
                                                          const RenderParams *__restrict__ rps, uint64_t *__restrict__ key, size_t npix,
                                                          int cull, uint32_t *__restrict__ skipped, uint8_t *__restrict__ hit)
{
    const uint32_t v = blockIdx.y;
    const RenderParams rp = rps[v];
    if (cull && maps_box_outside_image(maps_box_load(box, blockIdx.x), rp)) {               // (workgroup-uniform)
        if (threadIdx.x == 0) atomicAdd(&skipped[v], 1u);
        return;
    }
    if (threadIdx.x == 0) hit[v] = 1;
    const uint32_t k = blockIdx.x * (uint32_t)MAPS_BLOCK + threadIdx.x;
    if (k < n) render_surfel(rp, c.pos_conf, c.norm_rad, k, id_base + k, key + (size_t)v * npix);
}

// k_view_splat's split: a disc of at most fp_lane pixels by its own lane; a larger one by its wave, lanes over pixels, as soon
// as the wave's small ones are done (no list: a (record, view) pair would need one per view).
__global__ __launch_bounds__(256) void k_maps_splat_view(MapsSoA c, uint32_t n, uint32_t id_base, const float4 *__restrict__ box,
                                                         const ViewParams *__restrict__ vps, uint64_t *__restrict__ key, size_t npix,
                                                         int cull, uint32_t *__restrict__ skipped, uint8_t *__restrict__ hit)
{
    const uint32_t v = blockIdx.y;
    const ViewParams vp = vps[v];
    if (cull && maps_box_outside_view(maps_box_load(box, blockIdx.x), vp)) {
        if (threadIdx.x == 0) atomicAdd(&skipped[v], 1u);
        return;
    }
    if (threadIdx.x == 0) hit[v] = 1;
    uint64_t *kv = key + (size_t)v * npix;
    const uint32_t k = blockIdx.x * (uint32_t)MAPS_BLOCK + threadIdx.x;
    const bool big = k < n && view_surfel(vp, c.pos_conf, c.norm_rad, k, id_base + k, kv);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t m = __ballot(big); m; m &= m - 1ull) {
        const uint32_t kb = (uint32_t)__shfl((int)k, __ffsll((unsigned long long)m) - 1);
        view_surfel_wide(vp, c.pos_conf, c.norm_rad, kb, id_base + kb, lane, 64u, kv);
    }
}

// ---------------------------------------------------------------------------------------------
// Chunk resolve, grid (pixel blocks, views): the pixels this source holds at the moment are shaded while its rows are on the
// device; a later source that wins the pixel overwrites them.  Views the source did not touch are left at once.
// ---------------------------------------------------------------------------------------------
__global__ void k_maps_resolve_image(MapsSoA c, uint32_t base, uint32_t n, const uint64_t *__restrict__ key, size_t npix,
                                     const uint8_t *__restrict__ hit, uint8_t *__restrict__ bgr, uint8_t *__restrict__ sem)
{
    const uint32_t v = blockIdx.y;
    if (!hit[v]) return;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const size_t q = (size_t)v * npix + p;
    const uint64_t kk = key[q];
    if (kk == KEY_EMPTY) return;
    const uint32_t row = (uint32_t)(kk & 0xFFFFFFFFull) - base;             // wraps below the base
    if (row >= n) return;
    uint8_t b, g, r, s;
    render_shade(c.color[row], b, g, r, s);
    bgr[q * 3] = b; bgr[q * 3 + 1] = g; bgr[q * 3 + 2] = r;
    sem[q] = s;
}

__global__ void k_maps_resolve_view(MapsSoA c, uint32_t base, uint32_t n, const ViewShade *__restrict__ vss, const uint64_t *__restrict__ key,
                                    size_t npix, const uint8_t *__restrict__ hit, uint32_t *__restrict__ rgba, float *__restrict__ depth,
                                    int32_t *__restrict__ ids)
{
    const uint32_t v = blockIdx.y;
    if (!hit[v]) return;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const size_t q = (size_t)v * npix + p;
    const uint64_t kk = key[q];
    if (kk == KEY_EMPTY) return;
    const uint32_t id = (uint32_t)(kk & 0xFFFFFFFFull), row = id - base;
    if (row >= n) return;
    rgba[q] = view_shade(vss[v], c.norm_rad, c.color, c.time, row);
    depth[q] = view_depth(kk);
    ids[q] = (int32_t)id;
}

__global__ void k_maps_finish_image(const uint64_t *__restrict__ key, size_t total, uint8_t *__restrict__ bgr, uint8_t *__restrict__ sem)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total || key[q] != KEY_EMPTY) return;
    bgr[q * 3] = 0; bgr[q * 3 + 1] = 0; bgr[q * 3 + 2] = 0;
    sem[q] = 0;
}

__global__ void k_maps_finish_view(const ViewShade *__restrict__ vss, const uint64_t *__restrict__ key, size_t npix,
                                   uint32_t *__restrict__ rgba, float *__restrict__ depth, int32_t *__restrict__ ids)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const size_t q = (size_t)blockIdx.y * npix + p;
    if (key[q] != KEY_EMPTY) return;
    rgba[q] = vss[blockIdx.y].clear;
    depth[q] = 1.0f;
    ids[q] = -1;
}

}  // namespace sm
