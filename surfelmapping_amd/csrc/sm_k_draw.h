// sm_k_draw.h -- what the two renderers do to ONE surfel and to ONE pixel, as device functions over a surfel source: the
// novel view (sm_k_io.h: k_render_splat / k_render_resolve), the model view (sm_k_view.h, which states its rules) and their
// streamed forms over map files (sm_k_render_maps.h) all call these, so that a surfel drawn from a model slot and the same
// surfel drawn from a chunk row set the same key bits and take the same colour.  A source is the SoA planes of SurfelSet, a
// row `k` in them, and the id the key carries (`k` plus the source's base in the map set).  No kernels here.
#pragma once

#include "sm_device.h"

namespace sm {

// ---------------------------------------------------------------------------------------------
// Novel-view renderer: GlobalModel::renderImage (src/GlobalModel.cpp:772-833),
// draw_image.vert:18-28, draw_image_adaptive.geom:38-83, draw_image.frag:11-19.  Every surfel is a
// screen-space quad (two triangles) with a per-fragment circle test, z-buffered with GL_LESS.
// Rasterisation (DESIGN.md "Renderer"): 24.8 fixed-point vertices, 64-bit edge functions, top-left fill
// rule, barycentrics in double -> float, the same 64-bit atomicMin key (d24 << 32 | id) as the index map.
// ---------------------------------------------------------------------------------------------
struct RVert { long long X, Y; float zw, tx, ty; };

struct RenderParams {
    float t_inv[16];
    float fx, fy, cx, cy, cols, rows;
    int w, h;
};

__device__ __forceinline__ long long edge64(const RVert &a, const RVert &b, long long px, long long py)
{
    return (b.X - a.X) * (py - a.Y) - (b.Y - a.Y) * (px - a.X);
}

__device__ __forceinline__ bool top_left(const RVert &a, const RVert &b)
{
    const long long dx = b.X - a.X, dy = b.Y - a.Y;
    return (dy == 0 && dx > 0) || (dy < 0);
}

// What is done with a fragment -- a (surfel, pixel) pair that passed every test -- is the caller's: frag(p, d24, q) gets the pixel
// p = py * w + px, the 24-bit window depth and q = tx*tx + ty*ty, the value the circle test compared.  The key pass (KeyFrag) and
// the blended view's accumulation (sm_k_blend.h) are two such actions over one walk, so they see the same fragments.
struct KeyFrag {
    uint64_t *__restrict__ key;
    uint32_t id;
    __device__ __forceinline__ void operator()(size_t p, uint32_t d24, float) const
    {
        atomicMin((unsigned long long *)&key[p], (unsigned long long)(((uint64_t)d24 << 32) | id));
    }
};

template <typename Frag>
__device__ __forceinline__ void raster_tri(RVert v0, RVert v1, RVert v2, int w, int h, Frag &frag)
{
    long long area = edge64(v0, v1, v2.X, v2.Y);
    if (area == 0) return;
    if (area < 0) { const RVert t = v1; v1 = v2; v2 = t; area = -area; }
    long long minX = min(v0.X, min(v1.X, v2.X)), maxX = max(v0.X, max(v1.X, v2.X));
    long long minY = min(v0.Y, min(v1.Y, v2.Y)), maxY = max(v0.Y, max(v1.Y, v2.Y));
    long long x0 = (minX - 128) >> 8, x1 = (maxX - 128) >> 8, y0 = (minY - 128) >> 8, y1 = (maxY - 128) >> 8;
    x0 = max(x0, 0ll); y0 = max(y0, 0ll);
    x1 = min(x1, (long long)w - 1); y1 = min(y1, (long long)h - 1);
    const int b0 = top_left(v1, v2) ? 0 : -1, b1 = top_left(v2, v0) ? 0 : -1, b2 = top_left(v0, v1) ? 0 : -1;
    for (long long py = y0; py <= y1; ++py)
        for (long long px = x0; px <= x1; ++px) {
            const long long cx = px * 256 + 128, cy = py * 256 + 128;
            const long long e0 = edge64(v1, v2, cx, cy), e1 = edge64(v2, v0, cx, cy), e2 = edge64(v0, v1, cx, cy);
            if (e0 + b0 < 0 || e1 + b1 < 0 || e2 + b2 < 0) continue;
            const float l0 = (float)((double)e0 / (double)area), l1 = (float)((double)e1 / (double)area),
                        l2 = (float)((double)e2 / (double)area);
            const float tx = (l0 * v0.tx + l1 * v1.tx) + l2 * v2.tx;
            const float ty = (l0 * v0.ty + l1 * v1.ty) + l2 * v2.ty;
            const float q = tx * tx + ty * ty;
            if (q > 1.0f) continue;                                         // draw_image.frag:13-14
            const float zw = (l0 * v0.zw + l1 * v1.zw) + l2 * v2.zw;
            if (!(zw >= 0.0f && zw <= 1.0f)) continue;
            const uint32_t d24 = (uint32_t)floor((double)zw * 16777215.0 + 0.5);
            if (d24 >= 16777215u) continue;
            frag((size_t)py * w + px, d24, q);
        }
}

// One surfel of the novel view (draw_image.vert:18-28, draw_image_adaptive.geom:38-83): centre `pc`, normal and radius from
// nr_of() -- asked for only once the centre has passed the depth test --, its fragments to `frag`.  The one statement of the rule:
// the forms below say where the two float4 come from.
template <typename Frag, typename NormRad>
__device__ __forceinline__ void render_surfel_of(const RenderParams &rp, const float4 pc, NormRad nr_of, Frag &frag)
{
    const float maxDepth = 200.0f;                                          // src/GlobalModel.cpp:797
    const float3 ph = xform3(rp.t_inv, pc.x, pc.y, pc.z);                  // draw_image.vert:20
    if (ph.z >= maxDepth || ph.z <= 1.0f) return;                           // draw_image_adaptive.geom:41
    const float4 nr = nr_of();
    const float3 n = normalize3(rot3(rp.t_inv, nr.x, nr.y, nr.z));
    const float r = nr.w;
    float3 x, y;
    if (ph.z > 5.0f) {                                                      // :47-52
        const float3 tn = make_float3(0.0f, 0.0f, 1.0f);
        const float3 a = normalize3(make_float3(tn.y - tn.z, -tn.x, tn.x));
        x = make_float3(a.x * r * 1.41421356f, a.y * r * 1.41421356f, a.z * r * 1.41421356f);
        y = cross3(tn, x);
    } else {                                                                // :53-63
        const float cosAngle = dot3(ph, n) / (sqrtf(dot3(ph, ph)) * sqrtf(dot3(n, n)));
        const float radius = r / (1.0f + 0.5f * fabsf(cosAngle));
        const float3 a = normalize3(make_float3(n.y - n.z, -n.x, n.x));
        x = make_float3(a.x * radius * 1.41421356f, a.y * radius * 1.41421356f, a.z * radius * 1.41421356f);
        y = cross3(n, x);
    }
    const float sx[4] = {x.x, y.x, -y.x, -x.x}, sy[4] = {x.y, y.y, -y.y, -x.y}, sz[4] = {x.z, y.z, -y.z, -x.z};
    const float tcx[4] = {-1.0f, 1.0f, -1.0f, 1.0f}, tcy[4] = {-1.0f, -1.0f, 1.0f, 1.0f};
    RVert rv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float X = ph.x + sx[q], Y = ph.y + sy[q], Z = ph.z + sz[q];
        if (!(Z > 0.0f)) return;                                            // would need polygon clipping: not drawn
        const float xn = ((((rp.fx * X) / Z) + rp.cx) - (rp.cols * 0.5f)) / (rp.cols * 0.5f);   // projectPoint :31-36
        const float yn = ((((rp.fy * Y) / Z) + rp.cy) - (rp.rows * 0.5f)) / (rp.rows * 0.5f);
        const float zn = (2.0f * Z / maxDepth) - 1.0f;
        const float xw = (rp.cols * 0.5f) * xn + (rp.cols * 0.5f), yw = (rp.rows * 0.5f) * yn + (rp.rows * 0.5f);
        if (!(fabsf(xw) < 1.0e6f && fabsf(yw) < 1.0e6f)) return;
        rv[q].X = (long long)floor((double)xw * 256.0 + 0.5);
        rv[q].Y = (long long)floor((double)yw * 256.0 + 0.5);
        rv[q].zw = 0.5f * zn + 0.5f;
        rv[q].tx = tcx[q]; rv[q].ty = tcy[q];
    }
    raster_tri(rv[0], rv[1], rv[2], rp.w, rp.h, frag);                      // triangle strip
    raster_tri(rv[2], rv[1], rv[3], rp.w, rp.h, frag);
}

// ... row `k` of a source
template <typename Frag>
__device__ __forceinline__ void render_surfel(const RenderParams &rp, const float4 *__restrict__ pos_conf,
                                              const float4 *__restrict__ norm_rad, uint32_t k, Frag &frag)
{
    render_surfel_of(rp, pos_conf[k], [&]() { return norm_rad[k]; }, frag);
}

// ... a surfel the caller holds in registers (an actor's row placed by its pose: sm_k_scene.h), drawn under `id` into a key map
__device__ __forceinline__ void render_surfel(const RenderParams &rp, const float4 pc, const float4 nr, uint32_t id, uint64_t *__restrict__ key)
{
    KeyFrag frag{key, id};
    render_surfel_of(rp, pc, [&]() { return nr; }, frag);
}

// ... row `k` drawn under `id` into a key map
__device__ __forceinline__ void render_surfel(const RenderParams &rp, const float4 *__restrict__ pos_conf,
                                              const float4 *__restrict__ norm_rad, uint32_t k, uint32_t id, uint64_t *__restrict__ key)
{
    KeyFrag frag{key, id};
    render_surfel(rp, pos_conf, norm_rad, k, frag);
}

// draw_image.frag:11-19 from the winner's colour word: B, G, R (vBGR = srgb.wzy) and class + 1
__device__ __forceinline__ void render_shade(uint32_t sc, uint8_t &b, uint8_t &g, uint8_t &r, uint8_t &s)
{
    b = (uint8_t)(sc & 0xFFu); g = (uint8_t)((sc >> 8) & 0xFFu); r = (uint8_t)((sc >> 16) & 0xFFu);
    s = (uint8_t)(((sc >> 24) & 0xFFu) + 1u);
}

struct VVert { long long X, Y; float zw, iw, tx, ty; };
struct VTri { VVert a, b, c; long long area; int ba, bb, bc; };

struct ViewParams {
    float mvp[16];            // column-major
    float mvinv[16];          // column-major; columns 2 and 3 are read
    float threshold;
    int unstable, points;
    int w, h;
    uint32_t fp_lane;         // bounding-box pixels up to which a lane rasterises its own surfel
};

struct ViewShade {
    int color_type, window, time, time_delta;
    uint32_t clear;           // RGBA bytes, R in the low byte
};

constexpr int VIEW_SLICES = 16;          // waves per overflow surfel (each takes every 16th 64-pixel chunk of its box)
constexpr int VIEW_OVF_BLOCKS = 1024;    // grid of k_view_overflow (4 waves per workgroup, strided over the list)

// src/GlobalModel.cpp:718-736, R << 16 | G << 8 | B
__constant__ uint32_t VIEW_PALETTE[19] = {
    0x808080u, 0x00FF00u, 0x0000FFu, 0xFFFF00u, 0x800000u, 0xFF00FFu, 0x808000u, 0x008000u, 0x800080u, 0x008080u,
    0x00FFFFu, 0x000080u, 0xF5DEB3u, 0xFF0000u, 0xD2691Eu, 0xF4A460u, 0x778899u, 0xFF1493u, 0x8A2BE2u};

__device__ __forceinline__ float4 view_clip(const float *m, float x, float y, float z)
{
    float4 r;
    r.x = ((m[0] * x + m[4] * y) + m[8] * z) + m[12];
    r.y = ((m[1] * x + m[5] * y) + m[9] * z) + m[13];
    r.z = ((m[2] * x + m[6] * y) + m[10] * z) + m[14];
    r.w = ((m[3] * x + m[7] * y) + m[11] * z) + m[15];
    return r;
}

__device__ __forceinline__ bool view_vert(const ViewParams &vp, float x, float y, float z, float tx, float ty, VVert &v)
{
    const float4 c = view_clip(vp.mvp, x, y, z);
    if (!(c.w > 0.0f)) return false;                                        // would need polygon clipping: not drawn
    const float xw = ((c.x / c.w) * 0.5f + 0.5f) * (float)vp.w;
    const float yw = ((c.y / c.w) * 0.5f + 0.5f) * (float)vp.h;
    const float zw = (c.z / c.w) * 0.5f + 0.5f;
    const float iw = 1.0f / c.w;
    if (!(fabsf(xw) < 1.0e6f && fabsf(yw) < 1.0e6f && isfinite(zw) && isfinite(iw))) return false;
    v.X = (long long)floor((double)xw * 256.0 + 0.5);
    v.Y = (long long)floor((double)yw * 256.0 + 0.5);
    v.zw = zw; v.iw = iw; v.tx = tx; v.ty = ty;
    return true;
}

__device__ __forceinline__ long long vedge(const VVert &a, const VVert &b, long long px, long long py)
{
    return (b.X - a.X) * (py - a.Y) - (b.Y - a.Y) * (px - a.X);
}

__device__ __forceinline__ bool vtop_left(const VVert &a, const VVert &b)
{
    const long long dx = b.X - a.X, dy = b.Y - a.Y;
    return (dy == 0 && dx > 0) || (dy < 0);
}

// raster_tri's set-up: counter-clockwise winding (area > 0; 0 = nothing drawn) and the fill-rule biases
__device__ __forceinline__ VTri view_tri(const VVert &v0, const VVert &v1, const VVert &v2)
{
    VTri t;
    t.a = v0; t.b = v1; t.c = v2;
    t.area = vedge(v0, v1, v2.X, v2.Y);
    if (t.area < 0) { t.b = v2; t.c = v1; t.area = -t.area; }
    t.ba = vtop_left(t.b, t.c) ? 0 : -1;
    t.bb = vtop_left(t.c, t.a) ? 0 : -1;
    t.bc = vtop_left(t.a, t.b) ? 0 : -1;
    return t;
}

// the per-pixel function of both paths: one triangle, one pixel centre
__device__ __forceinline__ void view_px_tri(const VTri &t, int px, int py, int w, uint32_t id, uint64_t *__restrict__ key)
{
    if (t.area == 0) return;
    const long long cx = (long long)px * 256 + 128, cy = (long long)py * 256 + 128;
    const long long e0 = vedge(t.b, t.c, cx, cy), e1 = vedge(t.c, t.a, cx, cy), e2 = vedge(t.a, t.b, cx, cy);
    if (e0 + t.ba < 0 || e1 + t.bb < 0 || e2 + t.bc < 0) return;
    const float l0 = (float)((double)e0 / (double)t.area), l1 = (float)((double)e1 / (double)t.area),
                l2 = (float)((double)e2 / (double)t.area);
    const float wl0 = l0 * t.a.iw, wl1 = l1 * t.b.iw, wl2 = l2 * t.c.iw;
    const float s = (wl0 + wl1) + wl2;
    const float tx = ((wl0 * t.a.tx + wl1 * t.b.tx) + wl2 * t.c.tx) / s;
    const float ty = ((wl0 * t.a.ty + wl1 * t.b.ty) + wl2 * t.c.ty) / s;
    if (tx * tx + ty * ty > 1.0f) return;                                   // draw_surface.frag:30-31
    const float zw = (l0 * t.a.zw + l1 * t.b.zw) + l2 * t.c.zw;
    if (!(zw >= 0.0f && zw <= 1.0f)) return;
    const uint32_t d24 = (uint32_t)floor((double)zw * 16777215.0 + 0.5);
    if (d24 >= 16777215u) return;
    atomicMin((unsigned long long *)&key[(size_t)py * w + px], (unsigned long long)(((uint64_t)d24 << 32) | id));
}

// draw_surface_adaptive.geom:94-131 -> the strip's two triangles and their pixel box (clipped to the view); false: nothing to draw
__device__ __forceinline__ bool view_disc(const ViewParams &vp, float4 pc, float4 nr, VTri &t0, VTri &t1, int &x0, int &y0,
                                          int &x1, int &y1)
{
    const float *m = vp.mvp;
    const float zl = ((m[2] * pc.x + m[6] * pc.y) + m[10] * pc.z) + m[14];
    const float3 n = make_float3(nr.x, nr.y, nr.z);
    float3 x, y;
    if (zl > 5.0f) {
        const float3 a = make_float3(vp.mvinv[8], vp.mvinv[9], vp.mvinv[10]);
        const float3 u = normalize3(make_float3(a.y - a.z, -a.x, a.x));
        x = make_float3((u.x * nr.w) * 1.41421356f, (u.y * nr.w) * 1.41421356f, (u.z * nr.w) * 1.41421356f);
        y = cross3(a, x);
    } else {
        const float3 e = make_float3(pc.x - vp.mvinv[12], pc.y - vp.mvinv[13], pc.z - vp.mvinv[14]);
        const float cosAngle = dot3(e, n) / (sqrtf(dot3(e, e)) * sqrtf(dot3(n, n)));
        const float radius = nr.w / (1.0f + 0.5f * fabsf(cosAngle));
        const float3 u = normalize3(make_float3(n.y - n.z, -n.x, n.x));
        x = make_float3((u.x * radius) * 1.41421356f, (u.y * radius) * 1.41421356f, (u.z * radius) * 1.41421356f);
        y = cross3(n, x);
    }
    VVert v0, v1, v2, v3;
    if (!view_vert(vp, pc.x + x.x, pc.y + x.y, pc.z + x.z, -1.0f, -1.0f, v0)) return false;
    if (!view_vert(vp, pc.x + y.x, pc.y + y.y, pc.z + y.z, 1.0f, -1.0f, v1)) return false;
    if (!view_vert(vp, pc.x - y.x, pc.y - y.y, pc.z - y.z, -1.0f, 1.0f, v2)) return false;
    if (!view_vert(vp, pc.x - x.x, pc.y - x.y, pc.z - x.z, 1.0f, 1.0f, v3)) return false;
    t0 = view_tri(v0, v1, v2);                                              // triangle strip
    t1 = view_tri(v2, v1, v3);
    const long long minX = min(min(v0.X, v1.X), min(v2.X, v3.X)), maxX = max(max(v0.X, v1.X), max(v2.X, v3.X));
    const long long minY = min(min(v0.Y, v1.Y), min(v2.Y, v3.Y)), maxY = max(max(v0.Y, v1.Y), max(v2.Y, v3.Y));
    x0 = (int)max((minX - 128) >> 8, 0ll); x1 = (int)min((maxX - 128) >> 8, (long long)vp.w - 1);
    y0 = (int)max((minY - 128) >> 8, 0ll); y1 = (int)min((maxY - 128) >> 8, (long long)vp.h - 1);
    return x0 <= x1 && y0 <= y1;
}

// draw_feedback.vert:38,80 + glPointSize(1)
__device__ __forceinline__ void view_point(const ViewParams &vp, float4 pc, uint32_t id, uint64_t *__restrict__ key)
{
    const float4 c = view_clip(vp.mvp, pc.x, pc.y, pc.z);
    if (!(c.w > 0.0f && -c.w <= c.x && c.x <= c.w && -c.w <= c.y && c.y <= c.w && -c.w <= c.z && c.z <= c.w)) return;
    const float xw = ((c.x / c.w) * 0.5f + 0.5f) * (float)vp.w;
    const float yw = ((c.y / c.w) * 0.5f + 0.5f) * (float)vp.h;
    const float zw = (c.z / c.w) * 0.5f + 0.5f;
    const int px = (int)floorf(xw), py = (int)floorf(yw);
    if (px < 0 || py < 0 || px >= vp.w || py >= vp.h) return;
    const uint32_t d24 = (uint32_t)floor((double)zw * 16777215.0 + 0.5);
    if (d24 >= 16777215u) return;
    atomicMin((unsigned long long *)&key[(size_t)py * vp.w + px], (unsigned long long)(((uint64_t)d24 << 32) | id));
}

// One surfel of the model view by its own lane: row `k` of the source, drawn under `id`.  True: a disc whose pixel box is
// above vp.fp_lane, not drawn -- the caller hands it to view_surfel_wide (which path drew a pixel cannot change the image).
__device__ __forceinline__ bool view_surfel(const ViewParams &vp, const float4 *__restrict__ pos_conf,
                                            const float4 *__restrict__ norm_rad, uint32_t k, uint32_t id, uint64_t *__restrict__ key)
{
    const float4 pc = pos_conf[k];
    if (vp.points) {
        if (pc.w > vp.threshold) view_point(vp, pc, id, key);
    } else if (pc.w > vp.threshold || vp.unstable) {
        const float4 nr = norm_rad[k];
        VTri t0, t1;
        int x0, y0, x1, y1;
        if (view_disc(vp, pc, nr, t0, t1, x0, y0, x1, y1)) {
            if ((uint64_t)(x1 - x0 + 1) * (uint64_t)(y1 - y0 + 1) > vp.fp_lane) return true;
            for (int py = y0; py <= y1; ++py)
                for (int px = x0; px <= x1; ++px) {
                    view_px_tri(t0, px, py, vp.w, id, key);
                    view_px_tri(t1, px, py, vp.w, id, key);
                }
        }
    }
    return false;
}

// A large disc by many lanes: this lane takes the pixels first, first + step, ... of the disc's box (row-major).
__device__ __forceinline__ void view_surfel_wide(const ViewParams &vp, const float4 *__restrict__ pos_conf,
                                                 const float4 *__restrict__ norm_rad, uint32_t k, uint32_t id, uint32_t first,
                                                 uint32_t step, uint64_t *__restrict__ key)
{
    VTri t0, t1;
    int x0, y0, x1, y1;
    if (!view_disc(vp, pos_conf[k], norm_rad[k], t0, t1, x0, y0, x1, y1)) return;
    const uint32_t nx = (uint32_t)(x1 - x0 + 1), npx = nx * (uint32_t)(y1 - y0 + 1);     // <= w*h <= 2^28
    for (uint32_t i = first; i < npx; i += step) {
        const int py = y0 + (int)(i / nx), px = x0 + (int)(i % nx);
        view_px_tri(t0, px, py, vp.w, id, key);
        view_px_tri(t1, px, py, vp.w, id, key);
    }
}

__device__ __forceinline__ uint32_t view_u8(float c)
{
    return (uint32_t)floorf(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f + 0.5f);
}

// the colour of row `k` (draw_surface_adaptive.geom:46-91, draw_feedback.vert:40-79) as RGBA8, R in the low byte
__device__ __forceinline__ uint32_t view_shade(const ViewShade &vs, const float4 *__restrict__ norm_rad,
                                               const uint32_t *__restrict__ color, const float *__restrict__ time, uint32_t k)
{
    float r, g, b;
    if (vs.color_type == 1) {
        const float4 n = norm_rad[k];
        r = n.x; g = n.y; b = n.z;
    } else if (vs.color_type == 2) {
        const uint32_t sc = color[k];
        r = (float)((sc >> 16) & 0xFFu) / 255.0f; g = (float)((sc >> 8) & 0xFFu) / 255.0f; b = (float)(sc & 0xFFu) / 255.0f;
    } else if (vs.color_type == 3) {
        const uint32_t c = color[k] >> 24;
        const uint32_t pal = c <= 18u ? VIEW_PALETTE[c] : 0u;
        r = (float)((pal >> 16) & 0xFFu) / 255.0f; g = (float)((pal >> 8) & 0xFFu) / 255.0f; b = (float)(pal & 0xFFu) / 255.0f;
    } else {
        const float4 n = norm_rad[k];
        r = g = b = 0.5f * fabsf((n.x + n.y) + n.z) + 0.1f;
    }
    if (vs.window && (float)vs.time - time[k] > (float)vs.time_delta) { r *= 0.25f; g *= 0.25f; b *= 0.25f; }
    return view_u8(r) | (view_u8(g) << 8) | (view_u8(b) << 16) | 0xFF000000u;
}

// a key's window depth (1.0 = empty is the caller's)
__device__ __forceinline__ float view_depth(uint64_t kk) { return (float)(uint32_t)(kk >> 32) / 16777215.0f; }

}  // namespace sm
