// sm_k_view.h -- the model view: GlobalModel::renderModel (src/GlobalModel.cpp:683-758) into an image.
// Included by sm_view.hip only; shader citations: /root/reference/src/Shaders/<file>:<line>.
//
// Surfel mode is draw_surface.vert + draw_surface_adaptive.geom + draw_surface.frag (the program renderModel binds,
// src/GlobalModel.cpp:23-24); points mode is draw_feedback.vert/.frag (:22).  The `pose` uniform is the identity
// (src/GlobalModel.cpp:715-716), so vPosition = position and vNormRad = normal: no arithmetic is spent on it.
//
// Selection.  Surfel mode draws surfel k iff conf > threshold || unstable (draw_surface.vert:47); points mode iff
// conf > threshold (draw_feedback.vert:38; `unstable` is not read there).
//
// Disc (draw_surface_adaptive.geom:94-131), float32, in this order:
//   posLocal.z = ((MVP[2]*p.x + MVP[6]*p.y) + MVP[10]*p.z) + MVP[14]       -- the clip z, not the view depth (:96-97)
//   far  (posLocal.z > 5): a = MVINV[8..10] (mat3(MVINV)*(0,0,1)), x = (normalize(a.y-a.z, -a.x, a.x) * r) * 1.41421356,
//                          y = cross(a, x)                                                                 (:99-101)
//   near (otherwise):      e = p - MVINV[12..14], cosAngle = dot(e,n) / (sqrt(dot(e,e)) * sqrt(dot(n,n))),
//                          r' = r / (1 + 0.5*|cosAngle|), x = (normalize(n.y-n.z, -n.x, n.x) * r') * 1.41421356,
//                          y = cross(n, x)                                                                 (:105-111)
//   dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z; normalize(v) = v / sqrt(dot(v,v)) per component.
//   strip p+x, p+y, p-y, p-x with texcoords (-1,-1), (1,-1), (-1,1), (1,1) (:114-128): triangles (0,1,2), (2,1,3).
// Vertex: c = MVP*(v,1), each row ((m[r]*x + m[r+4]*y) + m[r+8]*z) + m[r+12]; xw = ((c.x/c.w)*0.5 + 0.5)*W,
//   yw likewise with H, zw = (c.z/c.w)*0.5 + 0.5, iw = 1/c.w.  Not drawn (DESIGN.md "Model view"): any vertex with c.w <= 0
//   (GL would clip the polygon), |xw| or |yw| >= 1e6, or a non-finite zw / iw.
// Raster: the novel-view renderer's rules (raster_tri, sm_k_io.h): 24.8 fixed point X = floor(xw*256 + 0.5) (double),
//   64-bit edge functions, top-left fill rule, pixel centres at +0.5, l_i = (float)((double)e_i / (double)area).
//   Texcoords perspective-correct: wl_i = l_i*iw_i, s = (wl0 + wl1) + wl2, t = ((wl0*t0 + wl1*t1) + wl2*t2) / s;
//   discarded if tx*tx + ty*ty > 1 (draw_surface.frag:30-31).  Depth screen-linear: zw = (l0*z0 + l1*z1) + l2*z2, kept iff
//   0 <= zw <= 1 (stands in for near/far clipping).
// Points (glPointSize 1): c = MVP*(p,1) as above, drawn iff c.w > 0 and -w <= x,y,z <= w; one fragment at
//   (floor(xw), floor(yw)) if that pixel lies in the viewport.
// Depth test: GL_LESS into a 24-bit buffer cleared to 1.0: d24 = floor(zw*16777215 + 0.5) (double), kept iff d24 < 16777215,
//   atomicMin of (d24 << 32) | k -- a tie goes to the lower id, so the image does not depend on scheduling.
// Colour (draw_surface_adaptive.geom:46-91, draw_feedback.vert:40-79), from the winning id in the resolve pass:
//   0 shaded  0.5*|((n.x+n.y)+n.z)| + 0.1 on all channels; 1 normals n.xyz; 2 colours decodeColor(.) .yzw / 255
//   (color.glsl:28-37); 3 the 19-entry class palette / 255 (src/GlobalModel.cpp:718-736), classes > 18 black.
//   Surfel mode only: drawWindow && float(time) - surfel.time > float(timeDelta) multiplies by 0.25 (:88-91).
//   RGBA8 unorm: floor(min(max(c,0),1)*255 + 0.5), alpha 255; an uncovered pixel takes the clear colour.
// Rows are in GL window order (row 0 = bottom), as glReadPixels returns them.
//
// Work split: k_view_splat makes one pass over the live surfels (32 B each: pos_conf + norm_rad); a surfel whose bounding
// box covers at most `fp_lane` pixels is rasterised by its own lane, a larger one is appended (one atomic per wave) to an
// overflow list that k_view_overflow rasterises with one wave per (surfel, slice of its 64-pixel chunks), lanes over pixels.
// Both paths call view_px_tri, so which path drew a pixel cannot change the image.

#pragma once

#include "sm_device.h"

namespace sm {

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

// one pass over the live surfels (the compacted model: `count` slots of the current set)
__global__ __launch_bounds__(256) void k_view_splat(Model M, const DevState *__restrict__ st, ViewParams vp, uint64_t *__restrict__ key,
                                                    uint32_t *__restrict__ ovf_n, uint32_t *__restrict__ ovf)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const SurfelSet cur = M.s[st->cur];
    bool big = false;
    if (k < st->count) {
        const float4 pc = cur.pos_conf[k];
        if (vp.points) {
            if (pc.w > vp.threshold) view_point(vp, pc, k, key);
        } else if (pc.w > vp.threshold || vp.unstable) {
            const float4 nr = cur.norm_rad[k];
            VTri t0, t1;
            int x0, y0, x1, y1;
            if (view_disc(vp, pc, nr, t0, t1, x0, y0, x1, y1)) {
                if ((uint64_t)(x1 - x0 + 1) * (uint64_t)(y1 - y0 + 1) > vp.fp_lane) big = true;
                else
                    for (int py = y0; py <= y1; ++py)
                        for (int px = x0; px <= x1; ++px) {
                            view_px_tri(t0, px, py, vp.w, k, key);
                            view_px_tri(t1, px, py, vp.w, k, key);
                        }
            }
        }
    }
    // large footprints: one atomic per wave, ranks by popcount (CDNA guide Guideline 12); the list holds at most `count` ids
    const uint64_t m = __ballot(big);
    if (m) {
        const int lane = threadIdx.x & 63;
        const int leader = __ffsll((unsigned long long)m) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(ovf_n, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, leader);
        if (big) ovf[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = k;
    }
}

// the overflow list: wave (entry, slice) takes the 64-pixel chunks slice, slice + VIEW_SLICES, ... of the entry's box
__global__ __launch_bounds__(256) void k_view_overflow(Model M, const DevState *__restrict__ st, ViewParams vp, uint64_t *__restrict__ key,
                                                       const uint32_t *__restrict__ ovf_n, const uint32_t *__restrict__ ovf)
{
    const uint64_t items = (uint64_t)*ovf_n * VIEW_SLICES;
    const SurfelSet cur = M.s[st->cur];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = (uint64_t)gridDim.x * 4u;
    for (uint64_t it = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); it < items; it += nwaves) {
        const uint32_t k = ovf[it / VIEW_SLICES];
        const uint32_t slice = (uint32_t)(it % VIEW_SLICES);
        VTri t0, t1;
        int x0, y0, x1, y1;
        if (!view_disc(vp, cur.pos_conf[k], cur.norm_rad[k], t0, t1, x0, y0, x1, y1)) continue;   // (wave-uniform)
        const uint32_t nx = (uint32_t)(x1 - x0 + 1), npx = nx * (uint32_t)(y1 - y0 + 1);     // <= w*h <= 2^28
        for (uint32_t i = slice * 64u + lane; i < npx; i += 64u * VIEW_SLICES) {
            const int py = y0 + (int)(i / nx), px = x0 + (int)(i % nx);
            view_px_tri(t0, px, py, vp.w, k, key);
            view_px_tri(t1, px, py, vp.w, k, key);
        }
    }
}

__device__ __forceinline__ uint32_t view_u8(float c)
{
    return (uint32_t)floorf(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f + 0.5f);
}

// one pass over the pixels: key -> id -> colour (+ the optional depth and id planes)
__global__ void k_view_resolve(Model M, const DevState *__restrict__ st, ViewShade vs, const uint64_t *__restrict__ key, int npix,
                               uint32_t *__restrict__ rgba, float *__restrict__ depth, int32_t *__restrict__ ids)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const uint64_t kk = key[p];
    uint32_t out = vs.clear;
    float d = 1.0f;
    int32_t id = -1;
    if (kk != KEY_EMPTY) {
        const SurfelSet cur = M.s[st->cur];
        id = (int32_t)(uint32_t)(kk & 0xFFFFFFFFull);
        d = (float)(uint32_t)(kk >> 32) / 16777215.0f;
        float r, g, b;
        if (vs.color_type == 1) {
            const float4 n = cur.norm_rad[id];
            r = n.x; g = n.y; b = n.z;
        } else if (vs.color_type == 2) {
            const uint32_t sc = cur.color[id];
            r = (float)((sc >> 16) & 0xFFu) / 255.0f; g = (float)((sc >> 8) & 0xFFu) / 255.0f; b = (float)(sc & 0xFFu) / 255.0f;
        } else if (vs.color_type == 3) {
            const uint32_t c = cur.color[id] >> 24;
            const uint32_t pal = c <= 18u ? VIEW_PALETTE[c] : 0u;
            r = (float)((pal >> 16) & 0xFFu) / 255.0f; g = (float)((pal >> 8) & 0xFFu) / 255.0f; b = (float)(pal & 0xFFu) / 255.0f;
        } else {
            const float4 n = cur.norm_rad[id];
            r = g = b = 0.5f * fabsf((n.x + n.y) + n.z) + 0.1f;
        }
        if (vs.window && (float)vs.time - cur.time[id] > (float)vs.time_delta) { r *= 0.25f; g *= 0.25f; b *= 0.25f; }
        out = view_u8(r) | (view_u8(g) << 8) | (view_u8(b) << 16) | 0xFF000000u;
    }
    rgba[p] = out;
    if (depth) depth[p] = d;
    if (ids) ids[p] = id;
}

}  // namespace sm
