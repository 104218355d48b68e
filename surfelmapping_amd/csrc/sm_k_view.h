// sm_k_view.h -- the model view: GlobalModel::renderModel (src/GlobalModel.cpp:683-758) into an image.
// Included by sm_view.hip only (the device functions these kernels call are sm_k_draw.h's); shader citations: /root/reference/src/Shaders/<file>:<line>.
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
#include "sm_k_draw.h"

namespace sm {

// one pass over the live surfels (the compacted model: `count` slots of the current set); `id_base`: what the keys carry above
// the slot number (0 unless the model is one source of a map set)
__global__ __launch_bounds__(256) void k_view_splat(Model M, const DevState *__restrict__ st, ViewParams vp, uint64_t *__restrict__ key,
                                                    uint32_t *__restrict__ ovf_n, uint32_t *__restrict__ ovf, uint32_t id_base)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const SurfelSet cur = M.s[st->cur];
    const bool big = k < st->count && view_surfel(vp, cur.pos_conf, cur.norm_rad, k, id_base + k, key);
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
                                                       const uint32_t *__restrict__ ovf_n, const uint32_t *__restrict__ ovf, uint32_t id_base)
{
    const uint64_t items = (uint64_t)*ovf_n * VIEW_SLICES;
    const SurfelSet cur = M.s[st->cur];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = (uint64_t)gridDim.x * 4u;
    for (uint64_t it = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); it < items; it += nwaves) {
        const uint32_t k = ovf[it / VIEW_SLICES];                                           // (wave-uniform)
        const uint32_t slice = (uint32_t)(it % VIEW_SLICES);
        view_surfel_wide(vp, cur.pos_conf, cur.norm_rad, k, id_base + k, slice * 64u + lane, 64u * VIEW_SLICES, key);
    }
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
        d = view_depth(kk);
        out = view_shade(vs, cur.norm_rad, cur.color, cur.time, (uint32_t)id);
    }
    rgba[p] = out;
    if (depth) depth[p] = d;
    if (ids) ids[p] = id;
}

}  // namespace sm
