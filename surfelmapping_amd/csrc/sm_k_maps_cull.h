// sm_k_maps_cull.h -- the per-block view tests of the streamed renderers (sm_k_render_maps.h) and of the blended views' accumulation
// over chunks (sm_k_blend.h): can any record of a block of 256 set a pixel of this view?  Device functions only, no kernel.
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

}  // namespace sm
