// sm_d_lidar.h -- the device functions of the lidar sweeps (sm_k_lidar.h states the rules (1)-(6) they follow): the footprint, the exact
// test, the per-wave work split and the box test of a block of 256 records.  No kernels here: sm_k_lidar.h (the model and map
// files) and sm_k_scene.h (resident actors) hold those, so a surfel tested from any of the three sets the same key bits.
#pragma once

#include "sm_device.h"
#include "sm_k_maps_box.h"

namespace sm {

constexpr uint32_t LIDAR_LANE_BEAMS = 64;    // beams a lane tests by itself (SM_LIDAR_LANE_BEAMS overrides it for A/B runs; not tuned: DESIGN.md 4k)
constexpr float LIDAR_R_REL = 1.0001f, LIDAR_R_ABS = 1.0e-5f;   // (1)
constexpr float LIDAR_SLACK_RAD = 1.0e-4f;                       // (4), (5)
constexpr float LIDAR_HUGE = 1.0e18f;                            // (3)
constexpr float LIDAR_RAD2DEG = 57.29577951308232f;

struct LidarGrid {
    const float *dir;          // n_el * n_az * 3: sm_lidar_directions' table
    const float *el;           // n_el elevations in radians (float of the double conversion): the row search
    int n_az, n_el;
    float u0;                  // az0 reduced to [-180, 180), degrees
    float step;                // degrees
    float min_range, max_range, min_conf;
    uint32_t lane_beams;
};
struct LidarPose { float tinv[16]; };        // world -> sensor
struct LidarTally { unsigned long long tests, wide, skipped; };
struct LidarFoot { int i0, i1, a0, wa, b0, wb; };   // rows [i0, i1), columns [a0, a0 + wa) and [b0, b0 + wb)

// first row with el >= x (strict: el > x), in [0, n]
__device__ __forceinline__ int lidar_row_search(const float *__restrict__ el, int n, float x, bool strict)
{
    int lo = 0, hi = n;
    for (int it = 0; it < 23 && lo < hi; ++it) {
        const int mid = (lo + hi) >> 1;
        const float e = el[mid];
        if (strict ? (e > x) : (e >= x)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ceil(x) clamped to [0, n] and floor(x) clamped to [-1, n - 1] as ints (a NaN: 0 resp. -1)
__device__ __forceinline__ int lidar_col_lo(float x, int n)
{
    const float c = ceilf(x);
    return (c > 0.0f) ? ((c < (float)n) ? (int)c : n) : 0;
}
__device__ __forceinline__ int lidar_col_hi(float x, int n)
{
    const float f = floorf(x);
    return (f >= 0.0f) ? ((f < (float)(n - 1)) ? (int)f : n - 1) : -1;
}

// the footprint of a disc (float centre c in the sensor frame, stored radius r); false: no beam
__device__ __forceinline__ bool lidar_footprint(const LidarGrid &g, float3 c, float r, LidarFoot &f)
{
    const float ra = fabsf(r);
    if (!(c.x == c.x) || !(c.y == c.y) || !(c.z == c.z) || !(ra == ra)) return false;          // (3): a NaN
    f.i0 = 0; f.i1 = g.n_el; f.a0 = 0; f.wa = g.n_az; f.b0 = 0; f.wb = 0;
    if (!(fabsf(c.x) <= LIDAR_HUGE) || !(fabsf(c.y) <= LIDAR_HUGE) || !(fabsf(c.z) <= LIDAR_HUGE) || !(ra <= LIDAR_HUGE)) return true;
    const float D = sqrtf((c.x * c.x + c.y * c.y) + c.z * c.z);
    const float R = ra * LIDAR_R_REL + LIDAR_R_ABS * D;
    if (D - R > g.max_range || D + R < g.min_range) return false;                              // (2)
    if (!(R / D < 1.0f)) return true;                                                           // (3) (0 / 0 included)
    const float rho = sqrtf(c.x * c.x + c.z * c.z);
    const float ec = atan2f(-c.y, rho), al = asinf(R / D) + LIDAR_SLACK_RAD;                    // (4)
    f.i0 = lidar_row_search(g.el, g.n_el, ec - al, false);
    f.i1 = lidar_row_search(g.el, g.n_el, ec + al, true);
    if (f.i1 <= f.i0) return false;
    if (!(R / rho < 1.0f)) return true;                                                         // (5): over the pole
    const float w = (asinf(R / rho) + LIDAR_SLACK_RAD) * LIDAR_RAD2DEG;
    float u = atan2f(c.x, c.z) * LIDAR_RAD2DEG - g.u0;
    if (u < 0.0f) u += 360.0f;
    const float sh = (u + w >= 360.0f) ? -360.0f : 360.0f;
    f.a0 = lidar_col_lo((u - w) / g.step, g.n_az);
    f.wa = max(0, lidar_col_hi((u + w) / g.step, g.n_az) - f.a0 + 1);
    f.b0 = lidar_col_lo(((u - w) + sh) / g.step, g.n_az);
    f.wb = max(0, lidar_col_hi(((u + w) + sh) / g.step, g.n_az) - f.b0 + 1);
    return f.wa + f.wb > 0;
}

// what the exact test needs of a surfel, and where its returns go
struct LidarSurfel { float3 c, m; float num, rr; uint32_t id; };

__device__ __forceinline__ void lidar_test(const LidarGrid &g, const LidarSurfel &s, int row, int col, uint64_t *__restrict__ key)
{
    const size_t b = (size_t)row * (size_t)g.n_az + (size_t)col;
    const float dx = g.dir[3 * b], dy = g.dir[3 * b + 1], dz = g.dir[3 * b + 2];
    const float den = (s.m.x * dx + s.m.y * dy) + s.m.z * dz;
    const float t = s.num / den;
    const float qx = t * dx - s.c.x, qy = t * dy - s.c.y, qz = t * dz - s.c.z;
    const float qq = (qx * qx + qy * qy) + qz * qz;
    if (t >= g.min_range && t <= g.max_range && qq <= s.rr)
        atomicMin((unsigned long long *)&key[b], ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)s.id);
}

// beams e = first, first + stride, ... of the footprint (row-major over its rows and its two column runs)
__device__ __forceinline__ uint32_t lidar_run(const LidarGrid &g, const LidarSurfel &s, const LidarFoot &f, uint32_t first, uint32_t stride,
                                              uint64_t *__restrict__ key)
{
    const uint32_t W = (uint32_t)(f.wa + f.wb), total = (uint32_t)(f.i1 - f.i0) * W;            // <= n_el * n_az <= 2^22
    uint32_t n = 0;
    for (uint32_t e = first; e < total; e += stride, ++n) {
        const uint32_t ri = e / W, ci = e - ri * W;
        lidar_test(g, s, f.i0 + (int)ri, ci < (uint32_t)f.wa ? f.a0 + (int)ci : f.b0 + (int)(ci - (uint32_t)f.wa), key);
    }
    return n;
}

// One surfel per lane (have: this lane holds one that takes part), then the wave's large ones together.  All 64 lanes of a
// wave call it.  Returns the lane's exact tests; *wide: large surfels of the wave (the same in every lane).
__device__ __forceinline__ uint32_t lidar_wave(const LidarGrid &g, const LidarPose &p, bool have, float4 pc, float4 nr, uint32_t id,
                                               uint64_t *__restrict__ key, uint32_t *wide)
{
    LidarSurfel s;
    LidarFoot f = {0, 0, 0, 0, 0, 0};
    s.c = xform3(p.tinv, pc.x, pc.y, pc.z);
    s.m = rot3(p.tinv, nr.x, nr.y, nr.z);
    s.num = (s.m.x * s.c.x + s.m.y * s.c.y) + s.m.z * s.c.z;
    s.rr = nr.w * nr.w;
    s.id = id;
    have = have && pc.w >= g.min_conf && lidar_footprint(g, s.c, nr.w, f);
    const uint32_t beams = have ? (uint32_t)(f.i1 - f.i0) * (uint32_t)(f.wa + f.wb) : 0u;
    const bool big = beams > g.lane_beams;
    uint32_t n = 0;
    if (have && !big) {
        for (int row = f.i0; row < f.i1; ++row) {
            for (int col = f.a0; col < f.a0 + f.wa; ++col) lidar_test(g, s, row, col, key);
            for (int col = f.b0; col < f.b0 + f.wb; ++col) lidar_test(g, s, row, col, key);
        }
        n = beams;
    }
    const uint64_t m0 = __ballot(big);
    *wide = (uint32_t)__popcll(m0);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t m = m0; m; m &= m - 1ull) {
        const int src = __ffsll((unsigned long long)m) - 1;
        LidarSurfel b;
        LidarFoot fb;
        b.c.x = __shfl(s.c.x, src); b.c.y = __shfl(s.c.y, src); b.c.z = __shfl(s.c.z, src);
        b.m.x = __shfl(s.m.x, src); b.m.y = __shfl(s.m.y, src); b.m.z = __shfl(s.m.z, src);
        b.num = __shfl(s.num, src); b.rr = __shfl(s.rr, src); b.id = (uint32_t)__shfl((int)s.id, src);
        fb.i0 = __shfl(f.i0, src); fb.i1 = __shfl(f.i1, src); fb.a0 = __shfl(f.a0, src); fb.wa = __shfl(f.wa, src);
        fb.b0 = __shfl(f.b0, src); fb.wb = __shfl(f.wb, src);
        n += lidar_run(g, b, fb, lane, 64u, key);
    }
    return n;
}

// the tallies of a wave: one atomic per counter and wave
__device__ __forceinline__ void lidar_count(LidarTally *__restrict__ tally, uint32_t tests, uint32_t wide)
{
    const uint32_t t = wave_sum_u32(tests);
    if ((threadIdx.x & 63u) == 0u) {
        if (t) atomicAdd(&tally->tests, (unsigned long long)t);
        if (wide) atomicAdd(&tally->wide, (unsigned long long)wide);
    }
}

// ---------------------------------------------------------------------------------------------
// The box test of a block of 256 records (MapsBox: k_maps_intake's).  True = no record of the block can give a return.
// Every record's float centre c = xform3(tinv, centre) lies, up to E, in the box spanned by the eight transformed corners
// (the map is affine, whatever the pose holds; E = 4e-6 * the largest sum of |terms|, as maps_box_outside_image charges).  So
// lo = the distance from the sensor to that box - E and hi = its farthest corner + E bound every D of the block, and every
// |radius| is at most rmax.  A record is out of range if D - R > max_range or D + R < min_range with R = |r| * 1.0001 + 1e-5 D
// (lidar_footprint (2)); both follow for the whole block from
//     lo > (max_range + reach) * 1.0002     or     (hi + reach) * 1.0002 < min_range,    reach = rmax * 1.0001,
// where 1.0002 pays for the 1e-5 D and the roundings.  A block with a non-finite member is never skipped (maps_box_finite), nor
// one with a coordinate or a radius beyond 1e18, where squares overflow and lidar_footprint (3) offers the whole grid.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool lidar_box_outside(const MapsBox &b, const LidarGrid &g, const LidarPose &p)
{
    if (!maps_box_finite(b)) return false;
    const float *m = p.tinv;
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, mag = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float x = (c & 1) ? b.hx : b.lx, y = (c & 2) ? b.hy : b.ly, z = (c & 4) ? b.hz : b.lz;
        const float3 q = xform3(m, x, y, z);
        const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
        mag = fmaxf(mag, fmaxf(((fabsf(m[0]) * ax + fabsf(m[4]) * ay) + fabsf(m[8]) * az) + fabsf(m[12]),
                           fmaxf(((fabsf(m[1]) * ax + fabsf(m[5]) * ay) + fabsf(m[9]) * az) + fabsf(m[13]),
                                 ((fabsf(m[2]) * ax + fabsf(m[6]) * ay) + fabsf(m[10]) * az) + fabsf(m[14]))));
        lo[0] = fminf(lo[0], q.x); lo[1] = fminf(lo[1], q.y); lo[2] = fminf(lo[2], q.z);
        hi[0] = fmaxf(hi[0], q.x); hi[1] = fmaxf(hi[1], q.y); hi[2] = fmaxf(hi[2], q.z);
    }
    if (!(mag <= LIDAR_HUGE) || !(b.rmax <= LIDAR_HUGE)) return false;                         // squares would overflow: lidar_footprint (3)
    const float E = 4.0e-6f * mag;
    float near2 = 0.0f, far2 = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float n = fmaxf(fmaxf(lo[a], -hi[a]), 0.0f), f = fmaxf(fabsf(lo[a]), fabsf(hi[a]));
        near2 += n * n; far2 += f * f;
    }
    const float reach = b.rmax * LIDAR_R_REL;
    const float dlo = sqrtf(near2) * 0.9999f - 2.0f * E, dhi = sqrtf(far2) * 1.0001f + 2.0f * E;
    if (dlo > (g.max_range + reach) * 1.0002f) return true;
    if ((dhi + reach) * 1.0002f < g.min_range) return true;
    return false;
}

}  // namespace sm
