// sm_k_lidar.h -- lidar sweeps (DESIGN.md "4k. Lidar sweeps"; the rules: include/sm_c_api.h "lidar sweeps"): an exact ray-against-disc
// test of every surfel against the beams of a spherical grid, the nearest return per beam kept by a 64-bit atomicMin.
// Included by sm_lidar.hip only; the device functions the kernels call are in sm_d_lidar.h, which the scenes' kernels share.
//   k_lidar_splat        one lane per occupied slot of the live model, gated by the alive bit
//   k_lidar_splat_maps   grid (blocks of a chunk of map-file records, sweeps of the pass): box test, then the same per record
//   k_lidar_resolve      one lane per beam: key -> (range, id, colour bytes, class + 1); the empty values where nobody won
//
// The exact test (lidar_test) is the header's, fp32 in the written order, built without contraction.  In front of it stands a
// FOOTPRINT: rows [i0, i1) x columns [a0, a0 + wa) and [b0, b0 + wb) of the beam grid.  It only saves tests -- every beam the
// exact test can pass lies inside it:
//
// (1) What a hit implies.  c is the float centre in the sensor frame, the one the exact test uses; D = |c|, r the stored
//     radius.  The test passes only if the float q = t*d - c has (q.q) <= r*r.  Each q_i carries at most 1.2e-7 (D + r) of
//     rounding (the product and the difference, both of magnitude <= D + r), q.q and r*r 2e-7 relative.  So the point
//     P = t*d of the ray lies within R' = r (1 + 2e-7) + 2.1e-7 (D + r) of c.  The filter works with
//         R = |r| * 1.0001 + 1e-5 * D,
//     which exceeds R' by more than 9.7e-6 (D + r): a margin 40 times the float error of anything computed from it below.
// (2) Range.  |d| = 1 within 2e-7 (each component is a double result rounded once), so t = |P| / |d| lies in
//     [D - R', D + R'] (1 +- 2e-7).  D - R > max_range or D + R < min_range therefore excludes min_range <= t <= max_range.
// (3) Whole grid.  D <= R (the sensor inside the disc's sphere), and a centre or radius beyond 1e18 (where D*D overflows):
//     every beam.  A NaN in the centre or the radius: no beam -- num or q is a NaN and every comparison false.
// (4) Rows.  For D > R the ray passes within R' of c, so its direction lies within asin(R'/D) of c/D; two directions are at
//     least as far apart as their elevations.  With e_c = atan2(-c.y, rho), rho = hypot(c.x, c.z):
//         |el - e_c| <= asin(R / D) + S,   S = 1e-4 rad,
//     where S covers atan2f / asinf (a few ulps of pi/2: 1e-6), the float elevation table (1e-7), the beam's direction
//     against its nominal angles (2e-7).  The interval is found by two binary searches of the strictly increasing table,
//     23 steps at most (n_el <= 2^22), so non-uniform rows cost nothing extra.
// (5) Columns.  rho <= R: the sphere's shadow on the horizontal plane covers the axis, the disc lies over the pole of the
//     grid: every column.  Otherwise P's horizontal projection lies on the half line of azimuth az, within R' of (c.x, c.z):
//         |az - a_c| <= asin(R / rho) + S  (mod 360 deg),  a_c = atan2(c.x, c.z).
//     In degrees relative to az0 (reduced to [-180, 180) by the host): u = a_c - az0 in [0, 360), column j at j * step in
//     [0, 360].  The interval [u - w, u + w], w < 90.01, and ONE copy of it moved by 360 (down if u + w >= 360, up
//     otherwise: both can not reach [0, 360] at once) are cut to the columns that exist -- that is the seam, and a sweep
//     narrower than 360 deg simply has no column where the moved copy lands.  The two column runs are disjoint (2w < 360).
//     Float error in u and in the division by step is below 1e-4 deg for every allowed grid (n_az * step <= 360); S is 57e-4.
// (6) Every loop bound is an int clamped to the grid BEFORE the loop: rows by the search (0..n_el), columns by lidar_col_lo /
//     lidar_col_hi, whose comparisons send a NaN to an empty or a whole run.  A record can make the footprint the whole
//     grid (2^22 beams at most), never more.
// tests/lidar_ref.py restates (1)-(5) in numpy; tests/test_lidar_filter_math.py checks that every exact hit lies inside.
//
// Work split, as k_maps_splat_view's: a surfel of at most `lane_beams` beams is tested by its own lane; larger ones are
// picked by a ballot, broadcast with readlane (__shfl), and the wave's 64 lanes stride over the footprint.  Both paths call
// lidar_test, so which path tested a beam cannot change the result.
#pragma once

#include "sm_d_lidar.h"

namespace sm {

// slots [0, st->count) of the current set; ids are id_base + slot
__global__ __launch_bounds__(256) void k_lidar_splat(Model M, const DevState *__restrict__ st, const uint64_t *__restrict__ alive, LidarGrid g,
                                                     LidarPose p, uint64_t *__restrict__ key, uint32_t id_base, LidarTally *__restrict__ tally)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const SurfelSet cur = M.s[st->cur];
    // slots a deferred-compaction cull has killed are no surfels
    const bool have = k < st->count && ((alive[k >> 6] >> (k & 63u)) & 1ull);
    float4 pc = make_float4(0, 0, 0, 0), nr = pc;
    if (have) { pc = cur.pos_conf[k]; nr = cur.norm_rad[k]; }
    uint32_t wide;
    const uint32_t n = lidar_wave(g, p, have, pc, nr, id_base + k, key, &wide);
    lidar_count(tally, n, wide);
}

// workgroup (b, v) tests block b of the chunk against sweep v, or leaves before loading a record
__global__ __launch_bounds__(256) void k_lidar_splat_maps(MapsSoA c, uint32_t n, uint32_t id_base, const float4 *__restrict__ box, LidarGrid g,
                                                          const LidarPose *__restrict__ poses, uint64_t *__restrict__ key, size_t nbeams, int cull,
                                                          LidarTally *__restrict__ tally)
{
    const uint32_t v = blockIdx.y;
    const LidarPose p = poses[v];
    if (cull && lidar_box_outside(maps_box_load(box, blockIdx.x), g, p)) {                     // (workgroup-uniform)
        if (threadIdx.x == 0) atomicAdd(&tally->skipped, 1ull);
        return;
    }
    const uint32_t k = blockIdx.x * (uint32_t)MAPS_BLOCK + threadIdx.x;
    const bool have = k < n;
    float4 pc = make_float4(0, 0, 0, 0), nr = pc;
    if (have) { pc = c.pos_conf[k]; nr = c.norm_rad[k]; }
    uint32_t wide;
    const uint32_t nt = lidar_wave(g, p, have, pc, nr, id_base + k, key + (size_t)v * nbeams, &wide);
    lidar_count(tally, nt, wide);
}

// Per beam of the pass (total = sweeps * beams): a key whose id lies in [base, base + n) is written out from `color`, the
// source's colour words; with `last` the beams nobody won take the empty values.  A later source that wins a beam overwrites it.
__global__ void k_lidar_resolve(const uint32_t *__restrict__ color, uint32_t base, uint32_t n, const uint64_t *__restrict__ key, size_t total,
                                int last, float *__restrict__ range, int32_t *__restrict__ ids, uint8_t *__restrict__ rgb, uint8_t *__restrict__ sem)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const uint64_t kk = key[q];
    if (kk == KEY_EMPTY) {
        if (!last) return;
        range[q] = 0.0f; ids[q] = -1; sem[q] = 0;
        rgb[q * 3] = 0; rgb[q * 3 + 1] = 0; rgb[q * 3 + 2] = 0;
        return;
    }
    const uint32_t id = (uint32_t)(kk & 0xFFFFFFFFull), row = id - base;                       // wraps below the base
    if (row >= n) return;
    const uint32_t sc = color[row];
    range[q] = __uint_as_float((uint32_t)(kk >> 32));
    ids[q] = (int32_t)id;
    rgb[q * 3] = (uint8_t)((sc >> 16) & 0xFFu); rgb[q * 3 + 1] = (uint8_t)((sc >> 8) & 0xFFu); rgb[q * 3 + 2] = (uint8_t)(sc & 0xFFu);
    sem[q] = (uint8_t)(((sc >> 24) & 0xFFu) + 1u);
}

}  // namespace sm
