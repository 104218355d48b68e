// sm_k_scene.h -- scenes (DESIGN.md "4w. Scenes"; the rules: include/sm_c_api.h "scenes"): actors -- map files resident on the device
// as SoA planes with one box per 256 records (k_maps_intake's) -- drawn under one rigid pose per view into the key planes the
// static set is drawn into.  Included by sm_scene.hip only.
//   k_scene_splat_image    grid (all (actor, block) pairs, views of the batch): presence, box test, then per record warp_apply
//                          and render_surfel
//   k_scene_splat_lidar    the same around lidar_wave
//   k_scene_resolve_image  per pixel of the batch, after all sources: a key whose id is an actor's is shaded from its resident row
//   k_scene_resolve_lidar  the same per beam; it is the last resolve of the pass, so it writes the empty values too
// A record is placed in its lane by warp_apply (sm_d_warp.h: sm_warp_by_time's row rule) and handed in registers to the rule every
// other source is drawn by (sm_k_draw.h: render_surfel; sm_d_lidar.h: lidar_wave), so it sets the key bits it would set as a
// record of a file that sm_warp_by_time had moved -- the header's equality.  Ids: A + off_j + r (SceneActor::id_base = A + off_j).
//
// The box test (scene_box_world, then the static sources' own maps_box_outside_image / lidar_box_outside) skips a superset of nothing:
// (1) The block's box [lo, hi] bounds the stored centres of its records in the ACTOR frame, rmax their |radius|, and a block with
//     a non-finite member has rnorm = +inf (k_maps_intake).  Such a block, a box with a non-finite bound, and a pose under which
//     a corner's terms reach 1e18 (where sums could overflow to an inf - inf) are handed on with rnorm = +inf: maps_box_finite
//     fails in both tests and the block is never skipped.
// (2) A placed centre is c' = fl(C (c, 1)), row by row in warp_apply's order.  The exact affine image of c is a convex combination
//     of the exact images of the eight corners, so it lies in their bounding box.  Every float evaluation of a row
//     ((a0 x + a1 y) + a2 z) + t errs by at most 3 ulps of A = |a0 x| + |a1 y| + |a2 z| + |t| (< 2e-7 A), and A is convex in
//     (x, y, z), so no larger at c than at the worst corner: M = the largest A over rows and corners.  The float corner images and
//     the float centre image are each within 2e-7 M of the exact ones, so c' lies in the box of the float corner images widened
//     by 4e-7 M; the test widens by E = 4e-6 M, ten times that, as lidar_box_outside charges its own transform.
// (3) The radius passes through the placement unchanged, and neither renderer's reach depends on the normal's length: render_surfel
//     normalises the rotated normal (maps_reach needs rmax alone), lidar_test's disc is (q.q) <= r*r whatever |m| is.  The box
//     is widened all the same by what a pose at the 1e-3 limit can add to a normal's length: |R n|^2 = n^T (R^T R) n <=
//     |n|^2 (1 + 3e-3) (each of the nine entries of R^T R - I is at most 1e-3), so |R n| <= 1.0015 |n|, and the three roundings of
//     a row add 2e-7: rmax and rnorm grow by SCENE_NORMAL_GROWTH = 1.002, which keeps |n'| * |r| <= rnorm' for a test that reads rnorm.
// (4) With (2) and (3) the world box meets the premises of the two static tests -- every drawn record's float centre inside, every
//     |radius| at most rmax -- and their own superset arguments (sm_k_maps_cull.h, sm_d_lidar.h) carry over unchanged.
// tests/scene_ref.py restates scene_box_world in numpy; tests/test_scene_filter_math.py checks (2) and (3) on random blocks.
#pragma once

#include "sm_device.h"
#include "sm_d_lidar.h"
#include "sm_d_warp.h"
#include "sm_k_draw.h"
#include "sm_k_maps_box.h"
#include "sm_k_maps_cull.h"

namespace sm {

constexpr float SCENE_BOX_ERR = 4.0e-6f;         // (2)
constexpr float SCENE_NORMAL_GROWTH = 1.002f;    // (3)
constexpr float SCENE_HUGE = 1.0e18f;            // (1)

// one actor of the call: its rows [row0, row0 + n) in the resident planes (row0 a multiple of 256, so blocks and boxes are the
// file's own), the id of its row 0, its first workgroup in the splat grid
struct SceneActor { uint32_t row0, n, id_base, wg0; };

struct SceneDev {
    MapsSoA rows;                  // the resident planes
    const float4 *box;             // two float4 per block of 256 rows
    const SceneActor *actors;
    uint32_t n_actors, n_views;    // n_views: of the call (the stride of poses and present)
    const float4 *poses;           // [actor][view] three float4: the rows of the 3x4 pose
    const uint8_t *present;        // [actor][view]
    LidarTally *tally;             // tests and wide (lidar), skipped (both)
};

// the last actor whose first workgroup (resp. id base) is at most x: an actor without records shares its value with its successor
// and is passed over.  The interval [lo, hi) halves every step: 12 steps reach SM_SCENE_MAX_ACTORS = 4096 actors.
__device__ __forceinline__ uint32_t scene_actor_of_wg(const SceneDev &sc, uint32_t x)
{
    uint32_t lo = 0, hi = sc.n_actors;               // actors[lo].wg0 <= x (actors[0].wg0 is 0)
    for (int it = 0; it < 12 && hi - lo > 1u; ++it) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sc.actors[mid].wg0 <= x) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t scene_actor_of_id(const SceneDev &sc, uint32_t id)
{
    uint32_t lo = 0, hi = sc.n_actors;               // actors[lo].id_base <= id (actors[0].id_base is A)
    for (int it = 0; it < 12 && hi - lo > 1u; ++it) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sc.actors[mid].id_base <= id) lo = mid; else hi = mid;
    }
    return lo;
}

// the block's box in the world under the pose (c0 | c1 | c2): see (1)-(3) above
__device__ __forceinline__ MapsBox scene_box_world(const MapsBox &b, const float4 &c0, const float4 &c1, const float4 &c2)
{
    const float INF = __uint_as_float(0x7F800000u);
    MapsBox w = b;
    w.rnorm = INF;
    if (!maps_box_finite(b)) return w;
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, mag = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float x = (c & 1) ? b.hx : b.lx, y = (c & 2) ? b.hy : b.ly, z = (c & 4) ? b.hz : b.lz;
        const float qx = ((c0.x * x + c0.y * y) + c0.z * z) + c0.w;
        const float qy = ((c1.x * x + c1.y * y) + c1.z * z) + c1.w;
        const float qz = ((c2.x * x + c2.y * y) + c2.z * z) + c2.w;
        const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
        mag = fmaxf(mag, fmaxf(((fabsf(c0.x) * ax + fabsf(c0.y) * ay) + fabsf(c0.z) * az) + fabsf(c0.w),
                           fmaxf(((fabsf(c1.x) * ax + fabsf(c1.y) * ay) + fabsf(c1.z) * az) + fabsf(c1.w),
                                 ((fabsf(c2.x) * ax + fabsf(c2.y) * ay) + fabsf(c2.z) * az) + fabsf(c2.w))));
        lo[0] = fminf(lo[0], qx); lo[1] = fminf(lo[1], qy); lo[2] = fminf(lo[2], qz);
        hi[0] = fmaxf(hi[0], qx); hi[1] = fmaxf(hi[1], qy); hi[2] = fmaxf(hi[2], qz);
    }
    if (!(mag <= SCENE_HUGE)) return w;                  // (a NaN included)
    const float E = SCENE_BOX_ERR * mag;
    w.lx = lo[0] - E; w.ly = lo[1] - E; w.lz = lo[2] - E;
    w.hx = hi[0] + E; w.hy = hi[1] + E; w.hz = hi[2] + E;
    w.rmax = b.rmax * SCENE_NORMAL_GROWTH;
    w.rnorm = b.rnorm * SCENE_NORMAL_GROWTH;
    return w;
}

// what a workgroup of either splat learns before it loads a record: its actor, its block, the pose row of (actor, view)
struct SceneWork { SceneActor a; uint32_t blk; float4 c0, c1, c2; bool present; };

__device__ __forceinline__ SceneWork scene_work(const SceneDev &sc, uint32_t wg, uint32_t view)
{
    SceneWork w;
    const uint32_t j = scene_actor_of_wg(sc, wg);        // (workgroup-uniform, like everything here)
    w.a = sc.actors[j];
    w.blk = wg - w.a.wg0;
    const size_t pv = (size_t)j * sc.n_views + view;
    w.present = sc.present[pv] != 0;
    if (w.present) { w.c0 = sc.poses[pv * 3]; w.c1 = sc.poses[pv * 3 + 1]; w.c2 = sc.poses[pv * 3 + 2]; }
    else w.c0 = w.c1 = w.c2 = make_float4(0, 0, 0, 0);   // (rows of absent views are not read: the host has not checked them)
    return w;
}

__device__ __forceinline__ MapsBox scene_block_box(const SceneDev &sc, const SceneWork &w)
{
    return scene_box_world(maps_box_load(sc.box, w.a.row0 / (uint32_t)MAPS_BLOCK + w.blk), w.c0, w.c1, w.c2);
}

// workgroup (g, v) draws block g - wg0 of its actor into view v0 + v's key plane (plane v of the batch), or leaves at once: the
// actor is absent from the view, or its block is outside it
__global__ __launch_bounds__(256) void k_scene_splat_image(SceneDev sc, const RenderParams *__restrict__ rps, uint32_t v0, uint64_t *__restrict__ key,
                                                           size_t npix, int cull)
{
    const uint32_t v = blockIdx.y;
    const SceneWork w = scene_work(sc, blockIdx.x, v0 + v);
    if (!w.present) return;
    const RenderParams rp = rps[v];
    if (cull && maps_box_outside_image(scene_block_box(sc, w), rp)) {
        if (threadIdx.x == 0) atomicAdd(&sc.tally->skipped, 1ull);
        return;
    }
    const uint32_t k = w.blk * (uint32_t)MAPS_BLOCK + threadIdx.x;
    if (k >= w.a.n) return;
    float4 pc = sc.rows.pos_conf[w.a.row0 + k], nr = sc.rows.norm_rad[w.a.row0 + k];
    warp_apply(w.c0, w.c1, w.c2, pc, nr);
    render_surfel(rp, pc, nr, w.a.id_base + k, key + (size_t)v * npix);
}

// the same shape around lidar_wave, which all 64 lanes of a wave call (every return above it is workgroup-uniform)
__global__ __launch_bounds__(256) void k_scene_splat_lidar(SceneDev sc, LidarGrid g, const LidarPose *__restrict__ poses, uint32_t v0,
                                                           uint64_t *__restrict__ key, size_t nbeams, int cull)
{
    const uint32_t v = blockIdx.y;
    const SceneWork w = scene_work(sc, blockIdx.x, v0 + v);
    if (!w.present) return;
    const LidarPose p = poses[v];
    if (cull && lidar_box_outside(scene_block_box(sc, w), g, p)) {
        if (threadIdx.x == 0) atomicAdd(&sc.tally->skipped, 1ull);
        return;
    }
    const uint32_t k = w.blk * (uint32_t)MAPS_BLOCK + threadIdx.x;
    const bool have = k < w.a.n;
    float4 pc = make_float4(0, 0, 0, 0), nr = pc;
    if (have) {
        pc = sc.rows.pos_conf[w.a.row0 + k]; nr = sc.rows.norm_rad[w.a.row0 + k];
        warp_apply(w.c0, w.c1, w.c2, pc, nr);
    }
    uint32_t wide;
    const uint32_t nt = lidar_wave(g, p, have, pc, nr, w.a.id_base + k, key + (size_t)v * nbeams, &wide);
    lidar_count(sc.tally, nt, wide);
}

// the colour word of the actor row that holds id (>= A), or false: not an actor's id
__device__ __forceinline__ bool scene_color_of(const SceneDev &sc, uint32_t A, uint32_t id, uint32_t &color)
{
    if (id < A) return false;
    const SceneActor a = sc.actors[scene_actor_of_id(sc, id)];
    const uint32_t row = id - a.id_base;
    if (row >= a.n) return false;
    color = sc.rows.color[a.row0 + row];
    return true;
}

// per pixel of the batch (total = views * pixels), once all sources are drawn
__global__ void k_scene_resolve_image(SceneDev sc, uint32_t A, const uint64_t *__restrict__ key, size_t total, uint8_t *__restrict__ bgr,
                                      uint8_t *__restrict__ sem)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const uint64_t kk = key[q];
    uint32_t sc_word;
    if (kk == KEY_EMPTY || !scene_color_of(sc, A, (uint32_t)(kk & 0xFFFFFFFFull), sc_word)) return;
    uint8_t b, g, r, s;
    render_shade(sc_word, b, g, r, s);
    bgr[q * 3] = b; bgr[q * 3 + 1] = g; bgr[q * 3 + 2] = r;
    sem[q] = s;
}

// per beam of the pass, k_lidar_resolve's outputs; the pass's last resolve: beams nobody won take the empty values
__global__ void k_scene_resolve_lidar(SceneDev sc, uint32_t A, const uint64_t *__restrict__ key, size_t total, float *__restrict__ range,
                                      int32_t *__restrict__ ids, uint8_t *__restrict__ rgb, uint8_t *__restrict__ sem)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const uint64_t kk = key[q];
    if (kk == KEY_EMPTY) {
        range[q] = 0.0f; ids[q] = -1; sem[q] = 0;
        rgb[q * 3] = 0; rgb[q * 3 + 1] = 0; rgb[q * 3 + 2] = 0;
        return;
    }
    const uint32_t id = (uint32_t)(kk & 0xFFFFFFFFull);
    uint32_t sc_word;
    if (!scene_color_of(sc, A, id, sc_word)) return;
    range[q] = __uint_as_float((uint32_t)(kk >> 32));
    ids[q] = (int32_t)id;
    rgb[q * 3] = (uint8_t)((sc_word >> 16) & 0xFFu); rgb[q * 3 + 1] = (uint8_t)((sc_word >> 8) & 0xFFu); rgb[q * 3 + 2] = (uint8_t)(sc_word & 0xFFu);
    sem[q] = (uint8_t)(((sc_word >> 24) & 0xFFu) + 1u);
}

}  // namespace sm
