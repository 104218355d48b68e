// sm_k_points.h -- point queries (DESIGN.md "4y. Point queries"; the rule: include/sm_c_api.h "point queries"): the nearest disc of a
// chunk to arbitrary points within a reach each, the exact point-to-disc distance of the header in front of a 64-bit atomicMin per
// point.  Included by sm_points.hip only.  The index is the ray casts': k_rays_count, k_rays_alloc, k_rays_fill, RaysChunk,
// rays_classify and rays_cell* of sm_k_rays.h, as they are; its rules (1) and (3) are referred to below by those numbers.
//   k_points_walk     one lane per point: the cells of the chunk's box that meet the point's cube, the best key in a register, one
//                     atomicMin per point and chunk
//   k_points_wide     one lane per point, the chunk's wide list through LDS in pieces of 128 records
//   k_points_resolve  one lane per point: centre, normal, radius, colour bytes and class + 1 of a key whose id lies in the chunk
//   k_points_finish   one lane per point: key -> (d2, id), the empty values where nobody won; the invalid points counted
//
// The index only saves tests.  Every (point, record) pair with `near` true whose dd could still win is tested, by these rules
// (u = 2^-24, half an ulp; x, p, r, R the float inputs taken as reals):
//
// (P1) What near implies.  The claim needs nothing of the normal, so it holds whatever h2 is (a normal in the denormals makes h2
//     wrong by tens of percent; a record whose nn is 0, infinite or a NaN never passes).  Let c = fl(x - p): |x_i - p_i| <= |c_i| (1 + u).
//     cc >= |c|^2 (1 - u)^3 less the squares that underflow (3 * 1.2e-38), so a = sqrt(cc) >= |c| (1 - 2u) - 2e-19.  near needs cc
//     finite (cc = inf makes rho2 inf or a NaN: dd = inf either way).  If h2 >= cc, dd >= h2 >= cc.  Otherwise rho2 >= (cc - h2)(1 - u),
//     s = fl(sqrt(rho2)) >= sqrt(cc - h2) (1 - u)^1.5, e >= (s - |r|)(1 - u) where that is positive, fl(e*e) >= e^2 (1 - u) - 1.5e-45 and
//     dd >= (h2 + fl(e*e)) (1 - u).  The real vector (sqrt(h2), sqrt(cc - h2)) has the length a, and taking (0, |r|) from it leaves at
//     least a - |r| (the triangle inequality), so in both cases
//         sqrt(dd) >= (1 - 3u) ((1 - 2u) a - |r|) - 4e-23,   hence   |x - p| - |r| <= sqrt(dd) (1 + 8u) + 8u |r| + 1e-18.
//     near has dd <= fl(R*R) <= R^2 (1 + u) (an R*R that overflows: cc finite already gives |x - p| < 1.9e19 <= R (1 + 2u)), and a
//     pair that can still lower or tie the point's key has dd <= B, the dd of that key.  With rho = min(R, sqrt(B)):
//         |x - p| - |r| <= rho (1 + 9u) + 8u |r| + 1e-18.
// (P2) The witness.  Let z = the point of the segment from x to p at the distance min(|r| (1 + 8u), |x - p|) from p.  It is within
//     |r| (1 + 8u) of p on every axis: by (3) (R_(3) = |r| * 1.0001 + ... + 1e-6, 1e-4 > 8u) its shifted coordinates lie in
//     [y_i - R_(3) + 1e-6, y_i + R_(3) - 1e-6] of the record, so cell(z) is a registered cell of a regular record, inside the chunk's
//     box.  And z is within rho (1 + 9u) + 1e-18 of x, as a Euclidean distance and so on every axis.
// (P3) The walk.  The point works in the shifted frame of (1), xs_i = (double)x_i - (double)g_i, with the reach in double
//         G = rho * (1 + 1e-6) + 1e-6                       (1e-6 > 9u; the absolute part pays (1)'s rounding, 2e-9 on the grid, twice)
//     and visits every cell of [cell(xs_i - G), cell(xs_i + G)] per axis, clamped to the chunk's box (a point off the grid, or an
//     infinite G, clamps to the box's ends: rays_cell_in), unless the cube misses the box on some axis by the same comparison in
//     metres -- then no z of (P2) exists.  cell() is monotone and z's shifted coordinates lie within G - 1e-6 + 4e-9 of xs on every
//     axis and inside the box: cell(z) is in the range.  So the walk would meet the registered cell of z.
// (P4) Skipped cells.  A cell whose box [k C, (k + 1) C]^3 lies farther from xs than G, as a Euclidean distance in double
//     (sum of squares > G^2; rounding 1e-15 relative against G's 1e-6), cannot hold z and is passed over without a probe; the
//     record's other cells that are passed over are not needed.  B only falls, during a walk and from chunk to chunk, so a G
//     taken from a later B is smaller, and a cell passed over under it holds no z of a pair that could lower or tie the key.
//     The lane starts from the key as earlier chunks left it and makes G anew whenever its best improves.  So that it improves
//     early, the cells are taken nearest first: m = the cell of xs clamped into the range, then for s = 1, 2, .. the shell of the
//     cells at the Chebyshev distance s from m, as six faces.  xs lies in m or beyond it as seen from the range, so every cell of
//     shell s is at least (s - 1) C away on one axis: a shell with (s - 1) C > G ends the walk, and so do all after it.
// (P5) Bounds.  Ranges are ints clamped to the chunk's box in cells before their loops; their product is taken in 64 bits; a
//     shell's faces are cut to the range before their loops, so the shells' loops pass over each cell of the range once.  A
//     cube over more than 64 + n / 8 cells of a chunk of n records is not walked: the chunk's regular records are tested one by one
//     (stats.gave_up counts these), so no point costs more than n tests per chunk that way, nor more than 64 + n / 8 probe walks the
//     other way (each ends as in (6) of sm_k_rays.h), whatever its reach and wherever it lies.
// Wide records are tested by every valid point (k_points_wide).  A record tested twice, through two of its cells, leaves the same
// key: the result is a minimum.  tests/points_ref.py restates (3), (P3), (P4) and (P5) in numpy; tests/test_points_filter_math.py
// checks that every near pair shares a visited, registered cell.
#pragma once

#include "sm_k_rays.h"

namespace sm {

constexpr double POINTS_REL = 1.0e-6, POINTS_ABS = 1.0e-6;   // (P3)

// the exact rule of the header; a nearer record (or an equal one with a lower id) lowers `best`.  R2 = fl(R*R).  The gate and a
// NaN in the centre or the radius are the index's business (rays_classify drops those records); the normal's is here.
__device__ __forceinline__ void points_test(const float4 &x, float R2, const float4 &pc, const float4 &nr, uint32_t id, unsigned long long &best)
{
    const float cx = x.x - pc.x, cy = x.y - pc.y, cz = x.z - pc.z;
    const float nn = (nr.x * nr.x + nr.y * nr.y) + nr.z * nr.z;
    const float h = (nr.x * cx + nr.y * cy) + nr.z * cz;
    const float h2 = (h * h) / nn;
    const float cc = (cx * cx + cy * cy) + cz * cz;
    float rho2 = cc - h2;
    if (!(rho2 > 0.0f)) rho2 = 0.0f;
    float e = sqrtf(rho2) - fabsf(nr.w);
    if (!(e > 0.0f)) e = 0.0f;
    const float dd = h2 + e * e;
    const float inf = __uint_as_float(0x7F800000u);
    if (nn > 0.0f && nn < inf && nr.w == nr.w && dd <= R2 && dd < inf) {
        const unsigned long long k = ((unsigned long long)__float_as_uint(dd + 0.0f) << 32) | (unsigned long long)id;
        best = k < best ? k : best;
    }
}

// a point is (pos, reach): the one statement of the validity rule, on the device
__device__ __forceinline__ bool points_valid(const float4 &x) { return simp_finite(x.x) && simp_finite(x.y) && simp_finite(x.z) && x.w >= 0.0f; }

// (P3): G of a reach and the key so far, squared for (P4)
__device__ __forceinline__ double points_reach(float R, unsigned long long best)
{
    double rho = (double)R;
    if (best != KEY_EMPTY) rho = fmin(rho, sqrt((double)__uint_as_float((uint32_t)(best >> 32))));
    return rho * (1.0 + POINTS_REL) + POINTS_ABS;
}
// (P4): the distance of a coordinate to the slab [k C, (k + 1) C]
__device__ __forceinline__ double points_gap(double xs, int k, double C) { return fmax(fmax((double)k * C - xs, xs - (double)(k + 1) * C), 0.0); }

// pts: one float4 per point.  The chunk's n records at rec have the ids gid0 ..
__global__ __launch_bounds__(256) void k_points_walk(const float4 *__restrict__ pts, uint32_t n_pts, const float4 *__restrict__ rec, uint32_t n,
                                                     uint32_t gid0, SimplifyArgs a, LeanTable T, const uint32_t *__restrict__ pairs,
                                                     const uint8_t *__restrict__ flag, const RaysChunk *__restrict__ ck,
                                                     unsigned long long *__restrict__ key, RaysTally *__restrict__ tally)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t probes = 0, tests = 0;
    const int lo[3] = {ck->lo[0], ck->lo[1], ck->lo[2]}, hi[3] = {ck->hi[0], ck->hi[1], ck->hi[2]};
    float4 x = make_float4(0, 0, 0, 0);
    bool go = i < n_pts && lo[0] <= hi[0];
    if (go) { x = pts[i]; go = points_valid(x); }
    if (go) {
        const unsigned long long seen = key[i];          // as earlier chunks left it: keys only fall
        unsigned long long best = seen;
        const float R2 = x.w * x.w;
        const double C = (double)a.V / 65536.0;
        const float xf[3] = {x.x, x.y, x.z};
        double xs[3], G = points_reach(x.w, best);
        int c0[3], c1[3], cm[3];
        long long cells = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {                    // (P3)
            xs[k] = (double)xf[k] - (double)a.origin[k];
            if (xs[k] + G < (double)lo[k] * C || xs[k] - G > (double)(hi[k] + 1) * C) go = false;
            c0[k] = rays_cell_in(xs[k] - G, a.V, lo[k], hi[k]);
            c1[k] = rays_cell_in(xs[k] + G, a.V, lo[k], hi[k]);
            cm[k] = rays_cell_in(xs[k], a.V, c0[k], c1[k]);
            cells *= (long long)(c1[k] - c0[k] + 1);
        }
        if (go && cells > (long long)(64u + n / 8u)) {   // (P5)
            atomicAdd(&tally->gave_up, 1ull);
            for (uint32_t r = 0; r < n; ++r)
                if (flag[r] == RAYS_REG) { points_test(x, R2, rec[(size_t)r * 3], rec[(size_t)r * 3 + 2], gid0 + r, best); ++tests; }
        } else if (go) {
            double G2 = G * G;
            const auto visit = [&](int cx, int cy, int cz) {
                uint32_t sl = 0;
                if (!lean_probe(T, rays_key(cx, cy, cz), false, sl, probes)) return;
                const uint2 run = T.run[sl];
                const unsigned long long was = best;
                for (uint32_t j = 0; j < run.x; ++j) {
                    const uint32_t r = pairs[run.y + j];
                    points_test(x, R2, rec[(size_t)r * 3], rec[(size_t)r * 3 + 2], gid0 + r, best);
                }
                tests += run.x;
                if (best < was) { G = points_reach(x.w, best); G2 = G * G; }
            };
            visit(cm[0], cm[1], cm[2]);
            int shells = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) shells = max(shells, max(cm[k] - c0[k], c1[k] - cm[k]));
            for (int s = 1; s <= shells && !((double)(s - 1) * C > G); ++s)      // (P4): nearest shells first
                for (int f = 0; f < 6; ++f) {
                    // face f of shell s: axis f / 2 fixed at cm -+ s, the axes before it within s - 1 of cm, those after it within s
                    const int ax = f >> 1, off = (f & 1) ? s : -s;
                    int b0[3], b1[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int w = k < ax ? s - 1 : s;
                        b0[k] = max(c0[k], k == ax ? cm[k] + off : cm[k] - w);
                        b1[k] = min(c1[k], k == ax ? cm[k] + off : cm[k] + w);
                    }
                    for (int cx = b0[0]; cx <= b1[0]; ++cx) {
                        const double dx = points_gap(xs[0], cx, C);
                        if (dx * dx > G2) continue;
                        for (int cy = b0[1]; cy <= b1[1]; ++cy) {
                            const double dy = points_gap(xs[1], cy, C), dxy = dx * dx + dy * dy;
                            if (dxy > G2) continue;
                            for (int cz = b0[2]; cz <= b1[2]; ++cz) {
                                const double dz = points_gap(xs[2], cz, C);
                                if (!(dxy + dz * dz > G2)) visit(cx, cy, cz);
                            }
                        }
                    }
                }
        }
        if (best < seen) atomicMin(&key[i], best);
    }
    rays_tally(tally, probes, tests);
}

__global__ __launch_bounds__(256) void k_points_wide(const float4 *__restrict__ pts, uint32_t n_pts, const float4 *__restrict__ rec, uint32_t gid0,
                                                     const uint32_t *__restrict__ wide, const RaysChunk *__restrict__ ck,
                                                     unsigned long long *__restrict__ key, RaysTally *__restrict__ tally)
{
    __shared__ float4 s_pc[RAYS_PIECE], s_nr[RAYS_PIECE];
    __shared__ uint32_t s_id[RAYS_PIECE];
    const uint32_t nw = ck->wide;                        // (the same for every lane of the launch)
    if (!nw) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    float4 x = make_float4(0, 0, 0, 0);
    bool go = i < n_pts;
    if (go) { x = pts[i]; go = points_valid(x); }
    const float R2 = x.w * x.w;
    unsigned long long best = KEY_EMPTY;
    uint32_t tests = 0;
    for (uint32_t base = 0; base < nw; base += RAYS_PIECE) {
        const uint32_t m = min(RAYS_PIECE, nw - base);
        __syncthreads();
        if (threadIdx.x < m) {
            const uint32_t r = wide[base + threadIdx.x];
            s_pc[threadIdx.x] = rec[(size_t)r * 3]; s_nr[threadIdx.x] = rec[(size_t)r * 3 + 2]; s_id[threadIdx.x] = gid0 + r;
        }
        __syncthreads();
        if (go) {
            for (uint32_t j = 0; j < m; ++j) points_test(x, R2, s_pc[j], s_nr[j], s_id[j], best);
            tests += m;
        }
    }
    if (best != KEY_EMPTY) atomicMin(&key[i], best);
    rays_tally(tally, 0u, tests);
}

// A later chunk that wins a point overwrites it.  The planes start as zeros: the empty values.  Any plane may be null.
__global__ void k_points_resolve(const float4 *__restrict__ rec, uint32_t gid0, uint32_t n, const unsigned long long *__restrict__ key, uint32_t n_pts,
                                 float *__restrict__ ctr, float *__restrict__ nrm, float *__restrict__ rad, uint8_t *__restrict__ rgb,
                                 uint8_t *__restrict__ sem)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pts) return;
    const unsigned long long kk = key[q];
    if (kk == KEY_EMPTY) return;
    const uint32_t row = (uint32_t)(kk & 0xFFFFFFFFull) - gid0;                                // wraps below the base
    if (row >= n) return;
    const uint32_t sc = __float_as_uint(rec[(size_t)row * 3 + 1].x);
    if (rgb) { rgb[(size_t)q * 3] = (uint8_t)((sc >> 16) & 0xFFu); rgb[(size_t)q * 3 + 1] = (uint8_t)((sc >> 8) & 0xFFu); rgb[(size_t)q * 3 + 2] = (uint8_t)(sc & 0xFFu); }
    if (sem) sem[q] = (uint8_t)(((sc >> 24) & 0xFFu) + 1u);
    if (ctr) { const float4 pc = rec[(size_t)row * 3]; ctr[(size_t)q * 3] = pc.x; ctr[(size_t)q * 3 + 1] = pc.y; ctr[(size_t)q * 3 + 2] = pc.z; }
    if (nrm || rad) {
        const float4 nr = rec[(size_t)row * 3 + 2];
        if (nrm) { nrm[(size_t)q * 3] = nr.x; nrm[(size_t)q * 3 + 1] = nr.y; nrm[(size_t)q * 3 + 2] = nr.z; }
        if (rad) rad[q] = nr.w;
    }
}

// ... and the invalid points are counted, by the rule the walks used (all 64 lanes of a wave reach the ballot)
__global__ __launch_bounds__(256) void k_points_finish(const float4 *__restrict__ pts, const unsigned long long *__restrict__ key, uint32_t n_pts,
                                                       float *__restrict__ d2, int32_t *__restrict__ ids, RaysTally *__restrict__ tally)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (q < n_pts) {
        const unsigned long long kk = key[q];
        d2[q] = __uint_as_float(kk == KEY_EMPTY ? 0x7F800000u : (uint32_t)(kk >> 32));
        ids[q] = kk == KEY_EMPTY ? -1 : (int32_t)(uint32_t)(kk & 0xFFFFFFFFull);
        bad = !points_valid(pts[q]);
    }
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&tally->bad, (unsigned long long)__popcll(m));
}

}  // namespace sm
