// sm_k_rays.h -- ray casts (DESIGN.md "4x. Ray casts"; the rule: include/sm_c_api.h "ray casts"): arbitrary rays against the records of
// a chunk, the exact ray-against-disc test of the header in front of a 64-bit atomicMin per ray.  Included by sm_rays.hip, and through
// sm_k_points.h by sm_points.hip, which builds the same index (k_rays_count, k_rays_alloc, k_rays_fill) and walks it otherwise
// -- so the kernels are static: each of the two sources has its own copy of those it launches.
//   k_rays_count    one lane per record: dropped, wide or regular; a regular record claims the cells of its cube in the lean
//                   table (key | count, first) and counts itself into each; the chunk's box in cells
//   k_rays_alloc    one lane per slot: a cell's run in the pair list, from a cursor one wave adds to once
//   k_rays_fill     one lane per regular record: its index into the run of each of its cells (order within a cell is open:
//                   the result is a minimum)
//   k_rays_cast     one lane per ray: the slab traversal below, the best key in a register, one atomicMin per ray and chunk
//   k_rays_wide     one lane per ray, the chunk's wide list through LDS in pieces of 128 records
//   k_rays_resolve  one lane per ray: colour bytes, class + 1 and normal of a key whose id lies in the chunk
//   k_rays_finish   one lane per ray: key -> (t, id), the empty values where nobody won; the invalid rays counted
//
// The index only saves tests.  Every (ray, record) pair that passes the exact test (rays_test) is tested, by these rules:
//
// (1) Frame and cells.  The grid is the simplification's: V = the cell edge in 2^-16 m, origin g.  Everything below is in the
//     SHIFTED frame y = (double)x - (double)g, per axis, in double.  cell(y) = floor(floor(y * 65536) / V) (rays_cell; simp_classify's
//     arithmetic), which is floor(y / C) with C = V / 65536 exactly, and is monotone in y.  A y with |y| >= 2^24 or a cell
//     outside [-65536, 65535] is off the grid.  The subtraction rounds by at most 1.2e-16 (|x| + |g|) <= 4e-9 m on the grid.
// (2) What a hit implies.  The test passes only if the float q = fl(fl(t*d) - c), c = fl(p - o), has q.q <= r*r, so
//     |q_i| <= |r| (1 + 3e-7) + 2e-19 (squares that underflow).  Each rounding is half an ulp: 2^-24 of its result.  From
//     |fl(t*d_i)| <= |c_i| + |q_i| (1 + 2^-24) and |c_i| <= (|p_i| + |o_i|) (1 + 2^-24), the real point H = o + t*d of the ray
//     at the float t has
//         |H_i - p_i| <= |q_i| + 2^-24 (|c_i| + |t*d_i| + |q_i|) <= |r| * 1.000001 + 1.2e-7 |p_i| + 1.2e-7 |o_i|  (+ 1e-18).
//     Also t_min <= t <= t_max in float, exactly.  W_i below = (the chunk box's largest |y_i|) + |g_i| bounds |H_i| of a hit.
// (3) Registration.  A record is registered in every cell of [cell(y_i - R), cell(y_i + R)] per axis, y = the shifted centre,
//         R = |r| * 1.0001 + 2.5e-7 * max_i |p_i| + 1e-6          (double).
//     More than 8 such cells, an end off the grid, a radius that is not finite, or no free slot within LEAN_WALK probes: the
//     record is WIDE and every ray tests it directly.  A NaN in the centre or the radius, or conf >= min_conf false: no ray can
//     hit it (num, q or r*r is a NaN; the gate) and it is dropped.
// (4) Traversal.  The ray works with the slack
//         S = max_i 2.5e-7 (2 |o_i| + W_i) + 1e-6,
//     so by (2) and (3) H's shifted coordinates h satisfy y_i - R + 1e-6 <= h_i <= y_i + R - 1e-6 and the 1e-6 pays (1)'s
//     rounding: cell(h_i) lies in the record's range on every axis, and the cell triple of h is a registered cell of the record.
//     The ray visits it: (a) the segment [t_min, t_max] is cut to the t where every y_i(t) = oy_i + t*d_i lies in the chunk
//     box grown by S (a miss skips the chunk); (b) m = the axis of the largest |d_i|; for every slab k of cells along m
//     between the cut segment's ends (grown by S, clamped to the box), T_k = the t with y_m(t) in [k*C - S, (k+1)*C + S], cut to
//     the segment; cell(h_m) = k implies t in T_k; (c) on the other two axes y_i(t) is linear, so over T_k it lies between its
//     values at T_k's ends; the cells of that interval grown by S, clamped to the box, are all visited.  Double rounding in
//     (a)-(c) is below 1e-15 (W_i + |oy_i| + S), a 1e-8 part of S; an error dt in T_k's ends moves y_i by |d_i| dt <= |d_m| dt,
//     which the S on the slab's faces covers.
// (5) Early stop.  Slabs are taken in the order of t.  Every hit in slab k or later has t >= T_k's lower end, and these ends
//     do not fall; a slab whose lower end lies above the best t so far ends the walk (strictly above: an equal t with a lower id
//     is still looked for).
// (6) Bounds.  Slabs and cells are ints clamped to the chunk's box in cells before their loops; a probe walk ends at the key,
//     at an empty slot or after LEAN_WALK slots (a key that was claimed lies within LEAN_WALK of its hash, and slots never
//     empty again, so a later walk finds it in as many steps).  A ray that has visited more than 64 + n / 8 cells of a chunk of n
//     records gives the walk up and tests the chunk's regular records one by one -- so no ray costs more than n tests and
//     probes per chunk, wherever its origin lies (stats.gave_up counts these walks).  The table and its walk are the voxel
//     owner's: LeanTable, lean_probe (sm_d_simplify.h).
// tests/rays_ref.py restates (1), (3) and (4) in numpy; tests/test_rays_filter_math.py checks that every exact hit shares a cell.
#pragma once

#include "sm_d_simplify.h"

namespace sm {

constexpr double RAYS_R_REL = 1.0001, RAYS_REL = 2.5e-7, RAYS_ABS = 1.0e-6;   // (3), (4)
constexpr double RAYS_GRID = 16777216.0;                 // (1)
constexpr long long RAYS_MAX_CELLS = 8;                  // (3)
constexpr uint32_t RAYS_PIECE = 128u;                    // records of the wide list in LDS at a time
enum { RAYS_DROP = 0, RAYS_REG = 1, RAYS_WIDE = 2 };

// per chunk, in device memory: the box in cells of the registered cubes (lo > hi: none), the pair cursor, cells, the wide list's length, those of it that found no slot
struct RaysChunk { int lo[3], hi[3]; uint32_t pairs, cells, wide, no_slot; };
struct RaysTally { unsigned long long probes, tests, gave_up, bad; };

// (1): the cell of a shifted coordinate; false: off the grid
__device__ __forceinline__ bool rays_cell(double y, long long V, int &c)
{
    if (!(fabs(y) < RAYS_GRID)) return false;
    const long long X = (long long)floor(y * 65536.0);
    long long q = X / V;
    if (X - q * V < 0) --q;                              // floor division
    if (q < -65536 || q > 65535) return false;
    c = (int)q;
    return true;
}
// ... clamped to [lo, hi] (lo <= hi), whatever y is
__device__ __forceinline__ int rays_cell_in(double y, long long V, int lo, int hi)
{
    if (!(y > -RAYS_GRID)) return lo;
    if (!(y < RAYS_GRID)) return hi;
    const long long X = (long long)floor(y * 65536.0);
    long long q = X / V;
    if (X - q * V < 0) --q;
    return q < lo ? lo : q > hi ? hi : (int)q;
}
__device__ __forceinline__ unsigned long long rays_key(int cx, int cy, int cz)
{
    return ((unsigned long long)(cx + 65536) << 34) | ((unsigned long long)(cy + 65536) << 17) | (unsigned long long)(cz + 65536);
}

// (3): what becomes of a record; regular: its cells [c0, c1] per axis
__device__ __forceinline__ int rays_classify(const SimplifyArgs &a, const float4 &pc, const float4 &nr, float min_conf, int no_index, int c0[3], int c1[3])
{
    if (!(pc.w >= min_conf)) return RAYS_DROP;
    if (!(pc.x == pc.x) || !(pc.y == pc.y) || !(pc.z == pc.z) || !(nr.w == nr.w)) return RAYS_DROP;
    if (no_index) return RAYS_WIDE;
    const float ra = fabsf(nr.w);
    if (!simp_finite(ra)) return RAYS_WIDE;
    const float p[3] = {pc.x, pc.y, pc.z};
    const double m = fmax(fmax(fabs((double)p[0]), fabs((double)p[1])), fabs((double)p[2]));
    const double R = ((double)ra * RAYS_R_REL + RAYS_REL * m) + RAYS_ABS;
    long long cells = 1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double y = (double)p[i] - (double)a.origin[i];
        if (!rays_cell(y - R, a.V, c0[i]) || !rays_cell(y + R, a.V, c1[i])) return RAYS_WIDE;
        cells *= (long long)(c1[i] - c0[i] + 1);
    }
    return cells > RAYS_MAX_CELLS ? RAYS_WIDE : RAYS_REG;
}

// the exact test of the header; a hit lowers `best`
__device__ __forceinline__ void rays_test(const float4 &o, const float4 &d, const float4 &pc, const float4 &nr, uint32_t id, unsigned long long &best)
{
    const float cx = pc.x - o.x, cy = pc.y - o.y, cz = pc.z - o.z;
    const float den = (nr.x * d.x + nr.y * d.y) + nr.z * d.z;
    const float num = (nr.x * cx + nr.y * cy) + nr.z * cz;
    const float t = num / den;
    const float qx = t * d.x - cx, qy = t * d.y - cy, qz = t * d.z - cz;
    const float qq = (qx * qx + qy * qy) + qz * qz;
    if (t >= o.w && t <= d.w && qq <= nr.w * nr.w) {
        const unsigned long long k = ((unsigned long long)__float_as_uint(t + 0.0f) << 32) | (unsigned long long)id;
        best = k < best ? k : best;
    }
}

// a[i] for an i known at run time, without an indexed register array
__device__ __forceinline__ double rays_pick(const double a[3], int i) { return i == 0 ? a[0] : i == 1 ? a[1] : a[2]; }
__device__ __forceinline__ int rays_pick(const int a[3], int i) { return i == 0 ? a[0] : i == 1 ? a[1] : a[2]; }

// a ray is (origin, t_min), (dir, t_max): the one statement of the validity rule, on the device
__device__ __forceinline__ bool rays_valid(const float4 &o, const float4 &d)
{
    const bool fin = simp_finite(o.x) && simp_finite(o.y) && simp_finite(o.z) && simp_finite(o.w) && simp_finite(d.x) && simp_finite(d.y) &&
                     simp_finite(d.z) && simp_finite(d.w);
    return fin && o.w >= 0.0f && d.w >= o.w && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f);
}

// the tallies of a wave: one atomic per counter and wave (all 64 lanes call it)
__device__ __forceinline__ void rays_tally(RaysTally *__restrict__ tally, uint32_t probes, uint32_t tests)
{
    const uint32_t p = wave_sum_u32(probes), t = wave_sum_u32(tests);
    if ((threadIdx.x & 63u) == 0u) {
        if (p) atomicAdd(&tally->probes, (unsigned long long)p);
        if (t) atomicAdd(&tally->tests, (unsigned long long)t);
    }
}

static __global__ __launch_bounds__(256) void k_rays_count(const float4 *__restrict__ rec, uint32_t n, SimplifyArgs a, float min_conf, int no_index, LeanTable T,
                                                           uint8_t *__restrict__ flag, uint32_t *__restrict__ wide, RaysChunk *__restrict__ ck)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const float4 pc = rec[(size_t)t * 3], nr = rec[(size_t)t * 3 + 2];
    int c0[3], c1[3];
    int kind = rays_classify(a, pc, nr, min_conf, no_index, c0, c1);
    if (kind == RAYS_REG) {
        uint32_t sl = 0, probes = 0;
        bool ok = true;                                  // every cell has its slot before any is counted into
        for (int x = c0[0]; x <= c1[0]; ++x)
            for (int y = c0[1]; y <= c1[1]; ++y)
                for (int z = c0[2]; z <= c1[2]; ++z) ok = ok && lean_probe(T, rays_key(x, y, z), true, sl, probes);
        if (!ok) { kind = RAYS_WIDE; atomicAdd(&ck->no_slot, 1u); }
    }
    if (kind == RAYS_REG) {
        uint32_t sl = 0, probes = 0;
        for (int x = c0[0]; x <= c1[0]; ++x)
            for (int y = c0[1]; y <= c1[1]; ++y)
                for (int z = c0[2]; z <= c1[2]; ++z)
                    if (lean_probe(T, rays_key(x, y, z), true, sl, probes)) atomicAdd(&T.run[sl].x, 1u);   // (claim: no stale "empty" can hide a key)
#pragma unroll
        for (int i = 0; i < 3; ++i) { atomicMin(&ck->lo[i], c0[i]); atomicMax(&ck->hi[i], c1[i]); }
    }
    flag[t] = (uint8_t)kind;
    if (kind == RAYS_WIDE) wide[atomicAdd(&ck->wide, 1u)] = t;
}

// run.y becomes the END of the cell's run; k_rays_fill counts it down to the start
static __global__ __launch_bounds__(256) void k_rays_alloc(LeanTable T, RaysChunk *__restrict__ ck)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t cnt = sl <= T.mask ? T.run[sl].x : 0u;
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    const uint32_t total = __shfl(incl, 63);
    const uint32_t cells = (uint32_t)__popcll(__ballot(cnt != 0u));
    uint32_t base = 0;
    if (lane == 0 && total) { base = atomicAdd(&ck->pairs, total); atomicAdd(&ck->cells, cells); }
    base = __shfl(base, 0);
    if (cnt) T.run[sl].y = base + incl;
}

static __global__ __launch_bounds__(256) void k_rays_fill(const float4 *__restrict__ rec, uint32_t n, SimplifyArgs a, float min_conf, LeanTable T,
                                                          const uint8_t *__restrict__ flag, uint32_t *__restrict__ pairs)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n || flag[t] != RAYS_REG) return;
    const float4 pc = rec[(size_t)t * 3], nr = rec[(size_t)t * 3 + 2];
    int c0[3], c1[3];
    if (rays_classify(a, pc, nr, min_conf, 0, c0, c1) != RAYS_REG) return;      // (the same arithmetic as k_rays_count's: it is)
    uint32_t sl = 0, probes = 0;
    for (int x = c0[0]; x <= c1[0]; ++x)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int z = c0[2]; z <= c1[2]; ++z)
                if (lean_probe(T, rays_key(x, y, z), false, sl, probes)) pairs[atomicSub(&T.run[sl].y, 1u) - 1u] = t;
}

// rays: two float4 per ray.  The chunk's n records at rec have the ids gid0 ..
static __global__ __launch_bounds__(256) void k_rays_cast(const float4 *__restrict__ rays, uint32_t n_rays, const float4 *__restrict__ rec, uint32_t n,
                                                          uint32_t gid0, SimplifyArgs a, LeanTable T, const uint32_t *__restrict__ pairs,
                                                          const uint8_t *__restrict__ flag, const RaysChunk *__restrict__ ck,
                                                          unsigned long long *__restrict__ key, RaysTally *__restrict__ tally)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t probes = 0, tests = 0;
    const int lo[3] = {ck->lo[0], ck->lo[1], ck->lo[2]}, hi[3] = {ck->hi[0], ck->hi[1], ck->hi[2]};
    float4 o = make_float4(0, 0, 0, 0), d = o;
    bool go = i < n_rays && lo[0] <= hi[0];
    if (go) { o = rays[(size_t)i * 2]; d = rays[(size_t)i * 2 + 1]; go = rays_valid(o, d); }
    unsigned long long best = KEY_EMPTY;
    if (go) {
        const double C = (double)a.V / 65536.0;
        const float of[3] = {o.x, o.y, o.z}, df[3] = {d.x, d.y, d.z};
        double oy[3], dd[3], S = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            oy[k] = (double)of[k] - (double)a.origin[k];
            dd[k] = (double)df[k];
            const double W = fmax(fabs((double)lo[k] * C), fabs((double)(hi[k] + 1) * C)) + fabs((double)a.origin[k]);
            S = fmax(S, RAYS_REL * (2.0 * fabs((double)of[k]) + W));
        }
        S += RAYS_ABS;
        // (4a) the segment inside the grown box
        double ta = (double)o.w, tb = (double)d.w;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double L = (double)lo[k] * C - S, U = (double)(hi[k] + 1) * C + S;
            if (dd[k] == 0.0) {
                if (oy[k] < L || oy[k] > U) go = false;
            } else {
                const double t1 = (L - oy[k]) / dd[k], t2 = (U - oy[k]) / dd[k];
                ta = fmax(ta, fmin(t1, t2));
                tb = fmin(tb, fmax(t1, t2));
            }
        }
        go = go && ta <= tb;
        if (go) {
            // (4b) the slabs along the major axis, in the order of t
            int m = 0;
            if (fabs(dd[1]) > fabs(dd[m])) m = 1;
            if (fabs(dd[2]) > fabs(dd[m])) m = 2;
            const int u = m == 0 ? 1 : 0, v = m == 2 ? 1 : 2;
            const double om = rays_pick(oy, m), dm = rays_pick(dd, m), ou = rays_pick(oy, u), du = rays_pick(dd, u), ov = rays_pick(oy, v), dv = rays_pick(dd, v);
            const int lom = rays_pick(lo, m), him = rays_pick(hi, m), lou = rays_pick(lo, u), hiu = rays_pick(hi, u), lov = rays_pick(lo, v), hiv = rays_pick(hi, v);
            const double ya = om + ta * dm, yb = om + tb * dm;
            const int kA = rays_cell_in(fmin(ya, yb) - S, a.V, lom, him), kB = rays_cell_in(fmax(ya, yb) + S, a.V, lom, him);
            const int step = dm > 0.0 ? 1 : -1, k0 = step > 0 ? kA : kB, slabs = kB - kA + 1;
            const uint32_t budget = 64u + n / 8u;
            uint32_t visits = 0;
            bool brute = false;
            for (int sidx = 0; sidx < slabs && !brute; ++sidx) {
                const int k = k0 + sidx * step;
                const double t1 = ((double)k * C - S - om) / dm, t2 = ((double)(k + 1) * C + S - om) / dm;
                const double tl = fmax(ta, fmin(t1, t2)), th = fmin(tb, fmax(t1, t2));
                if (best != KEY_EMPTY && (double)__uint_as_float((uint32_t)(best >> 32)) < tl) break;      // (5)
                if (!(tl <= th)) continue;
                // (4c) the cells of the other two axes over T_k
                const double ua = ou + tl * du, ub = ou + th * du, va = ov + tl * dv, vb = ov + th * dv;
                const int u0 = rays_cell_in(fmin(ua, ub) - S, a.V, lou, hiu), u1 = rays_cell_in(fmax(ua, ub) + S, a.V, lou, hiu);
                const int v0 = rays_cell_in(fmin(va, vb) - S, a.V, lov, hiv), v1 = rays_cell_in(fmax(va, vb) + S, a.V, lov, hiv);
                for (int cu = u0; cu <= u1 && !brute; ++cu)
                    for (int cv = v0; cv <= v1; ++cv) {
                        if (++visits > budget) { brute = true; break; }
                        const int cx = m == 0 ? k : cu, cy = m == 1 ? k : m == 0 ? cu : cv, cz = m == 2 ? k : cv;
                        uint32_t sl = 0;
                        if (!lean_probe(T, rays_key(cx, cy, cz), false, sl, probes)) continue;
                        const uint2 run = T.run[sl];
                        for (uint32_t j = 0; j < run.x; ++j) {
                            const uint32_t r = pairs[run.y + j];
                            rays_test(o, d, rec[(size_t)r * 3], rec[(size_t)r * 3 + 2], gid0 + r, best);
                        }
                        tests += run.x;
                    }
            }
            if (brute) atomicAdd(&tally->gave_up, 1ull);
            if (brute)                                   // (6)
                for (uint32_t r = 0; r < n; ++r)
                    if (flag[r] == RAYS_REG) { rays_test(o, d, rec[(size_t)r * 3], rec[(size_t)r * 3 + 2], gid0 + r, best); ++tests; }
        }
        if (best != KEY_EMPTY) atomicMin(&key[i], best);
    }
    rays_tally(tally, probes, tests);
}

static __global__ __launch_bounds__(256) void k_rays_wide(const float4 *__restrict__ rays, uint32_t n_rays, const float4 *__restrict__ rec, uint32_t gid0,
                                                          const uint32_t *__restrict__ wide, const RaysChunk *__restrict__ ck,
                                                          unsigned long long *__restrict__ key, RaysTally *__restrict__ tally)
{
    __shared__ float4 s_pc[RAYS_PIECE], s_nr[RAYS_PIECE];
    __shared__ uint32_t s_id[RAYS_PIECE];
    const uint32_t nw = ck->wide;                        // (the same for every lane of the launch)
    if (!nw) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    float4 o = make_float4(0, 0, 0, 0), d = o;
    bool go = i < n_rays;
    if (go) { o = rays[(size_t)i * 2]; d = rays[(size_t)i * 2 + 1]; go = rays_valid(o, d); }
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
            for (uint32_t j = 0; j < m; ++j) rays_test(o, d, s_pc[j], s_nr[j], s_id[j], best);
            tests += m;
        }
    }
    if (best != KEY_EMPTY) atomicMin(&key[i], best);
    rays_tally(tally, 0u, tests);
}

// A later chunk that wins a ray overwrites it.  The planes start as zeros: the empty values.  Any plane may be null.
static __global__ void k_rays_resolve(const float4 *__restrict__ rec, uint32_t gid0, uint32_t n, const unsigned long long *__restrict__ key, uint32_t n_rays,
                                      uint8_t *__restrict__ rgb, uint8_t *__restrict__ sem, float *__restrict__ nrm)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_rays) return;
    const unsigned long long kk = key[q];
    if (kk == KEY_EMPTY) return;
    const uint32_t row = (uint32_t)(kk & 0xFFFFFFFFull) - gid0;                                // wraps below the base
    if (row >= n) return;
    const uint32_t sc = __float_as_uint(rec[(size_t)row * 3 + 1].x);
    if (rgb) { rgb[(size_t)q * 3] = (uint8_t)((sc >> 16) & 0xFFu); rgb[(size_t)q * 3 + 1] = (uint8_t)((sc >> 8) & 0xFFu); rgb[(size_t)q * 3 + 2] = (uint8_t)(sc & 0xFFu); }
    if (sem) sem[q] = (uint8_t)(((sc >> 24) & 0xFFu) + 1u);
    if (nrm) { const float4 nr = rec[(size_t)row * 3 + 2]; nrm[(size_t)q * 3] = nr.x; nrm[(size_t)q * 3 + 1] = nr.y; nrm[(size_t)q * 3 + 2] = nr.z; }
}

// ... and the invalid rays are counted, by the rule the casts used (all 64 lanes of a wave reach the ballot)
static __global__ __launch_bounds__(256) void k_rays_finish(const float4 *__restrict__ rays, const unsigned long long *__restrict__ key, uint32_t n_rays,
                                                            float *__restrict__ t, int32_t *__restrict__ ids, RaysTally *__restrict__ tally)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    bool bad = false;
    if (q < n_rays) {
        const unsigned long long kk = key[q];
        t[q] = kk == KEY_EMPTY ? 0.0f : __uint_as_float((uint32_t)(kk >> 32));
        ids[q] = kk == KEY_EMPTY ? -1 : (int32_t)(uint32_t)(kk & 0xFFFFFFFFull);
        bad = !rays_valid(rays[(size_t)q * 2], rays[(size_t)q * 2 + 1]);
    }
    const unsigned long long m = __ballot(bad);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(&tally->bad, (unsigned long long)__popcll(m));
}

}  // namespace sm
