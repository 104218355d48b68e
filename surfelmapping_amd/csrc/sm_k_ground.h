// sm_k_ground.h -- a map set as a planner's ground map (DESIGN.md "4v. Ground map"; the specification is sm_c_api.h's "ground map").
// Included by sm_ground.hip only.  The regular-record test, the quantised normal, the weight and the run logic of neighbouring lanes
// are sm_d_simplify.h's.  Records come as 48-byte AoS rows (three float4), a chunk of a map file or the exported model.  Planes are
// row-major over the window: cell (u, v) at v * nu + u.
//   k_ground_min       reading 1: Z[cell] = min H over the cell's ground-like records.  The lanes of a run of equal cells in a wave
//                      go together: a segmented shuffle minimum, then the run's first lane issues one atomicMin
//   k_ground_fill      one lane per cell, 16 x 16 cells a workgroup: Z of the tile and a halo of fill_cells in LDS; a cell without
//                      ground scans the (2 fill_cells + 1)^2 window in (v', u') order and keeps the strictly nearest: R
//   k_ground_accum     reading 2: a record's kind and contribution (SW, SH, SC[3], best; n_obst, top), summed over the run of equal
//                      cells in the wave, then integer atomics without return value by the run's first lane; the counts by kind go
//                      to the tally, one add per wave and kind
//   k_ground_finish    per cell: ground, bgr, cls from the sums
//   k_ground_state     per cell: the state from n_obst, ground and the 4 neighbours' ground; the cells by state to the tally
//   k_ground_columns   one lane per column: the 1-D distance to the nearest blocking cell of the column, capped at reach_cells,
//                      by a sweep down and a sweep up
//   k_ground_rows      256 cells of a row a workgroup: the columns' distances of the cells and of reach_cells to either side in
//                      LDS; clear2 = min(reach^2, min over |du| <= reach of du^2 + g(u + du)^2), the scan outwards ended once du^2
//                      cannot improve.  Exact: a blocking cell nearer than reach_cells has |du| and |dv| below it, and a capped
//                      g adds reach^2 or more
// No lane waits for another; every loop has a fixed bound.  Integer atomics only.  Every index is checked against the window before
// it is used.
#pragma once

#include "sm_d_simplify.h"

namespace sm {

constexpr int GROUND_NO_Z = 0x7F7F7F7F;                  // Z and R of a cell without (a memset's bytes; above every H: |H| < 2^30)
constexpr int GROUND_NONE = (int)0x80000000;             // SM_GROUND_NONE
enum { GROUND_K_GROUND = 0, GROUND_K_OBSTACLE, GROUND_K_IGNORED, GROUND_K_UNREFERENCED, GROUND_K_OUTSIDE, GROUND_K_LOOSE, GROUND_KINDS };
enum { GROUND_UNKNOWN = 0, GROUND_FREE, GROUND_OBSTACLE, GROUND_STEP, GROUND_STATES };
// the tally's words: the records by kind, the cells by state
enum { GROUND_COUNTS = 0, GROUND_CELLS = GROUND_KINDS, GROUND_TALLY_WORDS = 16 };
constexpr int GROUND_TILE = 16, GROUND_MAX_FILL = 16, GROUND_TILE_W = GROUND_TILE + 2 * GROUND_MAX_FILL;
constexpr int GROUND_MAX_REACH = 255;

struct GroundArgs {
    long long C;                       // the cell edge in 2^-16 m
    int B, L, Hi, S;                   // band, body band, step, in 2^-16 m
    float origin[3];
    int a, ua, va, sgn;                // the up axis, the horizontal ones, +1 / -1
    int nsgn;                          // sgn * normal_sign: what a ground-like normal's up-component is multiplied with
    int nu, nv;
    int min_up;
    uint32_t ground_mask[8];
    uint32_t min_obstacle;
    int fill, reach, unknown_blocks, step_on;
    int combine;                       // 0: SM_GROUND_NO_COMBINE=1
};

// The accumulators of reading 2, one entry a cell each.
struct GroundSums {
    unsigned long long *SW, *SH, *SC;  // 0; SC: channel ch at [ch * N + cell]
    unsigned long long *best;          // 0
    uint32_t *n_obst;                  // 0
    int *top;                          // 0
};
constexpr size_t GROUND_ZERO_BYTES = 8 * 6 + 4 + 4;

struct GroundContrib {
    unsigned long long sw, sh, sc[3], best;
    uint32_t n_obst;
    int top;
};

__device__ __forceinline__ long long ground_pick(int k, long long x0, long long x1, long long x2) { return k == 0 ? x0 : k == 1 ? x1 : x2; }

// Where a record lies.  GROUND_K_LOOSE, GROUND_K_OUTSIDE, or GROUND_KINDS: in the window, in `cell` at height H, ground-like or not
__device__ __forceinline__ int ground_place(const GroundArgs &g, const float4 &pc, const float4 &ct, const float4 &nr, uint32_t &cell, int &H, bool &like)
{
    if (!simp_fields_ok(pc, ct, nr)) return GROUND_K_LOOSE;
    const double d0 = (double)pc.x - (double)g.origin[0], d1 = (double)pc.y - (double)g.origin[1], d2 = (double)pc.z - (double)g.origin[2];
    if (!(fabs(d0) < 16777216.0) || !(fabs(d1) < 16777216.0) || !(fabs(d2) < 16777216.0)) return GROUND_K_LOOSE;
    const long long X0 = (long long)floor(d0 * 65536.0), X1 = (long long)floor(d1 * 65536.0), X2 = (long long)floor(d2 * 65536.0);
    const long long Xu = ground_pick(g.ua, X0, X1, X2), Xv = ground_pick(g.va, X0, X1, X2);
    long long cu = Xu / g.C, cv = Xv / g.C;
    if (Xu - cu * g.C < 0) --cu;                         // floor division
    if (Xv - cv * g.C < 0) --cv;
    const long long Hl = (long long)g.sgn * ground_pick(g.a, X0, X1, X2);
    if (cu < 0 || cu >= g.nu || cv < 0 || cv >= g.nv || Hl >= (1ll << 30) || Hl <= -(1ll << 30)) return GROUND_K_OUTSIDE;
    cell = (uint32_t)(cv * g.nu + cu);
    H = (int)Hl;
    const uint32_t c = __float_as_uint(ct.x) >> 24;
    uint32_t word = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) word = (c >> 5) == i ? g.ground_mask[i] : word;
    const float n = g.a == 0 ? nr.x : g.a == 1 ? nr.y : nr.z;
    const int ni = (int)fminf(fmaxf(floorf(n * 16384.0f + 0.5f), -4194304.0f), 4194304.0f);
    like = ((word >> (c & 31u)) & 1u) && g.nsgn * ni >= g.min_up;
    return GROUND_KINDS;
}

// the run logic of sm_d_simplify.h with this call's switch
__device__ __forceinline__ bool ground_head(const GroundArgs &g, uint32_t cell, bool reg)
{
    SimplifyArgs a{};
    a.combine = g.combine;
    return simp_head(a, reg ? (unsigned long long)cell : SIMP_EMPTY, reg);
}

// ---- reading 1
__global__ __launch_bounds__(256) void k_ground_min(const float4 *__restrict__ rec, uint32_t n, GroundArgs g, int *__restrict__ Z)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t cell = 0;
    int H = 0x7FFFFFFF;
    bool reg = false;
    if (t < n) {
        bool like = false;
        reg = ground_place(g, rec[(size_t)t * 3], rec[(size_t)t * 3 + 1], rec[(size_t)t * 3 + 2], cell, H, like) == GROUND_KINDS && like;
    }
    const bool head = ground_head(g, cell, reg);
    if (__ballot(reg && !head)) {                        // wave-uniform: some run in this wave is longer than one lane
        const int last = simp_run_last(reg, head);
        for (int o = 1; o < 64; o <<= 1) {
            const bool take = lane + o <= last;
            if (!__ballot(take)) break;
            const int v = __shfl_down(H, o);
            if (take) H = min(H, v);
        }
    }
    if (head) atomicMin(&Z[cell], H);
}

// ---- the reference heights
__global__ __launch_bounds__(256) void k_ground_fill(GroundArgs g, const int *__restrict__ Z, int *__restrict__ R)
{
    __shared__ int s_z[GROUND_TILE_W * GROUND_TILE_W];
    const int F = g.fill, W = GROUND_TILE + 2 * F;
    const int u0 = (int)blockIdx.x * GROUND_TILE, v0 = (int)blockIdx.y * GROUND_TILE;
    for (int i = threadIdx.x; i < W * W; i += 256) {
        const int u = u0 - F + i % W, v = v0 - F + i / W;
        s_z[i] = (u >= 0 && u < g.nu && v >= 0 && v < g.nv) ? Z[(size_t)v * g.nu + u] : GROUND_NO_Z;
    }
    __syncthreads();
    const int lu = threadIdx.x & (GROUND_TILE - 1), lv = threadIdx.x / GROUND_TILE;
    const int u = u0 + lu, v = v0 + lv;
    if (u >= g.nu || v >= g.nv) return;
    int z = s_z[(lv + F) * W + lu + F];
    if (z == GROUND_NO_Z) {
        int best = 0x7FFFFFFF;
        for (int dv = -F; dv <= F; ++dv)                 // ascending (v', u'): of equally near cells the first stays
            for (int du = -F; du <= F; ++du) {
                const int zz = s_z[(lv + F + dv) * W + lu + F + du], d2 = du * du + dv * dv;
                if (zz != GROUND_NO_Z && d2 < best) { best = d2; z = zz; }
            }
    }
    R[(size_t)v * g.nu + u] = z;
}

// ---- reading 2
__device__ __forceinline__ void ground_take(GroundContrib &c, int o, bool take)
{
#define GROUND_ADD(x) { const auto v_ = __shfl_down(x, o); if (take) x += v_; }
#define GROUND_MAX(x) { const auto v_ = __shfl_down(x, o); if (take) x = max(x, v_); }
    GROUND_ADD(c.sw) GROUND_ADD(c.sh) GROUND_ADD(c.sc[0]) GROUND_ADD(c.sc[1]) GROUND_ADD(c.sc[2]) GROUND_MAX(c.best)
    GROUND_ADD(c.n_obst) GROUND_MAX(c.top)
#undef GROUND_ADD
#undef GROUND_MAX
}

__global__ __launch_bounds__(256) void k_ground_accum(const float4 *__restrict__ rec, uint32_t n, uint32_t gid0, GroundArgs g, const int *__restrict__ R,
                                                      GroundSums P, uint32_t *__restrict__ tally)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const size_t N = (size_t)g.nu * g.nv;
    int kind = GROUND_KINDS;                             // (no record)
    uint32_t cell = 0;
    GroundContrib c{};
    if (t < n) {
        const float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1];
        int H = 0;
        bool like = false;
        kind = ground_place(g, pc, ct, rec[(size_t)t * 3 + 2], cell, H, like);
        if (kind == GROUND_KINDS) {
            const int r = R[cell];
            const long long d = (long long)H - r;
            if (r == GROUND_NO_Z) kind = GROUND_K_UNREFERENCED;
            else if (like && d >= 0 && d <= g.B) {       // (a ground-like record's cell has ground: R is its Z)
                kind = GROUND_K_GROUND;
                const float tw = pc.w * 16.0f;
                const uint32_t w = tw >= 255.0f ? 255u : (uint32_t)max(1, (int)tw), col = __float_as_uint(ct.x);
                c.sw = w;
                c.sh = (unsigned long long)w * (unsigned long long)d;
#pragma unroll
                for (int k = 0; k < 3; ++k) c.sc[k] = (unsigned long long)w * ((col >> (8 * k)) & 255u);
                c.best = (unsigned long long)w << 40 | (unsigned long long)(0x7FFFFFFFu - (gid0 + t)) << 8 | (col >> 24);
            } else if (d > g.L && d < g.Hi) {
                kind = GROUND_K_OBSTACLE;
                c.n_obst = 1u;
                c.top = (int)d;
            } else kind = GROUND_K_IGNORED;
        }
    }
    const bool reg = kind == GROUND_K_GROUND || kind == GROUND_K_OBSTACLE;
    const bool head = ground_head(g, cell, reg);
    if (__ballot(reg && !head)) {                        // wave-uniform
        const int last = simp_run_last(reg, head);
        for (int o = 1; o < 64; o <<= 1) {
            const bool take = lane + o <= last;
            if (!__ballot(take)) break;
            ground_take(c, o, take);
        }
    }
    if (head) {
        if (c.sw) {
            atomicAdd(&P.SW[cell], c.sw);
            atomicAdd(&P.SH[cell], c.sh);
#pragma unroll
            for (int k = 0; k < 3; ++k) atomicAdd(&P.SC[k * N + cell], c.sc[k]);
            atomicMax(&P.best[cell], c.best);
        }
        if (c.n_obst) {
            atomicAdd(&P.n_obst[cell], c.n_obst);
            atomicMax(&P.top[cell], c.top);
        }
    }
#pragma unroll
    for (int l = 0; l < GROUND_KINDS; ++l) {
        const unsigned long long b = __ballot(kind == l);
        if (b && lane == 0) atomicAdd(&tally[GROUND_COUNTS + l], (uint32_t)__popcll(b));
    }
}

// ---- the planes
__global__ __launch_bounds__(256) void k_ground_finish(GroundArgs g, const int *__restrict__ Z, GroundSums P, int *__restrict__ ground,
                                                       uint8_t *__restrict__ cls, uint8_t *__restrict__ bgr)
{
    const size_t N = (size_t)g.nu * g.nv, i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const int z = Z[i];
    const unsigned long long sw = P.SW[i];
    if (z == GROUND_NO_Z || sw == 0ull) {                // (a cell with ground has its lowest record in the band: sw >= 1)
        ground[i] = z == GROUND_NO_Z ? GROUND_NONE : z;
        cls[i] = 255;
        bgr[i * 3] = bgr[i * 3 + 1] = bgr[i * 3 + 2] = 0;
        return;
    }
    ground[i] = z + (int)((P.SH[i] + sw / 2) / sw);
    cls[i] = (uint8_t)(P.best[i] & 255ull);
#pragma unroll
    for (int k = 0; k < 3; ++k) bgr[i * 3 + k] = (uint8_t)((P.SC[k * N + i] + sw / 2) / sw);
}

__global__ __launch_bounds__(256) void k_ground_state(GroundArgs g, const int *__restrict__ ground, const uint32_t *__restrict__ n_obst,
                                                      uint8_t *__restrict__ state, uint32_t *__restrict__ tally)
{
    const size_t N = (size_t)g.nu * g.nv, i = (size_t)blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int st = GROUND_STATES;                              // (no cell)
    if (i < N) {
        const int u = (int)(i % (size_t)g.nu), v = (int)(i / (size_t)g.nu);
        const int gr = ground[i];
        if (n_obst[i] >= g.min_obstacle) st = GROUND_OBSTACLE;
        else if (gr == GROUND_NONE) st = GROUND_UNKNOWN;
        else {
            bool step = false;
            if (g.step_on) {
                const auto differs = [&](size_t j) {
                    const int o = ground[j];
                    const long long e = (long long)gr - o;
                    return o != GROUND_NONE && (e < 0 ? -e : e) > g.S;
                };
                step = (u > 0 && differs(i - 1)) || (u + 1 < g.nu && differs(i + 1)) || (v > 0 && differs(i - g.nu)) || (v + 1 < g.nv && differs(i + g.nu));
            }
            st = step ? GROUND_STEP : GROUND_FREE;
        }
        state[i] = (uint8_t)st;
    }
#pragma unroll
    for (int l = 0; l < GROUND_STATES; ++l) {
        const unsigned long long b = __ballot(st == l);
        if (b && lane == 0) atomicAdd(&tally[GROUND_CELLS + l], (uint32_t)__popcll(b));
    }
}

// ---- the capped Euclidean distance transform
__device__ __forceinline__ bool ground_blocks(const GroundArgs &g, uint8_t st)
{
    return st == GROUND_OBSTACLE || st == GROUND_STEP || (st == GROUND_UNKNOWN && g.unknown_blocks);
}

__global__ __launch_bounds__(256) void k_ground_columns(GroundArgs g, const uint8_t *__restrict__ state, uint8_t *__restrict__ gcol)
{
    const int u = (int)(blockIdx.x * 256u + threadIdx.x);
    if (u >= g.nu) return;
    int d = g.reach;
    for (int v = 0; v < g.nv; ++v) {
        const size_t i = (size_t)v * g.nu + u;
        d = ground_blocks(g, state[i]) ? 0 : min(d + 1, g.reach);
        gcol[i] = (uint8_t)d;
    }
    d = g.reach;
    for (int v = g.nv - 1; v >= 0; --v) {
        const size_t i = (size_t)v * g.nu + u;
        d = ground_blocks(g, state[i]) ? 0 : min(d + 1, g.reach);
        if (d < (int)gcol[i]) gcol[i] = (uint8_t)d;
    }
}

__global__ __launch_bounds__(256) void k_ground_rows(GroundArgs g, const uint8_t *__restrict__ gcol, uint32_t *__restrict__ clear2)
{
    __shared__ uint8_t s_g[256 + 2 * GROUND_MAX_REACH];
    const int u0 = (int)blockIdx.x * 256, v = (int)blockIdx.y, reach = g.reach;
    for (int i = threadIdx.x; i < 256 + 2 * reach; i += 256) {
        const int u = u0 - reach + i;
        s_g[i] = (u >= 0 && u < g.nu) ? gcol[(size_t)v * g.nu + u] : (uint8_t)reach;       // (cells outside the window do not block)
    }
    __syncthreads();
    const int u = u0 + (int)threadIdx.x;
    if (u >= g.nu) return;
    const int c = (int)threadIdx.x + reach;
    int best = reach * reach;
    for (int du = 0; du <= reach && du * du < best; ++du) {
        const int m = min((int)s_g[c - du], (int)s_g[c + du]);
        best = min(best, du * du + m * m);
    }
    clear2[(size_t)v * g.nu + u] = (uint32_t)best;
}

}  // namespace sm
