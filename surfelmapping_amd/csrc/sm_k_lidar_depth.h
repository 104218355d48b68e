// sm_k_lidar_depth.h -- kernels of the lidar depth stage (DESIGN.md "4z. Lidar depth"; the rules: include/sm_c_api.h "lidar
// depth", restated by tests/lidar_depth_ref.py): a scan z-buffered into the camera, then completed to a dense depth image by a
// fixed chain of morphological steps on v = 65536 - mm (0 = empty; a u16).  Four launches:
//
//   k_ld_project   one lane per point: the projection in fp32 and the 64-bit atomicMin of (mm << 32 | i) into the key plane; the
//                  first W lanes reset the columns' topmost words
//   k_ld_chain     per 32 x 32 tile with a 9-pixel halo: keys -> v in LDS, DILATE, CLOSE (row and column pass each) and
//                  FILL_SMALL between two LDS planes; writes sparse_mm, index, the v plane and each column's topmost filled row
//   k_ld_rowmax    FILL_LARGE's row pass over the v plane with EXTEND_TOP applied on load (launched only with FILL_LARGE)
//   k_ld_finish    per 32 x 32 tile with a 4-pixel halo: EXTEND_TOP on load, FILL_LARGE's column pass for the empty pixels,
//                  MEDIAN and SMOOTH from LDS; writes depth_mm and puts the tile's keys back to empty for the next call
//
// Every pixel of every plane has one writer; the only atomics are the splat and the columns' topmost words.  Tallies are per
// block, summed on the host (as the fill stage's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sm_device.h"

namespace sm {

constexpr int LD_TILE = 32;                         // pixels per tile side of k_ld_chain and k_ld_finish
constexpr int LD_THREADS = 1024;                    // ... and their block: a lane per pixel of the tile, so that the 468 tiles of a KITTI
                                                    // image put 16 waves each on a CU (blocks of 256: 28.0 and 49.5 us; of 1024: 20.2 and 35.9 us)
constexpr int LD_HALO = 9;                          // DILATE 2 + CLOSE 2 + 2 + FILL_SMALL 3
constexpr int LD_S = LD_TILE + 2 * LD_HALO;         // side of k_ld_chain's LDS planes
constexpr int LD_FH = 4;                            // MEDIAN 2 + SMOOTH 2
constexpr int LD_FS = LD_TILE + 2 * LD_FH;          // side of k_ld_finish's LDS planes
constexpr int LD_MAX_R = 15;                        // FILL_LARGE's largest radius
constexpr int LD_ROW = 256;                         // pixels of a row per block of k_ld_rowmax
constexpr uint32_t LD_TOP_NONE = 0xFFFFFFFFu;       // a column's topmost word (row << 16 | v) with no filled pixel
enum { LD_DILATE = 1, LD_CLOSE = 2, LD_FILL_SMALL = 4, LD_EXTEND_TOP = 8, LD_FILL_LARGE = 16, LD_MEDIAN = 32, LD_SMOOTH = 64 };

struct LdProjectArgs {
    const float4 *points;
    uint32_t n;
    float T[12];
    float fx, fy, cx, cy, min_z, max_z;
    int W, H;
    uint64_t *key;
    uint32_t *top;                 // [W]
    uint32_t *part;                // per block: the points that reached the splat
};

struct LdArgs {
    uint64_t *key;                 // W * H, KEY_EMPTY where no point landed
    uint16_t *v, *rowmax;          // W * H each: after FILL_SMALL; the row pass of FILL_LARGE
    uint32_t *top;                 // [W]: row << 16 | v of the topmost filled pixel after FILL_SMALL
    uint16_t *depth, *sparse;      // outputs, any may be null
    int32_t *index;
    uint2 *part_chain;             // per tile: (measured, filled by FILL_SMALL)
    uint4 *part_finish;            // per tile: (filled by EXTEND_TOP, by FILL_LARGE, left empty, 0)
    int W, H, tiles_x;
    int stages, R, tol;            // R = large / 2
};

__global__ __launch_bounds__(256) void k_ld_project(const LdProjectArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < (uint32_t)a.W) a.top[i] = LD_TOP_NONE;
    bool landed = false;
    if (i < a.n) {
        const float4 p = a.points[i];
        const float X = ((a.T[0] * p.x + a.T[1] * p.y) + a.T[2] * p.z) + a.T[3];
        const float Y = ((a.T[4] * p.x + a.T[5] * p.y) + a.T[6] * p.z) + a.T[7];
        const float Z = ((a.T[8] * p.x + a.T[9] * p.y) + a.T[10] * p.z) + a.T[11];
        if (isfinite(X) && isfinite(Y) && isfinite(Z) && Z >= a.min_z && Z <= a.max_z) {
            const float u = (a.fx * X) / Z + a.cx, v = (a.fy * Y) / Z + a.cy;
            if (isfinite(u) && isfinite(v) && u >= -0.5f && u < (float)a.W - 0.5f && v >= -0.5f && v < (float)a.H - 0.5f) {
                const int px = (int)floorf(u + 0.5f), py = (int)floorf(v + 0.5f);
                const int mm = (int)floorf(Z * 1000.0f + 0.5f);
                if (mm >= 1 && mm <= 65535 && px >= 0 && py >= 0 && px < a.W && py < a.H) {
                    atomicMin((unsigned long long *)&a.key[(size_t)py * a.W + px], ((unsigned long long)mm << 32) | i);
                    landed = true;
                }
            }
        }
    }
    __shared__ uint32_t cnt[4];
    const unsigned long long b = __ballot(landed);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) a.part[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// the sum of a per-thread count over the block's LD_THREADS threads
__device__ __forceinline__ uint32_t ld_block_sum(uint32_t c, uint32_t *red)
{
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    __syncthreads();                                     // (red may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < LD_THREADS / 64; ++w) sum += red[w];
    return sum;
}

// Planes of LD_S x LD_S around the tile; a pixel outside the image holds 0 after every step, which a maximum ignores, and the
// minimum of CLOSE looks at coordinates.  `r` is the halo still valid: each step computes the positions within its new r.
__global__ __launch_bounds__(LD_THREADS) void k_ld_chain(const LdArgs a)
{
    __shared__ uint16_t A[LD_S * LD_S], B[LD_S * LD_S];
    __shared__ uint32_t red[LD_THREADS / 64];
    __shared__ uint32_t coltop[LD_TILE];
    const int tid = threadIdx.x;
    const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), ty = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const int x0 = tx * LD_TILE - LD_HALO, y0 = ty * LD_TILE - LD_HALO;
    const int W = a.W, H = a.H;
    uint32_t measured = 0, filled = 0;

    for (int q = tid; q < LD_S * LD_S; q += LD_THREADS) {
        const int lx = q % LD_S, ly = q / LD_S, x = x0 + lx, y = y0 + ly;
        uint16_t v = 0;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t g = (size_t)y * W + x;
            const uint64_t k = a.key[g];
            const uint32_t mm = k == KEY_EMPTY ? 0u : (uint32_t)(k >> 32);
            v = mm ? (uint16_t)(65536u - mm) : (uint16_t)0;
            if (lx >= LD_HALO && lx < LD_HALO + LD_TILE && ly >= LD_HALO && ly < LD_HALO + LD_TILE) {
                if (a.sparse) a.sparse[g] = (uint16_t)mm;
                if (a.index) a.index[g] = (int32_t)(uint32_t)k;      // (KEY_EMPTY's low word is -1)
                measured += mm != 0;
            }
        }
        A[q] = v;
    }
    if (tid < LD_TILE) coltop[tid] = LD_TOP_NONE;
    __syncthreads();
    int r = LD_HALO;

    // in: x within r, y within r2 of the tile
    auto inside = [&](int q, int rx, int ry) {
        const int lx = q % LD_S, ly = q / LD_S;
        return lx >= LD_HALO - rx && lx < LD_HALO + LD_TILE + rx && ly >= LD_HALO - ry && ly < LD_HALO + LD_TILE + ry;
    };
    auto in_image = [&](int q) {
        const int x = x0 + q % LD_S, y = y0 + q / LD_S;
        return x >= 0 && x < W && y >= 0 && y < H;
    };

    if (a.stages & LD_DILATE) {
        r -= 2;
        for (int q = tid; q < LD_S * LD_S; q += LD_THREADS) {
            if (!inside(q, r, r)) continue;
            uint16_t m = 0;
            if (in_image(q)) {
                m = max(max(A[q - 2 * LD_S], A[q + 2 * LD_S]), max(A[q - 2], A[q + 2]));
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) m = max(m, A[q + dy * LD_S + dx]);
            }
            B[q] = m;
        }
        __syncthreads();
        for (int q = tid; q < LD_S * LD_S; q += LD_THREADS)
            if (inside(q, r, r)) A[q] = B[q];
        __syncthreads();
    }
    if (a.stages & LD_CLOSE) {
        // maximum: rows A -> B, columns B -> A
        for (int q = tid; q < LD_S * LD_S; q += LD_THREADS) {
            if (!inside(q, r - 2, r)) continue;
            uint16_t m = A[q];
#pragma unroll
            for (int d = 1; d <= 2; ++d) m = max(m, max(A[q - d], A[q + d]));
            B[q] = m;
        }
        __syncthreads();
        r -= 2;
        for (int q = tid; q < LD_S * LD_S; q += LD_THREADS) {
            if (!inside(q, r, r)) continue;
            uint16_t m = 0;
            if (in_image(q)) {
                m = B[q];
#pragma unroll
                for (int d = 1; d <= 2; ++d) m = max(m, max(B[q - d * LD_S], B[q + d * LD_S]));
            }
            A[q] = m;
        }
        __syncthreads();
        // minimum over the taps inside the image: rows A -> B, columns B -> A
        for (int q = tid; q < LD_S * LD_S; q += LD_THREADS) {
            if (!inside(q, r - 2, r)) continue;
            const int x = x0 + q % LD_S;
            uint16_t m = A[q];
#pragma unroll
            for (int d = -2; d <= 2; ++d)
                if (d != 0 && x + d >= 0 && x + d < W) m = min(m, A[q + d]);
            B[q] = m;
        }
        __syncthreads();
        r -= 2;
        for (int q = tid; q < LD_S * LD_S; q += LD_THREADS) {
            if (!inside(q, r, r)) continue;
            const int y = y0 + q / LD_S;
            uint16_t m = 0;
            if (in_image(q)) {
                m = B[q];
#pragma unroll
                for (int d = -2; d <= 2; ++d)
                    if (d != 0 && y + d >= 0 && y + d < H) m = min(m, B[q + d * LD_S]);
            }
            A[q] = m;
        }
        __syncthreads();
    }
    if (a.stages & LD_FILL_SMALL) {
        // r is at least 3 here (9 less what DILATE and CLOSE took); the tile itself is all that is left to compute
        for (int q = tid; q < LD_S * LD_S; q += LD_THREADS) {
            if (!inside(q, 0, 3)) continue;
            uint16_t m = A[q];
#pragma unroll
            for (int d = 1; d <= 3; ++d) m = max(m, max(A[q - d], A[q + d]));
            B[q] = m;
        }
        __syncthreads();
        for (int q = tid; q < LD_S * LD_S; q += LD_THREADS) {
            if (!inside(q, 0, 0) || !in_image(q) || A[q] != 0) continue;
            uint16_t m = B[q];
#pragma unroll
            for (int d = 1; d <= 3; ++d) m = max(m, max(B[q - d * LD_S], B[q + d * LD_S]));
            A[q] = m;                                    // (only this thread reads or writes A[q] in this loop)
            filled += m != 0;
        }
        __syncthreads();
    }

    // the tile of the v plane, and the topmost filled row of each of its columns
    for (int q = tid; q < LD_TILE * LD_TILE; q += LD_THREADS) {
        const int lx = q % LD_TILE, ly = q / LD_TILE, x = x0 + LD_HALO + lx, y = y0 + LD_HALO + ly;
        if (x >= W || y >= H) continue;
        const uint16_t v = A[(ly + LD_HALO) * LD_S + lx + LD_HALO];
        a.v[(size_t)y * W + x] = v;
        if (v) atomicMin(&coltop[lx], ((uint32_t)y << 16) | v);
    }
    __syncthreads();
    if (tid < LD_TILE && coltop[tid] != LD_TOP_NONE) atomicMin(&a.top[x0 + LD_HALO + tid], coltop[tid]);
    const uint32_t m = ld_block_sum(measured, red), f = ld_block_sum(filled, red);
    if (tid == 0) a.part_chain[blockIdx.x] = make_uint2(m, f);
}

// v after EXTEND_TOP at (x, y) of the image
__device__ __forceinline__ uint16_t ld_load_top(const LdArgs &a, int x, int y)
{
    const uint16_t v = a.v[(size_t)y * a.W + x];
    if (!(a.stages & LD_EXTEND_TOP)) return v;
    const uint32_t t = a.top[x];
    return (t != LD_TOP_NONE && (uint32_t)y < (t >> 16)) ? (uint16_t)(t & 0xFFFFu) : v;
}

// grid (ceil(W / LD_ROW), H)
__global__ __launch_bounds__(LD_ROW) void k_ld_rowmax(const LdArgs a)
{
    __shared__ uint16_t row[LD_ROW + 2 * LD_MAX_R];
    const int y = (int)blockIdx.y, xb = (int)blockIdx.x * LD_ROW - a.R;
    for (int q = threadIdx.x; q < LD_ROW + 2 * a.R; q += LD_ROW) {
        const int x = xb + q;
        row[q] = (x >= 0 && x < a.W) ? ld_load_top(a, x, y) : (uint16_t)0;
    }
    __syncthreads();
    const int x = (int)blockIdx.x * LD_ROW + (int)threadIdx.x;
    if (x >= a.W) return;
    uint16_t m = 0;
    for (int d = 0; d <= 2 * a.R; ++d) m = max(m, row[threadIdx.x + d]);
    a.rowmax[(size_t)y * a.W + x] = m;
}

// element k (ascending, 0-based) of the values of t[25] that are not 0: the least x with more than k of them at or below it, by
// bisection between the least and the greatest of them -- a handful of steps where the window is one surface, 16 across an edge
__device__ __forceinline__ uint32_t ld_select(const uint32_t (&t)[25], uint32_t k)
{
    uint32_t lo = 0xFFFFu, hi = 0u, tm[25];
#pragma unroll
    for (int j = 0; j < 25; ++j) {
        tm[j] = t[j] - 1u;                               // (0 becomes the greatest word: below no x)
        if (t[j]) { lo = min(lo, t[j]); hi = max(hi, t[j]); }
    }
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        uint32_t at_or_below = 0;
#pragma unroll
        for (int j = 0; j < 25; ++j) at_or_below += tm[j] < mid;
        if (at_or_below > k) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

__global__ __launch_bounds__(LD_THREADS) void k_ld_finish(const LdArgs a)
{
    __shared__ uint16_t A[LD_FS * LD_FS], B[LD_FS * LD_FS];
    __shared__ uint16_t RM[(LD_FS + 2 * LD_MAX_R) * LD_FS];      // the row maxima: LD_FS columns, the rows of the planes and R more each way
    __shared__ uint32_t red[LD_THREADS / 64];
    const int tid = threadIdx.x;
    const int tx = (int)(blockIdx.x % (unsigned)a.tiles_x), ty = (int)(blockIdx.x / (unsigned)a.tiles_x);
    const int x0 = tx * LD_TILE - LD_FH, y0 = ty * LD_TILE - LD_FH;
    const int W = a.W, H = a.H, R = a.R;
    uint32_t f_top = 0, f_large = 0, empty = 0;
    auto tile = [](int lx, int ly) { return lx >= LD_FH && lx < LD_FH + LD_TILE && ly >= LD_FH && ly < LD_FH + LD_TILE; };

    if (a.stages & LD_FILL_LARGE)
        for (int q = tid; q < (LD_FS + 2 * R) * LD_FS; q += LD_THREADS) {
            const int x = x0 + q % LD_FS, y = y0 - R + q / LD_FS;
            RM[q] = (x >= 0 && x < W && y >= 0 && y < H) ? a.rowmax[(size_t)y * W + x] : (uint16_t)0;
        }
    for (int q = tid; q < LD_FS * LD_FS; q += LD_THREADS) {
        const int lx = q % LD_FS, ly = q / LD_FS, x = x0 + lx, y = y0 + ly;
        uint16_t v = 0;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            v = ld_load_top(a, x, y);
            if (tile(lx, ly)) {
                f_top += v != 0 && a.v[(size_t)y * W + x] == 0;
                a.key[(size_t)y * W + x] = KEY_EMPTY;               // clean for the next call: nothing reads the keys after k_ld_chain
            }
        }
        A[q] = v;
    }
    __syncthreads();
    if (a.stages & LD_FILL_LARGE) {
        for (int q = tid; q < LD_FS * LD_FS; q += LD_THREADS) {
            const int lx = q % LD_FS, ly = q / LD_FS, x = x0 + lx, y = y0 + ly;
            if (A[q] != 0 || x < 0 || x >= W || y < 0 || y >= H) continue;
            uint16_t m = 0;
            for (int d = 0; d <= 2 * R; ++d) m = max(m, RM[(ly + d) * LD_FS + lx]);
            A[q] = m;                                    // (RM is what the loop reads; A[q] has this one thread)
            f_large += m != 0 && tile(lx, ly);
        }
        __syncthreads();
    }
    if (a.stages & LD_MEDIAN) {
        for (int q = tid; q < LD_FS * LD_FS; q += LD_THREADS) {
            const int lx = q % LD_FS, ly = q / LD_FS;
            if (lx < 2 || lx >= LD_FS - 2 || ly < 2 || ly >= LD_FS - 2) continue;
            uint16_t out = 0;
            if (A[q] != 0) {
                uint32_t t[25], n = 0;
#pragma unroll
                for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
                    for (int dx = -2; dx <= 2; ++dx) {
                        const uint32_t v = A[q + dy * LD_FS + dx];
                        t[(dy + 2) * 5 + dx + 2] = v;
                        n += v != 0;
                    }
                out = (uint16_t)ld_select(t, (n - 1) / 2);
            }
            B[q] = out;
        }
        __syncthreads();
    }
    const uint16_t *src = (a.stages & LD_MEDIAN) ? B : A;
    for (int q = tid; q < LD_TILE * LD_TILE; q += LD_THREADS) {
        const int lx = q % LD_TILE + LD_FH, ly = q / LD_TILE + LD_FH, x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int c = ly * LD_FS + lx;
        uint32_t v = src[c];
        if (v != 0 && (a.stages & LD_SMOOTH)) {
            // sum of w * v at most 256 * 65535: 32 bits hold what the rule writes in 64
            const uint32_t z0 = 65536u - v, tol = 256u + (uint32_t)a.tol;
            uint32_t num = 0, den = 0;
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const uint32_t t = src[c + dy * LD_FS + dx], z = 65536u - t;
                    const uint32_t w = (uint32_t)((dy == 0 ? 6 : (dy == 1 || dy == -1) ? 4 : 1) * (dx == 0 ? 6 : (dx == 1 || dx == -1) ? 4 : 1));
                    if (t != 0 && max(z, z0) * 256u <= min(z, z0) * tol) { num += w * t; den += w; }
                }
            v = (num + den / 2) / den;
        }
        empty += v == 0;
        if (a.depth) a.depth[(size_t)y * W + x] = v ? (uint16_t)(65536u - v) : (uint16_t)0;
    }
    const uint32_t s0 = ld_block_sum(f_top, red), s1 = ld_block_sum(f_large, red), s2 = ld_block_sum(empty, red);
    if (tid == 0) a.part_finish[blockIdx.x] = make_uint4(s0, s1, s2, 0u);
}

// ---- every step as a launch of its own (SM_LIDAR_DEPTH_UNFUSED=1: what tools/lidar_depth_probe.py holds the four launches above
// against; same rules, same results).  One thread per pixel, every window read from global memory, the planes ping-pong.  The
// tallies are eight words the host clears: measured, FILL_SMALL, EXTEND_TOP, FILL_LARGE, left empty.
enum { LDU_DILATE, LDU_MAX5, LDU_MIN5, LDU_FILL7, LDU_ROWMAX, LDU_COLMAX, LDU_MEDIAN, LDU_SMOOTH, LDU_OUT };
enum { LDU_T_MEASURED, LDU_T_SMALL, LDU_T_TOP, LDU_T_LARGE, LDU_T_EMPTY };

// one atomic per wave for the lanes whose `ev` is set
__device__ __forceinline__ void ld_wave_tally(bool ev, uint32_t *addr)
{
    const unsigned long long b = __ballot(ev), act = __ballot(true);
    if (b && (int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(addr, (uint32_t)__popcll(b));
}

__global__ __launch_bounds__(256) void k_ld_u_init(const LdArgs a, uint16_t *__restrict__ out, uint32_t *tally)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)a.W * a.H) return;
    const uint64_t k = a.key[q];
    const uint32_t mm = k == KEY_EMPTY ? 0u : (uint32_t)(k >> 32);
    out[q] = mm ? (uint16_t)(65536u - mm) : (uint16_t)0;
    if (a.sparse) a.sparse[q] = (uint16_t)mm;
    if (a.index) a.index[q] = (int32_t)(uint32_t)k;
    ld_wave_tally(mm != 0, &tally[LDU_T_MEASURED]);
}

// a block of 64 x 16 threads per 64 columns: each thread finds the topmost filled pixel of its sixteenth of the rows, the
// column's is their minimum, and each thread writes its rows
__global__ __launch_bounds__(1024) void k_ld_u_top(const LdArgs a, const uint16_t *__restrict__ in, uint16_t *__restrict__ out, uint32_t *tally)
{
    __shared__ uint32_t top[64];
    const int x = (int)(blockIdx.x * 64 + threadIdx.x), per = (a.H + 15) / 16;
    const int ya = (int)threadIdx.y * per, yb = min(a.H, ya + per);
    if (threadIdx.y == 0) top[threadIdx.x] = LD_TOP_NONE;
    __syncthreads();
    if (x < a.W)
        for (int y = ya; y < yb; ++y) {
            const uint16_t v = in[(size_t)y * a.W + x];
            if (v) { atomicMin(&top[threadIdx.x], ((uint32_t)y << 16) | v); break; }
        }
    __syncthreads();
    if (x >= a.W) return;
    const uint32_t t = top[threadIdx.x];
    for (int y = ya; y < yb; ++y) {
        const size_t g = (size_t)y * a.W + x;
        out[g] = (t != LD_TOP_NONE && (uint32_t)y < (t >> 16)) ? (uint16_t)(t & 0xFFFFu) : in[g];
    }
    if (threadIdx.y == 0 && t != LD_TOP_NONE && (t >> 16) > 0) atomicAdd(&tally[LDU_T_TOP], t >> 16);
}

template <int S>
__global__ __launch_bounds__(256) void k_ld_u_step(const LdArgs a, const uint16_t *__restrict__ in, uint16_t *__restrict__ out, uint32_t *tally)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int W = a.W, H = a.H;
    if (q >= (size_t)W * H) return;
    const int x = (int)(q % (unsigned)W), y = (int)(q / (unsigned)W);
    const uint32_t c = in[q];
    // the tap at (x + dx, y + dy), or -1 outside the image
    auto at = [&](const uint16_t *p, int dx, int dy) {
        const int xx = x + dx, yy = y + dy;
        return (xx < 0 || xx >= W || yy < 0 || yy >= H) ? -1 : (int)p[(size_t)yy * W + xx];
    };
    auto boxmax = [&](int r) {
        int m = 0;
        for (int dy = -r; dy <= r; ++dy)
            for (int dx = -r; dx <= r; ++dx) m = max(m, at(in, dx, dy));
        return (uint32_t)m;
    };
    uint32_t v = c;
    if (S == LDU_DILATE) {
        int m = 0;
        for (int dy = -2; dy <= 2; ++dy)
            for (int dx = -2; dx <= 2; ++dx)
                if (abs(dx) + abs(dy) <= 2) m = max(m, at(in, dx, dy));
        v = (uint32_t)m;
    } else if (S == LDU_MAX5) {
        v = boxmax(2);
    } else if (S == LDU_MIN5) {
        for (int dy = -2; dy <= 2; ++dy)
            for (int dx = -2; dx <= 2; ++dx) {
                const int t = at(in, dx, dy);
                if (t >= 0) v = min(v, (uint32_t)t);
            }
    } else if (S == LDU_FILL7) {
        if (c == 0) v = boxmax(3);
        ld_wave_tally(c == 0 && v != 0, &tally[LDU_T_SMALL]);
    } else if (S == LDU_ROWMAX) {
        int m = 0;
        for (int dx = -a.R; dx <= a.R; ++dx) m = max(m, at(in, dx, 0));
        v = (uint32_t)m;
    } else if (S == LDU_COLMAX) {
        if (c == 0) {
            int m = 0;
            for (int dy = -a.R; dy <= a.R; ++dy) m = max(m, at(a.rowmax, 0, dy));
            v = (uint32_t)m;
        }
        ld_wave_tally(c == 0 && v != 0, &tally[LDU_T_LARGE]);
    } else if (S == LDU_MEDIAN) {
        if (c != 0) {
            uint32_t t[25], n = 0;
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const int w = at(in, dx, dy);
                    t[(dy + 2) * 5 + dx + 2] = w > 0 ? (uint32_t)w : 0u;
                    n += w > 0;
                }
            v = ld_select(t, (n - 1) / 2);
        }
    } else if (S == LDU_SMOOTH) {
        if (c != 0) {
            const uint32_t z0 = 65536u - c, tol = 256u + (uint32_t)a.tol;
            uint32_t num = 0, den = 0;
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const int t = at(in, dx, dy);
                    const uint32_t z = 65536u - (uint32_t)max(t, 0);
                    const uint32_t w = (uint32_t)((dy == 0 ? 6 : (dy == 1 || dy == -1) ? 4 : 1) * (dx == 0 ? 6 : (dx == 1 || dx == -1) ? 4 : 1));
                    if (t > 0 && max(z, z0) * 256u <= min(z, z0) * tol) { num += w * (uint32_t)t; den += w; }
                }
            v = (num + den / 2) / den;
        }
    } else {                                             // LDU_OUT: `out` is not used
        if (a.depth) a.depth[q] = c ? (uint16_t)(65536u - c) : (uint16_t)0;
        a.key[q] = KEY_EMPTY;
        ld_wave_tally(c == 0, &tally[LDU_T_EMPTY]);
        return;
    }
    out[q] = (uint16_t)v;
}

}  // namespace sm
