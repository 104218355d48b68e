// sm_k_stereo.h -- stereo depth (DESIGN.md "4m. Stereo depth").  Included by sm_stereo.hip only.
// The reference has no stereo matcher (its KittiReader's estimateDepth hands processFrame a null depth); the rules are those of
// include/sm_c_api.h, "stereo depth": semi-global matching over a 9 x 7 census transform, all integers up to the final division.
//
//   k_stereo_census    both images in one launch (blockIdx.z).  A workgroup takes a 32 x 8 tile: the luminance of the tile and its
//                      4 + 3 pixel halo (coordinates clamped to the image) goes into LDS once, then a lane compares its pixel
//                      with the 62 neighbours out of LDS.
//   k_stereo_cost      the u8 matching-cost volume, [y][x][d]: a lane makes four consecutive disparities of one pixel (one 32-bit
//                      store); the right codes it reads are consecutive along the row.
//   k_stereo_path<N>   one direction per launch, one wave per path, N = D / 64 consecutive disparities per lane.  A path is a 1-D
//                      recurrence: the previous step's L stays in registers, the minimum over d is a DPP wave reduction, the d-1 /
//                      d+1 terms of a lane's first and last disparity come from its neighbours by a one-lane shift.  Within a
//                      direction every pixel lies on exactly one path, so S is accumulated by plain read-modify-write; the first
//                      direction of a call stores instead of adding, which is what clears the volume.  The costs and sums of the
//                      next ST_CHUNK steps are fetched while the current ones are reduced.
//   k_stereo_select<N> one workgroup per image row.  Phase 1: the right view's winner of every column (a diagonal of the row's
//                      slab of the volume) into LDS.  Phase 2: the left view's winner, the validity tests, the sub-pixel step and
//                      the depth.  A wave takes one pixel at a time; argmin with ties to the lowest d is one minimum of S << 16 | d.

#pragma once

#include "sm_device.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sm {

constexpr int ST_TX = 32, ST_TY = 8;                     // the census tile
constexpr int ST_HX = 4, ST_HY = 3;                      // its halo: the window is 9 wide, 7 high
constexpr int ST_CHUNK = 4;                              // steps of a path fetched ahead as one batch
constexpr int ST_SELECT_THREADS = 512;
constexpr int ST_BIG = 1 << 20;                          // an absent term of the recurrence

struct StereoCensusArgs {
    const uint8_t *rgb[2];             // left, right: row-major H*W*3
    uint64_t *census[2];
    int W, H;
};

// grid: (ceil(W / 32), ceil(H / 8), 2), 256 threads
__global__ __launch_bounds__(256) void k_stereo_census(StereoCensusArgs A)
{
    constexpr int LW = ST_TX + 2 * ST_HX, LH = ST_TY + 2 * ST_HY;
    __shared__ uint8_t tile[LH][LW];
    const uint8_t *__restrict__ rgb = A.rgb[blockIdx.z];
    const int x0 = (int)blockIdx.x * ST_TX, y0 = (int)blockIdx.y * ST_TY;
    for (int i = (int)threadIdx.x; i < LW * LH; i += 256) {
        const int ly = i / LW, lx = i % LW;
        const int gx = min(max(x0 + lx - ST_HX, 0), A.W - 1), gy = min(max(y0 + ly - ST_HY, 0), A.H - 1);
        const uint8_t *q = rgb + ((size_t)gy * (size_t)A.W + (size_t)gx) * 3;
        tile[ly][lx] = (uint8_t)((77u * q[0] + 150u * q[1] + 29u * q[2] + 128u) >> 8);
    }
    __syncthreads();
    const int tx = (int)threadIdx.x % ST_TX, ty = (int)threadIdx.x / ST_TX;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= A.W || y >= A.H) return;
    const uint32_t c = tile[ty + ST_HY][tx + ST_HX];
    uint64_t code = 0;
#pragma unroll
    for (int dy = -ST_HY; dy <= ST_HY; ++dy)
#pragma unroll
        for (int dx = -ST_HX; dx <= ST_HX; ++dx) {
            if (dx == 0 && dy == 0) continue;
            code = (code << 1) | (uint64_t)(tile[ty + ST_HY + dy][tx + ST_HX + dx] < c ? 1u : 0u);
        }
    A.census[blockIdx.z][(size_t)y * (size_t)A.W + (size_t)x] = code;
}

struct StereoCostArgs {
    const uint64_t *cl, *cr;
    uint8_t *cost;                     // [y][x][d]
    int W, D;
    size_t n;                          // W * H * D / 4: one thread each
};

// grid: ceil(n / 256), 256 threads
__global__ __launch_bounds__(256) void k_stereo_cost(StereoCostArgs A)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t dq = (uint32_t)A.D / 4u;
    const size_t pix = i / dq;
    const int d0 = (int)(i % dq) * 4;
    const int x = (int)(pix % (size_t)A.W);
    const uint64_t cl = A.cl[pix];
    uint32_t w = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = d0 + k;
        const uint32_t c = x - d >= 0 ? (uint32_t)__popcll(cl ^ A.cr[pix - (size_t)d]) : 64u;
        w |= c << (8 * k);
    }
    *(uint32_t *)(A.cost + pix * (size_t)A.D + (size_t)d0) = w;
}

// the minimum of a value over the wave, in every lane (all 64 active): the DPP maximum of the complements
__device__ __forceinline__ uint32_t st_wave_min(uint32_t v) { return ~wave_max_u32(~v); }

// N consecutive costs (bytes, N of them in the word's low bytes) / sums (u16, in the halves of x then y) of a lane
template <int N>
__device__ __forceinline__ uint32_t st_load_cost(const uint8_t *__restrict__ p)
{
    if constexpr (N == 1) return p[0];
    else if constexpr (N == 2) return *(const uint16_t *)p;
    else if constexpr (N == 3) return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    else return *(const uint32_t *)p;
}
template <int N>
__device__ __forceinline__ uint2 st_load_sum(const uint16_t *__restrict__ p)
{
    if constexpr (N == 1) return make_uint2(p[0], 0u);
    else if constexpr (N == 2) return make_uint2(*(const uint32_t *)p, 0u);
    else if constexpr (N == 3) return make_uint2((uint32_t)p[0] | ((uint32_t)p[1] << 16), p[2]);
    else return *(const uint2 *)p;
}
template <int N>
__device__ __forceinline__ void st_store_sum(uint16_t *__restrict__ p, uint2 v)
{
    if constexpr (N == 1) p[0] = (uint16_t)v.x;
    else if constexpr (N == 2) *(uint32_t *)p = v.x;
    else if constexpr (N == 3) { p[0] = (uint16_t)v.x; p[1] = (uint16_t)(v.x >> 16); p[2] = (uint16_t)v.y; }
    else *(uint2 *)p = v;
}
__device__ __forceinline__ uint32_t st_half(uint2 v, int i) { return ((i < 2 ? v.x : v.y) >> (16 * (i & 1))) & 0xFFFFu; }

struct StereoPathArgs {
    const uint8_t *cost;               // [y][x][d]
    uint16_t *vol;                     // [y][x][d]
    int W, H, D;
    int dx, dy;                        // the direction
    int p1, p2;
    int first;                         // the call's first direction: S = L (no read); otherwise S += L
    int n_paths;                       // H (dy == 0), W (dx == 0), W + H - 1 (a diagonal)
};

// grid: n_paths workgroups of one wave
template <int N>
__global__ __launch_bounds__(64) void k_stereo_path(StereoPathArgs A)
{
    const int path = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (path >= A.n_paths) return;
    const int W = A.W, H = A.H, dx = A.dx, dy = A.dy;
    // the path's first pixel: the one whose predecessor lies outside the image
    int x0, y0;
    if (dy == 0) { x0 = dx > 0 ? 0 : W - 1; y0 = path; }
    else if (dx == 0) { x0 = path; y0 = dy > 0 ? 0 : H - 1; }
    else {
        const int ys = dy > 0 ? 0 : H - 1;
        if (path < W) { x0 = path; y0 = ys; }
        else { x0 = dx > 0 ? 0 : W - 1; y0 = ys + dy * (path - W + 1); }
    }
    const int nx = dx > 0 ? W - x0 : dx < 0 ? x0 + 1 : 0x7FFFFFFF;
    const int ny = dy > 0 ? H - y0 : dy < 0 ? y0 + 1 : 0x7FFFFFFF;
    const int len = min(nx, ny);
    const ptrdiff_t stride = ((ptrdiff_t)dy * W + dx) * (ptrdiff_t)A.D;
    const ptrdiff_t base = ((ptrdiff_t)y0 * W + x0) * (ptrdiff_t)A.D + (ptrdiff_t)(lane * N);
    const bool first = A.first != 0;

    uint32_t cur_c[ST_CHUNK], nxt_c[ST_CHUNK];
    uint2 cur_s[ST_CHUNK], nxt_s[ST_CHUNK];
#pragma unroll
    for (int j = 0; j < ST_CHUNK; ++j) {
        cur_c[j] = nxt_c[j] = 0u;
        cur_s[j] = nxt_s[j] = make_uint2(0u, 0u);
        if (j < len) {
            const ptrdiff_t off = base + (ptrdiff_t)j * stride;
            cur_c[j] = st_load_cost<N>(A.cost + off);
            if (!first) cur_s[j] = st_load_sum<N>(A.vol + off);
        }
    }
    int prev[N];
#pragma unroll
    for (int i = 0; i < N; ++i) prev[i] = 0;
    for (int s0 = 0; s0 < len; s0 += ST_CHUNK) {
#pragma unroll
        for (int j = 0; j < ST_CHUNK; ++j) {             // the next batch, in flight while this one is reduced
            const int s = s0 + ST_CHUNK + j;
            if (s < len) {
                const ptrdiff_t off = base + (ptrdiff_t)s * stride;
                nxt_c[j] = st_load_cost<N>(A.cost + off);
                if (!first) nxt_s[j] = st_load_sum<N>(A.vol + off);
            }
        }
#pragma unroll
        for (int j = 0; j < ST_CHUNK; ++j) {
            const int s = s0 + j;
            if (s >= len) break;                         // (the whole wave)
            int L[N];
            if (s == 0) {
#pragma unroll
                for (int i = 0; i < N; ++i) L[i] = (int)((cur_c[j] >> (8 * i)) & 0xFFu);
            } else {
                int mine = prev[0];
#pragma unroll
                for (int i = 1; i < N; ++i) mine = min(mine, prev[i]);
                const int m = (int)st_wave_min((uint32_t)mine);
                int below = __shfl_up(prev[N - 1], 1, 64), above = __shfl_down(prev[0], 1, 64);
                if (lane == 0) below = ST_BIG;
                if (lane == 63) above = ST_BIG;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const int a = i > 0 ? prev[i - 1] : below, b = i < N - 1 ? prev[i + 1] : above;
                    const int best = min(min(prev[i], min(a, b) + A.p1), m + A.p2);
                    L[i] = (int)((cur_c[j] >> (8 * i)) & 0xFFu) + best - m;
                }
            }
            uint2 out = make_uint2(0u, 0u);
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const uint32_t v = (uint32_t)L[i] + (first ? 0u : st_half(cur_s[j], i));
                if (i < 2) out.x |= v << (16 * i);
                else out.y |= v << (16 * (i - 2));
                prev[i] = L[i];
            }
            st_store_sum<N>(A.vol + base + (ptrdiff_t)s * stride, out);
        }
#pragma unroll
        for (int j = 0; j < ST_CHUNK; ++j) { cur_c[j] = nxt_c[j]; cur_s[j] = nxt_s[j]; }
    }
}

struct StereoSelectArgs {
    const uint16_t *vol;               // [y][x][d]
    uint16_t *depth, *disp;            // either may be null
    int W, D;
    int uniqueness, lr_max_diff;
    double K;                          // fx * baseline * 16000
};

// grid: H workgroups of ST_SELECT_THREADS, W bytes of dynamic LDS
template <int N>
__global__ __launch_bounds__(ST_SELECT_THREADS) void k_stereo_select(StereoSelectArgs A)
{
    extern __shared__ uint8_t d_right[];                 // per column of the right view: its winner
    constexpr int WAVES = ST_SELECT_THREADS / 64;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int W = A.W, D = A.D, y = (int)blockIdx.x;
    const uint16_t *__restrict__ row = A.vol + (size_t)y * (size_t)W * (size_t)D;
    for (int xr = wave; xr < W; xr += WAVES) {
        uint32_t key = 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int d = lane * N + i;
            if (xr + d < W) key = min(key, ((uint32_t)row[(size_t)(xr + d) * (size_t)D + (size_t)d] << 16) | (uint32_t)d);
        }
        key = st_wave_min(key);                          // (d = 0 always takes part)
        if (lane == 0) d_right[xr] = (uint8_t)(key & 0xFFFFu);
    }
    __syncthreads();
    for (int x = wave; x < W; x += WAVES) {
        const uint2 packed = st_load_sum<N>(row + (size_t)x * (size_t)D + (size_t)(lane * N));
        uint32_t s[N];
        uint32_t key = 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            s[i] = st_half(packed, i);
            key = min(key, (s[i] << 16) | (uint32_t)(lane * N + i));
        }
        key = st_wave_min(key);
        const int dstar = (int)(key & 0xFFFFu);
        const int smin = (int)(key >> 16);
        // the least S away from the winner and its two neighbours; the neighbours' own S (one lane holds each: a maximum finds it)
        uint32_t far = 0xFFFFFFFFu, below = 0u, above = 0u;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int d = lane * N + i;
            if (d < dstar - 1 || d > dstar + 1) far = min(far, s[i]);
            if (d == dstar - 1) below = s[i];
            if (d == dstar + 1) above = s[i];
        }
        far = st_wave_min(far);
        const int s_below = (int)wave_max_u32(below), s_above = (int)wave_max_u32(above);
        if (lane == 0) {
            const int xr = x - dstar;
            bool valid = dstar >= 1 && xr >= 0 && !((int)far * (100 - A.uniqueness) < smin * 100);
            if (valid) {
                const int diff = (int)d_right[xr] - dstar;
                valid = (diff < 0 ? -diff : diff) <= A.lr_max_diff;
            }
            uint32_t q = 0u;
            if (valid) {
                q = 16u * (uint32_t)dstar;
                if (dstar <= D - 2) {                    // (dstar >= 1: both neighbours exist)
                    const int a = s_below - smin, b = s_above - smin, den = a + b;
                    if (den > 0) q = (uint32_t)(16 * dstar - 8 + (32 * a + den) / (2 * den));
                }
            }
            const size_t pix = (size_t)y * (size_t)W + (size_t)x;
            if (A.disp) A.disp[pix] = (uint16_t)q;
            if (A.depth) {
                uint16_t mm = 0;
                if (q) {
                    const double v = floor(A.K / (double)q + 0.5);
                    if (!(v > 65535.0)) mm = (uint16_t)v;
                }
                A.depth[pix] = mm;
            }
        }
    }
}

}  // namespace sm
