// sm_k_fill.h -- kernels of the hole filling of novel views (DESIGN.md "4n. Hole filling"; the rules: include/sm_c_api.h "hole
// filling", restated in integers by tests/fill_ref.py): the depth of a novel view from its keys, and the depth-aware push-pull
// completion of a batch of (bgr, sem, depth_mm) images in place.  Every launch covers all images of the batch (blockIdx.y, and
// a loop beyond 65535 images); every cell of every level has one writer, so there is no atomic anywhere.
//
//   k_fill_key_depth   depth_mm of every key of a batch (the render path's own kernel, ahead of the stage)
//   k_fill_pull        per 32 x 32 tile of level 0: step 0 (see-through) with a one-pixel halo through LDS, the level-0 validity
//                      plane, the pull of levels 1..5 in LDS (tile-aligned: no halo), the tile's tally
//   k_fill_pull_top    levels 6..8, per 8 x 8 tile of level-5 cells (launched only when levels > 5)
//   k_fill_push<L0>    one level down: the coarse tile plus a one-cell halo through LDS; <true> writes bgr, sem and depth_mm in
//                      their final layout and the tile's tally
//
// A cell record is a uint2: x = b | g << 8 | r << 16 | label << 24; y = z (17 bits: 0..65536) | valid << 17 | may-fill << 18.
// The count of observed level-0 pixels under a cell lives beside z in LDS while a kernel pulls (bits 19..: at most 1024 at
// level 5) and, between the two pull launches, in one word per level-5 cell (cnt5).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sm_device.h"

namespace sm {

constexpr int FILL_TILE = 32;                      // level-0 pixels per tile side (k_fill_pull), cells of the fine level (k_fill_push)
constexpr int FILL_HALO = FILL_TILE + 2;
constexpr int FILL_MAX_LEVELS = 8;
constexpr int FILL_LDS_LEVELS = 5;                 // what one 32 x 32 tile pulls on its own: 32 -> 1
constexpr int FILL_TOP_TILE = 8;                   // level-5 cells per tile side of k_fill_pull_top: 8 -> 1 is levels 6..8
constexpr uint32_t FILL_FAR = 65536u;              // the depth of a valid pixel whose depth_mm is 0
constexpr uint32_t FILL_Z_MASK = 0x1FFFFu, FILL_VALID = 1u << 17, FILL_MAY = 1u << 18;
constexpr int FILL_CNT_SHIFT = 19;
constexpr uint32_t FILL_NONE = 0xFFFFFFFFu;        // step 0's LDS plane: no valid input pixel here

struct FillArgs {
    uint8_t *bgr, *sem;            // n images of w x h, in place
    uint16_t *depth;               // ... or null: every valid pixel has depth 0, none is written
    uint8_t *v0;                   // n * w * h: valid after step 0
    uint2 *rec[FILL_MAX_LEVELS + 1];   // [l], l = 1..levels: n * lw[l] * lh[l] records
    uint32_t *cnt5;                // n * lw[5] * lh[5]: observed pixels under each level-5 cell (levels > 5)
    uint2 *part_pull, *part_push;  // per (image, tile): (valid, seen through), (filled, left empty)
    int w, h;
    uint32_t n;
    int lw[FILL_MAX_LEVELS + 1], lh[FILL_MAX_LEVELS + 1];
    int levels, tol, through, prefer_far, cover;
};

__device__ __forceinline__ uint16_t fill_depth_of_key(uint64_t key)
{
    const uint64_t zmm = ((key >> 32) * 200000ull + 8388607ull) / 16777215ull;
    return zmm <= 65535ull ? (uint16_t)zmm : (uint16_t)0;
}

__global__ void k_fill_key_depth(const uint64_t *__restrict__ key, size_t total, uint16_t *__restrict__ depth)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const uint64_t kk = key[q];
    depth[q] = kk == KEY_EMPTY ? (uint16_t)0 : fill_depth_of_key(kk);
}

// the pull's rule for one cell from its four children in the order dy outer, dx inner (a child outside the level is invalid);
// zw carries valid and z, cnt the observed pixels under each child.  Returns the record without its may-fill bit.
__device__ __forceinline__ uint2 fill_pull_cell(const uint32_t cl[4], const uint32_t zw[4], const uint32_t cnt[4], uint32_t tol,
                                                uint32_t &cnt_out)
{
    uint32_t zmin = FILL_NONE;
    cnt_out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cnt_out += cnt[k];
        if (zw[k] & FILL_VALID) zmin = min(zmin, zw[k] & FILL_Z_MASK);
    }
    if (zmin == FILL_NONE) return make_uint2(0u, 0u);
    uint32_t n = 0, sb = 0, sg = 0, sr = 0, sz = 0, label = 0;
    bool have = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t z = zw[k] & FILL_Z_MASK;
        if (!(zw[k] & FILL_VALID)) continue;
        if (!have && z == zmin) { label = cl[k] >> 24; have = true; }
        if (z * 256u <= zmin * (256u + tol)) {
            ++n;
            sb += cl[k] & 0xFFu; sg += (cl[k] >> 8) & 0xFFu; sr += (cl[k] >> 16) & 0xFFu;
            sz += z;
        }
    }
    const uint32_t hn = n >> 1;
    return make_uint2(((sb + hn) / n) | (((sg + hn) / n) << 8) | (((sr + hn) / n) << 16) | (label << 24), ((sz + hn) / n) | FILL_VALID);
}

// may a cell (X, Y) of level `shift` with cnt observed pixels fill: cnt * 256 >= area * min_cover_256, area in level-0 pixels
// inside the image
__device__ __forceinline__ bool fill_may(int X, int Y, int shift, int w, int h, uint32_t cnt, uint32_t cover)
{
    const long long x0 = (long long)X << shift, y0 = (long long)Y << shift;
    const uint32_t ax = (uint32_t)(min((long long)w, x0 + (1ll << shift)) - x0), ay = (uint32_t)(min((long long)h, y0 + (1ll << shift)) - y0);
    return cnt * 256u >= ax * ay * cover;
}

// (a, b) summed over a workgroup of 256 or 64 threads into thread 0 (red: one uint2 per wave)
__device__ __forceinline__ uint2 fill_block_sum(uint32_t a, uint32_t b, uint2 *red)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) { a += __shfl_down(a, o); b += __shfl_down(b, o); }
    const int wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = make_uint2(a, b);
    __syncthreads();
    uint2 t = make_uint2(0u, 0u);
    if (threadIdx.x == 0)
        for (int k = 0; k < waves; ++k) { t.x += red[k].x; t.y += red[k].y; }
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(256) void k_fill_pull(FillArgs a)
{
    __shared__ uint32_t s_in[FILL_HALO * FILL_HALO];
    __shared__ uint32_t s_cl[2][FILL_TILE * FILL_TILE];        // [1] holds at most 16 x 16
    __shared__ uint32_t s_zw[2][FILL_TILE * FILL_TILE];
    __shared__ uint2 s_red[4];
    const int tiles_x = (a.w + FILL_TILE - 1) / FILL_TILE;
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const int tid = (int)threadIdx.x;
    const size_t npix = (size_t)a.w * a.h;
    const uint32_t tol = (uint32_t)a.tol;
    const int top = min(a.levels, FILL_LDS_LEVELS);
    for (uint32_t img = blockIdx.y; img < a.n; img += gridDim.y) {
        const size_t base = (size_t)img * npix;
        // ---- the input's validity and depth, with a one-pixel halo
        for (int i = tid; i < FILL_HALO * FILL_HALO; i += 256) {
            const int x = tx * FILL_TILE + i % FILL_HALO - 1, y = ty * FILL_TILE + i / FILL_HALO - 1;
            uint32_t z = FILL_NONE;
            if (x >= 0 && x < a.w && y >= 0 && y < a.h) {
                const size_t q = base + (size_t)y * a.w + x;
                if (a.sem[q]) {
                    const uint32_t d = a.depth ? a.depth[q] : 0u;
                    z = d ? d : FILL_FAR;
                }
            }
            s_in[i] = z;
        }
        __syncthreads();
        // ---- step 0 and the level-0 records
        uint32_t n_valid = 0, n_through = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = tid + j * 256, px = k & (FILL_TILE - 1), py = k >> 5;
            const int x = tx * FILL_TILE + px, y = ty * FILL_TILE + py;
            const int c = (py + 1) * FILL_HALO + px + 1;
            const uint32_t z = s_in[c];
            bool valid = z != FILL_NONE;                      // (outside the image: FILL_NONE)
            if (valid) {
                ++n_valid;
                if (a.through > 0) {
                    int nearer = 0;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (!dx && !dy) continue;
                            const uint32_t zn = s_in[c + dy * FILL_HALO + dx];
                            nearer += (zn != FILL_NONE && zn * (256u + tol) < z * 256u) ? 1 : 0;
                        }
                    if (nearer >= a.through) { valid = false; ++n_through; }
                }
            }
            uint32_t cl = 0, zw = 0;
            if (x < a.w && y < a.h) {
                const size_t q = base + (size_t)y * a.w + x;
                a.v0[q] = valid ? 1 : 0;
                if (valid) {
                    cl = (uint32_t)a.bgr[q * 3] | ((uint32_t)a.bgr[q * 3 + 1] << 8) | ((uint32_t)a.bgr[q * 3 + 2] << 16) | ((uint32_t)a.sem[q] << 24);
                    zw = z | FILL_VALID | (1u << FILL_CNT_SHIFT);
                }
            }
            s_cl[0][k] = cl;
            s_zw[0][k] = zw;
        }
        const uint2 tally = fill_block_sum(n_valid, n_through, s_red);     // (its barriers publish level 0 too)
        if (tid == 0) a.part_pull[(size_t)img * gridDim.x + blockIdx.x] = tally;
        // ---- the pull, level l - 1 (side 2 * cs) to level l (side cs), ping-pong between the two LDS planes
        for (int l = 1; l <= top; ++l) {
            const int cs = FILL_TILE >> l, src = (l - 1) & 1, dst = l & 1;
            if (tid < cs * cs) {
                const int cx = tid % cs, cy = tid / cs;
                uint32_t cl[4], zw[4], cnt[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = (2 * cy + (k >> 1)) * (2 * cs) + 2 * cx + (k & 1);
                    cl[k] = s_cl[src][i];
                    zw[k] = s_zw[src][i];
                    cnt[k] = zw[k] >> FILL_CNT_SHIFT;
                }
                uint32_t cn;
                uint2 r = fill_pull_cell(cl, zw, cnt, tol, cn);
                const int X = tx * cs + cx, Y = ty * cs + cy;
                if (X < a.lw[l] && Y < a.lh[l]) {
                    if ((r.y & FILL_VALID) && fill_may(X, Y, l, a.w, a.h, cn, (uint32_t)a.cover)) r.y |= FILL_MAY;
                    a.rec[l][((size_t)img * a.lh[l] + Y) * a.lw[l] + X] = r;
                    if (l == FILL_LDS_LEVELS && a.levels > FILL_LDS_LEVELS) a.cnt5[((size_t)img * a.lh[l] + Y) * a.lw[l] + X] = cn;
                }
                s_cl[dst][tid] = r.x;
                s_zw[dst][tid] = r.y | (cn << FILL_CNT_SHIFT);
            }
            __syncthreads();
        }
        __syncthreads();                                       // (levels == 0: the next image's step 0 rewrites s_in and level 0)
    }
}

__global__ __launch_bounds__(64) void k_fill_pull_top(FillArgs a)
{
    __shared__ uint32_t s_cl[2][FILL_TOP_TILE * FILL_TOP_TILE];
    __shared__ uint32_t s_zw[2][FILL_TOP_TILE * FILL_TOP_TILE];
    __shared__ uint32_t s_cnt[2][FILL_TOP_TILE * FILL_TOP_TILE];
    const int L5 = FILL_LDS_LEVELS;
    const int tiles_x = (a.lw[L5] + FILL_TOP_TILE - 1) / FILL_TOP_TILE;
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const int tid = (int)threadIdx.x;
    for (uint32_t img = blockIdx.y; img < a.n; img += gridDim.y) {
        {
            const int X = tx * FILL_TOP_TILE + (tid & 7), Y = ty * FILL_TOP_TILE + (tid >> 3);
            uint2 r = make_uint2(0u, 0u);
            uint32_t cn = 0;
            if (X < a.lw[L5] && Y < a.lh[L5]) {
                const size_t i = ((size_t)img * a.lh[L5] + Y) * a.lw[L5] + X;
                r = a.rec[L5][i];
                cn = a.cnt5[i];
            }
            s_cl[0][tid] = r.x; s_zw[0][tid] = r.y; s_cnt[0][tid] = cn;
        }
        __syncthreads();
        for (int l = L5 + 1; l <= a.levels; ++l) {
            const int cs = FILL_TOP_TILE >> (l - L5), src = (l - L5 - 1) & 1, dst = (l - L5) & 1;
            if (tid < cs * cs) {
                const int cx = tid % cs, cy = tid / cs;
                uint32_t cl[4], zw[4], cnt[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = (2 * cy + (k >> 1)) * (2 * cs) + 2 * cx + (k & 1);
                    cl[k] = s_cl[src][i]; zw[k] = s_zw[src][i]; cnt[k] = s_cnt[src][i];
                }
                uint32_t cn;
                uint2 r = fill_pull_cell(cl, zw, cnt, (uint32_t)a.tol, cn);
                const int X = tx * cs + cx, Y = ty * cs + cy;
                if (X < a.lw[l] && Y < a.lh[l]) {
                    if ((r.y & FILL_VALID) && fill_may(X, Y, l, a.w, a.h, cn, (uint32_t)a.cover)) r.y |= FILL_MAY;
                    a.rec[l][((size_t)img * a.lh[l] + Y) * a.lw[l] + X] = r;
                }
                s_cl[dst][tid] = r.x; s_zw[dst][tid] = r.y; s_cnt[dst][tid] = cn;
            }
            __syncthreads();
        }
        __syncthreads();
    }
}

// Level l + 1 (complete) to level l: every cell of level l that is invalid takes its four taps.  L0: level l is the image; which
// of its pixels are invalid says v0, and the result goes into bgr, sem and depth_mm (zeros where no tap counts).  levels == 0:
// there is no coarse level and every invalid pixel becomes zeros.
template <bool L0>
__global__ __launch_bounds__(256) void k_fill_push(FillArgs a, int l)
{
    constexpr int CT = FILL_TILE / 2 + 2;                      // the coarse tile with its halo
    __shared__ uint2 s_c[CT * CT];
    __shared__ uint2 s_red[4];
    const int fw = L0 ? a.w : a.lw[l], fh = L0 ? a.h : a.lh[l];
    const bool coarse = a.levels > 0;
    const int cw = coarse ? a.lw[l + 1] : 0, ch = coarse ? a.lh[l + 1] : 0;
    const int tiles_x = (fw + FILL_TILE - 1) / FILL_TILE;
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const int tid = (int)threadIdx.x;
    const uint32_t tol = (uint32_t)a.tol;
    const size_t fpix = (size_t)fw * fh;
    for (uint32_t img = blockIdx.y; img < a.n; img += gridDim.y) {
        for (int i = tid; i < CT * CT; i += 256) {
            const int X = tx * (FILL_TILE / 2) + i % CT - 1, Y = ty * (FILL_TILE / 2) + i / CT - 1;
            uint2 r = make_uint2(0u, 0u);
            if (X >= 0 && X < cw && Y >= 0 && Y < ch) r = a.rec[l + 1][((size_t)img * ch + Y) * cw + X];
            s_c[i] = r;
        }
        __syncthreads();
        uint32_t n_filled = 0, n_empty = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = tid + j * 256, px = k & (FILL_TILE - 1), py = k >> 5;
            const int x = tx * FILL_TILE + px, y = ty * FILL_TILE + py;
            if (x >= fw || y >= fh) continue;
            const size_t q = (size_t)img * fpix + (size_t)y * fw + x;
            if (L0 ? a.v0[q] != 0 : (a.rec[l][q].y & FILL_VALID) != 0u) continue;
            // the taps in their order, weights 9, 3, 3, 1 (the tile's origin is even: px and x have one parity)
            const int lx = (px >> 1) + 1, ly = (py >> 1) + 1, nx = lx + ((px & 1) ? 1 : -1), ny = ly + ((py & 1) ? 1 : -1);
            const uint2 t[4] = {s_c[ly * CT + lx], s_c[ly * CT + nx], s_c[ny * CT + lx], s_c[ny * CT + nx]};
            const uint32_t wt[4] = {9u, 3u, 3u, 1u};
            const uint32_t both = FILL_VALID | FILL_MAY;
            uint32_t zmin = FILL_NONE, zmax = 0;
            bool any = false;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if ((t[i].y & both) == both) {
                    const uint32_t z = t[i].y & FILL_Z_MASK;
                    zmin = min(zmin, z); zmax = max(zmax, z);
                    any = true;
                }
            uint2 r = make_uint2(0u, 0u);
            if (any) {
                uint32_t Wt = 0, sb = 0, sg = 0, sr = 0, sz = 0, label = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if ((t[i].y & both) != both) continue;
                    const uint32_t z = t[i].y & FILL_Z_MASK;
                    if (a.prefer_far ? z * (256u + tol) >= zmax * 256u : z * 256u <= zmin * (256u + tol)) {
                        if (!Wt) label = t[i].x >> 24;           // the weights fall in tap order: the group's first tap has its greatest
                        Wt += wt[i];
                        sb += wt[i] * (t[i].x & 0xFFu); sg += wt[i] * ((t[i].x >> 8) & 0xFFu); sr += wt[i] * ((t[i].x >> 16) & 0xFFu);
                        sz += wt[i] * z;
                    }
                }
                const uint32_t hw = Wt >> 1;
                r = make_uint2(((sb + hw) / Wt) | (((sg + hw) / Wt) << 8) | (((sr + hw) / Wt) << 16) | (label << 24),
                               ((sz + hw) / Wt) | FILL_VALID | FILL_MAY);
            }
            if (L0) {
                n_filled += any ? 1u : 0u;
                n_empty += any ? 0u : 1u;
                a.bgr[q * 3] = (uint8_t)(r.x & 0xFFu); a.bgr[q * 3 + 1] = (uint8_t)((r.x >> 8) & 0xFFu); a.bgr[q * 3 + 2] = (uint8_t)((r.x >> 16) & 0xFFu);
                a.sem[q] = (uint8_t)(r.x >> 24);
                const uint32_t z = r.y & FILL_Z_MASK;
                if (a.depth) a.depth[q] = (any && z < FILL_FAR) ? (uint16_t)z : (uint16_t)0;
            } else if (any) {
                a.rec[l][q] = r;
            }
        }
        if (L0) {
            const uint2 tally = fill_block_sum(n_filled, n_empty, s_red);
            if (tid == 0) a.part_push[(size_t)img * gridDim.x + blockIdx.x] = tally;
        }
        __syncthreads();
    }
}

}  // namespace sm
