// sm_k_warp.h -- the map warped by surfel time (DESIGN.md "4h. Closing loops"; sm_c_api.h "sm_warp_by_time").  Included by
// sm_warp.hip only.  Three kernels, the first two streaming and bound by HBM:
//   k_warp_model   one lane per slot of the live model's SoA planes, gated by the alive bit: 4 B of time in for every slot; for a
//                  selected one 16 B pos_conf + 16 B norm_rad + its 48-byte table row in, two 16-byte stores out.  One ballot
//                  and one atomic per wave count the selected.
//   k_warp_rows    a chunk of 48-byte AoS records in the staging buffer, 256 per workgroup, through LDS as k_recall_mark reads
//                  them (consecutive lanes on consecutive addresses both ways); a block without a selected row stores nothing.
//                  Per block: the box of the finite centres AFTER the warp and the largest non-NaN time.
//   k_warp_fold    one workgroup: the chunk's box, largest time and selected count for the host.
// The table stays in device memory: consecutive slots have near-equal times (the model is in creation order, map files in
// retirement order), so a wave's 64 gathers fall on a few 48-byte rows that the L2 serves.
#pragma once

#include "sm_device.h"
#include "sm_d_warp.h"                                   // warp_apply: the row rule itself

namespace sm {

constexpr int WARP_BLOCK = 256;                          // records per workgroup of k_warp_rows
constexpr int WARP_MAX_BLOCKS = 4096;                    // blocks of a full chunk (2^20 records)

struct WarpArgs {
    float t0;            // float(t0)
    float last;          // float(n - 1)
    uint32_t n;          // table rows
};

// the chunk's tally, read back by the host: selected rows, box of the finite centres after the warp (lo = +inf, hi = -inf: none),
// the largest non-NaN time (-inf: none)
struct WarpChunk { uint32_t selected, pad; float lx, ly, lz, hx, hy, hz, tmax, pad2; };

// the row rule's selection, in the header's order; k is valid only where the result is true
__device__ __forceinline__ bool warp_select(const WarpArgs &wa, float tau, uint32_t &k)
{
    const bool sel = tau >= wa.t0;                       // false on a NaN
    const float d = tau - wa.t0;
    k = sel ? (d >= wa.last ? wa.n - 1u : (uint32_t)d) : 0u;
    return sel;
}

__device__ __forceinline__ float warp_wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float warp_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// slots [0, st->count) of the current set; *moved += the selected live slots
__global__ __launch_bounds__(256) void k_warp_model(Model M, const DevState *__restrict__ st, const uint64_t *__restrict__ alive, WarpArgs wa,
                                                    const float4 *__restrict__ corr, uint32_t *__restrict__ moved)
{
    const uint32_t N = st->count;
    const SurfelSet cur = M.s[st->cur];
    const int lane = threadIdx.x & 63;
    for (uint64_t k0 = (uint64_t)blockIdx.x * 256u; k0 < N; k0 += (uint64_t)gridDim.x * 256u) {   // workgroup-uniform bound
        const uint32_t k = (uint32_t)k0 + threadIdx.x;
        const bool have = k < N;
        // slots a deferred-compaction cull has killed are no surfels: they keep their bytes
        const bool live = have && ((alive[k >> 6] >> (k & 63u)) & 1ull);
        const float tau = have ? cur.time[k] : 0.0f;
        uint32_t row;
        const bool sel = warp_select(wa, tau, row) && live;
        if (sel) {
            float4 pc = cur.pos_conf[k], nr = cur.norm_rad[k];
            const float4 c0 = corr[(size_t)row * 3], c1 = corr[(size_t)row * 3 + 1], c2 = corr[(size_t)row * 3 + 2];
            warp_apply(c0, c1, c2, pc, nr);
            cur.pos_conf[k] = pc;
            cur.norm_rad[k] = nr;
        }
        const uint64_t b = __ballot(sel);
        if (lane == 0 && b) atomicAdd(moved, (uint32_t)__popcll(b));
    }
}

// records [0, n) of the chunk at rec, in place; box[2 b], box[2 b + 1]: (min xyz | largest time) and (max xyz | 0) of block b;
// *selected += the chunk's selected rows
__global__ __launch_bounds__(256) void k_warp_rows(float4 *__restrict__ rec, uint32_t n, WarpArgs wa, const float4 *__restrict__ corr,
                                                   float4 *__restrict__ box, uint32_t *__restrict__ selected)
{
    __shared__ float4 s_rec[WARP_BLOCK * 3];             // 12 KiB
    __shared__ float s_red[4][7];
    __shared__ uint32_t s_cnt[4];
    const uint32_t first = blockIdx.x * (uint32_t)WARP_BLOCK;
    const uint32_t m = min((uint32_t)WARP_BLOCK, n - first);                // >= 1: the grid is ceil(n / 256)
    float4 *blk = rec + (size_t)first * 3;
    for (uint32_t i = threadIdx.x; i < m * 3u; i += 256u) s_rec[i] = blk[i];
    __syncthreads();
    const bool have = threadIdx.x < m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float4 pc = make_float4(0, 0, 0, 0), nr = pc;
    float tau = 0.0f;
    if (have) { pc = s_rec[threadIdx.x * 3]; tau = s_rec[threadIdx.x * 3 + 1].w; nr = s_rec[threadIdx.x * 3 + 2]; }
    uint32_t row;
    const bool sel = warp_select(wa, tau, row) && have;
    if (sel) {
        const float4 c0 = corr[(size_t)row * 3], c1 = corr[(size_t)row * 3 + 1], c2 = corr[(size_t)row * 3 + 2];
        warp_apply(c0, c1, c2, pc, nr);
        s_rec[threadIdx.x * 3] = pc;                     // its own record: nobody else reads or writes it
        s_rec[threadIdx.x * 3 + 2] = nr;
    }
    const uint64_t b = __ballot(sel);
    const uint32_t wcnt = (uint32_t)__popcll(b);
    if (lane == 0 && wcnt) atomicAdd(selected, wcnt);
    const float INF = __uint_as_float(0x7F800000u);
    // the box bounds the rows a recall can find near: those whose three coordinates are finite (x - x is 0 for a finite x only)
    const bool fin = have && (pc.x - pc.x == 0.0f) && (pc.y - pc.y == 0.0f) && (pc.z - pc.z == 0.0f);
    const float lx = warp_wave_min(fin ? pc.x : INF), ly = warp_wave_min(fin ? pc.y : INF), lz = warp_wave_min(fin ? pc.z : INF);
    const float hx = warp_wave_max(fin ? pc.x : -INF), hy = warp_wave_max(fin ? pc.y : -INF), hz = warp_wave_max(fin ? pc.z : -INF);
    const float tm = warp_wave_max(have && tau == tau ? tau : -INF);
    if (lane == 0) {
        s_cnt[wave] = wcnt;
        s_red[wave][0] = lx; s_red[wave][1] = ly; s_red[wave][2] = lz;
        s_red[wave][3] = hx; s_red[wave][4] = hy; s_red[wave][5] = hz; s_red[wave][6] = tm;
    }
    __syncthreads();                                     // (also: every selected record is back in LDS)
    if (threadIdx.x == 0) {
        float4 lo, hi;
        lo.x = fminf(fminf(s_red[0][0], s_red[1][0]), fminf(s_red[2][0], s_red[3][0]));
        lo.y = fminf(fminf(s_red[0][1], s_red[1][1]), fminf(s_red[2][1], s_red[3][1]));
        lo.z = fminf(fminf(s_red[0][2], s_red[1][2]), fminf(s_red[2][2], s_red[3][2]));
        lo.w = fmaxf(fmaxf(s_red[0][6], s_red[1][6]), fmaxf(s_red[2][6], s_red[3][6]));
        hi.x = fmaxf(fmaxf(s_red[0][3], s_red[1][3]), fmaxf(s_red[2][3], s_red[3][3]));
        hi.y = fmaxf(fmaxf(s_red[0][4], s_red[1][4]), fmaxf(s_red[2][4], s_red[3][4]));
        hi.z = fmaxf(fmaxf(s_red[0][5], s_red[1][5]), fmaxf(s_red[2][5], s_red[3][5]));
        hi.w = 0.0f;
        box[2 * (size_t)blockIdx.x] = lo;
        box[2 * (size_t)blockIdx.x + 1] = hi;
    }
    if ((s_cnt[0] | s_cnt[1] | s_cnt[2] | s_cnt[3]) == 0u) return;          // workgroup-uniform: nothing moved, nothing to store
    for (uint32_t i = threadIdx.x; i < m * 3u; i += 256u) blk[i] = s_rec[i];
}

// the chunk's tally from its nblk blocks (at most 4096: four rounds of 1024 threads)
__global__ __launch_bounds__(1024) void k_warp_fold(uint32_t nblk, const float4 *__restrict__ box, const uint32_t *__restrict__ selected,
                                                    WarpChunk *__restrict__ out)
{
    __shared__ float s_red[16][7];
    const float INF = __uint_as_float(0x7F800000u);
    float lx = INF, ly = INF, lz = INF, hx = -INF, hy = -INF, hz = -INF, tm = -INF;
    for (uint32_t b = threadIdx.x; b < nblk; b += 1024u) {
        const float4 lo = box[2 * (size_t)b], hi = box[2 * (size_t)b + 1];
        lx = fminf(lx, lo.x); ly = fminf(ly, lo.y); lz = fminf(lz, lo.z); tm = fmaxf(tm, lo.w);
        hx = fmaxf(hx, hi.x); hy = fmaxf(hy, hi.y); hz = fmaxf(hz, hi.z);
    }
    lx = warp_wave_min(lx); ly = warp_wave_min(ly); lz = warp_wave_min(lz);
    hx = warp_wave_max(hx); hy = warp_wave_max(hy); hz = warp_wave_max(hz); tm = warp_wave_max(tm);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = lx; s_red[wave][1] = ly; s_red[wave][2] = lz;
        s_red[wave][3] = hx; s_red[wave][4] = hy; s_red[wave][5] = hz; s_red[wave][6] = tm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            lx = fminf(lx, s_red[w][0]); ly = fminf(ly, s_red[w][1]); lz = fminf(lz, s_red[w][2]);
            hx = fmaxf(hx, s_red[w][3]); hy = fmaxf(hy, s_red[w][4]); hz = fmaxf(hz, s_red[w][5]); tm = fmaxf(tm, s_red[w][6]);
        }
        *out = WarpChunk{*selected, 0u, lx, ly, lz, hx, hy, hz, tm, 0.0f};
    }
}

}  // namespace sm
