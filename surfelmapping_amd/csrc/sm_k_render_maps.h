// sm_k_render_maps.h -- views of a map set (DESIGN.md "4f. Views of a map set"): the renderers of sm_k_io.h / sm_k_view.h over
// chunks of map-file records instead of the resident model.  Included by sm_render_maps.hip only.
//   k_maps_intake        48-byte records -> chunk-local SoA planes (the layout of SurfelSet) + one box per 256 records
//   k_maps_splat_image   grid (blocks of the chunk, views of the batch): box test, then render_surfel per record
//   k_maps_splat_view    the same for the model view: view_surfel per record, large discs by the record's wave
//   k_maps_resolve_*     per pixel of the views the chunk touched: a key whose id lies in the chunk is shaded from its row
//   k_maps_finish_*      after the last source: pixels nobody won take the clear values
// Every per-surfel and per-pixel rule is sm_k_draw.h's, shared with the resident kernels: a record drawn here sets the key
// bits it would set as slot `id` of a model holding the whole set, and the keys are merged by the same atomicMin.
// The chunk's planes and the box layout are in sm_k_maps_box.h, shared with the lidar sweeps (sm_k_lidar.h); the per-block view
// tests are in sm_k_maps_cull.h, shared with the blended views (sm_k_blend.h).
#pragma once

#include "sm_device.h"
#include "sm_k_draw.h"
#include "sm_k_maps_box.h"
#include "sm_k_maps_cull.h"

namespace sm {

// ---------------------------------------------------------------------------------------------
// Chunk intake: k_retire_gather in reverse.  A workgroup's 256 records are 768 consecutive float4s: read by consecutive lanes,
// laid out in LDS as they lie in memory, then each lane takes its own record out of LDS (12 KiB) and writes one element of every
// plane -- consecutive lanes on consecutive addresses both ways, no lane walks memory with the record's 48-byte stride.
// The box in the same pass: wave reductions (shuffles), then LDS across the four waves.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float maps_wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float maps_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(256) void k_maps_intake(const float4 *__restrict__ rec, uint32_t n, MapsSoA out, float4 *__restrict__ box)
{
    __shared__ float4 s_rec[MAPS_BLOCK * 3];             // 12 KiB
    __shared__ float s_red[4][9];
    const uint32_t first = blockIdx.x * (uint32_t)MAPS_BLOCK;
    const uint32_t m = min((uint32_t)MAPS_BLOCK, n - first);                // records of this block (>= 1: the grid is ceil(n / 256))
    const float4 *src = rec + (size_t)first * 3;
    for (uint32_t i = threadIdx.x; i < m * 3u; i += 256u) s_rec[i] = src[i];
    __syncthreads();
    const bool have = threadIdx.x < m;
    float4 pc = make_float4(0, 0, 0, 0), ct = pc, nr = pc;
    if (have) {
        pc = s_rec[threadIdx.x * 3 + 0]; ct = s_rec[threadIdx.x * 3 + 1]; nr = s_rec[threadIdx.x * 3 + 2];
        const uint32_t k = first + threadIdx.x;
        out.pos_conf[k] = pc;
        out.norm_rad[k] = nr;
        out.color[k] = __float_as_uint(ct.x);
        out.time[k] = ct.w;
    }
    const float INF = __uint_as_float(0x7F800000u);
    const float ra = fabsf(nr.w);
    const float ln = sqrtf((nr.x * nr.x + nr.y * nr.y) + nr.z * nr.z);     // (+inf / NaN if the normal is, or its square overflows)
    const float rn = ra * fmaxf(1.0f, ln);                                  // (fmaxf skips a NaN: ln is tested itself)
    const bool bad = have && !((pc.x - pc.x == 0.0f) && (pc.y - pc.y == 0.0f) && (pc.z - pc.z == 0.0f) && (ln - ln == 0.0f) && (rn - rn == 0.0f));
    const float lx = maps_wave_min(have ? pc.x : INF), ly = maps_wave_min(have ? pc.y : INF), lz = maps_wave_min(have ? pc.z : INF);
    const float hx = maps_wave_max(have ? pc.x : -INF), hy = maps_wave_max(have ? pc.y : -INF), hz = maps_wave_max(have ? pc.z : -INF);
    const float rm = maps_wave_max(have ? ra : 0.0f), rnm = maps_wave_max(have ? rn : 0.0f);
    const bool wbad = __ballot(bad) != 0ull;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_red[wave][0] = lx; s_red[wave][1] = ly; s_red[wave][2] = lz; s_red[wave][3] = rm;
        s_red[wave][4] = hx; s_red[wave][5] = hy; s_red[wave][6] = hz; s_red[wave][7] = wbad ? 1.0f : 0.0f; s_red[wave][8] = rnm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float4 lo, hi;
        lo.x = fminf(fminf(s_red[0][0], s_red[1][0]), fminf(s_red[2][0], s_red[3][0]));
        lo.y = fminf(fminf(s_red[0][1], s_red[1][1]), fminf(s_red[2][1], s_red[3][1]));
        lo.z = fminf(fminf(s_red[0][2], s_red[1][2]), fminf(s_red[2][2], s_red[3][2]));
        lo.w = fmaxf(fmaxf(s_red[0][3], s_red[1][3]), fmaxf(s_red[2][3], s_red[3][3]));
        hi.x = fmaxf(fmaxf(s_red[0][4], s_red[1][4]), fmaxf(s_red[2][4], s_red[3][4]));
        hi.y = fmaxf(fmaxf(s_red[0][5], s_red[1][5]), fmaxf(s_red[2][5], s_red[3][5]));
        hi.z = fmaxf(fmaxf(s_red[0][6], s_red[1][6]), fmaxf(s_red[2][6], s_red[3][6]));
        const bool any = (s_red[0][7] + s_red[1][7]) + (s_red[2][7] + s_red[3][7]) != 0.0f;
        hi.w = any ? INF : fmaxf(fmaxf(s_red[0][8], s_red[1][8]), fmaxf(s_red[2][8], s_red[3][8]));
        box[2 * (size_t)blockIdx.x] = lo;
        box[2 * (size_t)blockIdx.x + 1] = hi;
    }
}

// ---------------------------------------------------------------------------------------------
// Batched splat: workgroup (b, v) draws block b of the chunk into view v's key plane, or leaves before loading a record.
// skipped[v]: workgroups that left (one atomic each, one address per view); hit[v] = 1: view v was drawn into by this chunk.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_maps_splat_image(MapsSoA c, uint32_t n, uint32_t id_base, const float4 *__restrict__ box,
                                                          const RenderParams *__restrict__ rps, uint64_t *__restrict__ key, size_t npix,
                                                          int cull, uint32_t *__restrict__ skipped, uint8_t *__restrict__ hit)
{
    const uint32_t v = blockIdx.y;
    const RenderParams rp = rps[v];
    if (cull && maps_box_outside_image(maps_box_load(box, blockIdx.x), rp)) {               // (workgroup-uniform)
        if (threadIdx.x == 0) atomicAdd(&skipped[v], 1u);
        return;
    }
    if (threadIdx.x == 0) hit[v] = 1;
    const uint32_t k = blockIdx.x * (uint32_t)MAPS_BLOCK + threadIdx.x;
    if (k < n) render_surfel(rp, c.pos_conf, c.norm_rad, k, id_base + k, key + (size_t)v * npix);
}

// k_view_splat's split: a disc of at most fp_lane pixels by its own lane; a larger one by its wave, lanes over pixels, as soon
// as the wave's small ones are done (no list: a (record, view) pair would need one per view).
__global__ __launch_bounds__(256) void k_maps_splat_view(MapsSoA c, uint32_t n, uint32_t id_base, const float4 *__restrict__ box,
                                                         const ViewParams *__restrict__ vps, uint64_t *__restrict__ key, size_t npix,
                                                         int cull, uint32_t *__restrict__ skipped, uint8_t *__restrict__ hit)
{
    const uint32_t v = blockIdx.y;
    const ViewParams vp = vps[v];
    if (cull && maps_box_outside_view(maps_box_load(box, blockIdx.x), vp)) {
        if (threadIdx.x == 0) atomicAdd(&skipped[v], 1u);
        return;
    }
    if (threadIdx.x == 0) hit[v] = 1;
    uint64_t *kv = key + (size_t)v * npix;
    const uint32_t k = blockIdx.x * (uint32_t)MAPS_BLOCK + threadIdx.x;
    const bool big = k < n && view_surfel(vp, c.pos_conf, c.norm_rad, k, id_base + k, kv);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t m = __ballot(big); m; m &= m - 1ull) {
        const uint32_t kb = (uint32_t)__shfl((int)k, __ffsll((unsigned long long)m) - 1);
        view_surfel_wide(vp, c.pos_conf, c.norm_rad, kb, id_base + kb, lane, 64u, kv);
    }
}

// ---------------------------------------------------------------------------------------------
// Chunk resolve, grid (pixel blocks, views): the pixels this source holds at the moment are shaded while its rows are on the
// device; a later source that wins the pixel overwrites them.  Views the source did not touch are left at once.
// ---------------------------------------------------------------------------------------------
__global__ void k_maps_resolve_image(MapsSoA c, uint32_t base, uint32_t n, const uint64_t *__restrict__ key, size_t npix,
                                     const uint8_t *__restrict__ hit, uint8_t *__restrict__ bgr, uint8_t *__restrict__ sem)
{
    const uint32_t v = blockIdx.y;
    if (!hit[v]) return;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const size_t q = (size_t)v * npix + p;
    const uint64_t kk = key[q];
    if (kk == KEY_EMPTY) return;
    const uint32_t row = (uint32_t)(kk & 0xFFFFFFFFull) - base;             // wraps below the base
    if (row >= n) return;
    uint8_t b, g, r, s;
    render_shade(c.color[row], b, g, r, s);
    bgr[q * 3] = b; bgr[q * 3 + 1] = g; bgr[q * 3 + 2] = r;
    sem[q] = s;
}

__global__ void k_maps_resolve_view(MapsSoA c, uint32_t base, uint32_t n, const ViewShade *__restrict__ vss, const uint64_t *__restrict__ key,
                                    size_t npix, const uint8_t *__restrict__ hit, uint32_t *__restrict__ rgba, float *__restrict__ depth,
                                    int32_t *__restrict__ ids)
{
    const uint32_t v = blockIdx.y;
    if (!hit[v]) return;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const size_t q = (size_t)v * npix + p;
    const uint64_t kk = key[q];
    if (kk == KEY_EMPTY) return;
    const uint32_t id = (uint32_t)(kk & 0xFFFFFFFFull), row = id - base;
    if (row >= n) return;
    rgba[q] = view_shade(vss[v], c.norm_rad, c.color, c.time, row);
    depth[q] = view_depth(kk);
    ids[q] = (int32_t)id;
}

__global__ void k_maps_finish_image(const uint64_t *__restrict__ key, size_t total, uint8_t *__restrict__ bgr, uint8_t *__restrict__ sem)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total || key[q] != KEY_EMPTY) return;
    bgr[q * 3] = 0; bgr[q * 3 + 1] = 0; bgr[q * 3 + 2] = 0;
    sem[q] = 0;
}

__global__ void k_maps_finish_view(const ViewShade *__restrict__ vss, const uint64_t *__restrict__ key, size_t npix,
                                   uint32_t *__restrict__ rgba, float *__restrict__ depth, int32_t *__restrict__ ids)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const size_t q = (size_t)blockIdx.y * npix + p;
    if (key[q] != KEY_EMPTY) return;
    rgba[q] = vss[blockIdx.y].clear;
    depth[q] = 1.0f;
    ids[q] = -1;
}

}  // namespace sm
