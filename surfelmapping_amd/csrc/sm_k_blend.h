// sm_k_blend.h -- blended novel views (DESIGN.md "4o. Blended views"; the rules are in include/sm_c_api.h, "blended views"): over
// the finished key map of a view, every fragment of the visible layer adds its weight and its weighted colour to its pixel, and
// the pixel's colour is the rounded quotient.  Included by sm_blend.hip only.
//   k_blend_accum        the resident model: one lane per surfel, render_surfel with the accumulating action
//   k_maps_blend_accum   a chunk of map-file records, grid (blocks of the chunk, views of the batch), k_maps_splat_image's box test
//   k_blend_normalise    grid (pixel blocks, views): sums -> colour over the nearest colour already in `bgr`; counts
// The fragments are render_surfel's (sm_k_draw.h), walked with another action than the key pass's, so the two passes see the same
// (surfel, pixel) pairs, depths and q.  All sums are integer atomics: their order cannot change a bit of the result.
#pragma once

#include "sm_device.h"
#include "sm_k_draw.h"
#include "sm_k_maps_box.h"
#include "sm_k_maps_cull.h"

namespace sm {

typedef unsigned long long blend_u64;

constexpr int BLEND_TALLY_WORDS = 32;    // the tally ahead of the accumulators: contributions, drawn, changed (256 bytes)

// the weight of a fragment from the value the circle test compared (q in 0..1)
__device__ __forceinline__ uint32_t blend_weight(float q, int falloff)
{
    const int i = min(255, (int)(q * 256.0f));
    const uint32_t u = (uint32_t)(256 - i);
    return falloff == 0 ? 256u : falloff == 1 ? u : (u * u + 255u) >> 8;
}

// The accumulating action.  The pixel's key comes first: a fragment behind the band leaves without an atomic (in a fused map that
// is most of them), and only a surfel that contributes somewhere loads its colour word.  acc: SW, SB, SG, SR per pixel.
struct BlendFrag {
    const uint64_t *__restrict__ key;
    blend_u64 *__restrict__ acc;
    const uint32_t *__restrict__ color;
    uint32_t k;
    uint32_t band;                       // 256 + depth_tol_256
    int falloff;
    uint32_t sc;
    uint32_t n;                          // fragments of this lane that contributed

    __device__ __forceinline__ void operator()(size_t p, uint32_t d24, float q)
    {
        const uint32_t front = (uint32_t)(key[p] >> 32);
        if ((uint64_t)d24 * 256u > (uint64_t)front * band) return;
        if (n == 0) sc = color[k];
        ++n;
        const blend_u64 wt = blend_weight(q, falloff);
        blend_u64 *a = acc + p * 4;
        atomicAdd(a, wt);
        atomicAdd(a + 1, wt * (sc & 0xFFu));
        atomicAdd(a + 2, wt * ((sc >> 8) & 0xFFu));
        atomicAdd(a + 3, wt * ((sc >> 16) & 0xFFu));
    }
};

// n of every lane of the wave into one counter: waves with nothing to add leave at the ballot, the others add once
__device__ __forceinline__ void blend_wave_add(uint32_t n, blend_u64 *__restrict__ counter)
{
    if (__ballot(n != 0u) == 0ull) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(counter, (blend_u64)n);
}

__global__ __launch_bounds__(256) void k_blend_accum(Model M, const DevState *__restrict__ st, RenderParams rp,
                                                     const uint64_t *__restrict__ key, blend_u64 *__restrict__ acc, uint32_t band,
                                                     int falloff, blend_u64 *__restrict__ tally)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const SurfelSet cur = M.s[st->cur];
    BlendFrag f{key, acc, cur.color, k, band, falloff, 0u, 0u};
    if (k < st->count) render_surfel(rp, cur.pos_conf, cur.norm_rad, k, f);
    blend_wave_add(f.n, tally);
}

__global__ __launch_bounds__(256) void k_maps_blend_accum(MapsSoA c, uint32_t n, const float4 *__restrict__ box,
                                                          const RenderParams *__restrict__ rps, const uint64_t *__restrict__ key,
                                                          size_t npix, int cull, blend_u64 *__restrict__ acc, uint32_t band, int falloff,
                                                          blend_u64 *__restrict__ tally)
{
    const uint32_t v = blockIdx.y;
    const RenderParams rp = rps[v];
    if (cull && maps_box_outside_image(maps_box_load(box, blockIdx.x), rp)) return;         // (workgroup-uniform)
    const uint32_t k = blockIdx.x * (uint32_t)MAPS_BLOCK + threadIdx.x;
    BlendFrag f{key + (size_t)v * npix, acc + (size_t)v * npix * 4, c.color, k, band, falloff, 0u, 0u};
    if (k < n) render_surfel(rp, c.pos_conf, c.norm_rad, k, f);
    blend_wave_add(f.n, tally);
}

// bgr holds the nearest surfel's colour on every drawn pixel (the resolve's); tally[1] += pixels with sem != 0, tally[2] += those
// of them whose colour changes.  256 lanes per workgroup, whole waves: the ballots count.
__global__ __launch_bounds__(256) void k_blend_normalise(const uint64_t *__restrict__ key, size_t npix, const blend_u64 *__restrict__ acc,
                                                         uint8_t *__restrict__ bgr, const uint8_t *__restrict__ sem,
                                                         blend_u64 *__restrict__ tally)
{
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    const size_t q = (size_t)blockIdx.y * npix + p;
    bool drawn = false, changed = false;
    if (p < npix && key[q] != KEY_EMPTY) {
        drawn = sem[q] != 0;
        const blend_u64 sw = acc[q * 4];
        if (sw) {                                                          // (the winner always contributes)
            const blend_u64 half = sw >> 1;
            const uint8_t b = (uint8_t)((acc[q * 4 + 1] + half) / sw), g = (uint8_t)((acc[q * 4 + 2] + half) / sw),
                          r = (uint8_t)((acc[q * 4 + 3] + half) / sw);
            changed = drawn && (b != bgr[q * 3] || g != bgr[q * 3 + 1] || r != bgr[q * 3 + 2]);
            bgr[q * 3] = b; bgr[q * 3 + 1] = g; bgr[q * 3 + 2] = r;
        }
    }
    const uint64_t md = __ballot(drawn), mc = __ballot(changed);
    if ((threadIdx.x & 63u) == 0u) {
        if (md) atomicAdd(tally + 1, (blend_u64)__popcll(md));
        if (mc) atomicAdd(tally + 2, (blend_u64)__popcll(mc));
    }
}

}  // namespace sm
