// sm_k_search.h -- pose search before the tracker (DESIGN.md "4j. Pose search").  Included by sm_search.hip only.
// The reference has no tracker and no search; the pair tests are the tracker's own (sm_k_track.h, track_pair), in the same fp32
// expressions, so that a score is the tracker's inlier count at that pose.
//
// One scored list of candidate poses, after the tracker's own preparation (prediction slot map, vertex / normal per grid point):
//   k_search_samples  packs the valid grid points as two float4 each, (v.xyz, Y_f) and (n.xyz, 0); invalid ones are dropped (one
//                     ballot and one atomic per wave: the order is free, the result is a count).
//   k_search_gather   the slot map as two float4 per prediction pixel, (p_m.xyz, Y_m) and (n_m.xyz, valid): the hot loop then
//                     makes one dependent 32-byte gather per pair test instead of slot -> two SoA planes.
//   k_search_score    a workgroup = one chunk of samples x one run of consecutive candidates.  A lane keeps SEARCH_SPL samples in
//                     registers; the 12 pose floats of the candidate are wave-uniform (scalar loads); per candidate: transform,
//                     project, gather, test, ballot + popcount into a scalar, one atomicAdd per (wave, candidate) from one lane.
//                     Integer sums: the scores do not depend on how the work is split.

#pragma once

#include "sm_device.h"

namespace sm {

constexpr int SEARCH_BLOCK = 256;
constexpr int SEARCH_SPL = 4;             // samples per lane
constexpr int SEARCH_CHUNK = SEARCH_BLOCK * SEARCH_SPL;
constexpr int SEARCH_RUN = 32;            // consecutive candidates per workgroup

// Y = ((0.299 R + 0.587 G) + 0.114 B) / 255 of 8-bit channels (sm_k_track_rgb.h, track_luma)
__device__ __forceinline__ float search_luma(uint32_t r, uint32_t g, uint32_t b)
{
    return ((0.299f * (float)r + 0.587f * (float)g) + 0.114f * (float)b) / 255.0f;
}

// rgb may be null (Y_f = 0: the colour test is not made then)
__global__ __launch_bounds__(256) void k_search_samples(const float4 *__restrict__ vmap, const float4 *__restrict__ nmap,
                                                        const uint8_t *__restrict__ rgb, sm_impl::SearchFrame f,
                                                        float4 *__restrict__ samp, uint32_t *__restrict__ n_samp)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = v;
    bool valid = false;
    if (idx < f.n) {
        v = vmap[idx];
        valid = v.w != 0.0f;
        if (valid) {
            n = nmap[idx];
            float y = 0.0f;
            if (rgb) {
                const int gj = idx / f.ni;
                const int i = (idx - gj * f.ni) * f.stride, j = gj * f.stride;
                const uint8_t *c = rgb + ((size_t)j * f.W + i) * 3;
                y = search_luma(c[0], c[1], c[2]);
            }
            v.w = y;
            n.w = 0.0f;
        }
    }
    const uint64_t m = __ballot(valid);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t leader = (uint32_t)(__ffsll((unsigned long long)m) - 1);
    uint32_t base = 0u;
    if (lane == leader) base = atomicAdd(n_samp, (uint32_t)__popcll(m));
    base = __shfl(base, (int)leader, 64);
    if (valid) {
        const uint32_t k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        samp[2 * (size_t)k] = v;
        samp[2 * (size_t)k + 1] = n;
    }
}

__global__ __launch_bounds__(256) void k_search_gather(Model M, const DevState *__restrict__ st, const int32_t *__restrict__ pred,
                                                       int npix, float4 *__restrict__ plane)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int32_t k = pred[p];
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    if (k >= 0) {
        const SurfelSet cur = M.s[st->cur];
        const float4 pc = cur.pos_conf[k];
        const float4 nr = cur.norm_rad[k];
        const uint32_t c = cur.color[k];
        a = make_float4(pc.x, pc.y, pc.z, search_luma((c >> 16) & 0xFFu, (c >> 8) & 0xFFu, c & 0xFFu));
        b = make_float4(nr.x, nr.y, nr.z, 1.0f);
    }
    plane[2 * (size_t)p] = a;
    plane[2 * (size_t)p + 1] = b;
}

// track_pair's tests (sm_k_track.h) on one packed sample under the pose m (columns 0..3, rows 0..2: m[c * 3 + r]), and the
// colour gate when use_colour
__device__ __forceinline__ bool search_pair(const float4 v, const float4 n, const float *m, const sm_impl::SearchFrame &f,
                                            const float4 *__restrict__ plane, bool use_colour, float colour_thresh)
{
    float3 w, nw;
    w.x = ((m[0] * v.x + m[3] * v.y) + m[6] * v.z) + m[9];    // T v (xform3)
    w.y = ((m[1] * v.x + m[4] * v.y) + m[7] * v.z) + m[10];
    w.z = ((m[2] * v.x + m[5] * v.y) + m[8] * v.z) + m[11];
    nw.x = (m[0] * n.x + m[3] * n.y) + m[6] * n.z;            // R n (rot3)
    nw.y = (m[1] * n.x + m[4] * n.y) + m[7] * n.z;
    nw.z = (m[2] * n.x + m[5] * n.y) + m[8] * n.z;
    const float3 c = xform3(f.tinv_prev, w.x, w.y, w.z);      // into the prediction camera
    if (!(c.z > 0.0f)) return false;
    const float fu = floorf(((f.fx * c.x) / c.z + f.cx) + 0.5f);
    const float fv = floorf(((f.fy * c.y) / c.z + f.cy) + 0.5f);
    if (!(fu >= 0.0f && fu < (float)f.W && fv >= 0.0f && fv < (float)f.H)) return false;
    const size_t p = (size_t)(int)fv * f.W + (int)fu;
    const float4 pm = plane[2 * p];
    const float4 nm = plane[2 * p + 1];
    if (nm.w == 0.0f) return false;
    const float3 d = make_float3(w.x - pm.x, w.y - pm.y, w.z - pm.z);
    if (!(sqrtf(dot3(d, d)) <= f.dist)) return false;
    if (!(dot3(nw, make_float3(nm.x, nm.y, nm.z)) >= f.cos_angle)) return false;
    if (use_colour && !(fabsf(v.w - pm.w) <= colour_thresh)) return false;
    return true;
}

// Workgroup b: chunk b % n_chunks of the samples, candidates [(b / n_chunks) * SEARCH_RUN, + SEARCH_RUN).  The host makes
// n_chunks a multiple of 8 once there are 8: workgroups are dealt out round-robin over the 8 XCDs, so every workgroup of a chunk
// then runs on one XCD and the prediction pixels its samples land on under neighbouring candidates are shared in that XCD's L2.
// A chunk's samples are spread with stride n_chunks * 256 over the packed list, whose length only the device knows: every chunk
// gets the same share.  scores is zero on entry.
__global__ __launch_bounds__(SEARCH_BLOCK) void k_search_score(const float4 *__restrict__ samp, const uint32_t *__restrict__ n_samp,
                                                               const float4 *__restrict__ plane, const float *__restrict__ cand12,
                                                               uint32_t n_cand, uint32_t n_chunks, sm_impl::SearchFrame f,
                                                               int use_colour, float colour_thresh, uint32_t *__restrict__ scores)
{
    const uint32_t chunk = blockIdx.x % n_chunks, run = blockIdx.x / n_chunks;
    const uint32_t ns = *n_samp;
    float4 v[SEARCH_SPL], n[SEARCH_SPL];
    bool have[SEARCH_SPL];
#pragma unroll
    for (int k = 0; k < SEARCH_SPL; ++k) {
        const uint32_t i = chunk * SEARCH_BLOCK + threadIdx.x + (uint32_t)k * n_chunks * SEARCH_BLOCK;
        have[k] = i < ns;
        v[k] = have[k] ? samp[2 * (size_t)i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        n[k] = have[k] ? samp[2 * (size_t)i + 1] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if (!__syncthreads_or(have[0])) return;                   // (sample k + 1 of a lane exists only if its sample k does)
    const uint32_t c0 = run * SEARCH_RUN, c1 = min(c0 + (uint32_t)SEARCH_RUN, n_cand);
    const bool lead = (threadIdx.x & 63u) == 0u;
    for (uint32_t c = c0; c < c1; ++c) {
        float m[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) m[e] = cand12[(size_t)c * 12 + e];
        uint32_t cnt = 0u;
#pragma unroll
        for (int k = 0; k < SEARCH_SPL; ++k) {
            const bool ok = have[k] && search_pair(v[k], n[k], m, f, plane, use_colour != 0, colour_thresh);
            cnt += (uint32_t)__popcll(__ballot(ok));
        }
        if (lead && cnt) atomicAdd(&scores[c], cnt);
    }
}

}  // namespace sm
