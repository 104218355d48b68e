// sm_k_io.h -- off the hot path: AoS export / import, index-map textures, the raw feedback cloud, depth read-back, the
// novel-view renderer's kernels.  Included by sm_model_io.hip only; shader citations: /root/reference/src/Shaders/<file>:<line>.
#pragma once

#include "sm_device.h"
#include "sm_k_draw.h"

namespace sm {

// ---------------------------------------------------------------------------------------------
// export helpers (not on the hot path)
// ---------------------------------------------------------------------------------------------
__global__ void k_export_aos(Model M, const DevState *__restrict__ st, float *__restrict__ dst, uint32_t first, uint32_t n)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const SurfelSet cur = M.s[st->cur];
    const uint32_t k = first + t;
    const float4 pc = cur.pos_conf[k], nr = cur.norm_rad[k];
    float *o = dst + (size_t)t * 12;
    o[0] = pc.x; o[1] = pc.y; o[2] = pc.z; o[3] = pc.w;
    o[4] = __uint_as_float(cur.color[k]); o[5] = 0.0f; o[6] = cur.init_time[k]; o[7] = cur.time[k];
    o[8] = nr.x; o[9] = nr.y; o[10] = nr.z; o[11] = nr.w;
}

__global__ void k_import_aos(Model M, const DevState *__restrict__ st, const float *__restrict__ src, uint32_t first, uint32_t n)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const float *o = src + (size_t)t * 12;
    store_record(M.s[st->cur], first + t, make_float4(o[0], o[1], o[2], o[3]), make_float4(o[4], o[5], o[6], o[7]),
                 make_float4(o[8], o[9], o[10], o[11]));
}

// index-map textures (index_map.vert:61-63) materialised from the key map, row-major output
__global__ void k_export_index(Model M, const DevState *__restrict__ st, FrameParams fp,
                               const uint64_t *__restrict__ keyT, int32_t *__restrict__ id_out,
                               float4 *__restrict__ vc, float4 *__restrict__ ct, float4 *__restrict__ nr)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= fp.P) return;
    const int j = p / fp.W, i = p - j * fp.W;
    const uint64_t key = keyT[(size_t)i * fp.H + j];
    const SurfelSet cur = M.s[st->cur];
    int32_t id = 0;
    float4 a = make_float4(0, 0, 0, 0), b = a, c = a;
    if (key != KEY_EMPTY) {
        id = (int32_t)(uint32_t)(key & 0xFFFFFFFFull);
        const float4 pc = cur.pos_conf[id];
        const float3 ph = xform3(fp.t_inv, pc.x, pc.y, pc.z);
        a = make_float4(ph.x, ph.y, ph.z, pc.w);
        b = make_float4(__uint_as_float(cur.color[id]), 0.0f, cur.init_time[id], cur.time[id]);
        const float4 n = cur.norm_rad[id];
        const float3 nn = normalize3(rot3(fp.t_inv, n.x, n.y, n.z));
        c = make_float4(nn.x, nn.y, nn.z, n.w);
    }
    if (id_out) id_out[p] = id;
    if (vc) vc[p] = a;
    if (ct) ct[p] = b;
    if (nr) nr[p] = c;
}

// The raw per-frame surfel cloud of FeedbackBuffer::compute (src/FeedbackBuffer.cpp:85-145, surfel_feedback.vert:25-63,
// surfel_feedback.geom:17-26): every checkerboard pixel with 0 < z < maxDepth as a CAMERA-frame surfel
// (pos, 0.9 | colour, 0, time, time | normal, radius), no neighbour test.  One record slot per pixel + a flag; the host
// keeps the flagged ones in vertex order (x-outer / y-inner, src/FeedbackBuffer.cpp:47-54).  Not on the hot path: the
// reference fills this buffer every frame for the GUI's "Draw raw" view only (src/SurfelMapping.cpp:172).
__global__ __launch_bounds__(256) void k_raw_cloud(FrameParams fp, const float *__restrict__ depthT, const uint32_t *__restrict__ rgbsT,
                                                   const float *__restrict__ xs, const float *__restrict__ ys,
                                                   float4 *__restrict__ rec /* [P][3] */, uint8_t *__restrict__ flag)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= fp.P) return;
    LocalSurfel L;
    const bool ok = local_surfel(q, fp, depthT, rgbsT, xs, ys, L);       // fp.init_mode = 1: the feedback buffer's rules
    flag[q] = ok ? 1 : 0;
    if (!ok) return;
    rec[(size_t)q * 3 + 0] = make_float4(L.pos.x, L.pos.y, L.pos.z, 0.9f);                             // surfel_feedback.vert:96
    rec[(size_t)q * 3 + 1] = make_float4(__uint_as_float(encode_color(L.cr, L.cg, L.cb, L.sem)), 0.0f, (float)fp.time, (float)fp.time);
    rec[(size_t)q * 3 + 2] = make_float4(L.nrm.x, L.nrm.y, L.nrm.z, L.radius);
}

// column-major -> row-major read-back helper (tests / GUI textures)
__global__ void k_untranspose_f32(const float *__restrict__ srcT, float *__restrict__ dst, int W, int H)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= W * H) return;
    const int j = p / W, i = p - j * W;
    dst[p] = srcT[(size_t)i * H + j];
}

// ---------------------------------------------------------------------------------------------
// Novel-view renderer: one lane per surfel, one per pixel; the per-surfel and per-pixel rules are
// sm_k_draw.h's.  `id_base`: what the keys carry above the slot number (0 unless the model is one source of a map set).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_render_splat(Model M, const DevState *__restrict__ st, RenderParams rp,
                                                      uint64_t *__restrict__ key, uint32_t id_base)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= st->count) return;
    const SurfelSet cur = M.s[st->cur];
    render_surfel(rp, cur.pos_conf, cur.norm_rad, k, id_base + k, key);
}

__global__ void k_render_resolve(Model M, const DevState *__restrict__ st, const uint64_t *__restrict__ key, int npix,
                                 uint8_t *__restrict__ bgr, uint8_t *__restrict__ sem)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const uint64_t kk = key[p];
    uint8_t b = 0, g = 0, r = 0, s = 0;
    if (kk != KEY_EMPTY) render_shade(M.s[st->cur].color[(uint32_t)(kk & 0xFFFFFFFFull)], b, g, r, s);
    bgr[(size_t)p * 3] = b; bgr[(size_t)p * 3 + 1] = g; bgr[(size_t)p * 3 + 2] = r;
    sem[p] = s;
}

}  // namespace sm
