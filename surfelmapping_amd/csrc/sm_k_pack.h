// sm_k_pack.h -- the packed map-file format on the device (include/sm_c_api.h "packed map files"; DESIGN.md "4aa. Packed map
// files"; tests/pack_ref.py restates every operation below, bit for bit).  Included by sm_pack.hip only.
//   k_unpack       one workgroup per block of 256 records: the block's 20-byte records (or its 48 verbatim, RAW) -> 48-byte records
//   k_pack_plan    one workgroup per block: the block's minima and its vote -- packed, or RAW -- into its directory entry and size
//   k_pack_scan    one workgroup: the offsets of a chunk's (at most 4096) blocks behind the file's running total
//   k_pack_write   one workgroup per block: the 20-byte records (or the block verbatim) to the block's place in the payload
// All memory traffic is by consecutive lanes on consecutive addresses; a lane reaches its own record through LDS, as in
// k_maps_intake and k_retire_gather.  Every fp32 operation is one IEEE operation in the written order (-ffp-contract=off,
// correctly rounded / and sqrt: csrc/Makefile).
#pragma once

#include "sm_device.h"

namespace sm {

constexpr int PACK_BLOCK = 256;          // records per block = per workgroup
constexpr uint32_t PACK_RAW_FLAG = 1u;

// a directory entry as it lies in the file (sm_mapfile::PackDir)
struct PackDirDev {
    float ox, oy, oz, time_base, init_base;
    uint32_t flags;
    unsigned long long offset;
};
static_assert(sizeof(PackDirDev) == 32, "a directory entry is 32 bytes");

// ---- the normal: octahedral, 10 + 10 bits
__device__ __forceinline__ uint32_t pack_oct_code(float p)
{
    float v = floorf((p * 0.5f + 0.5f) * 1023.0f + 0.5f);
    v = v >= 0.0f ? v : 0.0f;                            // (a NaN becomes 0: such a record is never packed)
    return (uint32_t)fminf(v, 1023.0f);
}

__device__ __forceinline__ uint32_t pack_oct_encode(float nx, float ny, float nz)
{
    const float a = (fabsf(nx) + fabsf(ny)) + fabsf(nz);
    float px = nx / a, py = ny / a;
    if (nz < 0.0f) {
        const float fx = (1.0f - fabsf(py)) * (px >= 0.0f ? 1.0f : -1.0f), fy = (1.0f - fabsf(px)) * (py >= 0.0f ? 1.0f : -1.0f);
        px = fx; py = fy;
    }
    return pack_oct_code(px) | pack_oct_code(py) << 10;
}

// the fold in integers on the codes, then one fp32 normalisation
__device__ __forceinline__ void pack_oct_decode(uint32_t ou, uint32_t ov, float &nx, float &ny, float &nz)
{
    const int ui = 2 * (int)ou - 1023, vi = 2 * (int)ov - 1023;
    const int zi = 1023 - abs(ui) - abs(vi), t = max(-zi, 0);
    const int xi = ui >= 0 ? ui - t : ui + t, yi = vi >= 0 ? vi - t : vi + t;
    const float len = sqrtf((float)(xi * xi + yi * yi + zi * zi));        // (the sum is < 2^22: exact; zi is odd, never 0)
    nx = (float)xi / len; ny = (float)yi / len; nz = (float)zi / len;
}

// ---------------------------------------------------------------------------------------------
// k_unpack: block b of the chunk.  dir: the chunk's directory slice; payload: from the first block's offset on.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unpack(const PackDirDev *__restrict__ dir, const uint32_t *__restrict__ payload, uint32_t n, float down,
                                                float4 *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_in[PACK_BLOCK * 5];            // 5 KiB: a lane's record at a stride of 5 dwords (odd: no bank conflict)
    __shared__ float4 s_out[PACK_BLOCK * 3];             // 12 KiB
    const uint32_t first = blockIdx.x * (uint32_t)PACK_BLOCK;
    const uint32_t m = min((uint32_t)PACK_BLOCK, n - first);             // (>= 1: the grid is ceil(n / 256))
    const PackDirDev d = dir[blockIdx.x];
    const uint32_t *src = payload + (size_t)((d.offset - dir[0].offset) >> 2);
    float4 *dst = out + (size_t)first * 3;
    if (d.flags & PACK_RAW_FLAG) {                       // (workgroup-uniform) every block begins at a multiple of 16 bytes
        const float4 *src4 = (const float4 *)src;
        for (uint32_t i = threadIdx.x; i < m * 3u; i += 256u) dst[i] = src4[i];
        return;
    }
    const uint32_t words = m * 5u, quads = words >> 2;
    const uint4 *src4 = (const uint4 *)src;
    for (uint32_t i = threadIdx.x; i < quads; i += 256u) ((uint4 *)s_in)[i] = src4[i];
    for (uint32_t i = quads * 4u + threadIdx.x; i < words; i += 256u) s_in[i] = src[i];
    __syncthreads();
    if (threadIdx.x < m) {
        const uint32_t *w = s_in + threadIdx.x * 5u;
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
        float4 pc, ct, nr;
        pc.x = d.ox + (float)(w0 & 0xFFFFu) * down;
        pc.y = d.oy + (float)(w0 >> 16) * down;
        pc.z = d.oz + (float)(w1 & 0xFFFFu) * down;
        pc.w = (float)(w3 >> 20) * 0.0625f;
        ct.x = __uint_as_float(w2);
        ct.y = 0.0f;
        ct.z = d.init_base + (float)(w4 >> 16);
        ct.w = d.time_base + (float)(w4 & 0xFFFFu);
        pack_oct_decode(w3 & 1023u, (w3 >> 10) & 1023u, nr.x, nr.y, nr.z);
        nr.w = (float)(w1 >> 16) * (1.0f / 8192.0f);
        s_out[threadIdx.x * 3 + 0] = pc; s_out[threadIdx.x * 3 + 1] = ct; s_out[threadIdx.x * 3 + 2] = nr;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < m * 3u; i += 256u) dst[i] = s_out[i];
}

// ---------------------------------------------------------------------------------------------
// The encoder.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float pack_wave_min(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ bool pack_is_finite(float v) { return v - v == 0.0f; }      // (x - x is 0 for a finite x, NaN otherwise)

// k_pack_plan: the block's rule.  size[b]: the block's bytes in the payload; dir[b]: everything but the offset.
__global__ __launch_bounds__(256) void k_pack_plan(const float4 *__restrict__ rec, uint32_t n, float up, float down, PackDirDev *__restrict__ dir,
                                                   uint32_t *__restrict__ size)
{
    __shared__ float4 s_rec[PACK_BLOCK * 3];             // 12 KiB
    __shared__ float s_red[4][6];
    __shared__ uint32_t s_bad[4];
    const uint32_t first = blockIdx.x * (uint32_t)PACK_BLOCK;
    const uint32_t m = min((uint32_t)PACK_BLOCK, n - first);
    const float4 *src = rec + (size_t)first * 3;
    for (uint32_t i = threadIdx.x; i < m * 3u; i += 256u) s_rec[i] = src[i];
    __syncthreads();
    const bool have = threadIdx.x < m;
    const float INF = __uint_as_float(0x7F800000u);
    float4 pc = make_float4(INF, INF, INF, 0.0f), ct = make_float4(0.0f, 0.0f, INF, INF), nr = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    bool ok = true;
    if (have) {
        pc = s_rec[threadIdx.x * 3 + 0]; ct = s_rec[threadIdx.x * 3 + 1]; nr = s_rec[threadIdx.x * 3 + 2];
        ok = pack_is_finite(pc.x) && pack_is_finite(pc.y) && pack_is_finite(pc.z) && pack_is_finite(pc.w) && pack_is_finite(ct.y) &&
             pack_is_finite(ct.z) && pack_is_finite(ct.w) && pack_is_finite(nr.x) && pack_is_finite(nr.y) && pack_is_finite(nr.z) && pack_is_finite(nr.w);
        ok = ok && fabsf(pc.x) < 8192.0f && fabsf(pc.y) < 8192.0f && fabsf(pc.z) < 8192.0f;
        ok = ok && nr.w >= 0.0f && floorf(nr.w * 8192.0f + 0.5f) <= 65535.0f;
        ok = ok && pc.w >= 0.0f && floorf(pc.w * 16.0f + 0.5f) <= 4095.0f;
        ok = ok && __float_as_uint(ct.y) == 0u;
        // (as bits: +0 .. below 2^24, so that a base and a difference are exact and -0 is not taken for +0)
        ok = ok && __float_as_uint(ct.z) < 0x4B800000u && floorf(ct.z) == ct.z;
        ok = ok && __float_as_uint(ct.w) < 0x4B800000u && floorf(ct.w) == ct.w;
        const float n2 = (nr.x * nr.x + nr.y * nr.y) + nr.z * nr.z;
        ok = ok && fabsf(n2 - 1.0f) <= 0.0009765625f;
    }
    const float lx = pack_wave_min(pc.x), ly = pack_wave_min(pc.y), lz = pack_wave_min(pc.z), lt = pack_wave_min(ct.w), li = pack_wave_min(ct.z);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_red[wave][0] = lx; s_red[wave][1] = ly; s_red[wave][2] = lz; s_red[wave][3] = lt; s_red[wave][4] = li; }
    __syncthreads();
    float mn[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) mn[k] = fminf(fminf(s_red[0][k], s_red[1][k]), fminf(s_red[2][k], s_red[3][k]));
    // (+ 0: an origin of -0 becomes +0, whichever zero the minimum came out as)
    const float ox = floorf(mn[0] * up) * down + 0.0f, oy = floorf(mn[1] * up) * down + 0.0f, oz = floorf(mn[2] * up) * down + 0.0f;
    if (have && ok) {
        ok = floorf((pc.x - ox) * up + 0.5f) <= 65535.0f && floorf((pc.y - oy) * up + 0.5f) <= 65535.0f && floorf((pc.z - oz) * up + 0.5f) <= 65535.0f;
        ok = ok && ct.w - mn[3] <= 65535.0f && ct.z - mn[4] <= 65535.0f;
    }
    const bool wbad = __ballot(!ok) != 0ull;
    if (lane == 0) s_bad[wave] = wbad ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool raw = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) != 0u;
        PackDirDev d;
        d.ox = raw ? 0.0f : ox; d.oy = raw ? 0.0f : oy; d.oz = raw ? 0.0f : oz;
        d.time_base = raw ? 0.0f : mn[3]; d.init_base = raw ? 0.0f : mn[4];
        d.flags = raw ? PACK_RAW_FLAG : 0u;
        d.offset = 0ull;
        dir[blockIdx.x] = d;
        size[blockIdx.x] = m * (raw ? 48u : 20u);
    }
}

// k_pack_scan: one workgroup of 1024 threads, four blocks of the chunk each (nblk <= 4096).  dir[b].offset = *run + the bytes of
// the chunk's blocks before b; then *run grows by the chunk's bytes; tally[0]: those bytes, tally[1]: the chunk's RAW blocks.
__global__ __launch_bounds__(1024) void k_pack_scan(uint32_t nblk, const uint32_t *__restrict__ size, PackDirDev *__restrict__ dir,
                                                    unsigned long long *__restrict__ run, uint32_t *__restrict__ tally)
{
    __shared__ uint32_t s_sum[16], s_raw[16];
    const unsigned long long base = *run;
    uint32_t sz[4], mine = 0, raws = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = threadIdx.x * 4u + k;
        sz[k] = b < nblk ? size[b] : 0u;
        mine += sz[k];
        raws += (b < nblk && (dir[b].flags & PACK_RAW_FLAG)) ? 1u : 0u;
    }
    // inclusive scan within the wave, then across the 16 waves
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) raws += __shfl_xor(raws, o);
    if (lane == 63) s_sum[wave] = inc;
    if (lane == 0) s_raw[wave] = raws;
    __syncthreads();                                     // (every thread has read *run)
    uint32_t before = 0, total = 0, raw_total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) before += s_sum[w];
        total += s_sum[w];
        raw_total += s_raw[w];
    }
    unsigned long long at = base + before + (inc - mine);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = threadIdx.x * 4u + k;
        if (b < nblk) dir[b].offset = at;
        at += sz[k];
    }
    if (threadIdx.x == 0) {
        *run = base + total;
        tally[0] = total;
        tally[1] = raw_total;
    }
}

// k_pack_write: block b's records to out + (dir[b].offset - dir[0].offset)
__global__ __launch_bounds__(256) void k_pack_write(const float4 *__restrict__ rec, uint32_t n, float up, const PackDirDev *__restrict__ dir,
                                                    uint32_t *__restrict__ out)
{
    __shared__ float4 s_rec[PACK_BLOCK * 3];             // 12 KiB
    __shared__ __attribute__((aligned(16))) uint32_t s_out[PACK_BLOCK * 5];           // 5 KiB
    const uint32_t first = blockIdx.x * (uint32_t)PACK_BLOCK;
    const uint32_t m = min((uint32_t)PACK_BLOCK, n - first);
    const PackDirDev d = dir[blockIdx.x];
    const float4 *src = rec + (size_t)first * 3;
    uint32_t *dst = out + (size_t)((d.offset - dir[0].offset) >> 2);
    if (d.flags & PACK_RAW_FLAG) {                       // (workgroup-uniform)
        float4 *dst4 = (float4 *)dst;
        for (uint32_t i = threadIdx.x; i < m * 3u; i += 256u) dst4[i] = src[i];
        return;
    }
    for (uint32_t i = threadIdx.x; i < m * 3u; i += 256u) s_rec[i] = src[i];
    __syncthreads();
    if (threadIdx.x < m) {
        const float4 pc = s_rec[threadIdx.x * 3 + 0], ct = s_rec[threadIdx.x * 3 + 1], nr = s_rec[threadIdx.x * 3 + 2];
        const uint32_t qx = (uint32_t)floorf((pc.x - d.ox) * up + 0.5f), qy = (uint32_t)floorf((pc.y - d.oy) * up + 0.5f),
                       qz = (uint32_t)floorf((pc.z - d.oz) * up + 0.5f);
        const uint32_t qr = (uint32_t)floorf(nr.w * 8192.0f + 0.5f), qc = (uint32_t)floorf(pc.w * 16.0f + 0.5f);
        const uint32_t dt = (uint32_t)(ct.w - d.time_base), di = (uint32_t)(ct.z - d.init_base);
        uint32_t *w = s_out + threadIdx.x * 5u;
        w[0] = qx | qy << 16;
        w[1] = qz | qr << 16;
        w[2] = __float_as_uint(ct.x);
        w[3] = pack_oct_encode(nr.x, nr.y, nr.z) | qc << 20;
        w[4] = dt | di << 16;
    }
    __syncthreads();
    const uint32_t words = m * 5u, quads = words >> 2;
    for (uint32_t i = threadIdx.x; i < quads; i += 256u) ((uint4 *)dst)[i] = ((const uint4 *)s_out)[i];
    for (uint32_t i = quads * 4u + threadIdx.x; i < words; i += 256u) dst[i] = s_out[i];
}

}  // namespace sm
