// sm_k_place.h -- place recognition (DESIGN.md "4l. Place recognition").  Included by sm_place.hip only.
// The reference has no place recognition; the rules are those of include/sm_c_api.h, "place recognition".
//
//   k_fern_encode<CELL>  a wave makes one word of the code: its eight ferns, one after the other (four at a time at cell 4, where
//                        a fern's 16 pixels fill a quarter of the wave).  Only the cells that ferns name are read.  A lane takes
//                        cell^2 / 64 consecutive pixels of one row of the cell -- 1 at cell 8, 4 at 16, 16 at 32 -- with the widest
//                        loads the alignment of the image rows allows; the sums go across the lanes by __shfl_xor; the eight
//                        nibbles are combined in a register and lane 0 stores the word.  Integer sums: nothing depends on the order.
//   k_fern_match         a keyframe's code is n_ferns / 32 uint4; lpk lanes (a power of two, at most 64) share a keyframe, each with
//                        16-byte loads, the query's uint4 of a lane held in registers.  A workgroup covers 256 keyframes, reduces
//                        its best keys (dis << 32 | index) by shuffles and through 64 bytes of LDS, and makes one 64-bit atomicMin
//                        per key: the best in the time window and, for a caller that asks, the best in a second window.

#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sm {

struct FernEncodeArgs {
    const uint8_t *rgb;                // row-major H*W*3, may be null (the colour bits are 0 then)
    const uint16_t *depth;             // row-major H*W
    const uint4 *table;                // per fern: x | y << 16, tr | tg << 16, tb | td << 16, 0
    uint32_t *code;                    // n_words words
    int W;
    uint32_t n_words;
    uint32_t a_rgb, a_depth;           // alignment in bytes (a power of two, at most 16) of every row start of the two images
};

// NW 32-bit words from p, whose alignment in bytes is a (a power of two, the same for the whole wave)
template <int NW>
__device__ __forceinline__ void fern_load_run(const uint8_t *__restrict__ p, uint32_t a, uint32_t (&w)[NW])
{
    if (NW % 4 == 0 && a >= 16u) {
#pragma unroll
        for (int q = 0; q < NW / 4; ++q) {
            const uint4 v = ((const uint4 *)p)[q];
            w[(4 * q) % NW] = v.x; w[(4 * q + 1) % NW] = v.y; w[(4 * q + 2) % NW] = v.z; w[(4 * q + 3) % NW] = v.w;
        }
    } else if (NW % 2 == 0 && a >= 8u) {
#pragma unroll
        for (int q = 0; q < NW / 2; ++q) {
            const uint2 v = ((const uint2 *)p)[q];
            w[(2 * q) % NW] = v.x; w[(2 * q + 1) % NW] = v.y;
        }
    } else if (a >= 4u) {
#pragma unroll
        for (int q = 0; q < NW; ++q) w[q] = ((const uint32_t *)p)[q];
    } else if (a >= 2u) {
#pragma unroll
        for (int q = 0; q < NW; ++q) w[q] = (uint32_t)((const uint16_t *)p)[2 * q] | ((uint32_t)((const uint16_t *)p)[2 * q + 1] << 16);
    } else {
#pragma unroll
        for (int q = 0; q < NW; ++q)
            w[q] = (uint32_t)p[4 * q] | ((uint32_t)p[4 * q + 1] << 8) | ((uint32_t)p[4 * q + 2] << 16) | ((uint32_t)p[4 * q + 3] << 24);
    }
}

__device__ __forceinline__ uint32_t fern_min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// grid: ceil(n_words / 4) workgroups of 256 = one wave per word
template <int CELL>
__global__ __launch_bounds__(256) void k_fern_encode(FernEncodeArgs A)
{
    constexpr int FPW = CELL == 4 ? 4 : 1;               // ferns a wave takes at a time
    constexpr int GROUP = 64 / FPW;                      // lanes per fern
    constexpr int PPL = CELL * CELL / GROUP;             // pixels per lane: 1, 1, 4, 16
    constexpr int LPR = CELL / PPL;                      // lanes per row of the cell
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t word = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (word >= A.n_words) return;                       // (the whole wave)
    const uint32_t grp = lane / GROUP, l = lane % GROUP;
    uint32_t out = 0u;
#pragma unroll
    for (int it = 0; it < 8 / FPW; ++it) {
        const uint32_t slot = (uint32_t)(it * FPW) + grp;          // the fern's place in the word
        const uint4 t = A.table[word * 8u + slot];
        const uint32_t px = (t.x & 0xFFFFu) * CELL + (l % LPR) * PPL, py = (t.x >> 16) * CELL + l / LPR;
        const size_t pix = (size_t)py * (size_t)A.W + px;
        uint32_t r = 0u, g = 0u, b = 0u, d = 0u, c = 0u;
        if constexpr (PPL == 1) {
            if (A.rgb) {
                const uint8_t *q = A.rgb + pix * 3;
                r = q[0]; g = q[1]; b = q[2];
            }
            d = A.depth[pix];
            c = d != 0u ? 1u : 0u;
        } else {
            if (A.rgb) {
                uint32_t w[PPL * 3 / 4];
                fern_load_run(A.rgb + pix * 3, fern_min_u32(A.a_rgb, (uint32_t)((PPL * 3) & -(PPL * 3))), w);
#pragma unroll
                for (int i = 0; i < PPL * 3; ++i) {
                    const uint32_t v = (w[i / 4] >> (8 * (i % 4))) & 0xFFu;
                    if (i % 3 == 0) r += v;
                    else if (i % 3 == 1) g += v;
                    else b += v;
                }
            }
            uint32_t w[PPL / 2];
            fern_load_run((const uint8_t *)(A.depth + pix), fern_min_u32(A.a_depth, 16u), w);
#pragma unroll
            for (int i = 0; i < PPL / 2; ++i) {
                const uint32_t lo = w[i] & 0xFFFFu, hi = w[i] >> 16;
                d += lo + hi;
                c += (lo != 0u ? 1u : 0u) + (hi != 0u ? 1u : 0u);
            }
        }
#pragma unroll
        for (int off = GROUP / 2; off > 0; off >>= 1) {
            r += (uint32_t)__shfl_xor((int)r, off, 64);
            g += (uint32_t)__shfl_xor((int)g, off, 64);
            b += (uint32_t)__shfl_xor((int)b, off, 64);
            d += (uint32_t)__shfl_xor((int)d, off, 64);
            c += (uint32_t)__shfl_xor((int)c, off, 64);
        }
        const uint32_t R = r / (uint32_t)(CELL * CELL), G = g / (uint32_t)(CELL * CELL), B = b / (uint32_t)(CELL * CELL);
        const uint32_t D = c ? d / c : 0u;
        uint32_t nib = D > (t.z >> 16) ? 8u : 0u;
        if (A.rgb) nib |= (R > (t.y & 0xFFFFu) ? 1u : 0u) | (G > (t.y >> 16) ? 2u : 0u) | (B > (t.z & 0xFFFFu) ? 4u : 0u);
        out |= nib << (4u * slot);
    }
    if constexpr (FPW == 4) {                            // the four quarters hold a nibble each
        out |= (uint32_t)__shfl_xor((int)out, 16, 64);
        out |= (uint32_t)__shfl_xor((int)out, 32, 64);
    }
    if (lane == 0u) A.code[word] = out;
}

constexpr uint32_t FERN_MATCH_KPB = 256;                 // keyframes per workgroup

struct FernMatchArgs {
    const uint4 *codes;                // keyframe-major, Q uint4 each
    const int32_t *times;
    const uint4 *query;                // Q uint4
    uint32_t count, Q, lpk;            // keyframes; uint4 per code; lanes per keyframe: the largest power of two <= min(Q, 64)
    long long min_time, min_time2;     // (64 bits: INT32_MIN - 1 opens a lower end, so that a keyframe of time INT32_MIN is seen)
    int32_t max_time, max_time2;       // keys[0]: the best with min_time < time <= max_time; keys[1]: the same for the second window, when two != 0
    int two;
    uint32_t *dis_all;                 // may be null
    unsigned long long *keys;          // [2], all ones on entry
};

// the ferns whose nibbles differ between two words
__device__ __forceinline__ uint32_t fern_diff(uint32_t a, uint32_t b)
{
    uint32_t x = a ^ b;
    x |= x >> 1;
    x |= x >> 2;
    return (uint32_t)__popc(x & 0x11111111u);
}

__device__ __forceinline__ uint32_t fern_diff4(const uint4 a, const uint4 b)
{
    return (fern_diff(a.x, b.x) + fern_diff(a.y, b.y)) + (fern_diff(a.z, b.z) + fern_diff(a.w, b.w));
}

__device__ __forceinline__ unsigned long long fern_min_u64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

__device__ __forceinline__ unsigned long long fern_wave_min(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
        v = fern_min_u64(v, ((unsigned long long)hi << 32) | lo);
    }
    return v;
}

// grid: ceil(count / FERN_MATCH_KPB) workgroups of 256
__global__ __launch_bounds__(256) void k_fern_match(FernMatchArgs A)
{
    __shared__ unsigned long long best[2][4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t lpk = A.lpk, kpw = 64u / lpk;
    const uint32_t sub = lane & (lpk - 1u), grp = lane / lpk;
    const bool second = sub + lpk < A.Q;                 // (Q < 2 * lpk: a lane holds at most two uint4 of a code)
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    const uint4 q0 = A.query[sub], q1 = second ? A.query[sub + lpk] : zero;
    unsigned long long key0 = ~0ull, key1 = ~0ull;
    const uint32_t k0 = blockIdx.x * FERN_MATCH_KPB;
    for (uint32_t pass = 0; pass < lpk; ++pass) {
        const uint32_t k = k0 + (pass * 4u + wave) * kpw + grp;
        const bool have = k < A.count;
        uint32_t d = 0u;
        if (have) {
            const uint4 *c = A.codes + (size_t)k * A.Q;
            d = fern_diff4(c[sub], q0);
            if (second) d += fern_diff4(c[sub + lpk], q1);
        }
        for (uint32_t off = lpk >> 1; off > 0u; off >>= 1) d += (uint32_t)__shfl_xor((int)d, (int)off, 64);
        if (have && sub == 0u) {
            if (A.dis_all) A.dis_all[k] = d;
            const int32_t t = A.times[k];
            const unsigned long long key = ((unsigned long long)d << 32) | (unsigned long long)k;
            if ((long long)t > A.min_time && t <= A.max_time) key0 = fern_min_u64(key0, key);
            if (A.two && (long long)t > A.min_time2 && t <= A.max_time2) key1 = fern_min_u64(key1, key);
        }
    }
    key0 = fern_wave_min(key0);
    key1 = fern_wave_min(key1);
    if (lane == 0u) { best[0][wave] = key0; best[1][wave] = key1; }
    __syncthreads();
    if (threadIdx.x < 2u) {
        const unsigned long long *b = best[threadIdx.x];
        const unsigned long long m = fern_min_u64(fern_min_u64(b[0], b[1]), fern_min_u64(b[2], b[3]));
        if (m != ~0ull) atomicMin(&A.keys[threadIdx.x], m);
    }
}

}  // namespace sm
