// sm_k_simplify.h -- voxel-cell simplification (DESIGN.md "4p. Simplification"; the specification is sm_c_api.h's "sm_simplify").
// Included by sm_simplify.hip only.  Records come as 48-byte AoS rows (three float4), a chunk of a map file or the exported model.
//   k_simplify_insert  pass 1: per regular record the key into the open-addressing table (64-bit atomicCAS, a probe loop bounded
//                      by the table size) and the contribution into the key's accumulators (integer atomics, no return value).
//                      With `combine` the lanes of a wave that follow each other with one key -- a source column of one frame --
//                      are summed by a segmented shuffle reduction first and only the run's first lane goes to memory.
//   k_simplify_flag    pass 2: per record its code (not a representative | loose | the slot of the cell it is `first` of), the
//                      representatives per block of 256, and the call's tallies (one atomic per wave)
//   k_simplify_scan    exclusive prefix of the per-block counts on top of the running rank (one workgroup, block_scan_1024)
//   k_simplify_emit    every representative writes its finished record at its rank: three 16-byte stores
// No kernel waits for another lane: the accumulators are initialised before pass 1 starts (two memsets), so a claimed key can be
// added to at once, and a key that finds no slot sets the sticky error word and gives up.
#pragma once

#include "sm_device.h"

namespace sm {

constexpr uint64_t SIMP_EMPTY = ~0ull;                   // no key: a key has 62 bits
constexpr uint32_t SIMP_NONE = 0xFFFFFFFFu, SIMP_LOOSE = 0xFFFFFFFEu;   // codes; anything else is a slot (at most 2^31 of them)
constexpr uint32_t SIMP_MIN_SLOTS = 1024u;
// the tally's words
enum { SIMP_ERR = 0, SIMP_CELLS, SIMP_RUN, SIMP_N_LOOSE, SIMP_MERGED, SIMP_LARGEST, SIMP_TALLY_WORDS = 8 };

struct SimplifyArgs {
    long long V;                       // the cell edge in 2^-16 m
    float origin[3];
    int split;                         // split_normals
    uint32_t max_cells;
    int combine;                       // 0: SM_SIMPLIFY_NO_COMBINE=1
};

// The table: planes of S = mask + 1 slots; the three-component ones hold component k at [k * S + slot].  Bytes per slot: see
// simplify_table_bytes.  Planes whose empty value is all ones come first, so that two memsets initialise the table.
struct SimplifyTable {
    unsigned long long *key;           // SIMP_EMPTY
    uint32_t *lo, *init_min, *first;   // 0xFFFFFFFF
    unsigned long long *SW, *SP, *SN, *SC;   // 0 (SN: two's complement)
    uint32_t *n, *hi, *rmax, *conf_max, *time_max;   // 0
    uint32_t mask;
    uint32_t *tally;                   // SIMP_TALLY_WORDS words
};
constexpr size_t SIMP_ONES_BYTES = 8 + 12 + 4 + 4, SIMP_ZERO_BYTES = 8 * 10 + 4 + 12 + 4 + 4 + 4;
__host__ __device__ inline size_t simplify_table_bytes(size_t slots) { return slots * (SIMP_ONES_BYTES + SIMP_ZERO_BYTES); }

// what a regular record adds to its cell
struct SimpContrib {
    uint32_t n;
    unsigned long long sw, sp[3], sc[3];
    long long sn[3];
    uint32_t lo[3], hi[3], rmax, conf, time, init, first;
};

__device__ __forceinline__ unsigned long long simp_hash(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 33);
}

__device__ __forceinline__ bool simp_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// regular: the key, the cell and the offsets in it; false: the record is loose
__device__ __forceinline__ bool simp_classify(const SimplifyArgs &a, const float4 &pc, const float4 &ct, const float4 &nr, unsigned long long &key,
                                              uint32_t off[3])
{
    bool ok = simp_finite(pc.x) && simp_finite(pc.y) && simp_finite(pc.z) && simp_finite(pc.w) && pc.w > 0.0f;
    ok = ok && simp_finite(ct.z) && ct.z >= 0.0f && simp_finite(ct.w) && ct.w >= 0.0f;
    ok = ok && simp_finite(nr.w) && nr.w >= 0.0f && nr.w < 32768.0f;
    ok = ok && simp_finite(nr.x) && simp_finite(nr.y) && simp_finite(nr.z) && !(nr.x == 0.0f && nr.y == 0.0f && nr.z == 0.0f);
    if (!ok) return false;
    const float p[3] = {pc.x, pc.y, pc.z};
    unsigned long long k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double d = (double)p[i] - (double)a.origin[i];
        if (!(fabs(d) < 16777216.0)) return false;
        const long long X = (long long)floor(d * 65536.0);
        long long c = X / a.V;
        if (X - c * a.V < 0) --c;                        // floor division
        if (c < -65536 || c > 65535) return false;
        off[i] = (uint32_t)(X - c * a.V);
        k = (k << 17) | (unsigned long long)(c + 65536);
    }
    uint32_t face = 0;
    if (a.split) {
        const float n[3] = {nr.x, nr.y, nr.z};
        int ax = 0;
        if (fabsf(n[1]) > fabsf(n[ax])) ax = 1;
        if (fabsf(n[2]) > fabsf(n[ax])) ax = 2;
        face = 2u * (uint32_t)ax + (n[ax] < 0.0f ? 1u : 0u);
    }
    key = (k << 11) | ((unsigned long long)face << 8) | (unsigned long long)(__float_as_uint(ct.x) >> 24);
    return true;
}

__device__ __forceinline__ void simp_contribution(const float4 &pc, const float4 &ct, const float4 &nr, const uint32_t off[3], uint32_t gid, SimpContrib &c)
{
    const float t = pc.w * 16.0f;
    const uint32_t w = t >= 255.0f ? 255u : (uint32_t)max(1, (int)t);
    const uint32_t col = __float_as_uint(ct.x);
    const float n[3] = {nr.x, nr.y, nr.z};
    c.n = 1u;
    c.sw = w;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c.sp[k] = (unsigned long long)w * off[k];
        const float f = fminf(fmaxf(floorf(n[k] * 16384.0f + 0.5f), -4194304.0f), 4194304.0f);
        c.sn[k] = (long long)w * (long long)(int)f;
        c.sc[k] = (unsigned long long)w * ((col >> (8 * k)) & 255u);
        c.lo[k] = c.hi[k] = off[k];
    }
    c.rmax = (uint32_t)(long long)floor((double)nr.w * 65536.0);
    c.conf = __float_as_uint(pc.w);
    c.time = __float_as_uint(ct.w);
    c.init = __float_as_uint(ct.z);
    c.first = gid;
}

// b into a: lane `lane` takes lane + o's sums when that lane belongs to its run
__device__ __forceinline__ void simp_take(SimpContrib &c, int o, bool take)
{
#define SIMP_ADD(x) { const auto v_ = __shfl_down(x, o); if (take) x += v_; }
#define SIMP_MIN(x) { const uint32_t v_ = __shfl_down(x, o); if (take) x = min(x, v_); }
#define SIMP_MAX(x) { const uint32_t v_ = __shfl_down(x, o); if (take) x = max(x, v_); }
    SIMP_ADD(c.n) SIMP_ADD(c.sw)
#pragma unroll
    for (int k = 0; k < 3; ++k) { SIMP_ADD(c.sp[k]) SIMP_ADD(c.sn[k]) SIMP_ADD(c.sc[k]) SIMP_MIN(c.lo[k]) SIMP_MAX(c.hi[k]) }
    SIMP_MAX(c.rmax) SIMP_MAX(c.conf) SIMP_MAX(c.time) SIMP_MIN(c.init) SIMP_MIN(c.first)
#undef SIMP_ADD
#undef SIMP_MIN
#undef SIMP_MAX
}

// the slot that holds `key`, claiming an empty one if `claim`; false after mask + 1 probes without it
__device__ __forceinline__ bool simp_probe(const SimplifyTable &T, unsigned long long key, bool claim, uint32_t &slot, bool &claimed)
{
    uint32_t sl = (uint32_t)simp_hash(key) & T.mask;
    claimed = false;
    for (uint32_t i = 0; i <= T.mask; ++i) {
        unsigned long long cur = T.key[sl];              // (a stale "empty" is settled by the CAS; a key never changes)
        if (cur == SIMP_EMPTY) {
            if (!claim) return false;
            cur = atomicCAS(&T.key[sl], SIMP_EMPTY, key);
            if (cur == SIMP_EMPTY) { claimed = true; cur = key; }
        }
        if (cur == key) { slot = sl; return true; }
        sl = (sl + 1u) & T.mask;
    }
    return false;
}

// ---- pass 1: n records at rec, ids gid0 + t
__global__ __launch_bounds__(256) void k_simplify_insert(const float4 *__restrict__ rec, uint32_t n, uint32_t gid0, SimplifyArgs a, SimplifyTable T)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned long long key = SIMP_EMPTY;
    bool reg = false;
    SimpContrib c{};
    if (t < n) {
        const float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
        uint32_t off[3];
        reg = simp_classify(a, pc, ct, nr, key, off);
        if (reg) simp_contribution(pc, ct, nr, off, gid0 + t, c);
        else key = SIMP_EMPTY;
    }
    bool head = reg;
    if (a.combine) {
        const unsigned long long prev = __shfl_up(key, 1);
        const bool follows = reg && lane > 0 && prev == key;
        if (__ballot(follows)) {                         // wave-uniform: some run in this wave is longer than one lane
            head = reg && !follows;
            const unsigned long long bounds = __ballot(!follows);                // first lanes of runs, and every lane without a key
            const unsigned long long above = lane == 63 ? 0ull : bounds >> (lane + 1);
            const int last = above ? lane + __ffsll(above) - 1 : 63;             // the last lane of this lane's run
            for (int o = 1; o < 64; o <<= 1) {
                const bool take = lane + o <= last;
                if (!__ballot(take)) break;
                simp_take(c, o, take);
            }
        }
    }
    bool claimed = false, lost = false;
    if (head) {
        uint32_t sl = 0;
        if (simp_probe(T, key, true, sl, claimed)) {
            const size_t S = (size_t)T.mask + 1u;
            atomicAdd(&T.n[sl], c.n);
            atomicAdd(&T.SW[sl], c.sw);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                atomicAdd(&T.SP[k * S + sl], c.sp[k]);
                atomicAdd(&T.SN[k * S + sl], (unsigned long long)c.sn[k]);
                atomicAdd(&T.SC[k * S + sl], c.sc[k]);
                atomicMin(&T.lo[k * S + sl], c.lo[k]);
                atomicMax(&T.hi[k * S + sl], c.hi[k]);
            }
            atomicMax(&T.rmax[sl], c.rmax);
            atomicMax(&T.conf_max[sl], c.conf);
            atomicMax(&T.time_max[sl], c.time);
            atomicMin(&T.init_min[sl], c.init);
            atomicMin(&T.first[sl], c.first);
        } else {
            lost = true;
        }
    }
    // the distinct cells, one add per wave
    const unsigned long long cb = __ballot(claimed);
    if (cb && lane == __ffsll(cb) - 1) {
        const uint32_t m = (uint32_t)__popcll(cb);
        if (atomicAdd(&T.tally[SIMP_CELLS], m) + m > a.max_cells) atomicOr(&T.tally[SIMP_ERR], 1u);
    }
    if (lost) atomicOr(&T.tally[SIMP_ERR], 2u);
}

// ---- pass 2
__global__ __launch_bounds__(256) void k_simplify_flag(const float4 *__restrict__ rec, uint32_t n, uint32_t gid0, SimplifyArgs a, SimplifyTable T,
                                                       uint32_t *__restrict__ code, uint32_t *__restrict__ blk_cnt)
{
    __shared__ uint32_t s_cnt[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t c = SIMP_NONE, cell_n = 0;
    bool lost = false;
    if (t < n) {
        const float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
        unsigned long long key;
        uint32_t off[3], sl = 0;
        bool claimed;
        if (!simp_classify(a, pc, ct, nr, key, off)) c = SIMP_LOOSE;
        else if (!simp_probe(T, key, false, sl, claimed)) lost = true;
        else if (T.first[sl] == gid0 + t) { c = sl; cell_n = T.n[sl]; }
        code[t] = c;
    }
    const unsigned long long reps = __ballot(c != SIMP_NONE), loose = __ballot(c == SIMP_LOOSE), merged = __ballot(cell_n >= 2u);
    uint32_t largest = cell_n;
#pragma unroll
    for (int o = 32; o; o >>= 1) largest = max(largest, (uint32_t)__shfl_xor(largest, o));
    if (lane == 0) {
        s_cnt[wave] = (uint32_t)__popcll(reps);
        if (loose) atomicAdd(&T.tally[SIMP_N_LOOSE], (uint32_t)__popcll(loose));
        if (merged) atomicAdd(&T.tally[SIMP_MERGED], (uint32_t)__popcll(merged));
        if (largest > 1u) atomicMax(&T.tally[SIMP_LARGEST], largest);
    }
    if (lost) atomicOr(&T.tally[SIMP_ERR], 4u);
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// blk_base[b] = the rank of block b's first representative in the whole output; info (may be null): (this call's first rank, its count)
__global__ __launch_bounds__(1024) void k_simplify_scan(const uint32_t *__restrict__ blk_cnt, uint32_t nblk, uint32_t *__restrict__ blk_base,
                                                        uint32_t *__restrict__ tally, uint2 *__restrict__ info)
{
    __shared__ uint32_t s_scan[17];
    __shared__ uint32_t s_run;
    if (threadIdx.x == 0) s_run = tally[SIMP_RUN];
    __syncthreads();
    const uint32_t run0 = s_run;
    uint32_t run = run0;
    for (uint32_t b = 0; b < nblk; b += 1024u) {
        const uint32_t i = b + threadIdx.x;
        const uint32_t v = i < nblk ? blk_cnt[i] : 0u;
        uint32_t tot;
        const uint32_t excl = block_scan_1024(v, &tot, s_scan);
        if (i < nblk) blk_base[i] = run + excl;
        run += tot;
        __syncthreads();                                 // (s_scan is written again)
    }
    if (threadIdx.x == 0) {
        tally[SIMP_RUN] = run;
        if (info) *info = make_uint2(run0, run - run0);
    }
}

__device__ __forceinline__ unsigned long long simp_isqrt(unsigned long long v)
{
    unsigned long long r = (unsigned long long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// the record of a cell with two or more contributors; nr_first: the normal of its record `first`
__device__ __forceinline__ void simp_finish(const SimplifyArgs &a, const SimplifyTable &T, uint32_t sl, const float4 &nr_first, float4 &pc, float4 &ct,
                                            float4 &nr)
{
    const size_t S = (size_t)T.mask + 1u;
    const unsigned long long key = T.key[sl], SW = T.SW[sl], half = SW / 2;
    float p[3];
    uint32_t col = (uint32_t)(key & 255ull) << 24;
    long long sn[3], e2 = 0;
    unsigned long long big = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long cell = (long long)((key >> (45 - 17 * k)) & 0x1FFFFull) - 65536;
        const long long X = cell * a.V + (long long)((T.SP[k * S + sl] + half) / SW);
        p[k] = (float)((double)a.origin[k] + (double)X * (1.0 / 65536.0));
        col |= (uint32_t)((T.SC[k * S + sl] + half) / SW) << (8 * k);
        sn[k] = (long long)T.SN[k * S + sl];
        big = max(big, (unsigned long long)(sn[k] < 0 ? -sn[k] : sn[k]));
        const long long e = (long long)T.hi[k * S + sl] - (long long)T.lo[k * S + sl];
        e2 += e * e;
    }
    const int bits = big ? 64 - __clzll((long long)big) : 0, sh = max(0, bits - 24);
    const float f0 = (float)(sn[0] >> sh), f1 = (float)(sn[1] >> sh), f2 = (float)(sn[2] >> sh);
    if (f0 == 0.0f && f1 == 0.0f && f2 == 0.0f) {
        nr = nr_first;
    } else {
        const float len = sqrtf((f0 * f0 + f1 * f1) + f2 * f2);
        nr = make_float4(f0 / len, f1 / len, f2 / len, 0.0f);
    }
    const unsigned long long R = max((unsigned long long)T.rmax[sl], (simp_isqrt((unsigned long long)e2) + 1ull) / 2ull);
    nr.w = (float)((double)R * (1.0 / 65536.0));
    pc = make_float4(p[0], p[1], p[2], __uint_as_float(T.conf_max[sl]));
    ct = make_float4(__uint_as_float(col), 0.0f, __uint_as_float(T.init_min[sl]), __uint_as_float(T.time_max[sl]));
}

// out[(rank - base) * 3 ..]: base = info->x (a chunk's output begins at out), 0 without info (out is the whole output)
__global__ __launch_bounds__(256) void k_simplify_emit(const float4 *__restrict__ rec, uint32_t n, SimplifyArgs a, SimplifyTable T,
                                                       const uint32_t *__restrict__ code, const uint32_t *__restrict__ blk_base,
                                                       const uint2 *__restrict__ info, float4 *__restrict__ out)
{
    __shared__ uint32_t s_cnt[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c = t < n ? code[t] : SIMP_NONE;
    const unsigned long long reps = __ballot(c != SIMP_NONE);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(reps);
    __syncthreads();
    if (c == SIMP_NONE) return;
    uint32_t rank = blk_base[blockIdx.x] - (info ? info->x : 0u) + (uint32_t)__popcll(reps & ((1ull << lane) - 1ull));
    for (int x = 0; x < wave; ++x) rank += s_cnt[x];
    float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
    if (c != SIMP_LOOSE && T.n[c] >= 2u) simp_finish(a, T, c, nr, pc, ct, nr);
    out[(size_t)rank * 3] = pc;
    out[(size_t)rank * 3 + 1] = ct;
    out[(size_t)rank * 3 + 2] = nr;
}

}  // namespace sm
