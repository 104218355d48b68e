// sm_d_simplify.h -- the voxel-cell table as device functions, for every source that fills or reads such a table (sm_k_simplify.h;
// sm_k_voxel.h; through sm_d_register.h, sm_k_register.h and sm_k_compare.h; sm_k_tile.h, which keeps tiles and counts in one; sm_k_segment.h, whose slots are the nodes of a union-find; sm_k_mesh.h, which keeps cells in one and lattice points in another; sm_k_ground.h, which has no table and takes the record test and the run logic): the regular-record test, the key, a record's
// contribution, the probe, the insert in its pieces -- head of a run, in-wave combination, claim, adds --, a cell's merged
// position, normal and record, and the ranks of a pass that writes.  No kernels: a kernel is defined in the one header of the
// source that launches it.
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

// what a regular record's fields satisfy whatever the grid is
__device__ __forceinline__ bool simp_fields_ok(const float4 &pc, const float4 &ct, const float4 &nr)
{
    bool ok = simp_finite(pc.x) && simp_finite(pc.y) && simp_finite(pc.z) && simp_finite(pc.w) && pc.w > 0.0f;
    ok = ok && simp_finite(ct.z) && ct.z >= 0.0f && simp_finite(ct.w) && ct.w >= 0.0f;
    ok = ok && simp_finite(nr.w) && nr.w >= 0.0f && nr.w < 32768.0f;
    return ok && simp_finite(nr.x) && simp_finite(nr.y) && simp_finite(nr.z) && !(nr.x == 0.0f && nr.y == 0.0f && nr.z == 0.0f);
}

// regular: the key, the cell and the offsets in it; false: the record is loose
__device__ __forceinline__ bool simp_classify(const SimplifyArgs &a, const float4 &pc, const float4 &ct, const float4 &nr, unsigned long long &key,
                                              uint32_t off[3])
{
    if (!simp_fields_ok(pc, ct, nr)) return false;
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

// the slot that holds `key`, claiming an empty one if `claim`; false after mask + 1 probes without it -- or after `walk` probes, for
// a caller whose table may fill (meshing's lattice table): in a table at most half full no walk comes near a thousand slots
__device__ __forceinline__ bool simp_probe(const SimplifyTable &T, unsigned long long key, bool claim, uint32_t &slot, bool &claimed,
                                           uint32_t walk = 0xFFFFFFFFu)
{
    uint32_t sl = (uint32_t)simp_hash(key) & T.mask;
    claimed = false;
    for (uint32_t i = 0; i <= T.mask && i < walk; ++i) {
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

// What pass 1 does with a lane's key once it is known, in pieces; all 64 lanes of a wave call each (reg: the lane has a key).
// Is this lane the first of its run of equal keys?  Every regular lane is without `combine`.  A table of keys only has nothing
// to combine and stops here.
__device__ __forceinline__ bool simp_head(const SimplifyArgs &a, unsigned long long key, bool reg)
{
    if (!a.combine) return reg;
    const unsigned long long prev = __shfl_up(key, 1);
    return reg && !((threadIdx.x & 63) > 0 && prev == key);
}

// The last lane of this lane's run; all 64 lanes call it with what simp_head gave
__device__ __forceinline__ int simp_run_last(bool reg, bool head)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long bounds = __ballot(head || !reg);                    // first lanes of runs, and every lane without a key
    const unsigned long long above = lane == 63 ? 0ull : bounds >> (lane + 1);
    return above ? lane + __ffsll(above) - 1 : 63;
}

// The in-wave combination: a head's contribution becomes the sum of its run's (a segmented shuffle reduction); returns simp_head
__device__ __forceinline__ bool simp_combine(const SimplifyArgs &a, unsigned long long key, bool reg, SimpContrib &c)
{
    const int lane = threadIdx.x & 63;
    const bool head = simp_head(a, key, reg);
    if (__ballot(reg && !head)) {                        // wave-uniform: some run in this wave is longer than one lane
        const int last = simp_run_last(reg, head);
        for (int o = 1; o < 64; o <<= 1) {
            const bool take = lane + o <= last;
            if (!__ballot(take)) break;
            simp_take(c, o, take);
        }
    }
    return head;
}

// The claim: a head finds its key's slot or claims an empty one and adds(slot) what it has for it -- atomics without a return
// value, issued before this step waits for one of its own; then the distinct cells go to the tally, one add per wave, and with
// them the error bits (1: more than max_cells cells, 2: no slot)
template <typename Adds>
__device__ __forceinline__ void simp_claim(const SimplifyArgs &a, const SimplifyTable &T, unsigned long long key, bool head, Adds adds,
                                           uint32_t walk = 0xFFFFFFFFu)
{
    const int lane = threadIdx.x & 63;
    bool claimed = false, lost = false;
    if (head) {
        uint32_t sl = 0;
        if (simp_probe(T, key, true, sl, claimed, walk)) adds(sl);
        else lost = true;
    }
    const unsigned long long cb = __ballot(claimed);
    if (cb && lane == __ffsll(cb) - 1) {
        const uint32_t m = (uint32_t)__popcll(cb);
        if (atomicAdd(&T.tally[SIMP_CELLS], m) + m > a.max_cells) atomicOr(&T.tally[SIMP_ERR], 1u);
    }
    if (lost) atomicOr(&T.tally[SIMP_ERR], 2u);
}

// The combination, then the claim with the adds.  FULL: every accumulator of the table; otherwise the planes a cell's merged
// position and normal are made of -- SW, SP, SN -- and no others (the lookup tables of sm_k_voxel.h, which have only those).
template <bool FULL>
__device__ __forceinline__ void simp_insert(const SimplifyArgs &a, const SimplifyTable &T, unsigned long long key, bool reg, SimpContrib &c)
{
    const bool head = simp_combine(a, key, reg, c);
    simp_claim(a, T, key, head, [&](uint32_t sl) {
        const size_t S = (size_t)T.mask + 1u;
        if constexpr (FULL) atomicAdd(&T.n[sl], c.n);
        atomicAdd(&T.SW[sl], c.sw);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicAdd(&T.SP[k * S + sl], c.sp[k]);
            atomicAdd(&T.SN[k * S + sl], (unsigned long long)c.sn[k]);
            if constexpr (FULL) {
                atomicAdd(&T.SC[k * S + sl], c.sc[k]);
                atomicMin(&T.lo[k * S + sl], c.lo[k]);
                atomicMax(&T.hi[k * S + sl], c.hi[k]);
            }
        }
        if constexpr (FULL) {
            atomicMax(&T.rmax[sl], c.rmax);
            atomicMax(&T.conf_max[sl], c.conf);
            atomicMax(&T.time_max[sl], c.time);
            atomicMin(&T.init_min[sl], c.init);
            atomicMin(&T.first[sl], c.first);
        }
    });
}

__device__ __forceinline__ unsigned long long simp_isqrt(unsigned long long v)
{
    unsigned long long r = (unsigned long long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// a cell's merged position on axis k: the cell's corner plus the weighted mean offset, rounded to the nearest 2^-16 m
__device__ __forceinline__ float simp_merged_pos(const SimplifyArgs &a, unsigned long long key, int k, unsigned long long SW, unsigned long long SPk)
{
    const long long cell = (long long)((key >> (45 - 17 * k)) & 0x1FFFFull) - 65536;
    const long long X = cell * a.V + (long long)((SPk + SW / 2) / SW);
    return (float)((double)a.origin[k] + (double)X * (1.0 / 65536.0));
}

// a cell's merged normal from its sums; false (n untouched): all three components vanish
__device__ __forceinline__ bool simp_merged_normal(const long long sn[3], float n[3])
{
    unsigned long long big = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) big = max(big, (unsigned long long)(sn[k] < 0 ? -sn[k] : sn[k]));
    const int bits = big ? 64 - __clzll((long long)big) : 0, sh = max(0, bits - 24);
    const float f0 = (float)(sn[0] >> sh), f1 = (float)(sn[1] >> sh), f2 = (float)(sn[2] >> sh);
    if (f0 == 0.0f && f1 == 0.0f && f2 == 0.0f) return false;
    const float len = sqrtf((f0 * f0 + f1 * f1) + f2 * f2);
    n[0] = f0 / len; n[1] = f1 / len; n[2] = f2 / len;
    return true;
}

// the record of a cell with two or more contributors; nr_first: the normal of its record `first`
__device__ __forceinline__ void simp_finish(const SimplifyArgs &a, const SimplifyTable &T, uint32_t sl, const float4 &nr_first, float4 &pc, float4 &ct,
                                            float4 &nr)
{
    const size_t S = (size_t)T.mask + 1u;
    const unsigned long long key = T.key[sl], SW = T.SW[sl], half = SW / 2;
    float p[3], nn[3];
    uint32_t col = (uint32_t)(key & 255ull) << 24;
    long long sn[3], e2 = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = simp_merged_pos(a, key, k, SW, T.SP[k * S + sl]);
        col |= (uint32_t)((T.SC[k * S + sl] + half) / SW) << (8 * k);
        sn[k] = (long long)T.SN[k * S + sl];
        const long long e = (long long)T.hi[k * S + sl] - (long long)T.lo[k * S + sl];
        e2 += e * e;
    }
    if (simp_merged_normal(sn, nn)) nr = make_float4(nn[0], nn[1], nn[2], 0.0f);
    else nr = nr_first;
    const unsigned long long R = max((unsigned long long)T.rmax[sl], (simp_isqrt((unsigned long long)e2) + 1ull) / 2ull);
    nr.w = (float)((double)R * (1.0 / 65536.0));
    pc = make_float4(p[0], p[1], p[2], __uint_as_float(T.conf_max[sl]));
    ct = make_float4(__uint_as_float(col), 0.0f, __uint_as_float(T.init_min[sl]), __uint_as_float(T.time_max[sl]));
}

// Pass 2's ranks, by one workgroup of 1024 (all of its lanes call it): blk_base[b] = the running rank tally[SIMP_RUN] plus the
// exclusive prefix of blk_cnt, the running rank moved on by their sum; info (may be null): (this call's first rank, its count)
__device__ __forceinline__ void simp_scan_ranks(const uint32_t *__restrict__ blk_cnt, uint32_t nblk, uint32_t *__restrict__ blk_base,
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

// The rank of a lane's record in its chunk's output, by a workgroup of 256 (all of its lanes call it; kept: the lane has a record
// that stays): blk_base of the block, less the chunk's first rank info->x (no info: the output is the whole call's), plus the
// kept lanes below this one
__device__ __forceinline__ uint32_t simp_rank_in_chunk(bool kept, const uint32_t *__restrict__ blk_base, const uint2 *__restrict__ info)
{
    __shared__ uint32_t s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(kept);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!kept) return 0u;
    uint32_t rank = blk_base[blockIdx.x] - (info ? info->x : 0u) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (int x = 0; x < wave; ++x) rank += s_cnt[x];
    return rank;
}

// ---- the lean claim table (ray casts, DESIGN.md "4x"): a key plane and a plane of (count, first) per slot, nothing of the 148 bytes
// a SimplifyTable slot holds.  sm_voxel.hip sizes and clears it (lean_slots, lean_clear).  lean_probe is simp_probe's walk over
// the key plane alone, bounded by LEAN_WALK, counting the slots it reads: a key that was claimed lies within LEAN_WALK of its
// hash and slots never empty again, so a later walk finds it in as many steps.  With `claim` a stale "empty" is settled by the
// CAS, so a lane that has claimed or seen a key finds it again whatever its cache holds; without it the walk uses plain loads and
// belongs in a LATER launch than the claims.
constexpr uint32_t LEAN_WALK = 256u;
struct LeanTable { unsigned long long *key; uint2 *run; uint32_t mask; };   // run: (records of the cell, their first pair)

__device__ __forceinline__ bool lean_probe(const LeanTable &T, unsigned long long key, bool claim, uint32_t &slot, uint32_t &probes)
{
    uint32_t sl = (uint32_t)simp_hash(key) & T.mask;
    for (uint32_t i = 0; i < LEAN_WALK && i <= T.mask; ++i) {
        unsigned long long cur = T.key[sl];              // (a key never changes)
        ++probes;
        if (cur == SIMP_EMPTY) {
            if (!claim) return false;
            cur = atomicCAS(&T.key[sl], SIMP_EMPTY, key);
            if (cur == SIMP_EMPTY) cur = key;
        }
        if (cur == key) { slot = sl; return true; }
        sl = (sl + 1u) & T.mask;
    }
    return false;
}

}  // namespace sm
