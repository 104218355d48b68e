// sm_k_segment.h -- segmentation of a map set into connected voxel components (DESIGN.md "4t. Segmentation"; the specification is
// sm_c_api.h's "segmentation").  Included by sm_segment.hip only.  The grid, the regular-record test, the key, the probe and the
// claim are sm_d_simplify.h's; sm_voxel.hip ranks what a chunk keeps and opens (k_rank_scan) between k_segment_mark and the two
// kernels behind it.  Records come as 48-byte AoS rows (three float4), a chunk of a map file or the exported model.
//   k_segment_insert   reading 1: every node's key claimed in the open-addressing table (64-bit atomicCAS, a probe loop bounded by
//                      the table size); the lanes of a run of equal keys in a wave go together: the run's first lane adds its
//                      length to n, takes its own id for `first` (ids rise with the lanes) and sets parent[slot] = slot
//   k_segment_link     one lane per slot: an occupied slot makes the keys of the forward half of its neighbourhood (3, 9 or 13
//                      offsets; a neighbour cell outside the range is dropped before its key is packed), probes them read-only and
//                      unites itself with each one found.  Union-find on parent[]: only roots are hooked, the larger slot under
//                      the smaller, by compare-and-swap, so parent[x] <= x at all times and no cycle can form; a failed swap goes
//                      on from the value it returned.  Every access to parent[] in this launch is an agent-scope atomic: a plain
//                      load could be served from a stale line of the XCD's own L2.  Path halving by the same compare-and-swap.
//   k_segment_flatten  parent[s] = root(s)
//   k_segment_reduce   every occupied slot adds n, 1, first (min), its cell (min / max per axis) and n * (cell + 65536) to the
//                      planes of its root, in integer atomics.  Lanes of a wave with the root of the first lane still to go are
//                      summed by butterfly shuffles and that lane alone issues the atomics; after SEG_ROUNDS rounds the
//                      leftovers go alone (combine 0: all do)
//   k_segment_mark     reading 2: per record its label kind and code (root slot | SMALL | SKIPPED | LOOSE), the kind counts, the
//                      small components and the largest, and per block of 256 the kept records and the openers -- the record
//                      with the smallest id of a numbered component
//   k_segment_open     every opener at its rank: number[root] = rank, row `rank` of the component table if rank < cap
//   k_segment_label    labels[t] = number[root] or the code; every kept record, verbatim, at its rank (simp_rank_in_chunk)
// No lane waits for another.  Every loop is bounded: a probe walk by the table size, a find walk and a union's retries by the slot
// count; a lane that reaches a bound sets SEG_ERR_STALL in the tally's error word and leaves.  Integer atomics only.
#pragma once

#include "sm_d_simplify.h"

namespace sm {

constexpr uint32_t SEG_LOOSE = 0xFFFFFFFEu, SEG_SMALL = 0xFFFFFFFDu, SEG_SKIPPED = 0xFFFFFFFCu, SEG_NO_RECORD = 0xFFFFFFFFu;
enum { SEG_NUMBERED = 0, SEG_KIND_SMALL = 1, SEG_KIND_SKIPPED = 2, SEG_KIND_LOOSE = 3, SEG_KINDS = 4 };
// the tally's words: the table's (SIMP_RUN of it: the kept records' running rank), a block whose SIMP_RUN is the openers' running
// rank, the counts by kind, the small components, the largest component
enum { SEG_TABLE = 0, SEG_OPEN = SIMP_TALLY_WORDS, SEG_COUNTS = 2 * SIMP_TALLY_WORDS, SEG_SMALL_COMPONENTS = SEG_COUNTS + SEG_KINDS, SEG_LARGEST,
       SEG_TALLY_WORDS };
// bits of the error word beside the claim's 1 (more than max_cells) and 2 (no slot)
constexpr uint32_t SEG_ERR_STALL = 4u, SEG_ERR_CHANGED = 8u;             // a bound was reached; a node of reading 2 is not in the table
constexpr int SEG_ROUNDS = 4;

struct SegArgs {
    uint32_t class_mask[8];
    int by_class;
    int max_l1;                        // 1, 2, 3: connectivity 6, 18, 26
    uint32_t min_records;
    uint32_t write_mask;               // 0: nothing is kept
    int combine;                       // 0: SM_SEGMENT_NO_COMBINE=1
};

// The planes beside the table's key, n and first, of S = mask + 1 slots each; the component planes are used at root slots.  The
// three-component ones hold component k at [k * S + slot].  lo and hi hold cell + 65536.
struct SegPlanes {
    uint32_t *parent;                  // set by the insert
    uint32_t *c_first, *c_lo;          // 0xFFFFFFFF
    uint32_t *c_records, *c_cells, *c_hi;   // 0
    unsigned long long *c_sum;         // 0
    uint32_t *number;                  // written by k_segment_open
};
constexpr size_t SEG_ONES_BYTES = 8 + 4 + 4 + 12, SEG_ZERO_BYTES = 24 + 4 + 4 + 4 + 12, SEG_SLOT_BYTES = SEG_ONES_BYTES + SEG_ZERO_BYTES + 8;

struct SegRow {                        // sm_segment_component
    uint32_t first, records, cells;
    int32_t cls, cell_lo[3], cell_hi[3];
    unsigned long long sum_cell[3];
};
static_assert(sizeof(SegRow) == 64, "a component row has 64 bytes");

// the kind of a record; SEG_NUMBERED: it belongs to the node `key` (numbered or small is decided at its root)
__device__ __forceinline__ uint32_t seg_node(const SimplifyArgs &a, const SegArgs &sa, const float4 &pc, const float4 &ct, const float4 &nr,
                                             unsigned long long &key)
{
    uint32_t off[3];
    if (!simp_classify(a, pc, ct, nr, key, off)) return SEG_KIND_LOOSE;      // (a.split is 0: face 0)
    const uint32_t c = __float_as_uint(ct.x) >> 24;
    uint32_t word = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) word = (c >> 5) == i ? sa.class_mask[i] : word;
    if (!((word >> (c & 31u)) & 1u)) return SEG_KIND_SKIPPED;
    if (!sa.by_class) key &= ~0xFFull;
    return SEG_NUMBERED;
}

__device__ __forceinline__ uint32_t seg_kind_of_code(uint32_t code)
{
    return code < 0x80000000u ? SEG_NUMBERED : code == SEG_SMALL ? SEG_KIND_SMALL : code == SEG_SKIPPED ? SEG_KIND_SKIPPED : SEG_KIND_LOOSE;
}

// ---- reading 1: T has key, n and first
__global__ __launch_bounds__(256) void k_segment_insert(const float4 *__restrict__ rec, uint32_t n, uint32_t gid0, SimplifyArgs a, SegArgs sa,
                                                        SimplifyTable T, uint32_t *__restrict__ parent)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    unsigned long long key = SIMP_EMPTY;
    bool reg = false;
    if (t < n) {
        reg = seg_node(a, sa, rec[(size_t)t * 3], rec[(size_t)t * 3 + 1], rec[(size_t)t * 3 + 2], key) == SEG_NUMBERED;
        if (!reg) key = SIMP_EMPTY;
    }
    const bool head = simp_head(a, key, reg);
    const uint32_t len = (uint32_t)(simp_run_last(reg, head) - (int)(threadIdx.x & 63) + 1);
    simp_claim(a, T, key, head, [&](uint32_t sl) {
        atomicAdd(&T.n[sl], len);
        atomicMin(&T.first[sl], gid0 + t);
        parent[sl] = sl;                                 // (every claimer of the slot stores the same; nobody reads it in this launch)
    });
}

// ---- the union-find.  bound: the slot count; ok false: a bound was reached
__device__ __forceinline__ uint32_t seg_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t seg_cas(uint32_t *p, uint32_t expect, uint32_t v)
{
    __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;                                       // what was there
}

// the root of x's tree as of some moment of the walk; on the way parent[x] is moved to its grandparent (an ancestor stays one)
__device__ __forceinline__ uint32_t seg_find(uint32_t *parent, uint32_t x, uint32_t bound, bool &ok)
{
    for (uint32_t i = 0; i <= bound; ++i) {
        const uint32_t p = seg_load(parent + x);
        if (p == x) return x;
        const uint32_t gp = seg_load(parent + p);
        if (gp != p) seg_cas(parent + x, p, gp);
        x = gp;
    }
    ok = false;
    return x;
}

__device__ __forceinline__ void seg_unite(uint32_t *parent, uint32_t x, uint32_t y, uint32_t bound, bool &ok)
{
    for (uint32_t i = 0; i <= bound && ok; ++i) {
        x = seg_find(parent, x, bound, ok);
        y = seg_find(parent, y, bound, ok);
        if (x == y || !ok) return;
        const uint32_t hi = max(x, y), lo = min(x, y);
        const uint32_t was = seg_cas(parent + hi, hi, lo);
        if (was == hi) return;
        x = lo; y = was;                                 // hi has been hooked meanwhile: on from where it hangs now
    }
    ok = false;
}

__global__ __launch_bounds__(256) void k_segment_link(SimplifyTable T, uint32_t *__restrict__ parent, int max_l1)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    if (sl > T.mask) return;
    const unsigned long long key = T.key[sl];
    if (key == SIMP_EMPTY) return;
    const int u[3] = {(int)((key >> 45) & 0x1FFFFull), (int)((key >> 28) & 0x1FFFFull), (int)((key >> 11) & 0x1FFFFull)};
    const unsigned long long low = key & 0x7FFull;
    bool ok = true;
    // the offsets that follow (0, 0, 0) in the order of j = 9 (dx + 1) + 3 (dy + 1) + (dz + 1): each pair of neighbours once
#pragma unroll 1
    for (int j = 14; j < 27 && ok; ++j) {
        const int d[3] = {j / 9 - 1, (j / 3) % 3 - 1, j % 3 - 1};
        if (abs(d[0]) + abs(d[1]) + abs(d[2]) > max_l1) continue;
        const int v[3] = {u[0] + d[0], u[1] + d[1], u[2] + d[2]};
        if ((v[0] | v[1] | v[2]) < 0 || v[0] > 131071 || v[1] > 131071 || v[2] > 131071) continue;    // no such cell
        const unsigned long long nkey = ((((unsigned long long)v[0] << 17 | (unsigned long long)v[1]) << 17 | (unsigned long long)v[2]) << 11) | low;
        uint32_t nsl;
        bool claimed;
        if (simp_probe(T, nkey, false, nsl, claimed)) seg_unite(parent, sl, nsl, T.mask, ok);
    }
    if (!ok) atomicOr(&T.tally[SIMP_ERR], SEG_ERR_STALL);
}

__global__ __launch_bounds__(256) void k_segment_flatten(SimplifyTable T, uint32_t *__restrict__ parent)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    if (sl > T.mask || T.key[sl] == SIMP_EMPTY) return;
    bool ok = true;
    const uint32_t root = seg_find(parent, sl, T.mask, ok);
    if (!ok) { atomicOr(&T.tally[SIMP_ERR], SEG_ERR_STALL); return; }
    __hip_atomic_store(parent + sl, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the components' sums at their roots
struct SegSums {
    uint32_t records, cells, first, lo[3], hi[3];
    unsigned long long sum[3];
};

__device__ __forceinline__ void seg_add_at_root(const SegPlanes &P, size_t S, uint32_t root, const SegSums &c)
{
    atomicAdd(&P.c_records[root], c.records);
    atomicAdd(&P.c_cells[root], c.cells);
    atomicMin(&P.c_first[root], c.first);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        atomicMin(&P.c_lo[k * S + root], c.lo[k]);
        atomicMax(&P.c_hi[k * S + root], c.hi[k]);
        atomicAdd(&P.c_sum[k * S + root], c.sum[k]);
    }
}

// the wave's sums over the lanes with `mine` (every lane ends with them); the others bring the identities
__device__ __forceinline__ void seg_wave_sums(bool mine, SegSums &c)
{
    if (!mine) {
        c.records = c.cells = 0u; c.first = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < 3; ++k) { c.lo[k] = 0xFFFFFFFFu; c.hi[k] = 0u; c.sum[k] = 0ull; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c.records += __shfl_xor(c.records, o);
        c.cells += __shfl_xor(c.cells, o);
        c.first = min(c.first, __shfl_xor(c.first, o));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c.lo[k] = min(c.lo[k], __shfl_xor(c.lo[k], o));
            c.hi[k] = max(c.hi[k], __shfl_xor(c.hi[k], o));
            c.sum[k] += __shfl_xor(c.sum[k], o);
        }
    }
}

__global__ __launch_bounds__(256) void k_segment_reduce(SimplifyTable T, SegPlanes P, int combine)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const size_t S = (size_t)T.mask + 1u;
    const unsigned long long key = sl <= T.mask ? T.key[sl] : SIMP_EMPTY;
    bool todo = key != SIMP_EMPTY;
    uint32_t root = SEG_NO_RECORD;
    SegSums own{};
    if (todo) {
        root = P.parent[sl];
        own.records = T.n[sl];
        own.cells = 1u;
        own.first = T.first[sl];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            own.lo[k] = own.hi[k] = (uint32_t)((key >> (45 - 17 * k)) & 0x1FFFFull);
            own.sum[k] = (unsigned long long)own.records * own.lo[k];
        }
    }
    for (int round = 0; round < SEG_ROUNDS && combine; ++round) {
        const unsigned long long left = __ballot(todo);
        if (!left) return;
        const int leader = __ffsll(left) - 1;
        const bool mine = todo && root == __shfl(root, leader);
        const unsigned long long same = __ballot(mine);
        if (__popcll(same) > 1) {                        // (wave-uniform)
            SegSums c = own;
            seg_wave_sums(mine, c);
            if (lane == leader) seg_add_at_root(P, S, root, c);
        } else if (lane == leader) {
            seg_add_at_root(P, S, root, own);
        }
        todo = todo && !mine;
    }
    if (todo) seg_add_at_root(P, S, root, own);
}

// ---- reading 2
__global__ __launch_bounds__(256) void k_segment_mark(const float4 *__restrict__ rec, uint32_t n, uint32_t gid0, SimplifyArgs a, SegArgs sa,
                                                      SimplifyTable T, SegPlanes P, uint32_t *__restrict__ code, uint32_t *__restrict__ blk_keep,
                                                      uint32_t *__restrict__ blk_open)
{
    __shared__ uint32_t s_keep[4], s_open[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t kind = SEG_KINDS;                           // (no record)
    bool opener = false, small_first = false;
    if (t < n) {
        unsigned long long key;
        kind = seg_node(a, sa, rec[(size_t)t * 3], rec[(size_t)t * 3 + 1], rec[(size_t)t * 3 + 2], key);
        uint32_t c = kind == SEG_KIND_LOOSE ? SEG_LOOSE : SEG_SKIPPED;
        if (kind == SEG_NUMBERED) {
            uint32_t sl;
            bool claimed;
            if (simp_probe(T, key, false, sl, claimed)) {
                const uint32_t root = P.parent[sl], records = P.c_records[root];
                const bool is_first = P.c_first[root] == gid0 + t;
                if (records >= sa.min_records) { c = root; opener = is_first; }
                else { c = SEG_SMALL; kind = SEG_KIND_SMALL; small_first = is_first; }
                if (is_first) atomicMax(&T.tally[SEG_LARGEST], records);
            } else {                                     // (the set is not the one reading 1 saw)
                atomicOr(&T.tally[SIMP_ERR], SEG_ERR_CHANGED);
                c = SEG_LOOSE; kind = SEG_KIND_LOOSE;
            }
        }
        code[t] = c;
    }
#pragma unroll
    for (uint32_t l = 0; l < SEG_KINDS; ++l) {
        const unsigned long long b = __ballot(kind == l);
        if (b && lane == 0) atomicAdd(&T.tally[SEG_COUNTS + l], (uint32_t)__popcll(b));
    }
    const unsigned long long smalls = __ballot(small_first);
    if (smalls && lane == 0) atomicAdd(&T.tally[SEG_SMALL_COMPONENTS], (uint32_t)__popcll(smalls));
    const unsigned long long kept = __ballot(kind < SEG_KINDS && ((sa.write_mask >> kind) & 1u)), opens = __ballot(opener);
    if (lane == 0) { s_keep[wave] = (uint32_t)__popcll(kept); s_open[wave] = (uint32_t)__popcll(opens); }
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_keep[blockIdx.x] = (s_keep[0] + s_keep[1]) + (s_keep[2] + s_keep[3]);
        blk_open[blockIdx.x] = (s_open[0] + s_open[1]) + (s_open[2] + s_open[3]);
    }
}

// blk_base: the openers' ranks in the whole call (no info: they are not taken relative to the chunk)
__global__ __launch_bounds__(256) void k_segment_open(uint32_t n, uint32_t gid0, const uint32_t *__restrict__ code, SimplifyTable T, SegPlanes P,
                                                      int by_class, const uint32_t *__restrict__ blk_base, uint32_t cap, SegRow *__restrict__ rows)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t root = t < n ? code[t] : SEG_NO_RECORD;
    const bool opener = root < 0x80000000u && P.c_first[root] == gid0 + t;
    const uint32_t rank = simp_rank_in_chunk(opener, blk_base, nullptr);
    if (!opener) return;
    P.number[root] = rank;
    if (rank >= cap) return;
    const size_t S = (size_t)T.mask + 1u;
    SegRow r;
    r.first = gid0 + t;
    r.records = P.c_records[root];
    r.cells = P.c_cells[root];
    r.cls = by_class ? (int32_t)(T.key[root] & 0xFFull) : -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.cell_lo[k] = (int32_t)P.c_lo[k * S + root] - 65536;
        r.cell_hi[k] = (int32_t)P.c_hi[k * S + root] - 65536;
        r.sum_cell[k] = P.c_sum[k * S + root];
    }
    rows[rank] = r;
}

// out[(rank - info->x) * 3 ..]: a chunk's output begins at out (write_mask 0: no output, blk_base and info are not read)
__global__ __launch_bounds__(256) void k_segment_label(const float4 *__restrict__ rec, uint32_t n, const uint32_t *__restrict__ code,
                                                       const uint32_t *__restrict__ number, uint32_t write_mask, uint32_t *__restrict__ label,
                                                       const uint32_t *__restrict__ blk_base, const uint2 *__restrict__ info, float4 *__restrict__ out)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    bool kp = false;
    if (t < n) {
        const uint32_t c = code[t];
        label[t] = c < 0x80000000u ? number[c] : c;
        kp = ((write_mask >> seg_kind_of_code(c)) & 1u) != 0u;
    }
    const uint32_t rank = simp_rank_in_chunk(kp, blk_base, info);
    if (!kp) return;
    out[(size_t)rank * 3] = rec[(size_t)t * 3];
    out[(size_t)rank * 3 + 1] = rec[(size_t)t * 3 + 1];
    out[(size_t)rank * 3 + 2] = rec[(size_t)t * 3 + 2];
}

}  // namespace sm
