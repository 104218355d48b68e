// sm_k_mesh.h -- a map set turned into a triangle mesh (DESIGN.md "4u. Meshing"; the specification is sm_c_api.h's "meshing").
// Included by sm_mesh.hip only.  The grid, the regular-record test, the key, the probe, the run combination and the claim are
// sm_d_simplify.h's; sm_voxel.hip sorts the owners' (key, slot) pairs (pair_sort) and ranks them (k_rank_scan).
// Records come as 48-byte AoS rows (three float4), a chunk of a map file or the exported model.
//   k_mesh_insert    the reading: every USED record's cell claimed in the cell table (64-bit atomicCAS, a probe loop bounded by the
//                    table size); the lanes of a run of equal keys in a wave are summed by a segmented shuffle reduction and the
//                    run's first lane adds n, SW, SP, SN, SC and takes the minimum of cmin (64-bit atomicMin); the kinds counted
//   k_mesh_claim     one lane per cell slot finds the cells that exist; a wave then takes its cells one after the other, its lanes
//                    sharing a cell's 64 (reach 2) or 8 (reach 1) lattice points, each claimed in the lattice table: the lanes of
//                    a step name different points, and a point another cell has claimed is settled by the claim's read of the slot
//   k_mesh_field     one lane per lattice slot: its 8 inner cells probed read-only in the stated order, then, if none exists, its 64
//                    outer cells; F, W, NS, CS and cmin stored
//   k_mesh_cubes     one lane per lattice slot: the 7 other corners probed; a complete cube's 6 tetrahedra classified, its face
//                    count stored and the kinds of the cut edges ORed into `used` of the corner that owns them (atomicOr; read by
//                    the next launch only)
//   k_mesh_owners    the slots that own a vertex or a face as (key >> 11, slot) pairs, in any order, with the OR and the AND of
//                    their keys; a workgroup of 256 takes 4096 slots and reserves its pairs' places with one atomic
//   k_mesh_count     per block of 256 sorted owners their vertices and faces (two planes of block counts), and the 64-bit totals
//   k_mesh_base      every owner's first vertex and first face: the block's rank plus the owners before it in the block
//   k_mesh_vertices  one lane per lattice slot: its vertices, in ascending kind, at vbase
//   k_mesh_faces     one lane per lattice slot: its cube's triangles, in (tetrahedron, triangle) order, at fbase; a vertex's index
//                    is its owner's vbase plus the used kinds below its own
// No lane waits for another.  Every probe walk ends at the key, at an empty slot or after mask + 1 slots.  Integer atomics only.
#pragma once

#include "sm_d_simplify.h"

namespace sm {

enum { MESH_USED = 0, MESH_SKIPPED, MESH_LOOSE, MESH_OUTSIDE, MESH_KINDS };
// the tally's words: the cell table's block, the lattice table's, the vertices' and the faces' (SIMP_RUN of each: the running
// rank), the records by kind, the cells that exist, the cubes meshed, the owners listed, then four 64-bit values
enum { MESH_CELL = 0, MESH_LAT = SIMP_TALLY_WORDS, MESH_VRUN = 2 * SIMP_TALLY_WORDS, MESH_FRUN = 3 * SIMP_TALLY_WORDS,
       MESH_COUNTS = 4 * SIMP_TALLY_WORDS, MESH_EXIST = MESH_COUNTS + MESH_KINDS, MESH_CUBES, MESH_OWNERS, MESH_PAD,
       MESH_VTOTAL, MESH_FTOTAL = MESH_VTOTAL + 2, MESH_OR = MESH_FTOTAL + 2, MESH_AND = MESH_OR + 2, MESH_TALLY_WORDS = MESH_AND + 2 };
static_assert(MESH_VTOTAL % 2 == 0, "the 64-bit values are aligned");

struct MeshArgs {
    uint32_t class_mask[8];
    int reach;                         // 1 or 2
    uint32_t min_records;
};

// The cell table beside SimplifyTable's key, SW, SP, SN, SC and n: cmin.  Bytes per slot, planes of all ones first:
constexpr size_t MESH_CELL_ONES = 8 + 8, MESH_CELL_ZERO = 8 * 10 + 4;

// The lattice table, planes of S = mask + 1 slots; the three-component ones hold component k at [k * S + slot]
struct MeshLattice {
    unsigned long long *key;           // SIMP_EMPTY; the simplification's packing of l + 65536, face and class 0
    double *F;
    unsigned long long *W, *NS, *CS, *cmin;   // written by k_mesh_field for every sampled point
    uint32_t *faces;                   // written by k_mesh_cubes for every sampled point
    uint32_t *used;                    // 0; bit `kind` (1..7): the edge of that kind from this point carries a vertex
    uint32_t *vbase, *fbase;           // written by k_mesh_base for every owner
    uint32_t mask;
    uint32_t *tally;                   // the whole tally
};
constexpr size_t MESH_LAT_BYTES = 8 + 8 + 8 + 24 + 24 + 8 + 4 * 4;

struct MeshVertex { float pos[3], normal[3]; uint32_t colour; };   // sm_mesh_vertex
static_assert(sizeof(MeshVertex) == 28, "a vertex has 28 bytes");

// the lattice table as the probe and the claim see it: keys, and the lattice block of the tally
__device__ __forceinline__ SimplifyTable mesh_lat_table(const MeshLattice &L)
{
    SimplifyTable T{};
    T.key = L.key; T.mask = L.mask; T.tally = L.tally + MESH_LAT;
    return T;
}

// the key of the cell or lattice point u (each component in 0..131071)
__device__ __forceinline__ unsigned long long mesh_key(const int u[3])
{
    return ((((unsigned long long)u[0] << 17 | (unsigned long long)u[1]) << 17 | (unsigned long long)u[2]) << 11);
}
__device__ __forceinline__ void mesh_unkey(unsigned long long key, int u[3])
{
    u[0] = (int)((key >> 45) & 0x1FFFFull); u[1] = (int)((key >> 28) & 0x1FFFFull); u[2] = (int)((key >> 11) & 0x1FFFFull);
}
__device__ __forceinline__ bool mesh_on_grid(const int u[3]) { return (u[0] | u[1] | u[2]) >= 0 && u[0] <= 131071 && u[1] <= 131071 && u[2] <= 131071; }

// ---- the reading
struct MeshContrib {
    uint32_t n;
    unsigned long long sw, sp[3], sc[3], cmin;
    long long sn[3];
};

// lane `lane` takes lane + o's sums when that lane belongs to its run (simp_take, for what a cell of the mesh holds)
__device__ __forceinline__ void mesh_take(MeshContrib &c, int o, bool take)
{
#define MESH_ADD(x) { const auto v_ = __shfl_down(x, o); if (take) x += v_; }
    MESH_ADD(c.n) MESH_ADD(c.sw)
#pragma unroll
    for (int k = 0; k < 3; ++k) { MESH_ADD(c.sp[k]) MESH_ADD(c.sn[k]) MESH_ADD(c.sc[k]) }
#undef MESH_ADD
    const unsigned long long m = __shfl_down(c.cmin, o);
    if (take) c.cmin = min(c.cmin, m);
}

__global__ __launch_bounds__(256) void k_mesh_insert(const float4 *__restrict__ rec, uint32_t n, uint32_t gid0, SimplifyArgs a, MeshArgs ma,
                                                     SimplifyTable T, unsigned long long *__restrict__ cmin)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned long long key = SIMP_EMPTY;
    uint32_t kind = MESH_KINDS;                          // (no record)
    MeshContrib c{};
    if (t < n) {
        const float4 pc = rec[(size_t)t * 3], ct = rec[(size_t)t * 3 + 1], nr = rec[(size_t)t * 3 + 2];
        uint32_t off[3];
        if (!simp_classify(a, pc, ct, nr, key, off)) {   // (a.split is 0: face 0)
            kind = MESH_LOOSE;
        } else {
            const uint32_t cls = __float_as_uint(ct.x) >> 24;
            uint32_t word = 0;
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) word = (cls >> 5) == i ? ma.class_mask[i] : word;
            int u[3];
            mesh_unkey(key, u);
            const int lo = ma.reach, hi = 131071 - ma.reach;
            if (!((word >> (cls & 31u)) & 1u)) kind = MESH_SKIPPED;
            else if (u[0] < lo || u[1] < lo || u[2] < lo || u[0] > hi || u[1] > hi || u[2] > hi) kind = MESH_OUTSIDE;
            else {
                kind = MESH_USED;
                SimpContrib sc;
                simp_contribution(pc, ct, nr, off, 0u, sc);
                c.n = 1u; c.sw = sc.sw;
#pragma unroll
                for (int k = 0; k < 3; ++k) { c.sp[k] = sc.sp[k]; c.sn[k] = sc.sn[k]; c.sc[k] = sc.sc[k]; }
                c.cmin = ((unsigned long long)(gid0 + t) << 8) | cls;
                key &= ~0x7FFull;                        // no face, no class
            }
        }
    }
    const bool reg = kind == MESH_USED;
    if (!reg) key = SIMP_EMPTY;
    const bool head = simp_head(a, key, reg);
    if (__ballot(reg && !head)) {                        // wave-uniform: some run in this wave is longer than one lane
        const int last = simp_run_last(reg, head);
        for (int o = 1; o < 64; o <<= 1) {
            const bool take = lane + o <= last;
            if (!__ballot(take)) break;
            mesh_take(c, o, take);
        }
    }
    simp_claim(a, T, key, head, [&](uint32_t sl) {
        const size_t S = (size_t)T.mask + 1u;
        atomicAdd(&T.n[sl], c.n);
        atomicAdd(&T.SW[sl], c.sw);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicAdd(&T.SP[k * S + sl], c.sp[k]);
            atomicAdd(&T.SN[k * S + sl], (unsigned long long)c.sn[k]);
            atomicAdd(&T.SC[k * S + sl], c.sc[k]);
        }
        atomicMin(&cmin[sl], c.cmin);
    });
#pragma unroll
    for (uint32_t l = 0; l < MESH_KINDS; ++l) {
        const unsigned long long b = __ballot(kind == l);
        if (b && lane == 0) atomicAdd(&T.tally[MESH_COUNTS + l], (uint32_t)__popcll(b));
    }
}

constexpr uint32_t MESH_CLAIM_WALK = 1024u;             // the longest probe walk of a claim in the lattice table

// ---- the lattice points.  al: the grid with max_cells = the points the lattice table may hold; count_exist: the first attempt
__global__ __launch_bounds__(256) void k_mesh_claim(SimplifyTable T, MeshArgs ma, SimplifyArgs al, MeshLattice L, int count_exist)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const SimplifyTable TL = mesh_lat_table(L);
    const unsigned long long key = sl <= T.mask ? T.key[sl] : SIMP_EMPTY;
    const bool exists = key != SIMP_EMPTY && T.n[sl] >= ma.min_records;
    const unsigned long long b = __ballot(exists);
    // The table is sparse: a wave holds few cells.  Its cells go one after the other and the lanes share a cell's points -- 64 lanes
    // the 64 points of reach 2, 8 lanes the 8 of reach 1 --, so the lanes of a step name different points (wave-uniform loop: the
    // claim's ballots see whole waves).  The lattice table may be too small (the host then claims again in a larger one): no walk
    // is longer than MESH_CLAIM_WALK slots, so a table that fills costs a lane a bounded walk, never the table's length; and
    // before every fourth step a wave reads the table's error word and stops if it is set.  Not before every step: that word is
    // one address, and a read of it by every wave of a sparse cell table, where a wave has one step, doubled the kernel's time
    // (3.10 against 1.49 ms on the street map at 100 mm)
    int step = 0;
    for (unsigned long long todo = b; todo; todo &= todo - 1ull, ++step) {
        if ((step & 3) == 3 && __ballot(__hip_atomic_load(&TL.tally[SIMP_ERR], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) break;   // (wave-uniform)
        int u[3];
        mesh_unkey(__shfl(key, __ffsll(todo) - 1), u);
        const bool mine = ma.reach == 2 || lane < 8;
        const int v[3] = {ma.reach == 2 ? u[0] - 1 + (lane >> 4) : u[0] + ((lane >> 2) & 1), ma.reach == 2 ? u[1] - 1 + ((lane >> 2) & 3) : u[1] + ((lane >> 1) & 1),
                          ma.reach == 2 ? u[2] - 1 + (lane & 3) : u[2] + (lane & 1)};
        // (on the grid: a USED record's cell keeps `reach` from its edge)
        simp_claim(al, TL, mine ? mesh_key(v) : SIMP_EMPTY, mine, [](uint32_t) {}, MESH_CLAIM_WALK);
    }
    if (count_exist && b && lane == 0) atomicAdd(&T.tally[MESH_EXIST], (uint32_t)__popcll(b));
}

// ---- the field
struct MeshSums {
    double F;
    unsigned long long W, CS[3], cmin;
    long long NS[3];
    bool any;
};

// the cell at l + d, if it exists, into the sums
__device__ __forceinline__ void mesh_add_cell(const SimplifyArgs &a, const MeshArgs &ma, const SimplifyTable &T, const unsigned long long *__restrict__ cmin,
                                              const int l[3], int dx, int dy, int dz, MeshSums &m)
{
    const int d[3] = {dx, dy, dz};
    const int u[3] = {l[0] + dx, l[1] + dy, l[2] + dz};
    if (!mesh_on_grid(u)) return;                        // no such cell
    uint32_t sl;
    bool claimed;
    if (!simp_probe(T, mesh_key(u), false, sl, claimed) || T.n[sl] < ma.min_records) return;
    const size_t S = (size_t)T.mask + 1u;
    const unsigned long long SW = T.SW[sl];
    long long sn[3];
    double e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long mp = (long long)((T.SP[k * S + sl] + SW / 2) / SW);
        e[k] = (double)((long long)(-d[k]) * a.V - mp);
        sn[k] = (long long)T.SN[k * S + sl];
        m.NS[k] += sn[k];
        m.CS[k] += T.SC[k * S + sl];
    }
    m.W += SW;
    m.cmin = min(m.cmin, cmin[sl]);
    m.any = true;
    float nn[3];
    if (simp_merged_normal(sn, nn)) m.F += (double)SW * (((double)nn[0] * e[0] + (double)nn[1] * e[1]) + (double)nn[2] * e[2]);
}

__global__ __launch_bounds__(256) void k_mesh_field(SimplifyArgs a, MeshArgs ma, SimplifyTable T, const unsigned long long *__restrict__ cmin, MeshLattice L)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    if (sl > L.mask) return;
    const unsigned long long key = L.key[sl];
    if (key == SIMP_EMPTY) return;
    int l[3];
    mesh_unkey(key, l);
    MeshSums m{};
    m.cmin = ~0ull;
    // ascending lexicographic order of c - l
#pragma unroll 1
    for (int j = 0; j < 8; ++j) mesh_add_cell(a, ma, T, cmin, l, (j >> 2) - 1, ((j >> 1) & 1) - 1, (j & 1) - 1, m);
    if (!m.any && ma.reach == 2) {
#pragma unroll 1
        for (int j = 0; j < 64; ++j) mesh_add_cell(a, ma, T, cmin, l, (j >> 4) - 2, ((j >> 2) & 3) - 2, (j & 3) - 2, m);
    }
    const size_t S = (size_t)L.mask + 1u;
    L.F[sl] = m.F;
    L.W[sl] = m.W;
    L.cmin[sl] = m.cmin;
#pragma unroll
    for (int k = 0; k < 3; ++k) { L.NS[k * S + sl] = (unsigned long long)m.NS[k]; L.CS[k * S + sl] = m.CS[k]; }
}

// ---- the cubes
// the corners of Kuhn tetrahedron t as cube-corner masks b0 + 2 b1 + 4 b2, corner i in bits 4 i .. 4 i + 3: per permutation (a, b, c)
// of the axes, in lexicographic order, 0, e_a, e_a + e_b, 7, the last two exchanged for an odd permutation
__device__ __forceinline__ uint32_t mesh_tet(int t)
{
    return t == 0 ? 0x7310u : t == 1 ? 0x5710u : t == 2 ? 0x3720u : t == 3 ? 0x7620u : t == 4 ? 0x7540u : 0x6740u;
}

// the slots of the cube's corners at the lattice point u of slot sl, and which are inside; false: a corner is not sampled
__device__ __forceinline__ bool mesh_cube(const MeshLattice &L, const int u[3], uint32_t sl, uint32_t cs[8], uint32_t &in8)
{
    const SimplifyTable TL = mesh_lat_table(L);
    cs[0] = sl;
    bool complete = true;
#pragma unroll
    for (int b = 1; b < 8; ++b) {
        cs[b] = 0u;
        const int v[3] = {u[0] + (b & 1), u[1] + ((b >> 1) & 1), u[2] + ((b >> 2) & 1)};
        bool claimed;
        complete = complete && mesh_on_grid(v) && simp_probe(TL, mesh_key(v), false, cs[b], claimed);
    }
    in8 = 0u;
    if (!complete) return false;
#pragma unroll
    for (int b = 0; b < 8; ++b) in8 |= (L.F[cs[b]] < 0.0 ? 1u : 0u) << b;
    return true;
}

// which of the tetrahedron's corners are inside: bit i for corner i
__device__ __forceinline__ uint32_t mesh_tet_mask(uint32_t tc, uint32_t in8)
{
    uint32_t m4 = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) m4 |= ((in8 >> ((tc >> (4 * i)) & 15u)) & 1u) << i;
    return m4;
}

__global__ __launch_bounds__(256) void k_mesh_cubes(MeshLattice L)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned long long key = sl <= L.mask ? L.key[sl] : SIMP_EMPTY;
    const bool has = key != SIMP_EMPTY;
    bool complete = false;
    if (has) {
        int u[3];
        mesh_unkey(key, u);
        uint32_t cs[8], in8;
        complete = mesh_cube(L, u, sl, cs, in8);
        uint32_t faces = 0u;
        if (complete) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int pc = __popc(mesh_tet_mask(mesh_tet(t), in8));
                faces += pc == 2 ? 2u : (pc == 1 || pc == 3) ? 1u : 0u;
            }
            // the 19 edges of the six tetrahedra are the pairs (a, a + d) with a & d == 0: one is cut iff its ends differ
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                uint32_t bits = 0u;
#pragma unroll
                for (int d = 1; d < 8; ++d)
                    if ((c & d) == 0 && (((in8 >> c) ^ (in8 >> (c | d))) & 1u)) bits |= 1u << d;
                if (bits) atomicOr(&L.used[cs[c]], bits);
            }
        }
        L.faces[sl] = faces;
    }
    const unsigned long long b = __ballot(complete);
    if (b && lane == 0) atomicAdd(&L.tally[MESH_CUBES], (uint32_t)__popcll(b));
}

// ---- the owners.  cap: the pairs key and idx hold.  A workgroup takes MESH_OWNERS_BLOCK slots, 16 a lane, and reserves the places of
// its owners with one atomic: a wave's worth of slots per atomic on one address was the slowest step of the call
constexpr uint32_t MESH_OWNERS_BLOCK = 4096u;

// the exclusive prefix of v over the workgroup of 256 (all of its lanes call it); s_w: four words of LDS of its own
__device__ __forceinline__ uint32_t mesh_block_excl(uint32_t v, uint32_t *s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = inc - v;
    for (int x = 0; x < wave; ++x) before += s_w[x];
    return before;
}

__global__ __launch_bounds__(256) void k_mesh_owners(MeshLattice L, uint32_t cap, unsigned long long *__restrict__ key, uint32_t *__restrict__ idx)
{
    __shared__ uint32_t s_w[4], s_base;
    __shared__ unsigned long long s_or, s_and;
    const int lane = threadIdx.x & 63;
    const uint32_t first = blockIdx.x * MESH_OWNERS_BLOCK + threadIdx.x;
    if (threadIdx.x == 0) { s_or = 0ull; s_and = ~0ull; }
    uint32_t owns = 0u;                                  // bit r: slot first + 256 r owns a vertex or a face
    unsigned long long o = 0ull, d = ~0ull;
#pragma unroll
    for (uint32_t r = 0; r < MESH_OWNERS_BLOCK / 256u; ++r) {
        const uint32_t sl = first + r * 256u;
        if (sl > L.mask) continue;
        const unsigned long long k = L.key[sl];
        if (k == SIMP_EMPTY || (L.used[sl] | L.faces[sl]) == 0u) continue;
        owns |= 1u << r;
        o |= k >> 11; d &= k >> 11;                      // 51 bits: what the pair sort orders
    }
    const uint32_t before = mesh_block_excl((uint32_t)__popc(owns), s_w);            // (a barrier: s_or and s_and are set)
#pragma unroll
    for (int x = 32; x; x >>= 1) { o |= __shfl_xor(o, x); d &= __shfl_xor(d, x); }
    if (lane == 0 && o) { atomicOr(&s_or, o); atomicAnd(&s_and, d); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        s_base = total ? atomicAdd(&L.tally[MESH_OWNERS], total) : 0u;
        if (total) {
            // (OR only grows and AND only shrinks, so a value read earlier that already holds this workgroup's bits settles it)
            unsigned long long *bits_or = (unsigned long long *)(L.tally + MESH_OR), *bits_and = (unsigned long long *)(L.tally + MESH_AND);
            const unsigned long long seen_or = __atomic_load_n(bits_or, __ATOMIC_RELAXED), seen_and = __atomic_load_n(bits_and, __ATOMIC_RELAXED);
            if ((seen_or | s_or) != seen_or) atomicOr(bits_or, s_or);
            if ((seen_and & s_and) != seen_and) atomicAnd(bits_and, s_and);
        }
    }
    __syncthreads();
    uint32_t at = s_base + before;
#pragma unroll
    for (uint32_t r = 0; r < MESH_OWNERS_BLOCK / 256u; ++r) {
        if (!((owns >> r) & 1u)) continue;
        const uint32_t sl = first + r * 256u;
        if (at < cap) { key[at] = L.key[sl] >> 11; idx[at] = sl; }
        ++at;
    }
}

// the sorted owners [first, first + m) of idx: their vertices in plane 0 of the block counts, their faces in plane 1
__global__ __launch_bounds__(256) void k_mesh_count(MeshLattice L, const uint32_t *__restrict__ idx, uint32_t first, uint32_t m, uint32_t *__restrict__ blk_v,
                                                    uint32_t *__restrict__ blk_f)
{
    __shared__ uint32_t s_v[4], s_f[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t nv = 0u, nf = 0u;
    if (i < m) {
        const uint32_t sl = idx[first + i];
        nv = (uint32_t)__popc(L.used[sl]);
        nf = L.faces[sl];
    }
#pragma unroll
    for (int x = 32; x; x >>= 1) { nv += __shfl_xor(nv, x); nf += __shfl_xor(nf, x); }
    if (lane == 0) {
        s_v[wave] = nv; s_f[wave] = nf;
        if (nv) atomicAdd((unsigned long long *)(L.tally + MESH_VTOTAL), (unsigned long long)nv);
        if (nf) atomicAdd((unsigned long long *)(L.tally + MESH_FTOTAL), (unsigned long long)nf);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_v[blockIdx.x] = (s_v[0] + s_v[1]) + (s_v[2] + s_v[3]);
        blk_f[blockIdx.x] = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
    }
}

__global__ __launch_bounds__(256) void k_mesh_base(MeshLattice L, const uint32_t *__restrict__ idx, uint32_t first, uint32_t m, const uint32_t *__restrict__ base_v,
                                                   const uint32_t *__restrict__ base_f)
{
    __shared__ uint32_t s_v[4], s_f[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t sl = 0u, nv = 0u, nf = 0u;
    if (i < m) {
        sl = idx[first + i];
        nv = (uint32_t)__popc(L.used[sl]);
        nf = L.faces[sl];
    }
    const uint32_t bv = mesh_block_excl(nv, s_v), bf = mesh_block_excl(nf, s_f);
    if (i < m) { L.vbase[sl] = base_v[blockIdx.x] + bv; L.fbase[sl] = base_f[blockIdx.x] + bf; }
}

// ---- the vertices.  nv: the rows at out
__global__ __launch_bounds__(256) void k_mesh_vertices(SimplifyArgs a, MeshLattice L, uint32_t nv, MeshVertex *__restrict__ out)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    if (sl > L.mask) return;
    const unsigned long long key = L.key[sl];
    if (key == SIMP_EMPTY) return;
    const uint32_t used = L.used[sl];
    if (!used) return;
    const SimplifyTable TL = mesh_lat_table(L);
    const size_t S = (size_t)L.mask + 1u;
    int u[3];
    mesh_unkey(key, u);
    const double Fa = L.F[sl];
    const unsigned long long Wa = L.W[sl], ca = L.cmin[sl];
    uint32_t at = L.vbase[sl];
#pragma unroll 1
    for (uint32_t kind = 1; kind < 8; ++kind) {
        if (!((used >> kind) & 1u)) continue;
        const int d[3] = {(int)(kind & 1u), (int)((kind >> 1) & 1u), (int)((kind >> 2) & 1u)};
        const int v[3] = {u[0] + d[0], u[1] + d[1], u[2] + d[2]};
        uint32_t b;
        bool claimed;
        if (!mesh_on_grid(v) || !simp_probe(TL, mesh_key(v), false, b, claimed)) continue;   // (a used edge's other end is sampled)
        const unsigned long long Wb = L.W[b], W = Wa + Wb;
        const double A = Fa * (double)Wb, B = L.F[b] * (double)Wa;
        const double t = A / (A - B);
        MeshVertex r;
        long long ns[3];
        uint32_t col = (uint32_t)(min(ca, L.cmin[b]) & 255ull) << 24;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const long long lk = (long long)(u[k] - 65536) * a.V, dk = (long long)d[k] * a.V;
            r.pos[k] = (float)((double)a.origin[k] + ((double)lk + t * (double)dk) * (1.0 / 65536.0));
            ns[k] = (long long)L.NS[k * S + sl] + (long long)L.NS[k * S + b];
            col |= (uint32_t)(((L.CS[k * S + sl] + L.CS[k * S + b]) + W / 2) / W) << (8 * k);
        }
        float nn[3] = {0.0f, 0.0f, 0.0f};
        (void)simp_merged_normal(ns, nn);
        r.normal[0] = nn[0]; r.normal[1] = nn[1]; r.normal[2] = nn[2];
        r.colour = col;
        if (at < nv) out[at] = r;
        ++at;
    }
}

// ---- the faces
__device__ __forceinline__ uint32_t mesh_sel8(const uint32_t (&v)[8], uint32_t i)
{
    uint32_t r = v[0];
#pragma unroll
    for (uint32_t k = 1; k < 8; ++k) r = i == k ? v[k] : r;
    return r;
}

// The triangles of a tetrahedron whose corners with their bit in m4 are inside: their number; triangle j's three edges in
// e[j], edge i in bits 8 i .. 8 i + 7 as (x << 4) | y, x and y corners of the tetrahedron
__device__ __forceinline__ int mesh_tet_faces(uint32_t m4, uint32_t e[2])
{
    const int pc = __popc(m4);
    if (pc == 0 || pc == 4) return 0;
    const auto edge = [](uint32_t x, uint32_t y) { return (x << 4) | y; };
    if (pc == 2) {
        const uint32_t outs = ~m4 & 15u;
        const uint32_t i = (uint32_t)__ffs(m4) - 1u, j = 31u - (uint32_t)__clz(m4);
        uint32_t k = (uint32_t)__ffs(outs) - 1u, l = 31u - (uint32_t)__clz(outs);
        if (m4 == 5u || m4 == 10u) { const uint32_t x = k; k = l; l = x; }           // (i, j, k, l) = (0, 2, 1, 3), (1, 3, 0, 2): odd
        e[0] = edge(i, k) | edge(i, l) << 8 | edge(j, l) << 16;
        e[1] = edge(i, k) | edge(j, l) << 8 | edge(j, k) << 16;
        return 2;
    }
    const uint32_t lone = pc == 1 ? m4 : (~m4 & 15u);
    const uint32_t i = (uint32_t)__ffs(lone) - 1u, rest = 15u ^ lone;
    const uint32_t j = (uint32_t)__ffs(rest) - 1u;
    uint32_t l = 31u - (uint32_t)__clz(rest), k = (uint32_t)__ffs(rest & ~(1u << j)) - 1u;
    if (i & 1u) { const uint32_t x = k; k = l; l = x; }                              // (i, j, k, l) is odd iff i is
    e[0] = pc == 1 ? (edge(i, j) | edge(i, k) << 8 | edge(i, l) << 16) : (edge(i, l) | edge(i, k) << 8 | edge(i, j) << 16);
    return 1;
}

// nf: the rows (of three indices) at out
__global__ __launch_bounds__(256) void k_mesh_faces(MeshLattice L, uint32_t nf, uint32_t *__restrict__ out)
{
    const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
    if (sl > L.mask) return;
    const unsigned long long key = L.key[sl];
    if (key == SIMP_EMPTY || !L.faces[sl]) return;
    int u[3];
    mesh_unkey(key, u);
    uint32_t cs[8], in8;
    if (!mesh_cube(L, u, sl, cs, in8)) return;           // (a point with faces has its cube)
    uint32_t vb[8], us[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) { vb[b] = L.vbase[cs[b]]; us[b] = L.used[cs[b]]; }
    uint32_t at = L.fbase[sl];
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {
        const uint32_t tc = mesh_tet(t);
        uint32_t e[2] = {0u, 0u};
        const int tris = mesh_tet_faces(mesh_tet_mask(tc, in8), e);
        for (int j = 0; j < tris; ++j) {
            uint32_t v[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint32_t xy = ((j ? e[1] : e[0]) >> (8 * i)) & 255u;
                const uint32_t p = (tc >> (4 * (xy >> 4))) & 15u, q = (tc >> (4 * (xy & 15u))) & 15u;
                const uint32_t lower = min(p, q), kind = p ^ q;                       // (one corner's mask contains the other's)
                v[i] = mesh_sel8(vb, lower) + (uint32_t)__popc(mesh_sel8(us, lower) & ((1u << kind) - 1u));
            }
            // the smallest index first
            const int r = (v[1] < v[0] && v[1] <= v[2]) ? 1 : (v[2] < v[0] && v[2] < v[1]) ? 2 : 0;
            const uint32_t w0 = r == 0 ? v[0] : r == 1 ? v[1] : v[2], w1 = r == 0 ? v[1] : r == 1 ? v[2] : v[0], w2 = r == 0 ? v[2] : r == 1 ? v[0] : v[1];
            if (at < nf) { out[(size_t)at * 3] = w0; out[(size_t)at * 3 + 1] = w1; out[(size_t)at * 3 + 2] = w2; }
            ++at;
        }
    }
}

}  // namespace sm
