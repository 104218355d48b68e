// sm_k_locate.h -- one map set located in another without a guess (DESIGN.md "4ab. Locating"; the specification is sm_c_api.h's
// "locating one map set in another").  Included by sm_locate.hip only.  The regular-record test, the quantised normal and the run
// logic of neighbouring lanes are sm_d_simplify.h's, as in sm_k_ground.h.  Records come as 48-byte AoS rows (three float4).
//   k_locate_raster    one reading of a set: a structure-like record adds to its cell's count, a ground-like one lowers its cell's
//                      height.  The lanes of a run of equal cells in a wave go together: the run's first lane adds the run's length
//                      and issues one atomicMin of the run's minimum.  The target's planes are the window's, row-major; the source's
//                      span the 8191 x 8191 cells about source_origin.  The counts by kind go to the tally, one add per wave and kind
//   k_locate_count / k_locate_scan / k_locate_emit
//                      the source's planes compacted in (cv, cu) order into S (cells with min_records) and G (cells with ground):
//                      flags per block of 256 cells, one workgroup ranks the blocks, every block writes its cells at its rank
//   k_locate_rotate    the rotated cell of every cell of S under every coarse row, two int16 a word
//   k_locate_occ       occ = (count >= min_records) dilated, one byte a cell; the occupied cells to the tally
//   k_locate_pyramid   level h from level h - 1: P_h[v][u] = max of occ over [u, u + 2^h) x [v, v + 2^h), u from -(2^h - 1) on, cells outside
//                      the window 0
//   k_locate_bound     one wave per node (k, du0, dv0, h): the lanes stride over S, each reads P_h at its rotated cell plus the node's
//                      corner; the wave's sum bounds every score of the node's 2^h x 2^h offsets from above
//   k_locate_tiles     one wave per node of 8 x 8 offsets: lane = offset, the cells of S wave-uniform (scalar loads), one byte of occ a
//   k_locate_all       step and lane, the sum in a register; the wave's best (score, smallest key) by a shuffle maximum.  _all is the
//                      exhaustive form: every 64 x 1 strip of every coarse row, the best into one word by a 64-bit atomicMax per wave
//   k_locate_refine    one wave per fine row around the winner, nine lanes: the nine offsets' scores, the rotation computed per cell
//   k_locate_height    one lane per cell of G: Zt - Zs where the moved cell has ground, else LOCATE_NO_PAIR
// No lane waits for another; every loop has a fixed bound.  Integer atomics only.  Every index is checked against its plane before
// it is used.
#pragma once

#include "sm_d_simplify.h"

namespace sm {

constexpr int LOCATE_SPAN = 4095, LOCATE_SW = 2 * LOCATE_SPAN + 1;   // the source's cells: |cu|, |cv| <= 4095
constexpr int LOCATE_NO_Z = 0x7F7F7F7F;                  // a cell without ground (a memset's bytes; above every H: |H| < 2^30)
constexpr int LOCATE_NO_PAIR = (int)0x80000000;
enum { LOCATE_K_STRUCTURE = 0, LOCATE_K_GROUND, LOCATE_K_OTHER, LOCATE_K_OUTSIDE, LOCATE_K_LOOSE, LOCATE_KINDS };
// the tally's words: the records by kind of the source (side 1) at 8 .., of the target (side 0) at 0 ..; the occupied cells
enum { LOCATE_COUNTS = 0, LOCATE_OCC = 16, LOCATE_TALLY_WORDS = 24 };
constexpr int LOCATE_MAX_LEVELS = 13;                    // pyramid levels 0..12
constexpr int LOCATE_LEAF = 3;                           // a node of 2^3 x 2^3 offsets is scored offset by offset
constexpr unsigned long long LOCATE_KEY_MAX = (1ull << 40) - 1;

struct LocateArgs {
    long long C;                       // the cell edge in 2^-16 m
    float origin[2][3];                // [0] the target's, [1] the source's
    int a, ua, va, sgn;                // the up axis, the horizontal ones, +1 / -1
    int nsgn;                          // sgn * normal_sign
    int nu, nv;
    int max_up, min_up;
    uint32_t smask[8], gmask[8];
    uint32_t min_records;
    int dilate;
};

// a pyramid level: W x H bytes, entry (u + off, v + off)
struct LocateLevel { const uint8_t *p; int W, H, off; };
struct LocateLevels { LocateLevel l[LOCATE_MAX_LEVELS]; };

// what the searches share: the range, the exclusion of the runner-up's search (ex_on 0: none)
struct LocateSearch {
    const uint32_t *rot;               // [k * n_s + i]: ru & 0xFFFF | rv << 16
    uint32_t n_s;
    int R, nu, nv;                     // du in [-R, nu - 1 + R], dv in [-R, nv - 1 + R]
    int n_yaw;
    int ex_on, ex_k, ex_du, ex_dv, sep_yaw, sep_cells;
};

struct LocateNode { int k, du0, dv0, h; };

__device__ __forceinline__ long long locate_pick(int k, long long x0, long long x1, long long x2) { return k == 0 ? x0 : k == 1 ? x1 : x2; }
__device__ __forceinline__ long long locate_floor_div(long long x, long long c)
{
    long long q = x / c;
    if (x - q * c < 0) --q;
    return q;
}
__device__ __forceinline__ bool locate_bit(const uint32_t *mask, uint32_t c)
{
    uint32_t word = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) word = (c >> 5) == i ? mask[i] : word;
    return (word >> (c & 31u)) & 1u;
}

// Where a record lies: its kind; for the first three `cell` (in the side's plane), H, structure-like, ground-like
__device__ __forceinline__ int locate_place(const LocateArgs &g, int side, const float4 &pc, const float4 &ct, const float4 &nr, uint32_t &cell, int &H,
                                            bool &st, bool &gd)
{
    st = gd = false;
    if (!simp_fields_ok(pc, ct, nr)) return LOCATE_K_LOOSE;
    const float *o = g.origin[side];
    const double d0 = (double)pc.x - (double)o[0], d1 = (double)pc.y - (double)o[1], d2 = (double)pc.z - (double)o[2];
    if (!(fabs(d0) < 16777216.0) || !(fabs(d1) < 16777216.0) || !(fabs(d2) < 16777216.0)) return LOCATE_K_LOOSE;
    const long long X0 = (long long)floor(d0 * 65536.0), X1 = (long long)floor(d1 * 65536.0), X2 = (long long)floor(d2 * 65536.0);
    const long long cu = locate_floor_div(locate_pick(g.ua, X0, X1, X2), g.C), cv = locate_floor_div(locate_pick(g.va, X0, X1, X2), g.C);
    const long long Hl = (long long)g.sgn * locate_pick(g.a, X0, X1, X2);
    if (Hl >= (1ll << 30) || Hl <= -(1ll << 30)) return LOCATE_K_OUTSIDE;
    if (side == 0) {
        if (cu < 0 || cu >= g.nu || cv < 0 || cv >= g.nv) return LOCATE_K_OUTSIDE;
        cell = (uint32_t)(cv * g.nu + cu);
    } else {
        if (cu < -LOCATE_SPAN || cu > LOCATE_SPAN || cv < -LOCATE_SPAN || cv > LOCATE_SPAN) return LOCATE_K_OUTSIDE;
        cell = (uint32_t)((cv + LOCATE_SPAN) * LOCATE_SW + (cu + LOCATE_SPAN));
    }
    H = (int)Hl;
    const uint32_t c = __float_as_uint(ct.x) >> 24;
    const float n = g.a == 0 ? nr.x : g.a == 1 ? nr.y : nr.z;
    const int ni = (int)fminf(fmaxf(floorf(n * 16384.0f + 0.5f), -4194304.0f), 4194304.0f);
    st = locate_bit(g.smask, c) && (ni < 0 ? -ni : ni) <= g.max_up;
    gd = locate_bit(g.gmask, c) && g.nsgn * ni >= g.min_up;
    return st ? LOCATE_K_STRUCTURE : gd ? LOCATE_K_GROUND : LOCATE_K_OTHER;
}

// ---- the rasters
__global__ __launch_bounds__(256) void k_locate_raster(const float4 *__restrict__ rec, uint32_t n, LocateArgs g, int side, uint32_t *__restrict__ cnt,
                                                       int *__restrict__ Z, uint32_t *__restrict__ tally)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int kind = LOCATE_KINDS;                             // (no record)
    uint32_t cell = 0;
    int H = 0x7FFFFFFF;
    bool st = false, gd = false;
    if (t < n) kind = locate_place(g, side, rec[(size_t)t * 3], rec[(size_t)t * 3 + 1], rec[(size_t)t * 3 + 2], cell, H, st, gd);
    SimplifyArgs a{};
    a.combine = 1;
    {   // the counts: a run's first lane adds the run's length
        const bool head = simp_head(a, st ? (unsigned long long)cell : SIMP_EMPTY, st);
        const int last = simp_run_last(st, head);
        if (head) atomicAdd(&cnt[cell], (uint32_t)(last - lane + 1));
    }
    {   // the heights: a segmented shuffle minimum, then one atomicMin
        const bool head = simp_head(a, gd ? (unsigned long long)cell : SIMP_EMPTY, gd);
        if (!gd) H = 0x7FFFFFFF;
        if (__ballot(gd && !head)) {                     // wave-uniform: some run in this wave is longer than one lane
            const int last = simp_run_last(gd, head);
            for (int o = 1; o < 64; o <<= 1) {
                const bool take = lane + o <= last;
                if (!__ballot(take)) break;
                const int v = __shfl_down(H, o);
                if (take) H = min(H, v);
            }
        }
        if (head) atomicMin(&Z[cell], H);
    }
#pragma unroll
    for (int l = 0; l < LOCATE_KINDS; ++l) {
        const unsigned long long b = __ballot(kind == l);
        if (b && lane == 0) atomicAdd(&tally[LOCATE_COUNTS + side * 8 + l], (uint32_t)__popcll(b));
    }
}

// ---- the source's cells, compacted in plane order.  blk[0 .. nblk): cells of S per block, blk[nblk .. 2 nblk): cells of G
__global__ __launch_bounds__(256) void k_locate_count(const uint32_t *__restrict__ cnt, const int *__restrict__ Z, uint32_t N, uint32_t min_records,
                                                      uint32_t nblk, uint32_t *__restrict__ blk)
{
    __shared__ uint32_t s_n[2];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (threadIdx.x < 2) s_n[threadIdx.x] = 0;
    __syncthreads();
    const bool fs = i < N && cnt[i] >= min_records, fg = i < N && Z[i] != LOCATE_NO_Z;
    const unsigned long long bs = __ballot(fs), bg = __ballot(fg);
    if ((threadIdx.x & 63) == 0) {
        if (bs) atomicAdd(&s_n[0], (uint32_t)__popcll(bs));
        if (bg) atomicAdd(&s_n[1], (uint32_t)__popcll(bg));
    }
    __syncthreads();
    if (threadIdx.x < 2) blk[threadIdx.x * nblk + blockIdx.x] = s_n[threadIdx.x];
}

// one workgroup of 1024: the exclusive ranks of both halves of blk in place; the totals to total[0], total[1]
__global__ __launch_bounds__(1024) void k_locate_scan(uint32_t *__restrict__ blk, uint32_t nblk, uint32_t *__restrict__ total)
{
    __shared__ uint32_t s_sum[1024];
    const uint32_t per = (nblk + 1023u) / 1024u;
    for (int half = 0; half < 2; ++half) {
        uint32_t *b = blk + (size_t)half * nblk;
        const uint32_t lo = min(threadIdx.x * per, nblk), hi = min(lo + per, nblk);
        uint32_t sum = 0;
        for (uint32_t i = lo; i < hi; ++i) sum += b[i];
        s_sum[threadIdx.x] = sum;
        __syncthreads();
        for (uint32_t o = 1; o < 1024u; o <<= 1) {       // an inclusive scan of the 1024 partial sums
            const uint32_t v = threadIdx.x >= o ? s_sum[threadIdx.x - o] : 0u;
            __syncthreads();
            s_sum[threadIdx.x] += v;
            __syncthreads();
        }
        uint32_t run = s_sum[threadIdx.x] - sum;
        for (uint32_t i = lo; i < hi; ++i) { const uint32_t c = b[i]; b[i] = run; run += c; }
        if (threadIdx.x == 1023) total[half] = s_sum[1023];
        __syncthreads();
    }
}

// S[i]: cu + 4095 | (cv + 4095) << 16; G[i]: the same, Zs in GZ[i].  cap_s, cap_g: entries the arrays hold (a larger S is refused by
// the host after the scan; nothing is written past either)
__global__ __launch_bounds__(256) void k_locate_emit(const uint32_t *__restrict__ cnt, const int *__restrict__ Z, uint32_t N, uint32_t min_records,
                                                     uint32_t nblk, const uint32_t *__restrict__ blk, uint32_t *__restrict__ S, uint32_t cap_s,
                                                     uint32_t *__restrict__ G, int *__restrict__ GZ, uint32_t cap_g)
{
    __shared__ uint32_t s_w[2][4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = i < N ? Z[i] : LOCATE_NO_Z;
    const bool fs = i < N && cnt[i] >= min_records, fg = z != LOCATE_NO_Z;
    const unsigned long long bs = __ballot(fs), bg = __ballot(fg);
    if (lane == 0) { s_w[0][wave] = (uint32_t)__popcll(bs); s_w[1][wave] = (uint32_t)__popcll(bg); }
    __syncthreads();
    uint32_t rs = blk[blockIdx.x], rg = blk[nblk + blockIdx.x];
    for (int w = 0; w < wave; ++w) { rs += s_w[0][w]; rg += s_w[1][w]; }
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    rs += (uint32_t)__popcll(bs & below);
    rg += (uint32_t)__popcll(bg & below);
    const uint32_t word = (i % (uint32_t)LOCATE_SW) | ((i / (uint32_t)LOCATE_SW) << 16);
    if (fs && rs < cap_s) S[rs] = word;
    if (fg && rg < cap_g) { G[rg] = word; GZ[rg] = z; }
}

// ---- the rotation of a cell (cu, cv) under the table row (c, s): all int64, arithmetic shifts
__device__ __forceinline__ void locate_rotate(long long C, int c, int s, int cu, int cv, int &ru, int &rv)
{
    const long long x = (long long)cu * C + C / 2, y = (long long)cv * C + C / 2;
    const long long xr = ((long long)c * x - (long long)s * y + (1ll << 29)) >> 30, yr = ((long long)s * x + (long long)c * y + (1ll << 29)) >> 30;
    ru = (int)locate_floor_div(xr, C);
    rv = (int)locate_floor_div(yr, C);
}
__device__ __forceinline__ void locate_cell(uint32_t word, int &cu, int &cv)
{
    cu = (int)(word & 0xFFFFu) - LOCATE_SPAN;
    cv = (int)(word >> 16) - LOCATE_SPAN;
}

// table: the fine rows (c, s); coarse row k is fine row k * refine
__global__ __launch_bounds__(256) void k_locate_rotate(const uint32_t *__restrict__ S, uint32_t n_s, const int *__restrict__ table, int refine, long long C,
                                                       uint32_t *__restrict__ rot)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, k = blockIdx.y;
    if (i >= n_s) return;
    int cu, cv, ru, rv;
    locate_cell(S[i], cu, cv);
    locate_rotate(C, table[2 * k * refine], table[2 * k * refine + 1], cu, cv, ru, rv);
    rot[(size_t)k * n_s + i] = ((uint32_t)ru & 0xFFFFu) | ((uint32_t)rv << 16);
}

// ---- occ and the pyramid
__global__ __launch_bounds__(256) void k_locate_occ(const uint32_t *__restrict__ cnt, int nu, int nv, uint32_t min_records, int dilate, uint8_t *__restrict__ occ,
                                                    uint32_t *__restrict__ tally)
{
    const size_t N = (size_t)nu * nv, i = (size_t)blockIdx.x * 256u + threadIdx.x;
    bool on = false;
    if (i < N) {
        const int u = (int)(i % (size_t)nu), v = (int)(i / (size_t)nu);
        for (int dv = -dilate; dv <= dilate; ++dv)
            for (int du = -dilate; du <= dilate; ++du) {
                const int uu = u + du, vv = v + dv;
                if (uu >= 0 && uu < nu && vv >= 0 && vv < nv && cnt[(size_t)vv * nu + uu] >= min_records) on = true;
            }
        occ[i] = on ? 1 : 0;
    }
    const unsigned long long b = __ballot(on);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(&tally[LOCATE_OCC], (uint32_t)__popcll(b));
}

__device__ __forceinline__ uint32_t locate_at(const LocateLevel &L, int u, int v)
{
    const int iu = u + L.off, iv = v + L.off;
    return (iu >= 0 && iu < L.W && iv >= 0 && iv < L.H) ? (uint32_t)L.p[(size_t)iv * L.W + iu] : 0u;
}

// level `cur` (written at out) from level `prev`, s = 2^(h - 1)
__global__ __launch_bounds__(256) void k_locate_pyramid(LocateLevel prev, LocateLevel cur, uint8_t *__restrict__ out, int s)
{
    const size_t N = (size_t)cur.W * cur.H, i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const int u = (int)(i % (size_t)cur.W) - cur.off, v = (int)(i / (size_t)cur.W) - cur.off;
    out[i] = (uint8_t)(locate_at(prev, u, v) | locate_at(prev, u + s, v) | locate_at(prev, u, v + s) | locate_at(prev, u + s, v + s));
}

// ---- the search
__device__ __forceinline__ void locate_unrot(uint32_t w, int &ru, int &rv)
{
    ru = (int)(int16_t)(w & 0xFFFFu);
    rv = (int)(int16_t)(w >> 16);
}

// 4 nodes a workgroup, one wave each
__global__ __launch_bounds__(256) void k_locate_bound(LocateSearch q, LocateLevels lv, const LocateNode *__restrict__ nodes, uint32_t n_nodes,
                                                      uint32_t *__restrict__ bound)
{
    const uint32_t node = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (node >= n_nodes) return;                         // (the whole wave)
    const LocateNode nd = nodes[node];
    if (nd.h < 0 || nd.h >= LOCATE_MAX_LEVELS || nd.k < 0 || nd.k >= q.n_yaw) return;
    const LocateLevel L = lv.l[nd.h];
    const uint32_t *rot = q.rot + (size_t)nd.k * q.n_s;
    uint32_t sum = 0;
    for (uint32_t i = lane; i < q.n_s; i += 64u) {
        int ru, rv;
        locate_unrot(rot[i], ru, rv);
        sum += locate_at(L, ru + nd.du0, rv + nd.dv0);
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
    if (lane == 0) bound[node] = sum;
}

// is the candidate (k, du, dv) one of the runner-up's?
__device__ __forceinline__ bool locate_allowed(const LocateSearch &q, int k, int du, int dv)
{
    if (!q.ex_on) return true;
    int dk = k - q.ex_k;
    dk = dk < 0 ? -dk : dk;
    dk = min(dk, q.n_yaw - dk);
    const int eu = du - q.ex_du, ev = dv - q.ex_dv;
    return dk > q.sep_yaw || max(eu < 0 ? -eu : eu, ev < 0 ? -ev : ev) > q.sep_cells;
}

// The tile of TW x (64 / TW) offsets at (du0, dv0) of coarse row k, one offset a lane; k, du0, dv0 wave-uniform.  Returns the wave's
// best candidate, score << 40 | (LOCATE_KEY_MAX - key), key = k << 30 | (dv + R) << 15 | (du + R); 0 without a candidate
template <int TW>
__device__ __forceinline__ unsigned long long locate_tile(const LocateSearch &q, const LocateLevel &L0, int k, int du0, int dv0)
{
    const int lane = threadIdx.x & 63;
    const int du = du0 + lane % TW, dv = dv0 + lane / TW;
    const uint32_t *rot = q.rot + (size_t)k * q.n_s;
    uint32_t sum = 0;
    for (uint32_t i = 0; i < q.n_s; ++i) {               // (rot[i]: one address for the wave)
        int ru, rv;
        locate_unrot(rot[i], ru, rv);
        sum += locate_at(L0, ru + du, rv + dv);
    }
    const bool valid = du <= q.nu - 1 + q.R && dv <= q.nv - 1 + q.R && du >= -q.R && dv >= -q.R && locate_allowed(q, k, du, dv);
    const unsigned long long key = (unsigned long long)k << 30 | (unsigned long long)(dv + q.R) << 15 | (unsigned long long)(du + q.R);
    unsigned long long best = valid ? ((unsigned long long)sum << 40 | (LOCATE_KEY_MAX - key)) : 0ull;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_down(best, o);
        best = max(best, v);
    }
    return best;                                         // (lane 0's is the wave's)
}

__global__ __launch_bounds__(256) void k_locate_tiles(LocateSearch q, LocateLevel L0, const LocateNode *__restrict__ nodes, uint32_t n_nodes,
                                                      unsigned long long *__restrict__ best)
{
    const uint32_t node = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (node >= n_nodes) return;
    const LocateNode nd = nodes[node];
    const int k = __builtin_amdgcn_readfirstlane(nd.k), du0 = __builtin_amdgcn_readfirstlane(nd.du0), dv0 = __builtin_amdgcn_readfirstlane(nd.dv0);
    if (k < 0 || k >= q.n_yaw) return;
    const unsigned long long b = locate_tile<8>(q, L0, k, du0, dv0);
    if ((threadIdx.x & 63) == 0) best[node] = b;
}

// grid: (strips of 64 along du in groups of 4, the range's dv, n_yaw)
__global__ __launch_bounds__(256) void k_locate_all(LocateSearch q, LocateLevel L0, unsigned long long *__restrict__ best)
{
    const int strip = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const int du0 = -q.R + strip * 64, dv0 = -q.R + (int)blockIdx.y, k = (int)blockIdx.z;
    if (du0 > q.nu - 1 + q.R) return;
    const unsigned long long b = locate_tile<64>(q, L0, k, du0, dv0);
    if ((threadIdx.x & 63) == 0 && b) atomicMax(best, b);
}

// ---- refinement: workgroup b is dj = b - (refine - 1); out[b * 9 + lane]: the score at (du + lane % 3 - 1, dv + lane / 3 - 1)
__global__ __launch_bounds__(64) void k_locate_refine(const uint32_t *__restrict__ S, uint32_t n_s, const int *__restrict__ table, int n_fine, int refine,
                                                      int k, int du, int dv, long long C, LocateLevel L0, uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x, dj = (int)blockIdx.x - (refine - 1);
    int j = (k * refine + dj) % n_fine;
    if (j < 0) j += n_fine;
    const int c = table[2 * j], s = table[2 * j + 1];
    const int ou = du + lane % 3 - 1, ov = dv + (lane / 3) % 3 - 1;
    uint32_t sum = 0;
    for (uint32_t i = 0; i < n_s; ++i) {
        int cu, cv, ru, rv;
        locate_cell(S[i], cu, cv);
        locate_rotate(C, c, s, cu, cv, ru, rv);
        sum += locate_at(L0, ru + ou, rv + ov);
    }
    if (lane < 9) out[blockIdx.x * 9 + lane] = sum;
}

// ---- height
__global__ __launch_bounds__(256) void k_locate_height(const uint32_t *__restrict__ G, const int *__restrict__ GZ, uint32_t n_g, int c, int s, int du, int dv,
                                                       long long C, int nu, int nv, const int *__restrict__ Zt, int *__restrict__ d)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_g) return;
    int cu, cv, ru, rv;
    locate_cell(G[i], cu, cv);
    locate_rotate(C, c, s, cu, cv, ru, rv);
    const int u = ru + du, v = rv + dv;
    int out = LOCATE_NO_PAIR;
    if (u >= 0 && u < nu && v >= 0 && v < nv) {
        const int zt = Zt[(size_t)v * nu + u];
        if (zt != LOCATE_NO_Z) out = zt - GZ[i];
    }
    d[i] = out;
}

}  // namespace sm
