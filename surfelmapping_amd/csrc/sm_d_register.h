// sm_d_register.h -- a voxel table read through one lookup record per slot, as device functions, for every source that looks
// records of one map set up in the table of another (sm_k_register.h; sm_k_compare.h): the lookup record and how a slot's sums
// become it, a record moved by a pose, the cell of the moved point with its neighbour towards the point, a candidate's key, the
// lookup of the eight candidates.  The table itself, its keys and its sums are sm_d_simplify.h's; the kernels that fill and
// finish it are sm_k_voxel.h's.  No kernels: a kernel is defined in the one header of the source that launches it.
#pragma once

#include "sm_d_simplify.h"

namespace sm {

struct alignas(32) RegCell {
    unsigned long long key;            // SIMP_EMPTY: the slot holds none
    float p[3], n[3];
};

constexpr long long REG_NO_CELL = -(1ll << 40);          // no such cell: a neighbour outside the cell range

// the lookup record of slot sl: the key, the merged position and the merged normal of its sums ((0, 0, 0) where all three vanish)
__device__ __forceinline__ RegCell reg_cell_of(const SimplifyArgs &a, const SimplifyTable &T, uint32_t sl)
{
    const size_t S = (size_t)T.mask + 1u;
    RegCell c;
    c.key = T.key[sl];
    c.p[0] = c.p[1] = c.p[2] = 0.0f;
    c.n[0] = c.n[1] = c.n[2] = 0.0f;
    if (c.key != SIMP_EMPTY) {
        const unsigned long long SW = T.SW[sl];
        long long sn[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c.p[k] = simp_merged_pos(a, c.key, k, SW, T.SP[k * S + sl]);
            sn[k] = (long long)T.SN[k * S + sl];
        }
        simp_merged_normal(sn, c.n);                     // (all three zero: n stays (0, 0, 0))
    }
    return c;
}

// a record's centre and normal, widened, moved by the pose T (fp64, column-major)
__device__ __forceinline__ void reg_move(const double *T, const float4 &pf, const float4 &nf, double q[3], double nq[3])
{
    const double p0 = pf.x, p1 = pf.y, p2 = pf.z, n0 = nf.x, n1 = nf.y, n2 = nf.z;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        q[k] = ((T[k] * p0 + T[4 + k] * p1) + T[8 + k] * p2) + T[12 + k];
        nq[k] = (T[k] * n0 + T[4 + k] * n1) + T[8 + k] * n2;
    }
}

// the coordinate qk of a moved point on the grid of edge V: its cell c and the neighbour nb towards the point (REG_NO_CELL: outside
// the cell range); false: the point is off the grid on this axis
__device__ __forceinline__ bool reg_cells(double qk, float origin_k, long long V, long long &c, long long &nb)
{
    const double d = qk - (double)origin_k;
    if (!(fabs(d) < 16777216.0)) return false;
    const long long X = (long long)floor(d * 65536.0);
    c = X / V;
    if (X - c * V < 0) --c;                              // floor division
    if (c < -65536 || c > 65535) return false;
    const long long off = X - c * V;
    nb = 2 * off >= V ? c + 1 : c - 1;
    if (nb < -65536 || nb > 65535) nb = REG_NO_CELL;
    return true;
}

// candidate j of the 2 x 2 x 2 (bit k of j: the neighbour on axis k) with the key's low eleven bits `low` (face << 8 | class);
// SIMP_EMPTY and valid = false: a cell of it is REG_NO_CELL
__device__ __forceinline__ unsigned long long reg_candidate(const long long cell[3][2], int j, unsigned long long low, bool &valid)
{
    const long long cx = cell[0][j & 1], cy = cell[1][(j >> 1) & 1], cz = cell[2][j >> 2];
    valid = cx != REG_NO_CELL && cy != REG_NO_CELL && cz != REG_NO_CELL;
    const unsigned long long k3 = ((unsigned long long)(cx + 65536) << 34) | ((unsigned long long)(cy + 65536) << 17) | (unsigned long long)(cz + 65536);
    return valid ? (k3 << 11) | low : SIMP_EMPTY;
}

// The eight candidates of `cell` with the low key bits `low` looked up in a table of mask + 1 slots whose slot s holds the key
// key_at(s): hit(j, key, slot) for every candidate that is there.  Every first probe is on its way before one is looked at; a
// walk ends at the key, at an empty slot or after mask + 1 slots, so no lane waits for another.
template <typename KeyAt, typename Hit>
__device__ __forceinline__ void reg_lookup8(const long long cell[3][2], unsigned long long low, uint32_t mask, KeyAt key_at, Hit hit)
{
    unsigned long long ck[8], cur[8];
    uint32_t sl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bool valid;
        ck[j] = reg_candidate(cell, j, low, valid);
        sl[j] = (uint32_t)simp_hash(ck[j]) & mask;
        cur[j] = valid ? key_at(sl[j]) : SIMP_EMPTY;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        unsigned long long c = cur[j];
        uint32_t s = sl[j];
        for (uint32_t w = 0; w <= mask; ++w) {           // (at most the table's slots)
            if (c == SIMP_EMPTY) break;
            if (c == ck[j]) { hit(j, ck[j], s); break; }
            s = (s + 1u) & mask;
            c = key_at(s);
        }
    }
}

}  // namespace sm
