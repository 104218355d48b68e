// sm_d_track.h -- the trackers' normal equations as device functions, for every source that sums and solves such a system
// (sm_k_track.h; sm_k_register.h): the 29-value layout, the fixed-order sums of a workgroup and of the partials, the LDLT, the
// solve, the exponential and the degeneracy measure.  No kernels: a kernel is defined in the one header of the source that
// launches it.
#pragma once

#include "sm_device.h"

namespace sm {

constexpr int TRACK_BLOCK = 256;
constexpr int TRACK_MAX_PARTS = 1024;    // workgroups of k_track_reduce at most (each leaves 29 partial sums)
constexpr int TRACK_NSYS = 29;           // JtJ upper triangle (21, row-major), Jtr (6), r^2, inliers

__device__ __forceinline__ double track_wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// the workgroup's 29 wave-reduced sums -> one partial per value (fixed order: waves 0, 1, 2, 3)
__device__ __forceinline__ void track_block_sum(const double *acc, double (*s_w)[TRACK_NSYS], int nb, double *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < TRACK_NSYS; ++e) {
        const double x = track_wave_sum(acc[e]);
        if (lane == 0) s_w[wave][e] = x;
    }
    __syncthreads();
    if (threadIdx.x < TRACK_NSYS) {
        double x = s_w[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < TRACK_BLOCK / 64; ++w) x += s_w[w][threadIdx.x];
        part[(size_t)threadIdx.x * nb + blockIdx.x] = x;
    }
}

// exp of the twist (rho, phi) as R (row-major 3x3) and t, double
__device__ inline void track_exp(const double *xi, double R[3][3], double t[3])
{
    const double px = xi[3], py = xi[4], pz = xi[5];
    const double th2 = px * px + py * py + pz * pz, th = sqrt(th2);
    double A, B, C;                                           // sin(th)/th, (1-cos)/th^2, (th-sin)/th^3
    if (th < 1e-4) {
        A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; C = 1.0 / 6.0 - th2 / 120.0;
    } else {
        A = sin(th) / th; B = (1.0 - cos(th)) / th2; C = (th - sin(th)) / (th2 * th);
    }
    const double K[3][3] = {{0.0, -pz, py}, {pz, 0.0, -px}, {-py, px, 0.0}};
    double K2[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) K2[a][b] = K[a][0] * K[0][b] + K[a][1] * K[1][b] + K[a][2] * K[2][b];
    double V[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double I = a == b ? 1.0 : 0.0;
            R[a][b] = I + A * K[a][b] + B * K2[a][b];
            V[a][b] = I + B * K[a][b] + C * K2[a][b];
        }
    for (int a = 0; a < 3; ++a) t[a] = V[a][0] * xi[0] + V[a][1] * xi[1] + V[a][2] * xi[2];
}

// LDLT of the symmetric 6x6 A (no pivoting): d[] the pivots, L unit lower; false if a pivot is not positive
__device__ inline bool track_ldlt(const double A[6][6], double L[6][6], double d[6])
{
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k] * d[k];
        d[j] = s;
        if (!(s > 0.0)) return false;
        L[j][j] = 1.0;
        for (int i = j + 1; i < 6; ++i) {
            double u = A[i][j];
            for (int k = 0; k < j; ++k) u -= L[i][k] * L[j][k] * d[k];
            L[i][j] = u / s;
        }
    }
    return true;
}

// the fixed-order sum of the nb partials of each of the 29 values (all 256 threads; sys is valid in thread 0).  Thread (e, sub)
// sums partials sub, sub + 8, ... of value e into four interleaved accumulators (independent loads in flight) and adds them in a
// fixed order; thread 0 then adds the eight sub-sums of every value
__device__ __forceinline__ void track_sum_parts(const double *__restrict__ part, int nb, double (*s_p)[8], double *sys)
{
    const int t = threadIdx.x;
    if (t < TRACK_NSYS * 8) {
        const int e = t >> 3, sub = t & 7;
        const double *pe = part + (size_t)e * nb;
        double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0;
        int b = sub;
        for (; b + 24 < nb; b += 32) { x0 += pe[b]; x1 += pe[b + 8]; x2 += pe[b + 16]; x3 += pe[b + 24]; }
        for (; b < nb; b += 8) x0 += pe[b];
        s_p[e][sub] = (x0 + x1) + (x2 + x3);
    }
    __syncthreads();
    if (t != 0) return;
    for (int e = 0; e < TRACK_NSYS; ++e) {
        double x = s_p[e][0];
        for (int k = 1; k < 8; ++k) x += s_p[e][k];
        sys[e] = x;
    }
}

__device__ inline void track_unpack(const double *sys, double A[6][6], double b[6])
{
    int e = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) { A[a][c] = sys[e]; A[c][a] = sys[e]; ++e; }
    for (int a = 0; a < 6; ++a) b[a] = sys[21 + a];
}

// degeneracy: the same system with the rotation taken about the prediction camera centre c (rows [n, (Tv - c) x n]: B = M^T A M,
// M = [[I, [c]x], [0, I]]) and the rotation columns scaled by 1/s, s^2 = (trace of its rotation block) / (trace of its
// translation block): unit-free and independent of where the world origin lies.  Smallest / largest LDLT pivot (0: not positive)
__device__ inline double track_pivot_ratio(const double A[6][6], const double *c)
{
    const double cx = c[0], cy = c[1], cz = c[2];
    const double Mx[6][6] = {{1, 0, 0, 0, -cz, cy}, {0, 1, 0, cz, 0, -cx}, {0, 0, 1, -cy, cx, 0},
                             {0, 0, 0, 1, 0, 0}, {0, 0, 0, 0, 1, 0}, {0, 0, 0, 0, 0, 1}};
    double AM[6][6], B[6][6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double x = 0.0;
            for (int k = 0; k < 6; ++k) x += A[i][k] * Mx[k][j];
            AM[i][j] = x;
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double x = 0.0;
            for (int k = 0; k < 6; ++k) x += Mx[k][i] * AM[k][j];
            B[i][j] = x;
        }
    const double tr_t = B[0][0] + B[1][1] + B[2][2], tr_r = B[3][3] + B[4][4] + B[5][5];
    const double sc = tr_r > 0.0 && tr_t > 0.0 ? sqrt(tr_t / tr_r) : 1.0;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) B[i][j] *= (i >= 3 ? sc : 1.0) * (j >= 3 ? sc : 1.0);
    double L[6][6], d[6];
    double ratio = 0.0;
    if (track_ldlt(B, L, d)) {
        double lo = d[0], hi = d[0];
        for (int k = 1; k < 6; ++k) { lo = fmin(lo, d[k]); hi = fmax(hi, d[k]); }
        ratio = lo / hi;
    }
    return ratio;
}

// (J^T J) xi = -J^T r through the LDLT and its two substitutions; false if A is not positive definite
__device__ inline bool track_solve_xi(const double A[6][6], const double *b, double xi[6])
{
    double L[6][6], d[6], y[6];
    if (!track_ldlt(A, L, d)) return false;
    for (int i = 0; i < 6; ++i) {
        double x = -b[i];
        for (int k = 0; k < i; ++k) x -= L[i][k] * y[k];
        y[i] = x;
    }
    for (int i = 5; i >= 0; --i) {
        double x = y[i] / d[i];
        for (int k = i + 1; k < 6; ++k) x -= L[k][i] * xi[k];
        xi[i] = x;
    }
    return true;
}

}  // namespace sm
