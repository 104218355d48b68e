// sm_pose.h -- the arithmetic of rigid camera poses on the host, once: column-major 4x4, camera -> world, computed in double from
// float poses widened.  The trackers' guess and prediction camera (sm_track.hip) and the loop correction D = T_old * pose^-1
// (sm_warp.hip) are made of these, operation for operation; tests/track_ref.py restates them and tests/cpp/pose_check.cpp prints
// them for a bit-for-bit comparison.  Host only: no HIP header, not sm_ctx.h (a plain C++ compiler compiles it).
// Not here, because they are other operations: the general fp32 4x4 inverse and product of sm_api.hip (invert4, mul4), the
// candidate grids of sm_search.hip (compose, mul3) and products with a pose's own fourth row (sm_warp.hip).
#pragma once

#include <cmath>

namespace sm_pose {

template <typename T>
inline void identity(T *m)
{
    for (int e = 0; e < 16; ++e) m[e] = (e % 5 == 0) ? T(1) : T(0);
}

inline void widen(const float *m, double *o)
{
    for (int e = 0; e < 16; ++e) o[e] = (double)m[e];
}

// [R^T | -R^T t] of a rigid pose
inline void rigid_inv_d(const double *m, double *o)
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[c * 4 + r] = m[r * 4 + c];
        o[12 + r] = -((m[r * 4 + 0] * m[12] + m[r * 4 + 1] * m[13]) + m[r * 4 + 2] * m[14]);
    }
    o[3] = 0.0; o[7] = 0.0; o[11] = 0.0; o[15] = 1.0;
}

// the rigid product a * b: each element ((a0*b0 + a1*b1) + a2*b2), + a's translation in the last column
inline void mul_rigid_d(const double *a, const double *b, double *o)
{
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r)
            o[c * 4 + r] = ((a[r] * b[c * 4] + a[4 + r] * b[c * 4 + 1]) + a[8 + r] * b[c * 4 + 2]) + (c == 3 ? a[12 + r] : 0.0);
    o[3] = 0.0; o[7] = 0.0; o[11] = 0.0; o[15] = 1.0;
}

// the rotation of a pose made orthonormal (Gram-Schmidt on columns 0 and 1, column 2 = 0 x 1).  Float poses are orthonormal to
// ~1e-7 only; products of them (the constant-velocity guess, exp(xi) * guess) would carry and, frame after frame, multiply that
// error, so every product starts from orthonormal factors.
inline void orthonormalize_d(double *m)
{
    double *a = m, *b = m + 4, *c = m + 8;
    const double na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (int k = 0; k < 3; ++k) a[k] /= na;
    const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    for (int k = 0; k < 3; ++k) b[k] -= ab * a[k];
    const double nb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    for (int k = 0; k < 3; ++k) b[k] /= nb;
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
    m[3] = 0.0; m[7] = 0.0; m[11] = 0.0; m[15] = 1.0;
}

}  // namespace sm_pose
