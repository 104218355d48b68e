// pose_check.cpp -- the rigid-pose arithmetic of sm_pose.h alone (no HIP, no GPU), printed for a bit-for-bit comparison with
// tests/track_ref.py.  Arguments: 16 * k hex floats, k >= 1 column-major poses.  For every pose A and its successor B (the last
// pose's is the first) it prints, as hex doubles of the widened floats' results,
//   inv    rigid_inv_d(A)          mul    mul_rigid_d(A, B)          ortho  orthonormalize_d(A)
// and, first of all, the two identity fills.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sm_pose.h"

static void line(const char *what, const double *m)
{
    std::printf("%s", what);
    for (int e = 0; e < 16; ++e) std::printf(" %a", m[e]);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 17 || (argc - 1) % 16 != 0) return 2;
    const int k = (argc - 1) / 16;
    std::vector<float> poses((size_t)k * 16);
    for (int i = 0; i < k * 16; ++i) {
        char *end = nullptr;
        const double v = std::strtod(argv[1 + i], &end);
        poses[i] = (float)v;
        if (*end || (double)poses[i] != v) return 2;          // not a number, or not a float
    }
    float eye_f[16];
    double eye_d[16], wide[16];
    sm_pose::identity(eye_f);
    sm_pose::identity(eye_d);
    sm_pose::widen(eye_f, wide);
    line("eye", wide);
    line("eye", eye_d);
    for (int i = 0; i < k; ++i) {
        double a[16], b[16], o[16];
        sm_pose::widen(&poses[(size_t)i * 16], a);
        sm_pose::widen(&poses[(size_t)((i + 1) % k) * 16], b);
        sm_pose::rigid_inv_d(a, o);
        line("inv", o);
        sm_pose::mul_rigid_d(a, b, o);
        line("mul", o);
        sm_pose::orthonormalize_d(a);
        line("ortho", a);
    }
    return 0;
}
