// register_demo.cpp -- a headless caller that brings one saved map into the world of another, through the drop-in facade and the
// C-ABI only.  SurfelMapping::registerMaps measures the transform from `source` to `target` (nothing changes) and prints it;
// with align = 1 SurfelMapping::alignMaps then moves the source file by it and SurfelMapping::simplifyMaps writes target and
// source together, merged per cell of voxel_mm, to `out`.  The pivot is the point the twist is taken about.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 10) {
        std::printf("usage: register_demo source.bin target.bin min_inliers pivot_x pivot_y pivot_z align voxel_mm out.bin\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = 64;
    SurfelMapping core;
    const std::vector<std::string> source{argv[1]}, target{argv[2]};
    sm_register_params p;
    sm_default_register_params(&p);
    p.min_inliers = std::atoi(argv[3]);
    for (int k = 0; k < 3; ++k) p.pivot[k] = (float)std::atof(argv[4 + k]);
    const bool align = std::atoi(argv[7]) != 0;
    Eigen::Matrix4f guess = Eigen::Matrix4f::Identity(), pose;
    sm_register_info info;
    const int status = align ? core.alignMaps(source, target, guess, pose, &p, &info) : core.registerMaps(source, target, guess, pose, &p, &info);
    if (status < 0) return 1;
    std::printf("status %d iterations %d %d %d inliers %u samples %u\n", status, info.iterations[0], info.iterations[1], info.iterations[2],
                info.inliers, info.samples);
    std::printf("pose");
    for (int e = 0; e < 16; ++e) std::printf(" %.9g", pose.data()[e]);
    std::printf("\n");
    if (status != SM_REGISTER_OK || !align) return 0;
    const long n = core.simplifyMaps({argv[2], argv[1]}, argv[9], std::atoi(argv[8]));
    if (n < 0) return 1;
    std::printf("merged %ld\n", n);
    return 0;
}
