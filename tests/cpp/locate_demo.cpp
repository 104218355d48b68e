// locate_demo.cpp -- a headless caller that finds one saved map in the world of another without a guess and then registers it,
// through the drop-in facade and the C-ABI only.  SurfelMapping::locateMaps places `source` in `target` (nothing changes) and
// prints what it found; with min_inliers > 0 its pose is SurfelMapping::registerMaps' guess, pivot at the middle of the window.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 14) {
        std::printf("usage: locate_demo source.bin target.bin up normal_sign origin_x origin_y origin_z nu nv source_x source_y source_z min_inliers\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = 64;
    SurfelMapping core;
    const std::vector<std::string> source{argv[1]}, target{argv[2]};
    sm_locate_params p;
    sm_default_locate_params(&p);
    p.up = std::atoi(argv[3]);
    p.normal_sign = std::atoi(argv[4]);
    for (int k = 0; k < 3; ++k) p.origin[k] = (float)std::atof(argv[5 + k]);
    p.nu = std::atoi(argv[8]);
    p.nv = std::atoi(argv[9]);
    for (int k = 0; k < 3; ++k) p.source_origin[k] = (float)std::atof(argv[10 + k]);
    Eigen::Matrix4f guess;
    sm_locate_info info;
    const int status = core.locateMaps(source, target, guess, &p, &info);
    if (status < 0) return 1;
    std::printf("status %d row %d du %d dv %d score %u coarse %d %d %d %u runner_up %u n_s %u cells %u pairs %u dh %d\n", status, info.row, info.du, info.dv,
                info.score, info.coarse_k, info.coarse_du, info.coarse_dv, info.coarse_score, info.runner_up, info.n_s, info.target_cells,
                info.height_pairs, info.dh);
    std::printf("pose");
    for (int e = 0; e < 16; ++e) std::printf(" %.9g", guess.data()[e]);
    std::printf("\n");
    const int min_inliers = std::atoi(argv[13]);
    if (status == SM_LOCATE_OK && min_inliers > 0) {
        sm_register_params rp;
        sm_default_register_params(&rp);
        rp.min_inliers = min_inliers;
        const int axis[3] = {p.up >> 1 == 0 ? 1 : 0, p.up >> 1 == 2 ? 1 : 2, p.up >> 1};
        const float cell = (float)p.cell_mm * 0.001f;
        for (int k = 0; k < 3; ++k) rp.pivot[k] = p.origin[k];
        rp.pivot[axis[0]] += 0.5f * (float)p.nu * cell;
        rp.pivot[axis[1]] += 0.5f * (float)p.nv * cell;
        Eigen::Matrix4f pose;
        sm_register_info ri;
        const int rs = core.registerMaps(source, target, guess, pose, &rp, &ri);
        if (rs < 0) return 1;
        std::printf("register %d inliers %u\nrefined", rs, ri.inliers);
        for (int e = 0; e < 16; ++e) std::printf(" %.9g", pose.data()[e]);
        std::printf("\n");
    }
    // a window that is refused
    p.nu = 0;
    if (core.locateMaps(source, target, guess, &p) >= 0) return 1;
    return 0;
}
