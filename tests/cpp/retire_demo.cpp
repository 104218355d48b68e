// retire_demo.cpp -- a headless caller that maps a sequence longer than the model's capacity through the drop-in facade:
// kitti_demo's loop with the periodic retirement on (SurfelMapping::setAutoRetire), which replaces the operator's save / reset
// buttons (build_map.cpp:235-263).  Frames come from a raw dump (u32 W,H,n; f32 fx,fy,cx,cy; per frame rgb|depth|sem|pose16).
// Prints the map files / surfels written and the final count, retires what is left behind the last camera through
// GlobalModel::retire, and saves the rest.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 8) { std::printf("usage: retire_demo frames.bin max_sqrt_vertices every min_age min_distance prefix out_map.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[3]; float intr[4];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(intr, 4, 4, f) != 4) return 2;
    const int W = (int)hdr[0], H = (int)hdr[1], n = (int)hdr[2];
    Config::getInstance(intr[0], intr[1], intr[2], intr[3], H, W);
    Config::maxSqrtVertices() = std::atoi(argv[2]);
    const int minAge = std::atoi(argv[4]);
    const float minDistance = (float)std::atof(argv[5]);
    setenv("SM_PREPROCESS", "0", 0);
    SurfelMapping core;
    if (!core.setAutoRetire(std::atoi(argv[3]), argv[6], minAge, minDistance)) return 1;
    std::vector<unsigned char> rgb((size_t)W * H * 3), sem((size_t)W * H);
    std::vector<unsigned short> depth((size_t)W * H);
    Eigen::Matrix4f pose;
    for (int k = 0; k < n; ++k) {
        if (std::fread(rgb.data(), 1, rgb.size(), f) != rgb.size() || std::fread(depth.data(), 2, depth.size(), f) != depth.size() ||
            std::fread(sem.data(), 1, sem.size(), f) != sem.size() || std::fread(pose.data(), 4, 16, f) != 16) return 2;
        core.processFrame(rgb.data(), depth.data(), sem.data(), &pose);
    }
    std::fclose(f);
    const unsigned count = core.getGlobalModel().getModel().second;      // (waits for the frames in flight)
    const auto st = core.autoRetireStats();
    std::printf("files %u surfels %llu count %u\n", st.first, st.second, count);
    std::vector<float> rest;
    if (!core.getGlobalModel().retire(pose, minAge, minDistance, rest)) return 1;
    core.getGlobalModel().getModelMapVC();                               // a caller of refreshHostModel()
    std::printf("retired at the end %zu count %u mirror %zu\n", rest.size() / 12, core.getGlobalModel().getModel().second,
                core.getGlobalModel().mirrorHost(0).size() / 4);
    return core.getGlobalModel().downloadMap(argv[7], 0, n - 1) ? 0 : 1;
}
