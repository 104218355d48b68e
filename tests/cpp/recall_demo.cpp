// recall_demo.cpp -- a headless caller that pages retired surfels back in through the drop-in facade: retire_demo's loop with both
// periodic policies on (SurfelMapping::setAutoRetire + setAutoRecall), then one GlobalModel::recall around an earlier pose of the
// drive, first with the files kept, then moving the records out of them.  Frames come from a raw dump (u32 W,H,n; f32
// fx,fy,cx,cy; per frame rgb|depth|sem|pose16).  Prints the policies' tallies and what each recall brought back, saves the model.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 10) { std::printf("usage: recall_demo frames.bin max_sqrt_vertices every min_age min_distance radius prefix back_to_frame out_map.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[3]; float intr[4];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(intr, 4, 4, f) != 4) return 2;
    const int W = (int)hdr[0], H = (int)hdr[1], n = (int)hdr[2];
    Config::getInstance(intr[0], intr[1], intr[2], intr[3], H, W);
    Config::maxSqrtVertices() = std::atoi(argv[2]);
    const float radius = (float)std::atof(argv[6]);
    const int back = std::atoi(argv[8]);
    setenv("SM_PREPROCESS", "0", 0);
    SurfelMapping core;
    if (!core.setAutoRetire(std::atoi(argv[3]), argv[7], std::atoi(argv[4]), (float)std::atof(argv[5]))) return 1;
    if (core.setAutoRecall(2.0f * (float)std::atof(argv[5]))) return 1;  // beyond the retirement's distance: refused
    if (!core.setAutoRecall(radius)) return 1;
    std::vector<unsigned char> rgb((size_t)W * H * 3), sem((size_t)W * H);
    std::vector<unsigned short> depth((size_t)W * H);
    Eigen::Matrix4f pose, poseBack = Eigen::Matrix4f::Identity();
    for (int k = 0; k < n; ++k) {
        if (std::fread(rgb.data(), 1, rgb.size(), f) != rgb.size() || std::fread(depth.data(), 2, depth.size(), f) != depth.size() ||
            std::fread(sem.data(), 1, sem.size(), f) != sem.size() || std::fread(pose.data(), 4, 16, f) != 16) return 2;
        core.processFrame(rgb.data(), depth.data(), sem.data(), &pose);
        if (k == back) poseBack = pose;
    }
    std::fclose(f);
    const unsigned count = core.getGlobalModel().getModel().second;      // (waits for the frames in flight)
    const auto st = core.autoRetireStats();
    const auto rc = core.autoRecallStats();
    std::printf("files %u surfels %llu rounds %u recalled %llu count %u\n", st.first, st.second, rc.first, rc.second, count);
    std::vector<std::string> files;
    for (unsigned i = 0; i < st.first; ++i) {
        char name[32];
        std::snprintf(name, sizeof name, "_%06u.bin", i);
        files.push_back(std::string(argv[7]) + name);
    }
    core.setAutoRetire(0, "");
    const long kept = core.getGlobalModel().recall(files, poseBack, radius, true);
    const unsigned c1 = core.getGlobalModel().getModel().second;
    const long moved = core.getGlobalModel().recall(files, poseBack, radius);
    std::printf("copy %ld count %u move %ld count %u\n", kept, c1, moved, core.getGlobalModel().getModel().second);
    files.push_back(std::string(argv[7]) + "_missing.bin");
    if (core.getGlobalModel().recall(files, poseBack, radius) != -1) return 1;
    return core.getGlobalModel().downloadMap(argv[9], 0, n - 1) ? 0 : 1;
}
