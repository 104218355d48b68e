// track_demo.cpp -- a caller that maps a sequence through the drop-in facade with only its first poses known: frames
// 0 .. given-1 get their pose, every later one calls processFrame(rgb, depth, semantic, nullptr), which tracks the camera
// (src/SurfelMapping.h:31-34: "if provided, we don't attempt to perform tracking").  Frames come from a raw dump (u32 W,H,n;
// f32 fx,fy,cx,cy; per frame rgb|depth|sem|pose16).  Writes getHistoryPoses() (n x 16 floats, column-major) and the map.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 5) { std::printf("usage: track_demo frames.bin given out_poses.bin out_map.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const int given = std::atoi(argv[2]);
    uint32_t hdr[3]; float intr[4];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(intr, 4, 4, f) != 4) return 2;
    const int W = (int)hdr[0], H = (int)hdr[1], n = (int)hdr[2];
    Config::getInstance(intr[0], intr[1], intr[2], intr[3], H, W);
    setenv("SM_PREPROCESS", "0", 0);
    SurfelMapping core;
    std::vector<unsigned char> rgb((size_t)W * H * 3), sem((size_t)W * H);
    std::vector<unsigned short> depth((size_t)W * H);
    int ok = 0;
    for (int k = 0; k < n; ++k) {
        Eigen::Matrix4f pose;
        if (std::fread(rgb.data(), 1, rgb.size(), f) != rgb.size() || std::fread(depth.data(), 2, depth.size(), f) != depth.size() ||
            std::fread(sem.data(), 1, sem.size(), f) != sem.size() || std::fread(pose.data(), 4, 16, f) != 16) return 2;
        core.processFrame(rgb.data(), depth.data(), sem.data(), k < given ? &pose : nullptr);
        if (k >= given && core.getLastTrackInfo().status == SM_TRACK_OK) ok++;
    }
    std::fclose(f);
    FILE *o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    for (const Eigen::Matrix4f &p : core.getHistoryPoses()) std::fwrite(p.data(), 4, 16, o);
    std::fclose(o);
    std::printf("tracked %d of %d, last %d iterations %u inliers\n", ok, n - given, core.getLastTrackInfo().iterations,
                core.getLastTrackInfo().inliers);
    return core.getGlobalModel().downloadMap(argv[4], 0, n - 1) ? 0 : 1;
}
