// loop_demo.cpp -- a headless caller that closes a loop through the drop-in facade: a camera that starts at tick `first_tick`
// fuses its frames at the (drifted) poses it believes in, pages the old world back in from a map file (GlobalModel::recall, files
// kept), and then asks SurfelMapping::closeLoop whether the last depth image -- which is tracked and not fused -- says it is back:
// the model and the map file `new_map` move with the correction.  One GlobalModel::warpByTime with the identity follows (nothing
// moves bit-wise, the count is printed).  Frames come from a raw dump (u32 W,H,n; f32 fx,fy,cx,cy; per frame
// rgb|depth|sem|pose16); the last frame of the dump is the one the loop is closed with.  Prints status, t_a, t_b, D and the
// corrected pose as hexadecimal floats, saves the model.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

static void print16(const char *what, const float *m)
{
    std::printf("%s", what);
    for (int i = 0; i < 16; ++i) std::printf(" %a", (double)m[i]);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 7) { std::printf("usage: loop_demo frames.bin first_tick old_map.bin radius new_map.bin out_map.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[3]; float intr[4];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(intr, 4, 4, f) != 4) return 2;
    const int W = (int)hdr[0], H = (int)hdr[1], n = (int)hdr[2];
    Config::getInstance(intr[0], intr[1], intr[2], intr[3], H, W);
    setenv("SM_PREPROCESS", "0", 0);
    SurfelMapping core;
    if (sm_set_tick(core.context(), std::atoi(argv[2])) != SM_OK) return 1;
    std::vector<unsigned char> rgb((size_t)W * H * 3), sem((size_t)W * H);
    std::vector<unsigned short> depth((size_t)W * H);
    Eigen::Matrix4f pose, last = Eigen::Matrix4f::Identity();
    for (int k = 0; k < n; ++k) {
        if (std::fread(rgb.data(), 1, rgb.size(), f) != rgb.size() || std::fread(depth.data(), 2, depth.size(), f) != depth.size() ||
            std::fread(sem.data(), 1, sem.size(), f) != sem.size() || std::fread(pose.data(), 4, 16, f) != 16) return 2;
        if (k == n - 1) break;                                           // the returning frame: tracked below, not fused
        core.processFrame(rgb.data(), depth.data(), sem.data(), &pose);
        last = pose;
    }
    std::fclose(f);
    if (!core.getGlobalModel().downloadMap(argv[5], std::atoi(argv[2]), std::atoi(argv[2]) + n - 2)) return 1;
    const long old = core.getGlobalModel().recall({argv[3]}, last, (float)std::atof(argv[4]), true);
    std::printf("recalled %ld count %u\n", old, core.getGlobalModel().getModel().second);
    const Eigen::Matrix4f fixed = core.closeLoop(depth.data(), pose, {argv[5]});
    const sm_loop_info &li = core.getLastLoopInfo();
    std::printf("status %d t_a %d t_b %d track %d inliers %u\n", li.status, li.t_a, li.t_b, li.track.status, li.track.inliers);
    print16("D", li.D);
    print16("pose", fixed.data());
    const std::vector<float> ident = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::printf("identity moved %ld\n", core.getGlobalModel().warpByTime({argv[5]}, li.t_a, ident));
    if (core.getGlobalModel().warpByTime({std::string(argv[5]) + ".missing"}, 0, ident) != -1) return 1;
    return core.getGlobalModel().downloadMap(argv[6], 0, 0) ? 0 : 1;
}
