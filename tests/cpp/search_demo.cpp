// search_demo.cpp -- a headless caller that closes a loop from metres of drift, through the drop-in facade.  As auto_loop_demo.cpp:
// a camera that starts at tick `first_tick` fuses its frames at the (drifted) poses it believes in, saves them as the map file
// `new_map` and pages the old world back in from `old_map`.  Then setTrackColour(true) and, by mode:
//   plain   closeLoop(rgb, depth, pose, {new_map}) with the last frame of the dump, which is not fused: one track from the
//           believed pose.
//   search  setLoopSearch(true) first: the loop is measured by a pose search around the believed pose.
//   auto    setLoopSearch(true), setAutoLoop(true, {new_map}) and one processFrame WITHOUT a pose: the policy's attempt searches.
// Frames come from a raw dump (u32 W,H,n; f32 fx,fy,cx,cy; per frame rgb|depth|sem|pose16).  Prints the status, t_a, t_b, D and
// the pose as hexadecimal floats, saves the model.
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
    if (argc < 8) { std::printf("usage: search_demo frames.bin first_tick old_map.bin radius new_map.bin out_map.bin plain|search|auto\n"); return 2; }
    const std::string mode = argv[7];
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
        if (k == n - 1) break;                                           // the returning frame
        core.processFrame(rgb.data(), depth.data(), sem.data(), &pose);
        last = pose;
    }
    std::fclose(f);
    if (!core.getGlobalModel().downloadMap(argv[5], std::atoi(argv[2]), std::atoi(argv[2]) + n - 2)) return 1;
    const long old = core.getGlobalModel().recall({argv[3]}, last, (float)std::atof(argv[4]), true);
    std::printf("recalled %ld count %u\n", old, core.getGlobalModel().getModel().second);
    core.setTrackColour(true);
    if (mode != "plain" && !core.setLoopSearch(true)) return 1;
    sm_loop_info li;
    Eigen::Matrix4f fixed;
    if (mode == "auto") {
        if (!core.setAutoLoop(true, {argv[5]})) return 1;
        core.processFrame(rgb.data(), depth.data(), sem.data(), nullptr);
        const sm_auto_loop_stats_t st = core.autoLoopStats();
        std::printf("checked %u attempts %u closed %u census %u\n", st.checked, st.attempts, st.closed, st.last_census);
        li = st.last;
        fixed = core.getCurrPose();
        if (!core.setAutoLoop(false)) return 1;
    } else {
        fixed = core.closeLoop(rgb.data(), depth.data(), pose, {argv[5]});
        li = core.getLastLoopInfo();
    }
    std::printf("status %d t_a %d t_b %d track %d inliers %u\n", li.status, li.t_a, li.t_b, li.track.status, li.track.inliers);
    print16("D", li.D);
    print16("pose", fixed.data());
    return core.getGlobalModel().downloadMap(argv[6], 0, 0) ? 0 : 1;
}
