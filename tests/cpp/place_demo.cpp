// place_demo.cpp -- a headless caller that recognises a place it has been to, through the drop-in facade.  As auto_loop_demo.cpp: a
// camera that starts at tick `first_tick` fuses the frames of a raw dump at the (drifted) poses it believes in -- all but the last --
// and pages the old world back in from `old_map` (GlobalModel::recall, files kept).  Then SurfelMapping::setAutoPlace(true),
// loadKeyframes(keyframes) -- the keyframes of the drive that mapped the old world -- and one processFrame WITHOUT a pose for the
// last frame of the dump: it is tracked, encoded, matched against the keyframes, the loop is closed from the matched keyframe's
// pose and the frame is fused at the corrected pose.  Nobody tells it where it is.
// Frames come from a raw dump (u32 W,H,n; f32 fx,fy,cx,cy; per frame rgb|depth|sem|pose16).  Prints the policy's tally, the status,
// t_a, t_b, D and the pose as hexadecimal floats, saves the keyframes and the model.
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
    if (argc < 8) { std::printf("usage: place_demo frames.bin first_tick old_map.bin radius keyframes.fern out_keyframes.fern out_map.bin\n"); return 2; }
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
        if (k == n - 1) break;                                           // the frame that recognises the place
        core.processFrame(rgb.data(), depth.data(), sem.data(), &pose);
        last = pose;
    }
    std::fclose(f);
    const long old = core.getGlobalModel().recall({argv[3]}, last, (float)std::atof(argv[4]), true);
    std::printf("recalled %ld count %u\n", old, core.getGlobalModel().getModel().second);
    core.setTrackColour(true);
    if (!core.setAutoPlace(true) || !core.loadKeyframes(argv[5])) return 1;
    core.processFrame(rgb.data(), depth.data(), sem.data(), nullptr);
    const sm_auto_place_stats_t st = core.autoPlaceStats();
    std::printf("encoded %u added %u matched %u attempts %u closed %u keyframe %d dis %u\n", st.encoded, st.added, st.matched, st.attempts,
                st.closed, st.last_k, st.last_dis);
    const sm_loop_info &li = st.last;
    std::printf("status %d t_a %d t_b %d track %d inliers %u\n", li.status, li.t_a, li.t_b, li.track.status, li.track.inliers);
    print16("D", li.D);
    print16("pose", core.getCurrPose().data());
    if (!core.saveKeyframes(argv[6])) return 1;
    return core.getGlobalModel().downloadMap(argv[7], 0, 0) ? 0 : 1;
}
