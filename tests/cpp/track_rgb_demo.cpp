// track_rgb_demo.cpp -- a caller that maps a street of flat ground and flat walls through the drop-in facade with only its first
// poses known: frames 0 .. given-1 get their pose, every later one calls processFrame(rgb, depth, semantic, nullptr).  With
// colour = 1 the caller has asked for the colour term (setTrackColour(true)); with 0 the facade tracks on depth alone, which
// cannot see motion along such a street.  Frames come from a raw dump (u32 W,H,n; f32 fx,fy,cx,cy; per frame
// rgb|depth|sem|pose16).  Prints one line per tracked frame and writes getHistoryPoses() (n x 16 floats, column-major).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 5) { std::printf("usage: track_rgb_demo frames.bin given colour out_poses.bin\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const int given = std::atoi(argv[2]);
    const bool colour = std::atoi(argv[3]) != 0;
    uint32_t hdr[3]; float intr[4];
    if (std::fread(hdr, 4, 3, f) != 3 || std::fread(intr, 4, 4, f) != 4) return 2;
    const int W = (int)hdr[0], H = (int)hdr[1], n = (int)hdr[2];
    Config::getInstance(intr[0], intr[1], intr[2], intr[3], H, W);
    setenv("SM_PREPROCESS", "0", 0);
    SurfelMapping core;
    core.setTrackColour(colour);
    std::vector<unsigned char> rgb((size_t)W * H * 3), sem((size_t)W * H);
    std::vector<unsigned short> depth((size_t)W * H);
    static const char *const names[] = {"SM_TRACK_OK", "SM_TRACK_LOST", "SM_TRACK_DEGENERATE", "SM_TRACK_NO_MODEL"};
    for (int k = 0; k < n; ++k) {
        Eigen::Matrix4f pose;
        if (std::fread(rgb.data(), 1, rgb.size(), f) != rgb.size() || std::fread(depth.data(), 2, depth.size(), f) != depth.size() ||
            std::fread(sem.data(), 1, sem.size(), f) != sem.size() || std::fread(pose.data(), 4, 16, f) != 16) return 2;
        core.processFrame(rgb.data(), depth.data(), sem.data(), k < given ? &pose : nullptr);
        if (k < given) continue;
        const sm_track_info &ti = core.getLastTrackInfo();
        std::printf("frame %d: %s, %d iterations, %u inliers", k, ti.status >= 0 && ti.status <= 3 ? names[ti.status] : "?",
                    ti.iterations, ti.inliers);
        if (colour) std::printf(", %u colour samples, pivot ratio %.3g", core.getLastTrackRgbInfo().rgb_inliers,
                                core.getLastTrackRgbInfo().pivot_ratio);
        std::printf("\n");
    }
    std::fclose(f);
    FILE *o = std::fopen(argv[4], "wb");
    if (!o) return 2;
    for (const Eigen::Matrix4f &p : core.getHistoryPoses()) std::fwrite(p.data(), 4, 16, o);
    std::fclose(o);
    return 0;
}
