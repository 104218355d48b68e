// stereo_demo.cpp -- a headless caller that maps a drive from a stereo rig alone, through the drop-in facade: a dataset in the
// KITTI layout with image_2/ and image_3/ and no PSMNet/ is read with estimateDepth = true (the reference's own flag, which there
// only hands on a null depth), and every frame goes through SurfelMapping::processFrameStereo -- frames 0 .. given-1 at the
// reader's pose, every later one with a null gtPose, which tracks with the estimated depth.  Writes getHistoryPoses() (n x 16
// floats, column-major), the last estimated depth image and the map.  Exit 3: the reader could not deliver a frame.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/KittiReader.h"
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 8) { std::printf("usage: stereo_demo dataset_dir given baseline max_disp out_poses.bin out_depth.bin out_map.bin\n"); return 2; }
    KittiReader reader(argv[1], true, true, 0, true);
    if (!reader.good()) { std::printf("reader: bad dataset\n"); return 3; }
    const int given = std::atoi(argv[2]), n = (int)reader.numFrames();
    if (!reader.getNext()) { std::printf("\nreader: no frame 0\n"); return 3; }         // (before anything asks for a GPU)
    Config::getInstance(reader.fx(), reader.fy(), reader.cx(), reader.cy(), reader.H(), reader.W());
    setenv("SM_PREPROCESS", "0", 0);
    SurfelMapping core;
    if (!core.setStereo(true, (float)std::atof(argv[3]), std::atoi(argv[4]))) return 1;
    int ok = 0;
    for (int k = 0; k < n; ++k) {
        if (k && !reader.getNext()) { std::printf("\nreader: no frame %d\n", k); return 3; }
        if (reader.depth || !reader.rgbRight) return 1;                  // estimateDepth: no depth from a file, the right image instead
        if (!core.processFrameStereo(reader.rgb, reader.rgbRight, reader.semantic, k < given ? &reader.gtPose : nullptr)) return 1;
        if (k >= given && core.getLastTrackInfo().status == SM_TRACK_OK) ok++;
    }
    std::printf("tracked %d of %d\n", ok, n - given);
    FILE *o = std::fopen(argv[5], "wb");
    if (!o) return 2;
    for (const Eigen::Matrix4f &p : core.getHistoryPoses()) std::fwrite(p.data(), 4, 16, o);
    std::fclose(o);
    o = std::fopen(argv[6], "wb");
    if (!o) return 2;
    std::fwrite(core.getLastStereoDepth().data(), 2, core.getLastStereoDepth().size(), o);
    std::fclose(o);
    return core.getGlobalModel().downloadMap(argv[7], 0, n - 1) ? 0 : 1;
}
