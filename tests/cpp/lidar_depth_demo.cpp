// lidar_depth_demo.cpp -- a headless caller that maps a drive from a camera and a lidar, through the drop-in facade: a dataset in
// the KITTI layout with image_2/, velodyne/ and velo_to_cam.txt and no PSMNet/ is read with setUseLidar(true), and every frame
// goes through SurfelMapping::processFrameLidar at the reader's pose.  Writes the last frame's depth image and the map.
// Exit 3: the reader could not deliver a frame.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/KittiReader.h"
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 5) { std::printf("usage: lidar_depth_demo dataset_dir large out_depth.bin out_map.bin\n"); return 2; }
    KittiReader reader(argv[1], false, true, 0, true);
    if (!reader.good()) { std::printf("reader: bad dataset\n"); return 3; }
    if (reader.velodyne || reader.numPoints) return 1;                   // off by default
    if (!reader.setUseLidar(true)) { std::printf("reader: no lidar\n"); return 3; }
    const int n = (int)reader.numFrames();
    if (!reader.getNext()) { std::printf("\nreader: no frame 0\n"); return 3; }         // (before anything asks for a GPU)
    Config::getInstance(reader.fx(), reader.fy(), reader.cx(), reader.cy(), reader.H(), reader.W());
    setenv("SM_PREPROCESS", "0", 0);
    SurfelMapping core;
    sm_config c;
    sm_default_config(&c, Config::W(), Config::H(), Config::fx(), Config::fy(), Config::cx(), Config::cy());
    sm_lidar_depth_params lp;
    sm_default_lidar_depth_params(&c, &lp);
    lp.large = std::atoi(argv[2]);
    if (!core.setLidarDepth(true, &lp)) return 1;
    unsigned points = 0;
    for (int k = 0; k < n; ++k) {
        if (k && !reader.getNext()) { std::printf("\nreader: no frame %d\n", k); return 3; }
        if (reader.depth || !reader.velodyne) return 1;                  // the scan instead of a depth image
        if (!core.processFrameLidar(reader.rgb, reader.velodyne, reader.numPoints, reader.veloToCam, reader.semantic, &reader.gtPose)) return 1;
        points += reader.numPoints;
    }
    std::printf("points %u in %d frames\n", points, n);
    FILE *o = std::fopen(argv[3], "wb");
    if (!o) return 2;
    std::fwrite(core.getLastLidarDepth().data(), 2, core.getLastLidarDepth().size(), o);
    std::fclose(o);
    return core.getGlobalModel().downloadMap(argv[4], 0, n - 1) ? 0 : 1;
}
