// fill_demo.cpp -- a headless caller that dumps camera ground truth from a saved map: image, label and depth, with the holes of
// the novel views closed, through the drop-in facade and the C-ABI only.  The map file `live_map` is loaded into the model
// (uploadMap); `views` holds u32 n and n camera->world poses of 16 floats.  setFillHoles(fill, levels) and setWriteDepth(depth)
// are applied, then SurfelMapping::acquireImages writes <out_dir>/live/{image,semantic[,depth]}/%06d.png from the model alone and,
// if map files follow, <out_dir>/set/... from those files followed by the model.  The completion's tally goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 14) {
        std::printf("usage: fill_demo live_map.bin max_sqrt_vertices views.bin w h fx fy cx cy fill levels depth out_dir [map files...]\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = std::atoi(argv[2]);
    SurfelMapping core;
    std::vector<int> ids;
    if (!core.getGlobalModel().uploadMap(argv[1], ids)) return 1;
    FILE *f = std::fopen(argv[3], "rb");
    uint32_t n = 0;
    if (!f || std::fread(&n, 4, 1, f) != 1) return 2;
    std::vector<Eigen::Matrix4f> views(n);
    for (auto &v : views)
        if (std::fread(v.data(), 4, 16, f) != 16) return 2;
    std::fclose(f);
    const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
    const float fx = (float)std::atof(argv[6]), fy = (float)std::atof(argv[7]), cx = (float)std::atof(argv[8]), cy = (float)std::atof(argv[9]);
    const bool fill = std::atoi(argv[10]) != 0, depth = std::atoi(argv[12]) != 0;
    core.setFillHoles(fill, std::atoi(argv[11]));
    core.setWriteDepth(depth);
    const std::string out = argv[13];
    ::mkdir(out.c_str(), 0755);
    ::mkdir((out + "/live").c_str(), 0755);
    core.acquireImages(out + "/live", views, w, h, fx, fy, cx, cy, 0);
    {   // what the live-model overload leaves in the model, with or without the switches: the last view
        const GlobalModel &gm = core.getGlobalModel();
        unsigned long long bgrSum = 0, semSum = 0;
        for (unsigned char v : gm.imageBGR()) bgrSum += v;
        for (unsigned char v : gm.imageSemantic()) semSum += v;
        std::printf("model image %d x %d bgr %zu sum %llu sem %zu sum %llu\n", gm.imageWidth(), gm.imageHeight(), gm.imageBGR().size(), bgrSum,
                    gm.imageSemantic().size(), semSum);
    }
    std::vector<std::string> files;
    for (int i = 14; i < argc; ++i) files.push_back(argv[i]);
    if (!files.empty()) {
        ::mkdir((out + "/set").c_str(), 0755);
        if (!core.acquireImages(out + "/set", files, views, w, h, fx, fy, cx, cy, 5)) return 1;
    }
    if (fill) {
        sm_fill_stats_t st;
        if (sm_fill_stats(core.context(), &st) != SM_OK) return 1;
        std::printf("views %u valid %llu seen_through %llu filled %llu left_empty %llu launches %u\n", n, (unsigned long long)st.valid,
                    (unsigned long long)st.seen_through, (unsigned long long)st.filled, (unsigned long long)st.left_empty, st.launches);
    }
    return 0;
}
