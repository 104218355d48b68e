// blend_demo.cpp -- a headless caller that dumps blended novel views from a saved map, through the drop-in facade and the C-ABI
// only.  The map file `live_map` is loaded into the model (uploadMap); `views` holds u32 n and n camera->world poses of 16 floats.
// setBlend(blend, tol, falloff) is applied, then SurfelMapping::acquireImages writes <out_dir>/live/{image,semantic}/%06d.png from
// the model alone and, if map files follow, <out_dir>/set/... from those files followed by the model.  With blending on, the
// tally of the last call goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 14) {
        std::printf("usage: blend_demo live_map.bin max_sqrt_vertices views.bin w h fx fy cx cy blend tol falloff out_dir [map files...]\n");
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
    const bool blend = std::atoi(argv[10]) != 0;
    core.setBlend(blend, std::atoi(argv[11]), std::atoi(argv[12]));
    const std::string out = argv[13];
    ::mkdir(out.c_str(), 0755);
    ::mkdir((out + "/live").c_str(), 0755);
    core.acquireImages(out + "/live", views, w, h, fx, fy, cx, cy, 0);
    std::vector<std::string> files;
    for (int i = 14; i < argc; ++i) files.push_back(argv[i]);
    if (!files.empty()) {
        ::mkdir((out + "/set").c_str(), 0755);
        if (!core.acquireImages(out + "/set", files, views, w, h, fx, fy, cx, cy, 5)) return 1;
    }
    sm_blend_stats_t st;
    const int rc = sm_blend_stats(core.context(), &st);
    if (blend != (rc == SM_OK)) return 1;                               // no blended call was made with the switch off
    if (blend)
        std::printf("views %u drawn %llu contributions %llu changed %llu launches %u\n", n, (unsigned long long)st.drawn,
                    (unsigned long long)st.contributions, (unsigned long long)st.changed, st.launches);
    return 0;
}
