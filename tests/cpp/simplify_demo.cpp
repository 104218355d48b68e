// simplify_demo.cpp -- a headless caller that makes a saved map smaller, through the drop-in facade and the C-ABI only.  The map
// file `live_map` is loaded into the model (uploadMap).  If map files follow, SurfelMapping::simplifyMaps writes the simplification
// of those files followed by the model to <out_dir>/set.bin.  Then GlobalModel::simplify merges the model in place and downloadMap
// saves it as <out_dir>/live.bin.  The tally of each call goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

static void report(const char *what, SurfelMapping &core, long n)
{
    sm_simplify_stats_t st;
    if (sm_simplify_stats(core.context(), &st) != SM_OK) return;
    std::printf("%s %ld in %llu out %llu merged %llu loose %llu largest %u\n", what, n, (unsigned long long)st.records_in,
                (unsigned long long)st.records_out, (unsigned long long)st.cells_merged, (unsigned long long)st.loose, st.largest_cell);
}

int main(int argc, char **argv)
{
    if (argc < 6) {
        std::printf("usage: simplify_demo live_map.bin max_sqrt_vertices voxel_mm split_normals out_dir [map files...]\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = std::atoi(argv[2]);
    SurfelMapping core;
    std::vector<int> ids;
    if (!core.getGlobalModel().uploadMap(argv[1], ids)) return 1;
    const int voxel = std::atoi(argv[3]);
    const bool split = std::atoi(argv[4]) != 0;
    const std::string out = argv[5];
    ::mkdir(out.c_str(), 0755);
    std::vector<std::string> files;
    for (int i = 6; i < argc; ++i) files.push_back(argv[i]);
    if (!files.empty()) {
        const long n = core.simplifyMaps(files, out + "/set.bin", voxel, split, true);
        if (n < 0) return 1;
        report("set", core, n);
        if (core.simplifyMaps(files, files[0], voxel, split) != -1) return 1;     // (the output may not be a source)
    }
    const long n = core.getGlobalModel().simplify(voxel, split);
    if (n < 0) return 1;
    report("live", core, n);
    return core.getGlobalModel().downloadMap(out + "/live.bin", 0, 0) ? 0 : 1;
}
