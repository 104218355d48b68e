// points_demo.cpp -- a headless caller that asks a saved map for the nearest disc to a list of points, through the drop-in facade
// and the C-ABI only.  The map file `live_map` is loaded into the model (uploadMap); `points` holds u32 n and n points of 4 floats
// (position, reach).  SurfelMapping::queryPoints queries the map files given after `out` followed by the model and writes the
// planes d2 | id | centre | normal | radius | rgb | sem one after the other into `out`; GlobalModel::queryPoints of the model alone
// is summed up on stdout.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::printf("usage: points_demo live_map.bin max_sqrt_vertices points.bin out.bin [map files...]\n");
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
    std::vector<sm_point> points(n);
    if (n && std::fread(points.data(), sizeof(sm_point), n, f) != n) return 2;
    std::fclose(f);
    std::vector<std::string> files;
    for (int i = 5; i < argc; ++i) files.push_back(argv[i]);

    GlobalModel::PointReturns r;
    if (!core.queryPoints(files, points, r)) return 1;
    sm_points_stats_t st;
    if (sm_query_points_stats(core.context(), &st) != SM_OK) return 1;
    std::printf("points %llu bad %llu records %llu chunks %u\n", (unsigned long long)st.points, (unsigned long long)st.bad_points,
                (unsigned long long)st.records, st.chunks);
    FILE *o = std::fopen(argv[4], "wb");
    if (!o) return 1;
    bool ok = std::fwrite(r.d2.data(), 4, n, o) == n && std::fwrite(r.id.data(), 4, n, o) == n && std::fwrite(r.centre.data(), 12, n, o) == n &&
              std::fwrite(r.normal.data(), 12, n, o) == n && std::fwrite(r.radius.data(), 4, n, o) == n && std::fwrite(r.rgb.data(), 3, n, o) == n &&
              std::fwrite(r.sem.data(), 1, n, o) == n;
    ok = std::fclose(o) == 0 && ok;
    if (!ok) return 1;

    GlobalModel::PointReturns m;
    if (!core.getGlobalModel().queryPoints(points, m)) return 1;
    size_t got = 0;
    double sum = 0.0;
    for (size_t b = 0; b < m.d2.size(); ++b)
        if (m.id[b] >= 0) { ++got; sum += std::sqrt((double)m.d2[b]); }
    std::printf("model answers %zu of %zu mean distance %.6f\n", got, m.d2.size(), got ? sum / (double)got : 0.0);
    return 0;
}
