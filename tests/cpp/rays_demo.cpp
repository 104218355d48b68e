// rays_demo.cpp -- a headless caller that casts a list of rays into a saved map, through the drop-in facade and the C-ABI only.
// The map file `live_map` is loaded into the model (uploadMap); `rays` holds u32 n and n rays of 8 floats (origin, t_min, dir,
// t_max).  SurfelMapping::castRays casts them into the map files given after `out` followed by the model and writes the planes
// t | id | rgb | sem | normal one after the other into `out`; GlobalModel::castRays of the model alone is summed up on stdout.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::printf("usage: rays_demo live_map.bin max_sqrt_vertices rays.bin out.bin [map files...]\n");
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
    std::vector<sm_ray> rays(n);
    if (n && std::fread(rays.data(), sizeof(sm_ray), n, f) != n) return 2;
    std::fclose(f);
    std::vector<std::string> files;
    for (int i = 5; i < argc; ++i) files.push_back(argv[i]);

    GlobalModel::RayReturns r;
    if (!core.castRays(files, rays, r)) return 1;
    sm_rays_stats_t st;
    if (sm_cast_rays_stats(core.context(), &st) != SM_OK) return 1;
    std::printf("rays %llu bad %llu records %llu chunks %u\n", (unsigned long long)st.rays, (unsigned long long)st.bad_rays,
                (unsigned long long)st.records, st.chunks);
    FILE *o = std::fopen(argv[4], "wb");
    if (!o) return 1;
    bool ok = std::fwrite(r.t.data(), 4, n, o) == n && std::fwrite(r.id.data(), 4, n, o) == n && std::fwrite(r.rgb.data(), 3, n, o) == n &&
              std::fwrite(r.sem.data(), 1, n, o) == n && std::fwrite(r.normal.data(), 12, n, o) == n;
    ok = std::fclose(o) == 0 && ok;
    if (!ok) return 1;

    GlobalModel::RayReturns m;
    if (!core.getGlobalModel().castRays(rays, m)) return 1;
    size_t got = 0;
    double sum = 0.0;
    for (size_t b = 0; b < m.t.size(); ++b)
        if (m.id[b] >= 0) { ++got; sum += (double)m.t[b]; }
    std::printf("model returns %zu of %zu mean t %.6f\n", got, m.t.size(), got ? sum / (double)got : 0.0);
    return 0;
}
