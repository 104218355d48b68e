// lidar_demo.cpp -- a headless caller that simulates a lidar in a saved map, through the drop-in facade and the C-ABI only.
// The map file `live_map` is loaded into the model (uploadMap); `poses` holds u32 n and n sensor->world poses of 16 floats; the
// sensor is n_az x n_el from azimuth az0 in steps of `step` degrees, elevations el0, el0 + el_step, ..., ranges 1 .. max_range.
// SurfelMapping::acquireSweeps writes <out_dir>/velodyne/%06d.bin, one file per pose, of the map files given after the sensor
// followed by the model; GlobalModel::lidarSweep of the first pose is summed up on stdout.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 12) {
        std::printf("usage: lidar_demo live_map.bin max_sqrt_vertices poses.bin out_dir n_az n_el az0 step el0 el_step max_range [map files...]\n");
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
    std::vector<Eigen::Matrix4f> poses(n);
    for (auto &p : poses)
        if (std::fread(p.data(), 4, 16, f) != 16) return 2;
    std::fclose(f);

    sm_lidar_sensor sn;
    if (sm_default_lidar_sensor(&sn) != SM_OK) return 1;
    sn.n_az = std::atoi(argv[5]); sn.n_el = std::atoi(argv[6]);
    sn.az0_deg = (float)std::atof(argv[7]); sn.az_step_deg = (float)std::atof(argv[8]);
    std::vector<float> el((size_t)(sn.n_el > 0 ? sn.n_el : 0));
    for (size_t i = 0; i < el.size(); ++i) el[i] = (float)std::atof(argv[9]) + (float)i * (float)std::atof(argv[10]);
    sn.el_deg = el.data();
    sn.max_range = (float)std::atof(argv[11]);
    std::vector<std::string> files;
    for (int i = 12; i < argc; ++i) files.push_back(argv[i]);

    if (!core.acquireSweeps(argv[4], files, poses, sn)) return 1;
    sm_lidar_stats_t st;
    if (sm_lidar_stats(core.context(), &st) != SM_OK) return 1;
    std::printf("sweeps %u surfels %llu tests %llu chunks %u passes %u\n", n, (unsigned long long)st.surfels, (unsigned long long)st.tests, st.chunks, st.passes);
    if (n) {
        GlobalModel::LidarReturns r;
        if (!core.getGlobalModel().lidarSweep(poses[0], sn, r)) return 1;
        size_t got = 0;
        double sum = 0.0;
        for (size_t b = 0; b < r.range.size(); ++b)
            if (r.id[b] >= 0) { ++got; sum += (double)r.range[b]; }
        std::printf("model returns %zu of %zu mean range %.6f\n", got, r.range.size(), got ? sum / (double)got : 0.0);
    }
    return 0;
}
