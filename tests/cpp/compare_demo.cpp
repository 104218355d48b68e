// compare_demo.cpp -- a headless caller that tells what changed between two saved maps, through the drop-in facade and the C-ABI
// only.  "compare": SurfelMapping::compareMaps labels every record of `query` against `reference` (pose: query world ->
// reference world, sixteen column-major values) and writes the records whose label is in write_mask to `out`.  "diff":
// SurfelMapping::diffMaps writes what b holds and a does not to `appeared` and the reverse to `vanished` (pose: a's world -> b's).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

static void print_info(const char *what, const sm_compare_info &i)
{
    std::printf("%s counts %llu %llu %llu %llu cells %u %u written %llu\n", what, (unsigned long long)i.counts[0], (unsigned long long)i.counts[1],
                (unsigned long long)i.counts[2], (unsigned long long)i.counts[3], i.cells_fine, i.cells_cover, (unsigned long long)i.written);
}

int main(int argc, char **argv)
{
    const bool diff = argc > 1 && std::strcmp(argv[1], "diff") == 0;
    if (argc < 2 || (!diff && std::strcmp(argv[1], "compare") != 0) || argc != (diff ? 27 : 26)) {
        std::printf("usage: compare_demo compare query.bin reference.bin voxel_mm cover_shift reach_cells plane_mm write_mask out.bin pose x16\n"
                    "       compare_demo diff a.bin b.bin voxel_mm cover_shift reach_cells plane_mm write_mask appeared.bin vanished.bin pose x16\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = 64;
    SurfelMapping core;
    const std::vector<std::string> first{argv[2]}, second{argv[3]};
    sm_compare_params p;
    sm_default_compare_params(&p);
    p.voxel_mm = std::atoi(argv[4]);
    p.cover_shift = std::atoi(argv[5]);
    p.reach_cells = (float)std::atof(argv[6]);
    p.plane_mm = std::atoi(argv[7]);
    p.write_mask = (uint32_t)std::atoi(argv[8]);
    const int at = diff ? 11 : 10;
    Eigen::Matrix4f pose = Eigen::Matrix4f::Identity();
    for (int e = 0; e < 16; ++e) pose.data()[e] = (float)std::atof(argv[at + e]);
    if (diff) {
        sm_compare_info appeared, vanished;
        if (!core.diffMaps(first, second, pose, argv[9], argv[10], &p, &appeared, &vanished)) return 1;
        print_info("appeared", appeared);
        print_info("vanished", vanished);
        return 0;
    }
    sm_compare_info info;
    const long changed = core.compareMaps(first, second, pose, argv[9], &p, &info);
    if (changed < 0) return 1;
    print_info("compared", info);
    std::printf("changed %ld\n", changed);
    return 0;
}
