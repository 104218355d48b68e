// ground_demo.cpp -- a headless caller that turns saved maps into a planner's ground map, through the drop-in facade and the C-ABI
// only.  SurfelMapping::groundMaps rasters the records of the map files over the window given on the command line and the planes go
// to stdout, a row of cells a line; GlobalModel::groundMap does the same for the (empty) live model.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

template <typename T>
static void plane(const char *name, const std::vector<T> &v, int nu, int nv, int per_cell = 1)
{
    for (int r = 0; r < nv; ++r) {
        std::printf("%s %d:", name, r);
        for (int i = 0; i < nu * per_cell; ++i) std::printf(" %lld", (long long)v[(size_t)r * nu * per_cell + i]);
        std::printf("\n");
    }
}

int main(int argc, char **argv)
{
    if (argc < 7) {
        std::printf("usage: ground_demo cell_mm up nu nv normal_sign map files...\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = 64;
    SurfelMapping core;
    sm_ground_params p;
    sm_default_ground_params(&p);
    p.cell_mm = std::atoi(argv[1]);
    p.up = std::atoi(argv[2]);
    p.nu = std::atoi(argv[3]);
    p.nv = std::atoi(argv[4]);
    p.normal_sign = std::atoi(argv[5]);
    std::vector<std::string> files;
    for (int i = 6; i < argc; ++i) files.push_back(argv[i]);
    const GroundMap m = core.groundMaps(files, &p);
    if (!m.ok) return 1;
    std::printf("ground: records %llu counts", (unsigned long long)m.info.records);
    for (uint64_t c : m.info.counts) std::printf(" %llu", (unsigned long long)c);
    std::printf(" cells %u %u %u %u\n", m.info.cells[0], m.info.cells[1], m.info.cells[2], m.info.cells[3]);
    plane("ground", m.ground, m.nu, m.nv);
    plane("top", m.top, m.nu, m.nv);
    plane("state", m.state, m.nu, m.nv);
    plane("cls", m.cls, m.nu, m.nv);
    plane("bgr", m.bgr, m.nu, m.nv, 3);
    plane("clear2", m.clear2, m.nu, m.nv);
    // the live model alone: empty, every cell UNKNOWN
    const GroundMap live = core.getGlobalModel().groundMap(&p);
    if (!live.ok) return 1;
    std::printf("model: records %llu unknown %u\n", (unsigned long long)live.info.records, live.info.cells[0]);
    // a window that is refused
    p.nu = 0;
    if (core.groundMaps(files, &p).ok) return 1;
    return 0;
}
