// segment_demo.cpp -- a headless caller that groups the surfels of saved maps into objects, through the drop-in facade and the
// C-ABI only.  SurfelMapping::segmentMaps labels the records of the map files, lists the components to stdout and writes the records
// of the components of at least min_records records to out_path: the set without its specks.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::printf("usage: segment_demo voxel_mm min_records out_path map files...\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = 64;
    SurfelMapping core;
    sm_segment_params p;
    sm_default_segment_params(&p);
    p.voxel_mm = std::atoi(argv[1]);
    std::vector<std::string> files;
    for (int i = 4; i < argc; ++i) files.push_back(argv[i]);
    std::vector<sm_segment_component> rows;
    std::vector<uint32_t> labels;
    sm_segment_info info;
    // every component, then the set without the components of fewer than min_records records
    if (core.segmentMaps(files, "", &p, rows, &labels, false, &info) < 0) return 1;
    std::printf("all: records %llu components %u small %u largest %u\n", (unsigned long long)info.records, info.components, info.small_components,
                info.largest);
    for (size_t i = 0; i < rows.size(); ++i)
        std::printf("component %zu first %u records %u cells %u class %d box %d %d %d .. %d %d %d\n", i, rows[i].first, rows[i].records, rows[i].cells,
                    rows[i].cls, rows[i].cell_lo[0], rows[i].cell_lo[1], rows[i].cell_lo[2], rows[i].cell_hi[0], rows[i].cell_hi[1], rows[i].cell_hi[2]);
    if (labels.size() != info.records) return 1;
    p.min_records = (uint32_t)std::atol(argv[2]);
    const long kept = core.segmentMaps(files, argv[3], &p, rows, &labels, false, &info);
    if (kept < 0) return 1;
    std::printf("kept: components %ld small %u written %llu\n", kept, info.small_components, (unsigned long long)info.written);
    size_t small = 0;
    for (uint32_t l : labels) small += l == SM_SEGMENT_SMALL;
    std::printf("labelled small %zu\n", small);
    // the output may not be one of the sources
    if (core.segmentMaps(files, files[0], &p, rows) >= 0) return 1;
    return 0;
}
