// tile_demo.cpp -- a headless caller that sorts a saved map in space, through the drop-in facade and the C-ABI only.  The map file
// `live_map` is loaded into the model (uploadMap); SurfelMapping::tileMaps then writes the map files that follow, then the model,
// as the tiled set <out_prefix>_000000.bin, ...  The tally and the files written go to stdout.  A second call whose first output
// name is the first map file shows the refusal.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

int main(int argc, char **argv)
{
    if (argc < 7) {
        std::printf("usage: tile_demo live_map.bin max_sqrt_vertices cell_mm tile_shift max_file_records out_prefix [map files...]\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = std::atoi(argv[2]);
    SurfelMapping core;
    std::vector<int> ids;
    if (!core.getGlobalModel().uploadMap(argv[1], ids)) return 1;
    sm_tile_params p;
    sm_default_tile_params(&p);
    p.cell_mm = std::atoi(argv[3]);
    p.tile_shift = std::atoi(argv[4]);
    p.max_file_records = (uint32_t)std::atol(argv[5]);
    std::vector<std::string> files;
    for (int i = 7; i < argc; ++i) files.push_back(argv[i]);
    const std::vector<std::string> written = core.tileMaps(files, argv[6], true, &p);
    sm_tile_stats_t st;
    if (sm_tile_stats(core.context(), &st) != SM_OK) return 1;
    std::printf("tiled %llu placed %llu loose %llu tiles %u largest %u files %u readings %u\n", (unsigned long long)st.records_in,
                (unsigned long long)st.placed, (unsigned long long)st.loose, st.tiles, st.largest_tile, st.files_written, st.readings);
    for (const std::string &f : written) std::printf("wrote %s\n", f.c_str());
    if (written.size() != st.files_written) return 1;
    if (!files.empty()) {
        // a source named like the first output: "<stem>_000000.bin" is refused under the prefix <stem>
        const std::string &f0 = files[0];
        const std::string tail = "_000000.bin";
        if (f0.size() > tail.size() && f0.compare(f0.size() - tail.size(), tail.size(), tail) == 0 &&
            !core.tileMaps(files, f0.substr(0, f0.size() - tail.size()), false, &p).empty())
            return 1;
    }
    return 0;
}
