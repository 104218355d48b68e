// pack_demo.cpp -- a headless caller that packs a drive's map files and views the packed set, through the drop-in facade and the
// C-ABI only.  The map file `live_map` is loaded into the model (uploadMap); SurfelMapping::packMaps writes the map files that
// follow, then the model, as <prefix>_000000.smp, ...; unpackMaps writes them back as <prefix>_000000.bin, ...; one novel view of
// the packed set and one of its unpacked twin go to <prefix>_packed.bgr / <prefix>_plain.bgr (raw bytes).  The tally and the
// files written go to stdout.  A second packing whose first output name is the first map file shows the refusal.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../surfelmapping_amd/csrc/facade/SurfelMapping.h"

static bool view_of(SurfelMapping &core, const std::vector<std::string> &files, const std::string &out)
{
    const int w = 160, h = 60;
    std::vector<const char *> paths;
    for (const std::string &f : files) paths.push_back(f.c_str());
    const sm_map_source src{paths.data(), (uint32_t)paths.size(), 0};
    const float view[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::vector<uint8_t> bgr((size_t)w * h * 3), sem((size_t)w * h);
    if (sm_render_image_maps(core.context(), &src, view, 1, w, h, 90.0f, 90.0f, 79.5f, 29.5f, bgr.data(), sem.data()) != SM_OK) {
        std::printf("view: %s\n", sm_last_error());
        return false;
    }
    size_t drawn = 0;
    for (uint8_t s : sem) drawn += s != 0;
    std::printf("view %s pixels %zu\n", out.c_str(), drawn);
    FILE *f = std::fopen(out.c_str(), "wb");
    const bool ok = f && std::fwrite(bgr.data(), 1, bgr.size(), f) == bgr.size();
    if (f) std::fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 5) {
        std::printf("usage: pack_demo live_map.bin max_sqrt_vertices pos_step_log2 prefix [map files...]\n");
        return 2;
    }
    Config::getInstance(100.0f, 100.0f, 32.0f, 24.0f, 48, 64);          // (no frame is processed: any camera will do)
    Config::maxSqrtVertices() = std::atoi(argv[2]);
    SurfelMapping core;
    std::vector<int> ids;
    if (!core.getGlobalModel().uploadMap(argv[1], ids)) return 1;
    sm_pack_params p;
    sm_default_pack_params(&p);
    p.pos_step_log2 = std::atoi(argv[3]);
    const std::string prefix = argv[4];
    std::vector<std::string> files;
    for (int i = 5; i < argc; ++i) files.push_back(argv[i]);
    const std::vector<std::string> packed = core.packMaps(files, prefix, true, &p);
    sm_pack_stats_t st;
    if (packed.size() != files.size() + 1 || sm_pack_stats(core.context(), &st) != SM_OK) return 1;
    std::printf("packed files %u records %llu blocks %u raw %u bytes %llu -> %llu\n", st.files, (unsigned long long)st.records, st.blocks, st.raw_blocks,
                (unsigned long long)st.bytes_in, (unsigned long long)st.bytes_out);
    for (const std::string &f : packed) std::printf("wrote %s\n", f.c_str());
    const std::vector<std::string> plain = core.unpackMaps(packed, prefix);
    if (plain.size() != packed.size() || sm_pack_stats(core.context(), &st) != SM_OK) return 1;
    std::printf("unpacked files %u records %llu bytes %llu -> %llu\n", st.files, (unsigned long long)st.records, (unsigned long long)st.bytes_in,
                (unsigned long long)st.bytes_out);
    for (const std::string &f : plain) std::printf("wrote %s\n", f.c_str());
    if (!view_of(core, packed, prefix + "_packed.bgr") || !view_of(core, plain, prefix + "_plain.bgr")) return 1;
    if (!files.empty()) {
        // a source named like the first output: "<stem>_000000.smp" is refused under the prefix <stem>
        const std::string &f0 = files[0];
        const std::string tail = "_000000.smp";
        if (f0.size() > tail.size() && f0.compare(f0.size() - tail.size(), tail.size(), tail) == 0 &&
            !core.packMaps(files, f0.substr(0, f0.size() - tail.size()), false, &p).empty())
            return 1;
    }
    return 0;
}
