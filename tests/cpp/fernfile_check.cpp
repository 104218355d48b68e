// Stand-alone check of surfelmapping_amd/csrc/sm_fernfile.h (host only; tests/test_place.py builds it plain and with the address
// and undefined-behaviour sanitizers):
//   fernfile_check table <n_ferns> <cell> <seed> <lo> <hi> <width> <height>   prints the table, one fern per line
//   fernfile_check parse <path>...                                          per file: "ok <count> <sum of times> <xor of the code words>"
//                                                                           or "err <text>"
//   fernfile_check copy <from> <to>                                          reads a file and writes it again through the writer
#include "sm_fernfile.h"

#include <cinttypes>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "table" && argc == 9) {
        sm_fern_params p;
        p.n_ferns = atoi(argv[2]); p.cell = atoi(argv[3]); p.seed = strtoull(argv[4], nullptr, 10);
        p.depth_lo_mm = atoi(argv[5]); p.depth_hi_mm = atoi(argv[6]);
        const int w = atoi(argv[7]), h = atoi(argv[8]);
        if (const char *why = sm_fernfile::check_params(p)) { printf("err %s\n", why); return 0; }
        if (w < p.cell || h < p.cell) { printf("err no cell\n"); return 0; }
        std::vector<sm_fern> t((size_t)p.n_ferns);
        sm_fernfile::make_table(p, w, h, t.data());
        for (const sm_fern &f : t) printf("%u %u %u %u %u %u\n", f.x, f.y, f.tr, f.tg, f.tb, f.td);
        return 0;
    }
    if (mode == "parse") {
        for (int i = 2; i < argc; ++i) {
            sm_fernfile::Header h;
            std::string err;
            sm_fernfile::File f = sm_fernfile::open_checked(argv[i], h, err);
            if (!f) { printf("err %s\n", err.c_str()); continue; }
            std::vector<int32_t> times(h.count);
            std::vector<float> poses((size_t)h.count * 16);
            std::vector<uint32_t> codes((size_t)h.count * sm_fernfile::code_words(h.p));
            if (!sm_fernfile::read_records(f.get(), h, times.data(), poses.data(), codes.data(), err, argv[i])) { printf("err %s\n", err.c_str()); continue; }
            int64_t st = 0;
            uint32_t x = 0;
            for (int32_t t : times) st += t;
            for (uint32_t c : codes) x ^= c;
            printf("ok %u %" PRId64 " %u\n", h.count, st, x);
        }
        return 0;
    }
    if (mode == "copy" && argc == 4) {
        sm_fernfile::Header h;
        std::string err;
        sm_fernfile::File f = sm_fernfile::open_checked(argv[2], h, err);
        if (!f) { printf("err %s\n", err.c_str()); return 0; }
        std::vector<int32_t> times(h.count);
        std::vector<float> poses((size_t)h.count * 16);
        std::vector<uint32_t> codes((size_t)h.count * sm_fernfile::code_words(h.p));
        if (!sm_fernfile::read_records(f.get(), h, times.data(), poses.data(), codes.data(), err, argv[2]) ||
            !sm_fernfile::write_file(argv[3], h, times.data(), poses.data(), codes.data(), err)) {
            printf("err %s\n", err.c_str());
            return 0;
        }
        printf("ok %u\n", h.count);
        return 0;
    }
    return 2;
}
