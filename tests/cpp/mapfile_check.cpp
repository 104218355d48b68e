// mapfile_check.cpp -- drives surfelmapping_amd/csrc/sm_mapfile.h alone for tests/test_mapfile_cpu.py: no HIP header, any C++17
// compiler.  One command per run; the result goes to stdout as one line per item, "ok ..." or "err <message>".
//   write <path> <count|unknown> <startId> <endId> <rows file> <commit|drop> <piece> ...   rows of the file appended in pieces
//   open  <strict|lenient> <path> ...                                                       the checked open of each path
//   plan  <chunk> <path> ...                                                                the chunk plan of the listed files
#include "sm_mapfile.h"

#include <cstdlib>
#include <cstring>

using namespace sm_mapfile;

static int do_write(int argc, char **argv)
{
    if (argc < 8) return 2;
    const uint32_t count = strcmp(argv[3], "unknown") == 0 ? Writer::UNKNOWN : (uint32_t)strtoul(argv[3], nullptr, 10);
    std::vector<char> rows;
    {
        File in(fopen(argv[6], "rb"));
        if (!in) return 2;
        char buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof buf, in.get())) > 0;) rows.insert(rows.end(), buf, buf + k);
    }
    const bool commit = strcmp(argv[7], "commit") == 0;
    std::string err;
    {
        Writer w;
        bool ok = w.open(argv[2], count, atoi(argv[4]), atoi(argv[5]), "check", err);
        size_t at = 0;
        for (int i = 8; ok && i < argc; ++i) {
            const size_t n = (size_t)strtoul(argv[i], nullptr, 10);
            if ((at + n) * RECORD_BYTES > rows.size()) return 2;
            ok = w.append(rows.data() + at * RECORD_BYTES, n, err);
            at += n;
        }
        if (ok && commit) ok = w.commit(err);
        if (!ok) { printf("err %s\n", err.c_str()); return 0; }
        printf("ok %llu\n", (unsigned long long)w.rows());
    }                                                    // (a writer that was not committed goes away here)
    return 0;
}

static int do_open(int argc, char **argv)
{
    if (argc < 3) return 2;
    const bool lenient = strcmp(argv[2], "lenient") == 0;
    for (int i = 3; i < argc; ++i) {
        Header h;
        std::string err;
        File f = open_checked(argv[i], "check", h, err, lenient);
        if (!f) { printf("err %s\n", err.c_str()); continue; }
        printf("ok %u %d %d %llu %ld\n", h.count, h.start_id, h.end_id, (unsigned long long)h.size, ftell(f.get()));
    }
    return 0;
}

static int do_plan(int argc, char **argv)
{
    if (argc < 3) return 2;
    std::vector<Header> hs;
    for (int i = 3; i < argc; ++i) {
        Header h;
        std::string err;
        if (!open_checked(argv[i], "check", h, err)) { printf("err %s\n", err.c_str()); return 0; }
        hs.push_back(h);
    }
    for (const Job &j : chunk_plan(hs, (uint32_t)strtoul(argv[2], nullptr, 10))) printf("%u %u %u\n", j.file, j.first, j.n);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (strcmp(argv[1], "write") == 0) return do_write(argc, argv);
    if (strcmp(argv[1], "open") == 0) return do_open(argc, argv);
    if (strcmp(argv[1], "plan") == 0) return do_plan(argc, argv);
    if (strcmp(argv[1], "name") == 0 && argc == 4) { printf("%s\n", policy_file(argv[2], (uint32_t)strtoul(argv[3], nullptr, 10)).c_str()); return 0; }
    return 2;
}
