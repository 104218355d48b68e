// packfile_check.cpp -- drives the packed map-file format of surfelmapping_amd/csrc/sm_mapfile.h alone for tests/test_pack_cpu.py:
// no HIP header, any C++17 compiler (the test builds it with the address and undefined-behaviour sanitizers).  One command per
// run; the result goes to stdout as one line per item, "ok ..." or "err <message>".
//   open   <plain|both> <path> ...   the checked open of each path, as a caller that takes plain files only or both formats:
//                                    ok <packed> <count> <startId> <endId> <size> <position> <blocks> <raw blocks> <pos_step_log2>
//   decode <path> <out>              the records of a packed file, decoded on the host, as count x 12 floats into <out>
//   looks  <path> ...                whether each path begins as a packed file does
#include "sm_mapfile.h"

#include <cstdlib>
#include <cstring>

using namespace sm_mapfile;

static int do_open(int argc, char **argv)
{
    if (argc < 3) return 2;
    const Accept accept = strcmp(argv[2], "both") == 0 ? PACKED_OK : PLAIN_ONLY;
    for (int i = 3; i < argc; ++i) {
        Header h;
        std::string err;
        File f = open_checked(argv[i], "check", h, err, false, accept);
        if (!f) { printf("err %s\n", err.c_str()); continue; }
        unsigned raw = 0;
        for (const PackDir &d : h.dir) raw += d.flags & PACK_RAW;
        printf("ok %d %u %d %d %llu %ld %zu %u %d\n", h.packed ? 1 : 0, h.count, h.start_id, h.end_id, (unsigned long long)h.size, ftell(f.get()),
               h.dir.size(), raw, h.pos_step_log2);
    }
    return 0;
}

static int do_decode(int argc, char **argv)
{
    if (argc != 4) return 2;
    Header h;
    std::string err;
    File f = open_checked(argv[2], "check", h, err, false, PACKED_OK);
    if (!f || !h.packed) { printf("err %s\n", f ? "not a packed file" : err.c_str()); return 0; }
    std::vector<float> rows((size_t)h.count * 12);
    if (!read_packed_rows(f.get(), h, rows.data())) { printf("err read\n"); return 0; }
    File out(fopen(argv[3], "wb"));
    if (!out || (!rows.empty() && fwrite(rows.data(), 4, rows.size(), out.get()) != rows.size())) return 2;
    printf("ok %u\n", h.count);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (strcmp(argv[1], "open") == 0) return do_open(argc, argv);
    if (strcmp(argv[1], "decode") == 0) return do_decode(argc, argv);
    if (strcmp(argv[1], "looks") == 0) {
        for (int i = 2; i < argc; ++i) printf("%d\n", looks_packed(argv[i]) ? 1 : 0);
        return 0;
    }
    return 2;
}
