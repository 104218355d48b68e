// mapset_check.cpp -- drives surfelmapping_amd/csrc/sm_map_set.h alone for tests/test_mapset_cpu.py: no HIP header, any C++17
// compiler.  One session per run: commands come one per line on stdin (words separated by blanks), so that the test can change
// files between two of them while the index and the opened set live on; every answer is some lines and then a line ".".
//   note <path> <max_time>                  the index notes the file with the header of its stat() now (box 1 2 3 | 4 5 6)
//   note_now <path> <max_time>              ... as the file is now, or erases
//   erase <path>
//   valid <path>                            "valid <size> <mtime_ns> <max_time>" or "none"
//   distinct <who> <path> ...               "ok" or "err <message>"
//   read <chunk> <path> ...                 the set that is read whole: "file <i> <count> <id_base>", "job <file> <first> <n>", "total <n>"
//   rewrite <chunk> <known_skip> <t0> <path> ...   the set that may be rewritten, skipping entries with max_time < t0:
//                                           "counters <listed> <skipped> <read>", "file <i> <skipped> <count> <chunks_left>", "job ..."
//   keep <job> <changed> <suffix> <count|unknown|file> <rows file> <n>   MapFile::keep of the first n rows of the rows file
//   drop                                    the opened set goes away
//   replace <leave|remove>                  the replacement pass: "replaced <n> first <path of the first failure|->"
//   lookahead <jobs> <enqueue fails at|-1> <finish fails at|-1>          the look-ahead loop over a fake stream: "e0 e1 f0 ... rc <rc>"
#include "sm_map_set.h"

#include <iostream>
#include <sstream>

using namespace sm_mapset;

// what stream_files asks of a stream
struct FakeStream {
    struct Chunk { const Job *job; int c; };
    const std::vector<Job> *jobs = nullptr;
    size_t c = 0;
    void begin(const std::vector<Job> &j) { jobs = &j; c = 0; }
    bool more() const { return c < jobs->size(); }
};

static std::vector<char> slurp(const std::string &path)
{
    std::vector<char> all;
    sm_mapfile::File in(fopen(path.c_str(), "rb"));
    char buf[4096];
    if (in) for (size_t k; (k = fread(buf, 1, sizeof buf, in.get())) > 0;) all.insert(all.end(), buf, buf + k);
    return all;
}

int main()
{
    FileIndex index;
    std::unique_ptr<RewriteSet> set;
    const float lo[3] = {1, 2, 3}, hi[3] = {4, 5, 6};
    std::string line, err;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::vector<std::string> a;
        for (std::string w; in >> w;) a.push_back(w);
        if (a.empty()) continue;
        std::vector<const char *> paths;
        auto paths_from = [&](size_t k) { for (; k < a.size(); ++k) paths.push_back(a[k].c_str()); };
        const std::string &cmd = a[0];
        if (cmd == "note" && a.size() == 3) {
            sm_mapfile::Header h;
            if (sm_mapfile::stat_of(a[1], h)) { index.note(a[1], h, lo, hi, strtof(a[2].c_str(), nullptr)); printf("ok\n"); }
            else printf("err no file\n");
        } else if (cmd == "note_now" && a.size() == 3) {
            index.note_now(a[1], lo, hi, strtof(a[2].c_str(), nullptr));
            printf("ok\n");
        } else if (cmd == "erase" && a.size() == 2) {
            index.erase(a[1]);
            printf("ok\n");
        } else if (cmd == "valid" && a.size() == 2) {
            sm_mapfile::Header h;
            if (const FileIndex::Entry *e = index.valid(a[1], h))
                printf("valid %llu %lld %g\n", (unsigned long long)h.size, (long long)h.mtime_ns, (double)e->max_time);
            else printf("none\n");
        } else if (cmd == "distinct" && a.size() >= 2) {
            paths_from(2);
            if (check_distinct_paths(paths.data(), (uint32_t)paths.size(), a[1].c_str(), err)) printf("ok\n");
            else printf("err %s\n", err.c_str());
        } else if (cmd == "read" && a.size() >= 2) {
            paths_from(2);
            ReadSet rs;
            if (!open_read_set(paths.data(), (uint32_t)paths.size(), (uint32_t)strtoul(a[1].c_str(), nullptr, 10), "check", rs, err)) printf("err %s\n", err.c_str());
            else {
                for (size_t i = 0; i < rs.files.size(); ++i) printf("file %zu %u %llu\n", i, rs.files[i].count, (unsigned long long)rs.id_base[i]);
                for (const Job &j : rs.jobs) printf("job %u %u %u\n", j.file, j.first, j.n);
                printf("total %llu\n", (unsigned long long)rs.file_total);
            }
        } else if (cmd == "rewrite" && a.size() >= 4) {
            paths_from(4);
            const float t0 = strtof(a[3].c_str(), nullptr);
            set.reset(new RewriteSet);
            if (!open_rewrite_set(paths.data(), (uint32_t)paths.size(), (uint32_t)strtoul(a[1].c_str(), nullptr, 10), index, atoll(a[2].c_str()),
                                  [&](const FileIndex::Entry &e) { return e.max_time < t0; }, "check", *set, err)) {
                printf("err %s\n", err.c_str());
                set.reset();
            } else {
                printf("counters %u %u %u\n", set->listed, set->skipped, set->read);
                for (size_t i = 0; i < set->files.size(); ++i)
                    printf("file %zu %d %u %u\n", i, (int)set->files[i].skipped, set->files[i].h.count, set->files[i].chunks_left);
                for (const Job &j : set->jobs) printf("job %u %u %u\n", j.file, j.first, j.n);
            }
        } else if (cmd == "keep" && a.size() == 7 && set) {
            const Job &j = set->jobs.at(strtoul(a[1].c_str(), nullptr, 10));
            MapFile &mf = set->files[j.file];
            const uint32_t n = (uint32_t)strtoul(a[6].c_str(), nullptr, 10);
            const uint32_t count = a[4] == "unknown" ? sm_mapfile::Writer::UNKNOWN : a[4] == "file" ? mf.h.count : (uint32_t)strtoul(a[4].c_str(), nullptr, 10);
            const std::vector<char> rows = slurp(a[5]);
            if (rows.size() < (size_t)n * sm_mapfile::RECORD_BYTES) return 2;
            if (mf.keep(j, rows.data(), n, a[2] == "1", a[3].c_str(), count, "check", err)) printf("ok %d %d %u\n", (int)mf.tmp.is_open(), (int)mf.tmp_done, mf.chunks_left);
            else printf("err %s\n", err.c_str());
        } else if (cmd == "drop") {
            set.reset();
            printf("ok\n");
        } else if (cmd == "replace" && a.size() == 2 && set) {
            std::string first = "-";
            const uint32_t n = replace_files(set->files, index, a[1] == "leave", [&](const MapFile &mf) { if (first == "-") first = mf.path; });
            printf("replaced %u first %s\n", n, first.c_str());
        } else if (cmd == "lookahead" && a.size() == 4) {
            std::vector<Job> jobs((size_t)atoi(a[1].c_str()), Job{0, 0, 1});
            const int bad_e = atoi(a[2].c_str()), bad_f = atoi(a[3].c_str());
            FakeStream fs;
            std::string seq;
            const int rc = stream_files(fs, jobs,
                                        [&](FakeStream::Chunk &ck) {
                                            if ((int)fs.c == bad_e) return 7;
                                            ck = {&jobs[fs.c], (int)fs.c};
                                            seq += "e" + std::to_string(fs.c++) + " ";
                                            return 0;
                                        },
                                        [&](const FakeStream::Chunk &ck) {
                                            if (ck.c == bad_f) return 9;
                                            seq += "f" + std::to_string(ck.c) + " ";
                                            return 0;
                                        });
            printf("%src %d\n", seq.c_str(), rc);
        } else return 2;
        printf(".\n");
        fflush(stdout);
    }
    return 0;
}
