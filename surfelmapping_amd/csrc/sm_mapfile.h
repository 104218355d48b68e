// sm_mapfile.h -- the map-file format, once: u32 count | i32 startId | i32 endId | count records of 12 fp32
// (src/GlobalModel.cpp:927-932).  The checked open, the writer and the chunk plan that every reader and writer of map files in
// the core goes through.  Host only: no HIP header, not sm_ctx.h (tests/cpp/mapfile_check.cpp compiles it with a plain C++
// compiler).  Errors come back as text in `err`, which the callers move into g_err; `who` (may be null) is the entry point that
// the message starts with.
#pragma once

#include <cstdint>
#include <cstdio>
#include <ctime>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>

namespace sm_mapfile {

constexpr uint64_t HEADER_BYTES = 12, RECORD_BYTES = 48;

struct FileCloser { void operator()(FILE *f) const { if (f) fclose(f); } };
using File = std::unique_ptr<FILE, FileCloser>;

inline double now_ms()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);                 // (the steady clock)
    return (double)ts.tv_sec * 1.0e3 + (double)ts.tv_nsec * 1.0e-6;
}

// file number i of the periodic retirement policy
inline std::string policy_file(const std::string &prefix, uint32_t i)
{
    char name[32];
    snprintf(name, sizeof name, "_%06u.bin", i);
    return prefix + name;
}

inline std::string said(const char *who, const std::string &path, const char *what)
{
    return (who ? std::string(who) + ": " : std::string()) + path + what;
}

struct Header {
    uint32_t count = 0;
    int32_t start_id = 0, end_id = 0;
    uint64_t size = 0;                 // of the file, from fstat()
    int64_t mtime_ns = 0;
    void note(const struct stat &sb)
    {
        size = (uint64_t)sb.st_size;
        mtime_ns = (int64_t)sb.st_mtim.tv_sec * 1000000000ll + (int64_t)sb.st_mtim.tv_nsec;
    }
};

// size and mtime of the file now, as its checked open would report them; false if it cannot be stat()ed
inline bool stat_of(const std::string &path, Header &h)
{
    struct stat sb;
    if (stat(path.c_str(), &sb) != 0) return false;
    h.note(sb);
    return true;
}

// The file open for reading, positioned at its first record, with its header checked against its length; null with `err` set
// otherwise.  lenient (sm_load_map alone, the reference's own reader): bytes after the last record are accepted, and a file too
// short for its header or its records is "<path> read err!!" as that entry point has always said.
inline File open_checked(const std::string &path, const char *who, Header &h, std::string &err, bool lenient = false)
{
    File f(fopen(path.c_str(), "rb"));
    if (!f) { err = said(who, path, " is not open!"); return nullptr; }
    uint32_t hdr[3];
    struct stat sb;
    if (fread(hdr, 4, 3, f.get()) != 3 || fstat(fileno(f.get()), &sb) != 0) {
        err = said(who, path, lenient ? " read err!!" : " read err!! (no header)");
        return nullptr;
    }
    const uint64_t size = (uint64_t)sb.st_size, want = HEADER_BYTES + RECORD_BYTES * hdr[0];
    if (lenient ? size < want : size != want) {
        err = lenient ? said(who, path, " read err!!")
                      : said(who, path, " holds ") + std::to_string(size) + " bytes, its header's " + std::to_string(hdr[0]) + " records need " +
                            std::to_string(want);
        return nullptr;
    }
    h.count = hdr[0]; h.start_id = (int32_t)hdr[1]; h.end_id = (int32_t)hdr[2];
    h.note(sb);
    return f;
}

// the next n records of a file from open_checked
inline bool read_rows(FILE *f, void *dst, size_t n) { return n == 0 || fread(dst, RECORD_BYTES, n, f) == n; }

// One map file being written: the header, rows appended in any number of pieces, commit().  A writer that goes away without a
// successful commit() removes its file, so no reader ever meets a half-written one.
class Writer {
public:
    static constexpr uint32_t UNKNOWN = 0xFFFFFFFFu;     // count: commit() writes the number of rows appended
    ~Writer() { discard(); }
    bool open(const std::string &path, uint32_t count, int32_t start_id, int32_t end_id, const char *who, std::string &err)
    {
        discard();
        path_ = path; who_ = who; count_ = count; rows_ = 0;
        f_.reset(fopen(path.c_str(), "wb"));
        if (!f_) { err = said(who, path, " is not open!"); return false; }
        const uint32_t hdr[3] = {count == UNKNOWN ? 0u : count, (uint32_t)start_id, (uint32_t)end_id};
        return fwrite(hdr, 4, 3, f_.get()) == 3 || fail(err);
    }
    bool append(const void *rows, size_t n, std::string &err)
    {
        if (!f_ || (n && fwrite(rows, RECORD_BYTES, n, f_.get()) != n)) return fail(err);
        rows_ += n;
        return true;
    }
    // the first n records of the map file `from`, as they are
    bool append_head_of(const std::string &from, uint64_t n, std::string &err)
    {
        File in(fopen(from.c_str(), "rb"));
        if (!in || fseek(in.get(), (long)HEADER_BYTES, SEEK_SET) != 0) return fail(err);
        std::vector<char> buf((size_t)RECORD_BYTES << 14);
        for (uint64_t left = n; left;) {
            const size_t m = left < ((uint64_t)1 << 14) ? (size_t)left : (size_t)1 << 14;
            if (!read_rows(in.get(), buf.data(), m) || !append(buf.data(), m, err)) return fail(err);
            left -= m;
        }
        return true;
    }
    // completes the header, closes the file; true = the file is whole and stays
    bool commit(std::string &err)
    {
        if (!f_) return fail(err);
        bool ok = count_ == UNKNOWN ? rows_ <= 0xFFFFFFFFull : rows_ == count_;
        if (ok && count_ == UNKNOWN) {
            const uint32_t n = (uint32_t)rows_;
            ok = fseek(f_.get(), 0, SEEK_SET) == 0 && fwrite(&n, 4, 1, f_.get()) == 1;
        }
        ok = (fclose(f_.release()) == 0) && ok;
        if (!ok) { std::remove(path_.c_str()); return fail(err); }
        return true;
    }
    bool is_open() const { return (bool)f_; }
    uint64_t rows() const { return rows_; }
    const std::string &path() const { return path_; }

private:
    void discard()
    {
        if (f_) { f_.reset(); std::remove(path_.c_str()); }
    }
    bool fail(std::string &err)
    {
        discard();
        err = said(who_, path_, " saved err!!");
        return false;
    }
    File f_;
    std::string path_;
    const char *who_ = nullptr;
    uint32_t count_ = 0;
    uint64_t rows_ = 0;
};

// The chunk plan: the records of the listed files, in order, in jobs of at most `chunk` records.  A job never spans two files;
// an empty file has none.
struct Job { uint32_t file, first, n; };

inline std::vector<Job> chunk_plan(const std::vector<Header> &files, uint32_t chunk)
{
    std::vector<Job> jobs;
    for (uint32_t i = 0; i < (uint32_t)files.size(); ++i)
        for (uint64_t first = 0; first < files[i].count; first += chunk)
            jobs.push_back({i, (uint32_t)first, (uint32_t)(files[i].count - first < chunk ? files[i].count - first : chunk)});
    return jobs;
}

}  // namespace sm_mapfile
