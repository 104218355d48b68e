// sm_mapfile.h -- the map-file format, once: u32 count | i32 startId | i32 endId | count records of 12 fp32
// (src/GlobalModel.cpp:927-932).  The checked open, the writer and the chunk plan that every reader and writer of map files in
// the core goes through.  Host only: no HIP header, not sm_ctx.h (tests/cpp/mapfile_check.cpp compiles it with a plain C++
// compiler).  Errors come back as text in `err`, which the callers move into g_err; `who` (may be null) is the entry point that
// the message starts with.
//
// Beside it the packed format (include/sm_c_api.h "packed map files"; tests/pack_ref.py restates its codec): a 32-byte header
// "SMPK" | version | count | startId | endId | pos_step_log2 | n_blocks | 0, a directory of one 32-byte entry per block of 256
// records, then the blocks' payload, 20 bytes a record (or the 48 verbatim of a RAW block).  open_checked tells the two apart
// and checks either as strictly; only the callers that say PACKED_OK ever see a packed file.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>

namespace sm_mapfile {

constexpr uint64_t HEADER_BYTES = 12, RECORD_BYTES = 48;
// the packed format
constexpr uint32_t PACK_MAGIC = 0x4B504D53u, PACK_VERSION = 1u, PACK_BLOCK = 256u;      // ("SMPK")
constexpr uint64_t PACK_HEADER_BYTES = 32, PACK_DIR_BYTES = 32, PACK_RECORD_BYTES = 20;
constexpr int32_t PACK_STEP_MIN = -14, PACK_STEP_MAX = -6, PACK_STEP_DEFAULT = -10;
constexpr uint32_t PACK_RAW = 1u;                        // PackDir::flags: the block's records are stored verbatim
struct PackDir {
    float origin[3], time_base, init_base;
    uint32_t flags;
    uint64_t offset;                   // of the block in the payload
};
static_assert(sizeof(PackDir) == PACK_DIR_BYTES, "a directory entry is 32 bytes");
// bytes of a block of m records in the payload
inline uint64_t pack_block_bytes(uint32_t flags, uint32_t m) { return (uint64_t)m * ((flags & PACK_RAW) ? RECORD_BYTES : PACK_RECORD_BYTES); }

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
    bool packed = false;               // a packed file: the members below
    int32_t pos_step_log2 = 0;
    std::vector<PackDir> dir;          // one entry per block of 256 records, checked against the file's length
    uint64_t payload_at() const { return PACK_HEADER_BYTES + PACK_DIR_BYTES * dir.size(); }
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

// what a caller of open_checked takes: plain files alone (sm_load_map, a scene's actor files, a set that may be rewritten), or both
enum Accept { PLAIN_ONLY, PACKED_OK };

// the rest of a packed file's checked open: hdr[0..2] are read, the magic seen
inline File open_packed_rest(File f, const uint32_t *hdr3, const struct stat &sb, const std::string &path, const char *who, Header &h, std::string &err)
{
    const auto bad = [&](const std::string &what) { err = said(who, path, " is a packed map file, but ") + what; return File(); };
    const uint64_t size = (uint64_t)sb.st_size;
    uint32_t hdr[8] = {hdr3[0], hdr3[1], hdr3[2]};
    if (size < PACK_HEADER_BYTES || fread(hdr + 3, 4, 5, f.get()) != 5) return bad("too short for its header");
    if (hdr[1] != PACK_VERSION) return bad("of version " + std::to_string(hdr[1]) + ", not " + std::to_string(PACK_VERSION));
    const uint32_t count = hdr[2], n_blocks = hdr[6];
    const int32_t step = (int32_t)hdr[5];
    if (hdr[7] != 0) return bad("its reserved word is not 0");
    if (step < PACK_STEP_MIN || step > PACK_STEP_MAX) return bad("its pos_step_log2 is outside -14..-6");
    if (n_blocks != (uint32_t)(((uint64_t)count + PACK_BLOCK - 1) / PACK_BLOCK)) return bad("its header's " + std::to_string(count) + " records need another number of blocks than " + std::to_string(n_blocks));
    if (size < PACK_HEADER_BYTES + PACK_DIR_BYTES * n_blocks) return bad("too short for its directory");
    h.dir.resize(n_blocks);
    if (n_blocks && fread(h.dir.data(), PACK_DIR_BYTES, n_blocks, f.get()) != n_blocks) return bad("its directory cannot be read");
    uint64_t at = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const PackDir &d = h.dir[b];
        if (d.flags & ~PACK_RAW) return bad("block " + std::to_string(b) + " has unknown flags");
        if (d.offset != at) return bad("block " + std::to_string(b) + " lies at offset " + std::to_string(d.offset) + ", the blocks before it end at " + std::to_string(at));
        at += pack_block_bytes(d.flags, std::min<uint64_t>(PACK_BLOCK, (uint64_t)count - (uint64_t)b * PACK_BLOCK));
    }
    const uint64_t want = PACK_HEADER_BYTES + PACK_DIR_BYTES * n_blocks + at;
    if (size != want) return bad("it holds " + std::to_string(size) + " bytes, its directory needs " + std::to_string(want));
    h.count = count; h.start_id = (int32_t)hdr[3]; h.end_id = (int32_t)hdr[4];
    h.packed = true; h.pos_step_log2 = step;
    h.note(sb);
    return f;
}

// The file open for reading, positioned at its first record (a packed one: at its payload), with its header checked against its
// length; null with `err` set otherwise.  lenient (sm_load_map alone, the reference's own reader): bytes after the last record are
// accepted, and a file too short for its header or its records is "<path> read err!!" as that entry point has always said.
// A file that begins with the packed format's magic is a packed one unless it has the very length of a plain file of that many
// records (60 GB): PACKED_OK callers get it checked as strictly as a plain one -- the offsets of its directory are the prefix
// sums of its blocks' sizes and its length is exactly what they imply --, the others the refusal that names the way out.
inline File open_checked(const std::string &path, const char *who, Header &h, std::string &err, bool lenient = false, Accept accept = PLAIN_ONLY)
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
    h.packed = false; h.pos_step_log2 = 0; h.dir.clear();
    if (hdr[0] == PACK_MAGIC && size != want) {
        if (accept == PACKED_OK) return open_packed_rest(std::move(f), hdr, sb, path, who, h, err);
        err = said(who, path, " is a packed map file; sm_unpack_maps makes a plain one");
        return nullptr;
    }
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
// whether the file at `path` begins as a packed one does (no more is checked); false if it cannot be read
inline bool looks_packed(const std::string &path)
{
    File f(fopen(path.c_str(), "rb"));
    uint32_t magic = 0;
    struct stat sb;
    return f && fread(&magic, 4, 1, f.get()) == 1 && magic == PACK_MAGIC && fstat(fileno(f.get()), &sb) == 0 &&
           (uint64_t)sb.st_size != HEADER_BYTES + RECORD_BYTES * (uint64_t)PACK_MAGIC;
}

// The m records of a packed (not RAW) block decoded on the host as k_unpack (sm_k_pack.h) decodes them: w: m x 5 words, out:
// m x 12 floats.  IEEE fp32, one operation at a time (compile without contraction).
inline void unpack_block(const PackDir &d, const uint32_t *w, uint32_t m, int32_t pos_step_log2, float *out)
{
    const float down = std::ldexp(1.0f, pos_step_log2);
    for (uint32_t i = 0; i < m; ++i, w += 5, out += 12) {
        const uint32_t q[3] = {w[0] & 0xFFFFu, w[0] >> 16, w[1] & 0xFFFFu};
        for (int k = 0; k < 3; ++k) {
            const float step = (float)q[k] * down;
            out[k] = d.origin[k] + step;
        }
        out[3] = (float)(w[3] >> 20) * 0.0625f;
        memcpy(out + 4, w + 2, 4);
        out[5] = 0.0f;
        out[6] = d.init_base + (float)(w[4] >> 16);
        out[7] = d.time_base + (float)(w[4] & 0xFFFFu);
        // the normal: the fold in integers on the codes, then one fp32 normalisation
        const int ui = 2 * (int)(w[3] & 1023u) - 1023, vi = 2 * (int)((w[3] >> 10) & 1023u) - 1023;
        const int zi = 1023 - std::abs(ui) - std::abs(vi), t = std::max(-zi, 0);
        const int xi = ui >= 0 ? ui - t : ui + t, yi = vi >= 0 ? vi - t : vi + t;
        const float len = std::sqrt((float)(xi * xi + yi * yi + zi * zi));
        out[8] = (float)xi / len; out[9] = (float)yi / len; out[10] = (float)zi / len;
        out[11] = (float)(w[1] >> 16) * (1.0f / 8192.0f);
    }
}

// All records of a packed file from open_checked(PACKED_OK), decoded into out (count x 12 floats); false if the file cannot be read
inline bool read_packed_rows(FILE *f, const Header &h, float *out)
{
    std::vector<uint32_t> w(PACK_BLOCK * 5);
    if (fseeko(f, (off_t)h.payload_at(), SEEK_SET) != 0) return false;
    for (size_t b = 0; b < h.dir.size(); ++b) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(PACK_BLOCK, (uint64_t)h.count - b * PACK_BLOCK);
        float *dst = out + b * PACK_BLOCK * 12;
        if (h.dir[b].flags & PACK_RAW) {
            if (fread(dst, RECORD_BYTES, m, f) != m) return false;
            continue;
        }
        if (fread(w.data(), PACK_RECORD_BYTES, m, f) != m) return false;
        unpack_block(h.dir[b], w.data(), m, h.pos_step_log2, dst);
    }
    return true;
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
