// sm_fernfile.h -- place recognition's host-only parts (DESIGN.md "4l. Place recognition"): the rules of sm_fern_params, the fern
// table (sm_fern_table) and the keyframe file of sm_fern_save / sm_fern_load, each once.  Host only: no HIP header, not sm_ctx.h
// (tests/cpp/fernfile_check.cpp compiles it with a plain C++ compiler).  Errors come back as text in `err`, which the callers
// move into g_err.
//
// The keyframe file, little-endian, no padding:
//     offset  0  u32  magic 0x4E524653 ("SFRN")
//             4  u32  format version, 1
//             8  i32  n_ferns      12  i32  cell      16  u64  seed      24  i32  depth_lo_mm      28  i32  depth_hi_mm
//            32  i32  width        36  i32  height    40  u32  count     44  u32  0
//            48  count records of 68 + n_ferns / 2 bytes:  i32 time | 16 f32 pose (column-major) | n_ferns / 8 u32 code
// The file's length is exactly 48 + count * (68 + n_ferns / 2).
#pragma once

#include "../../include/sm_c_api.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>

namespace sm_fernfile {

constexpr uint32_t MAGIC = 0x4E524653u, VERSION = 1u;
constexpr uint64_t HEADER_BYTES = 48;

inline size_t code_words(const sm_fern_params &p) { return (size_t)p.n_ferns / 8; }
inline uint64_t record_bytes(const sm_fern_params &p) { return 68ull + (uint64_t)p.n_ferns / 2; }

// sm_fern_params' rules; null = fine, otherwise what is wrong
inline const char *check_params(const sm_fern_params &p)
{
    if (p.n_ferns < 32 || p.n_ferns > 2048 || p.n_ferns % 32 != 0) return "n_ferns is not a multiple of 32 in 32..2048";
    if (p.cell != 4 && p.cell != 8 && p.cell != 16 && p.cell != 32) return "cell is not 4, 8, 16 or 32";
    if (p.depth_lo_mm < 0 || p.depth_lo_mm >= p.depth_hi_mm || p.depth_hi_mm > 65535) return "depth thresholds outside 0 <= lo < hi <= 65535";
    return nullptr;
}

inline bool same_params(const sm_fern_params &a, const sm_fern_params &b)
{
    return a.n_ferns == b.n_ferns && a.cell == b.cell && a.seed == b.seed && a.depth_lo_mm == b.depth_lo_mm && a.depth_hi_mm == b.depth_hi_mm;
}

// splitmix64: one draw of [0, r)
struct SplitMix {
    uint64_t state;
    uint32_t draw(uint32_t r)
    {
        state += 0x9E3779B97F4A7C15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return (uint32_t)(((z >> 32) * (uint64_t)r) >> 32);
    }
};

// the table of sm_fern_table (arguments checked by the caller: check_params, gw and gh >= 1)
inline void make_table(const sm_fern_params &p, int width, int height, sm_fern *out)
{
    const uint32_t gw = (uint32_t)(width / p.cell), gh = (uint32_t)(height / p.cell);
    SplitMix g{p.seed};
    for (int f = 0; f < p.n_ferns; ++f) {
        sm_fern &o = out[f];
        o.x = (uint16_t)g.draw(gw);
        o.y = (uint16_t)g.draw(gh);
        o.tr = (uint16_t)g.draw(255u);
        o.tg = (uint16_t)g.draw(255u);
        o.tb = (uint16_t)g.draw(255u);
        o.td = (uint16_t)((uint32_t)p.depth_lo_mm + g.draw((uint32_t)(p.depth_hi_mm - p.depth_lo_mm)));
    }
}

struct Header {
    sm_fern_params p{};
    int32_t width = 0, height = 0;
    uint32_t count = 0;
};

inline void put_header(const Header &h, unsigned char *b)
{
    const uint32_t zero = 0u;
    memcpy(b, &MAGIC, 4); memcpy(b + 4, &VERSION, 4);
    memcpy(b + 8, &h.p.n_ferns, 4); memcpy(b + 12, &h.p.cell, 4); memcpy(b + 16, &h.p.seed, 8);
    memcpy(b + 24, &h.p.depth_lo_mm, 4); memcpy(b + 28, &h.p.depth_hi_mm, 4);
    memcpy(b + 32, &h.width, 4); memcpy(b + 36, &h.height, 4); memcpy(b + 40, &h.count, 4); memcpy(b + 44, &zero, 4);
}

struct FileCloser { void operator()(FILE *f) const { if (f) fclose(f); } };
using File = std::unique_ptr<FILE, FileCloser>;

// The file open for reading, positioned at its first record: magic, version, parameters, count (at most SM_FERN_MAX_KEYFRAMES)
// and the length checked.  Null with `err` set otherwise.
inline File open_checked(const std::string &path, Header &h, std::string &err)
{
    File f(fopen(path.c_str(), "rb"));
    if (!f) { err = path + " is not open!"; return nullptr; }
    unsigned char b[HEADER_BYTES];
    struct stat sb;
    if (fread(b, 1, HEADER_BYTES, f.get()) != HEADER_BYTES || fstat(fileno(f.get()), &sb) != 0) { err = path + " is too short for a keyframe file's header"; return nullptr; }
    uint32_t magic, version;
    memcpy(&magic, b, 4); memcpy(&version, b + 4, 4);
    if (magic != MAGIC || version != VERSION) { err = path + " is not a keyframe file of format version 1"; return nullptr; }
    memcpy(&h.p.n_ferns, b + 8, 4); memcpy(&h.p.cell, b + 12, 4); memcpy(&h.p.seed, b + 16, 8);
    memcpy(&h.p.depth_lo_mm, b + 24, 4); memcpy(&h.p.depth_hi_mm, b + 28, 4);
    memcpy(&h.width, b + 32, 4); memcpy(&h.height, b + 36, 4); memcpy(&h.count, b + 40, 4);
    if (const char *why = check_params(h.p)) { err = path + ": " + why; return nullptr; }
    if (h.width < h.p.cell || h.height < h.p.cell) { err = path + ": an image smaller than a cell"; return nullptr; }
    if (h.count > SM_FERN_MAX_KEYFRAMES) { err = path + " holds more than 2^20 keyframes"; return nullptr; }
    const uint64_t want = HEADER_BYTES + record_bytes(h.p) * h.count;
    if ((uint64_t)sb.st_size != want) {
        err = path + " holds " + std::to_string((uint64_t)sb.st_size) + " bytes, its header's " + std::to_string(h.count) + " keyframes need " + std::to_string(want);
        return nullptr;
    }
    return f;
}

// the records of a checked file into three planes (times: count, poses: count * 16, codes: count * n_ferns / 8)
inline bool read_records(FILE *f, const Header &h, int32_t *times, float *poses, uint32_t *codes, std::string &err, const std::string &path)
{
    const size_t words = code_words(h.p), rb = (size_t)record_bytes(h.p);
    std::vector<unsigned char> rec(rb);
    for (uint32_t k = 0; k < h.count; ++k) {
        if (fread(rec.data(), 1, rb, f) != rb) { err = path + " read err!!"; return false; }
        memcpy(times + k, rec.data(), 4);
        memcpy(poses + (size_t)k * 16, rec.data() + 4, 64);
        memcpy(codes + (size_t)k * words, rec.data() + 68, words * 4);
    }
    return true;
}

// the whole file through "<path>.tmp" in the same directory, renamed over `path` once it is complete
inline bool write_file(const std::string &path, const Header &h, const int32_t *times, const float *poses, const uint32_t *codes, std::string &err)
{
    const std::string tmp = path + ".tmp";
    File f(fopen(tmp.c_str(), "wb"));
    if (!f) { err = tmp + " is not open!"; return false; }
    const size_t words = code_words(h.p);
    unsigned char b[HEADER_BYTES];
    put_header(h, b);
    bool ok = fwrite(b, 1, HEADER_BYTES, f.get()) == HEADER_BYTES;
    for (uint32_t k = 0; ok && k < h.count; ++k)
        ok = fwrite(times + k, 4, 1, f.get()) == 1 && fwrite(poses + (size_t)k * 16, 4, 16, f.get()) == 16 &&
             fwrite(codes + (size_t)k * words, 4, words, f.get()) == words;
    ok = (fclose(f.release()) == 0) && ok;
    if (ok && std::rename(tmp.c_str(), path.c_str()) != 0) ok = false;
    if (!ok) { std::remove(tmp.c_str()); err = path + " saved err!!"; }
    return ok;
}

}  // namespace sm_fernfile
