// sm_map_set.h -- a listed set of map files, as far as it needs no device: the file index, the opening of a set that is read
// whole (the streamed renderers, the lidar) and of one that may be rewritten (the recall's MOVE, the warp), the per-file record
// of a rewrite with its temporary, the look-ahead loop over the chunk stream and the pass that puts the temporaries in place.
// Host only, like sm_mapfile.h: no HIP header, not sm_ctx.h (tests/cpp/mapset_check.cpp compiles it with a plain C++ compiler).
// Errors come back as text in `err`; `who` is the entry point that the message starts with.
#pragma once

#include "sm_mapfile.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>

namespace sm_mapset {

using sm_mapfile::Header, sm_mapfile::Job;

// false, with the message in `err`, for the first path that repeats an earlier one
inline bool check_distinct_paths(const char *const *paths, uint32_t n, const char *who, std::string &err)
{
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t k = 0; k < i; ++k)
            if (strcmp(paths[i], paths[k]) == 0) { err = sm_mapfile::said(who, paths[i], " is listed twice"); return false; }
    return true;
}

// What a context knows of the map files it has read or written: valid while the file has the size and mtime it was noted with.
class FileIndex {
public:
    // box of the rows' finite centres (lo > hi: none); largest non-NaN m[7] (-inf: none)
    struct Entry { uint64_t size; int64_t mtime_ns; float lo[3], hi[3]; float max_time; };
    // SM_RECALL_NO_INDEX=1: the opening of a rewrite looks nothing up (notes are made all the same); read per call
    static bool lookups_on() { const char *e = std::getenv("SM_RECALL_NO_INDEX"); return !(e && e[0] == '1'); }
    // the entry of `path` if the file is still the one that was noted, else null; h gets the file's size and mtime of now
    const Entry *valid(const std::string &path, Header &h) const
    {
        if (!sm_mapfile::stat_of(path, h)) return nullptr;
        const auto it = map_.find(path);
        return it != map_.end() && it->second.size == h.size && it->second.mtime_ns == h.mtime_ns ? &it->second : nullptr;
    }
    void note(const std::string &path, const Header &h, const float lo[3], const float hi[3], float max_time)
    {
        map_[path] = Entry{h.size, h.mtime_ns, {lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}, max_time};
    }
    // as the file is now (one the context has just written); a file that cannot be stat()ed has no entry
    void note_now(const std::string &path, const float lo[3], const float hi[3], float max_time)
    {
        Header h;
        sm_mapfile::stat_of(path, h) ? note(path, h, lo, hi, max_time) : erase(path);
    }
    void erase(const std::string &path) { map_.erase(path); }
private:
    std::map<std::string, Entry> map_;
};

// ---- a set that is read whole: every header checked against its file's length, in list order; false with the first bad file's
// message in `err`.  Plain and packed files may be mixed: a record's id is its position in the set either way.
struct ReadSet {
    std::vector<Header> files;
    std::vector<Job> jobs;             // the chunk plan
    std::vector<uint64_t> id_base;     // of each file's first record in the set
    uint64_t file_total = 0;           // records in all files
};
inline bool open_read_set(const char *const *paths, uint32_t n, uint32_t chunk, const char *who, ReadSet &set, std::string &err)
{
    set = ReadSet{std::vector<Header>(n), {}, std::vector<uint64_t>(n), 0};
    for (uint32_t i = 0; i < n; ++i) {
        if (!sm_mapfile::open_checked(paths[i], who, set.files[i], err, false, sm_mapfile::PACKED_OK)) return false;
        set.id_base[i] = set.file_total;
        set.file_total += set.files[i].count;
    }
    set.jobs = sm_mapfile::chunk_plan(set.files, chunk);
    return true;
}

// ---- a set that may be rewritten: one listed file through the call
struct MapFile {
    static constexpr float INF = __builtin_inff();
    std::string path;
    bool skipped = false;              // by the index or by the caller: not opened
    Header h;                          // count 0 unless the file is read
    float lo[3] = {INF, INF, INF}, hi[3] = {-INF, -INF, -INF};   // box of this read
    float tmax = -INF;                 // largest non-NaN time of this read
    uint32_t chunks_left = 0;          // of the plan, not yet through keep()
    // the temporary, opened by the first chunk that changes a row; a call that ends before the file is replaced removes it
    sm_mapfile::Writer tmp;
    bool tmp_done = false;             // complete and closed, not yet renamed
    ~MapFile() { if (tmp_done) std::remove(tmp.path().c_str()); }

    void fold(float lx, float ly, float lz, float hx, float hy, float hz, float t)
    {
        lo[0] = std::min(lo[0], lx); lo[1] = std::min(lo[1], ly); lo[2] = std::min(lo[2], lz);
        hi[0] = std::max(hi[0], hx); hi[1] = std::max(hi[1], hy); hi[2] = std::max(hi[2], hz);
        tmax = std::max(tmax, t);
    }
    // What stays of the chunk of job j: n rows at p.  The first chunk that `changed` opens "<path><suffix>" (header count
    // `count`, Writer::UNKNOWN = the rows appended) with the chunks before it, which changed nothing, from the file itself; an
    // open temporary gets the rows, and the file's last chunk commits it.  A file none of whose chunks changed gets no temporary.
    bool keep(const Job &j, const void *p, uint32_t n, bool changed, const char *suffix, uint32_t count, const char *who, std::string &err)
    {
        chunks_left--;
        if (changed && !tmp.is_open() && !(tmp.open(path + suffix, count, h.start_id, h.end_id, who, err) && tmp.append_head_of(path, j.first, err)))
            return false;
        if (!tmp.is_open()) return true;
        return tmp.append(p, n, err) && (chunks_left || (tmp_done = tmp.commit(err)));
    }
    void note_in(FileIndex &index) const { index.note(path, h, lo, hi, tmax); }
};

struct RewriteSet {
    std::vector<MapFile> files;        // by Job::file
    std::vector<Job> jobs;             // the chunk plan of the files that are read
    uint32_t listed = 0, skipped = 0, read = 0;
    bool packed_refused = false;       // the opening failed at a packed file that the caller does not take (`err` names it)
};

// Every file is checked before anything changes: skipped on its stat() alone where skip(entry) says so of its valid index
// entry (never asked while SM_RECALL_NO_INDEX=1, nor about `known_skip`, a file the caller knows it need not read, -1: none),
// else its header against its length.  false with the first bad file's message in `err`.  accept: PACKED_OK for a call that
// only reads (a packed file is never rewritten); PLAIN_ONLY refuses a packed file by name and says so in set.packed_refused.
template <typename Skip>
bool open_rewrite_set(const char *const *paths, uint32_t n, uint32_t chunk, const FileIndex &index, int64_t known_skip, Skip skip, const char *who,
                      RewriteSet &set, std::string &err, sm_mapfile::Accept accept = sm_mapfile::PLAIN_ONLY)
{
    const bool use_index = FileIndex::lookups_on();
    set.files = std::vector<MapFile>(n);
    set.listed = n;
    std::vector<Header> headers(n);                      // (count 0: a file that is not read)
    for (uint32_t i = 0; i < n; ++i) {
        MapFile &mf = set.files[i];
        mf.path = paths[i];
        mf.skipped = (int64_t)i == known_skip;
        if (!mf.skipped && use_index)
            if (const FileIndex::Entry *e = index.valid(mf.path, mf.h)) mf.skipped = skip(*e);
        if (mf.skipped) { set.skipped++; continue; }
        if (!sm_mapfile::open_checked(mf.path, who, mf.h, err, false, accept)) {
            if (accept == sm_mapfile::PLAIN_ONLY && sm_mapfile::looks_packed(mf.path)) {
                set.packed_refused = true;
                err = sm_mapfile::said(who, mf.path, " is a packed map file, which is never rewritten; sm_unpack_maps makes a plain one");
            }
            return false;
        }
        headers[i] = mf.h;
        set.read++;
    }
    set.jobs = sm_mapfile::chunk_plan(headers, chunk);
    for (const Job &j : set.jobs) set.files[j.file].chunks_left++;
    return true;
}

// The look-ahead loop: enqueue(chunk c) -- the host reads chunk c while the device works on chunk c - 1 -- then finish(chunk
// c - 1) -- ... and writes what stays of chunk c - 1 while it works on chunk c; the last chunk is finished after the loop.  It
// stops at the first non-zero return, and nothing is finished that was not enqueued.  Stream: MapStream (sm_map_stream.h).
template <typename Stream, typename Enqueue, typename Finish>
int stream_files(Stream &in, const std::vector<Job> &jobs, Enqueue enqueue, Finish finish)
{
    int rc;
    typename Stream::Chunk cur{}, prev{};
    for (in.begin(jobs); in.more(); prev = cur) {
        if ((rc = enqueue(cur))) return rc;
        if (prev.job && (rc = finish(prev))) return rc;
    }
    return prev.job ? finish(prev) : 0;
}

// The files, last: every finished temporary is renamed over its file, and the index gets the file as it is now with the box
// and time of this read (no entry if it cannot be stat()ed).  A rename that fails is failed(file)'s to report and does not stop
// the others; its temporary is left in place (leave_tmp) or goes with the file's record.  Returns the files replaced.
template <typename Failed>
uint32_t replace_files(std::vector<MapFile> &files, FileIndex &index, bool leave_tmp, Failed failed)
{
    uint32_t replaced = 0;
    for (MapFile &mf : files) {
        if (!mf.tmp_done) continue;
        if (leave_tmp) mf.tmp_done = false;
        if (std::rename(mf.tmp.path().c_str(), mf.path.c_str()) != 0) { failed(mf); continue; }
        mf.tmp_done = false;
        replaced++;
        if (sm_mapfile::stat_of(mf.path, mf.h)) mf.note_in(index);
        else index.erase(mf.path);
    }
    return replaced;
}

}  // namespace sm_mapset
