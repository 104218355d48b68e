// sm_map_stream.h -- private to the sources that read map files ($(MAPS) in csrc/Makefile names them; sm_scene.hip takes the planes'
// layout and the file format from here, no stream): the double-buffered stream of map-file chunks through the context's
// MapStaging, one object per call; behind it what the readers of whole sets do alike: the opening (maps_open; its tail
// maps_counts also ends the openings with rules of their own -- sm_set_call.h's, the calls on two sets) and the batch of views
// (maps_batch), the opening of two sets (check_sets, open_sets) and the pass over a set that only launches (maps_feed).  Chunk c
// of a pass goes through buffer q = c & 1: read into h_rec[q] (timed into read_ms), copied on `copy` into d_rec[q], and the
// context's stream waits for the copy; the caller then launches its kernels on d_rec[q] and says done(q).  fold(q) waits for them
// and adds the buffer's event times to the caller's tally.  The host reads chunk c while chunk c - 1 is on the device: next()
// waits only for chunk c - 2, the last user of its buffer, and that one wait frees both sides (the copy out of h_rec[q] and the
// kernels that read d_rec[q] precede the event).  A chunk of a PACKED file (sm_mapfile.h) takes the same way with fewer bytes: the
// directory slice of its blocks and their payload are read (h_dir[q], h_rec[q]) and copied (d_dir[q], d_pk[q]), and the context's
// stream decodes them into d_rec[q] before the start of the caller's kernels is marked; the decode's time counts as copy_ms.
#pragma once

#include "sm_ctx.h"
#include "sm_k_maps_box.h"

#include <cstdlib>

namespace sm_impl __attribute__((visibility("hidden"))) {

// a switch of the environment, read per call: on iff the variable begins with 1
inline bool env_is_one(const char *name)
{
    const char *e = std::getenv(name);
    return e && e[0] == '1';
}

inline MapsSoA planes(const MapStaging &st) { return {st.d_pos_conf, st.d_norm_rad, st.d_color, st.d_time}; }

class MapStream {
public:
    struct Tally { float *read_ms, *copy_ms, *device_ms; };
    struct Chunk { int q; const sm_mapfile::Job *job; const float4 *d_rec; };

    // paths: by Job::file.  The staging exists (maps_ensure_staging) before the first next().
    MapStream(sm_ctx *s, const char *who, const char *const *paths, Tally t) : s_(s), st_(s->staging), who_(who), paths_(paths), t_(t) {}
    // A stream that goes away with a chunk in flight -- any failed call -- drains `copy` and the context's stream, nothing wider.
    ~MapStream()
    {
        if (!in_flight_[0] && !in_flight_[1]) return;
        (void)hipStreamSynchronize(st_.copy);
        (void)hipStreamSynchronize(s_->stream);
    }
    // a pass over `jobs` begins (nothing of an earlier pass is in flight: it ended with fold() of both buffers)
    void begin(const std::vector<sm_mapfile::Job> &jobs) { jobs_ = &jobs; c_ = 0; in_.reset(); in_file_ = NO_FILE; }
    // of the copy_ms folded so far: the decode of packed chunks
    float unpack_ms() const { return unpack_ms_; }
    bool more() const { return c_ < jobs_->size(); }

    // the next chunk: read, on its way to the device, the context's stream waiting for it, the start of its kernels marked
    int next(Chunk &ck)
    {
        const sm_mapfile::Job &j = (*jobs_)[c_];
        const int q = (int)(c_ & 1u);
        if (int rc = fold(q)) return rc;                 // buffer q is free on both sides
        if (in_file_ != j.file) {
            in_ = sm_mapfile::open_checked(paths_[j.file], who_, in_h_, g_err, false, sm_mapfile::PACKED_OK);
            in_file_ = j.file;
            if (!in_) return SM_E_ARG;
        }
        const sm_mapfile::Header &h = in_h_;
        // a packed file: the job's blocks (jobs begin at multiples of the chunk, so at a block) and their bytes in the payload
        const size_t b0 = j.first / sm_mapfile::PACK_BLOCK, nblk = ((size_t)j.n + sm_mapfile::PACK_BLOCK - 1) / sm_mapfile::PACK_BLOCK;
        uint64_t at = 0, bytes = 0;
        if (h.packed) {
            if ((uint64_t)j.first + j.n > h.count || j.first % sm_mapfile::PACK_BLOCK) { g_err = sm_mapfile::said(who_, paths_[j.file], " read err!! (changed while it was read)"); return SM_E_ARG; }
            if (int rc = maps_ensure_packed(s_)) return rc;
            const sm_mapfile::PackDir &last = h.dir[b0 + nblk - 1];
            at = h.dir[b0].offset;
            bytes = last.offset + sm_mapfile::pack_block_bytes(last.flags, j.n - (uint32_t)(nblk - 1) * sm_mapfile::PACK_BLOCK) - at;
            if (bytes > (uint64_t)MapStaging::CHUNK * sm_mapfile::RECORD_BYTES) { g_err = sm_mapfile::said(who_, paths_[j.file], " read err!!"); return SM_E_ARG; }
        }
        const double t0 = sm_mapfile::now_ms();
        bool got;
        if (h.packed) {
            memcpy(st_.h_dir[q].get(), h.dir.data() + b0, nblk * sm_mapfile::PACK_DIR_BYTES);
            got = fseeko(in_.get(), (off_t)(h.payload_at() + at), SEEK_SET) == 0 && (bytes == 0 || fread(st_.h_rec[q].get(), 1, bytes, in_.get()) == bytes);
        } else
            got = sm_mapfile::read_rows(in_.get(), st_.h_rec[q].get(), j.n);
        *t_.read_ms += (float)(sm_mapfile::now_ms() - t0);
        if (!got) { g_err = sm_mapfile::said(who_, paths_[j.file], " read err!!"); return SM_E_ARG; }
        in_flight_[q] = true;
        packed_[q] = h.packed;
        HIPCK(hipEventRecord(st_.ev_copy0[q], st_.copy));
        if (h.packed) {
            HIPCK(hipMemcpyAsync(st_.d_dir[q], st_.h_dir[q], nblk * sm_mapfile::PACK_DIR_BYTES, hipMemcpyHostToDevice, st_.copy));
            HIPCK(hipMemcpyAsync(st_.d_pk[q], st_.h_rec[q], bytes, hipMemcpyHostToDevice, st_.copy));
        } else
            HIPCK(hipMemcpyAsync(st_.d_rec[q], st_.h_rec[q], (size_t)j.n * sm_mapfile::RECORD_BYTES, hipMemcpyHostToDevice, st_.copy));
        HIPCK(hipEventRecord(st_.ev_copied[q], st_.copy));
        HIPCK(hipStreamWaitEvent(s_->stream, st_.ev_copied[q], 0));
        if (h.packed) {
            HIPCK(hipEventRecord(st_.ev_u0[q], s_->stream));
            maps_unpack(s_, st_.d_dir[q], st_.d_pk[q], j.n, h.pos_step_log2, st_.d_rec[q]);
            HIPCK(hipGetLastError());
            HIPCK(hipEventRecord(st_.ev_u1[q], s_->stream));
        }
        HIPCK(hipEventRecord(st_.ev_k0[q], s_->stream));
        ck = {q, &j, st_.d_rec[q].get()};
        ++c_;
        return SM_OK;
    }
    // the caller has launched everything that belongs to the chunk in buffer q
    int done(int q)
    {
        HIPCK(hipEventRecord(st_.ev_k1[q], s_->stream));
        return SM_OK;
    }
    // waits for the chunk in buffer q, if there is one, and folds its times into the tally
    int fold(int q)
    {
        if (!in_flight_[q]) return SM_OK;
        float ms = 0.0f;
        HIPCK(hipEventSynchronize(st_.ev_k1[q]));
        HIPCK(hipEventElapsedTime(&ms, st_.ev_copy0[q], st_.ev_copied[q]));
        *t_.copy_ms += ms;
        if (packed_[q]) {
            HIPCK(hipEventElapsedTime(&ms, st_.ev_u0[q], st_.ev_u1[q]));
            *t_.copy_ms += ms;
            unpack_ms_ += ms;
        }
        HIPCK(hipEventElapsedTime(&ms, st_.ev_k0[q], st_.ev_k1[q]));
        *t_.device_ms += ms;
        in_flight_[q] = false;
        return SM_OK;
    }

private:
    static constexpr uint32_t NO_FILE = 0xFFFFFFFFu;
    sm_ctx *s_;
    MapStaging &st_;
    const char *who_;
    const char *const *paths_;
    Tally t_;
    const std::vector<sm_mapfile::Job> *jobs_ = nullptr;
    size_t c_ = 0;                     // chunks handed out in this pass
    sm_mapfile::File in_;              // the file being read
    sm_mapfile::Header in_h_;          // ... and its header (a packed file's directory)
    bool packed_[2] = {false, false};  // the chunk in the buffer came from a packed file
    float unpack_ms_ = 0.0f;
    uint32_t in_file_ = NO_FILE;
    bool in_flight_[2] = {false, false};   // the buffer's events have been recorded and not yet folded
};

// The tail of every opening, once the headers of its n sets (1 or 2) are read: the device, the model compact and its count known
// (waits for frames in flight); per set the live surfels that take part (cnt) and the limit of its ids.
inline int maps_counts(sm_ctx *s, const char *fn, int n, const sm_map_source *const *src, const sm_mapset::ReadSet *const *set, uint32_t *cnt)
{
    int rc;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = ensure_compact(s)) || (rc = pull_state(s))) return rc;
    for (int i = 0; i < n; ++i) cnt[i] = src[i]->include_model ? s->h_state->count : 0u;
    for (int i = 0; i < n; ++i) {
        const uint64_t total = set[i]->file_total + cnt[i];
        if (total <= 0x7FFFFFFFull) continue;
        g_err = std::string(fn) + (n == 1 ? ": the map set holds " + std::to_string(total) + " surfels, ids end at 2^31 - 1" : ": a set of more than 2^31 - 1 records");
        return SM_E_CAPACITY;
    }
    return SM_OK;
}

// What sm_render_*_maps and sm_lidar_sweep* do between their own argument checks and their own scratch: `whole` (the entry
// point's own refusal of a context that holds a part of the map), the half-done cull, the source; every file's header against
// its length before the device is touched; then the tail above.  cnt: the live surfels that take part.
template <typename Whole>
int maps_open(sm_ctx *s, const sm_map_source *src, const char *fn, Whole whole, sm_mapset::ReadSet &set, uint32_t &cnt)
{
    int rc;
    if ((rc = whole(s, fn)) || (rc = check_not_mid_cull(s, fn)) || (rc = check_map_source(src, fn))) return rc;
    if (!sm_mapset::open_read_set(src->paths, src->n_paths, MapStaging::CHUNK, fn, set, g_err)) return SM_E_ARG;
    const sm_mapset::ReadSet *sets[1] = {&set};
    return maps_counts(s, fn, 1, &src, sets, &cnt);
}

// What a call on two sets asks of them, without the device (registration, change detection), in two steps so that a caller's own
// rules for its paths come between them: the sources and no path in both (check_sets), then every header of both (open_sets)
inline int check_sets(const sm_map_source *a, const sm_map_source *b, const char *who)
{
    int rc;
    if ((rc = check_map_source(a, who)) || (rc = check_map_source(b, who))) return rc;
    for (uint32_t i = 0; i < a->n_paths; ++i)
        for (uint32_t k = 0; k < b->n_paths; ++k)
            if (strcmp(a->paths[i], b->paths[k]) == 0) { g_err = sm_mapfile::said(who, a->paths[i], " is in both sets"); return SM_E_ARG; }
    return SM_OK;
}
inline int open_sets(const sm_map_source *a, const sm_map_source *b, const char *who, sm_mapset::ReadSet &aset, sm_mapset::ReadSet &bset)
{
    if (!sm_mapset::open_read_set(a->paths, a->n_paths, MapStaging::CHUNK, who, aset, g_err)) return SM_E_ARG;
    if (!sm_mapset::open_read_set(b->paths, b->n_paths, MapStaging::CHUNK, who, bset, g_err)) return SM_E_ARG;
    return SM_OK;
}

// One pass over a set that only launches: launch(d_rec, n, gid0) for every chunk of the files (paths: the source's), through a
// stream of its own with the tally t, then for every chunk of the `cnt` live records at d_model; gid0: the set id of the chunk's
// first record.  model_begins is recorded between the two; the caller marks the end of that stretch once everything it counts
// into it is enqueued.
template <typename Launch>
int maps_feed(sm_ctx *s, const char *who, const sm_mapset::ReadSet &set, const char *const *paths, uint32_t cnt, const float4 *d_model,
              MapStream::Tally t, const Event &model_begins, Launch launch)
{
    int rc;
    MapStream in(s, who, paths, t);
    for (in.begin(set.jobs); in.more();) {
        MapStream::Chunk ck;
        if ((rc = in.next(ck))) return rc;
        launch(ck.d_rec, ck.job->n, (uint32_t)(set.id_base[ck.job->file] + ck.job->first));
        if ((rc = in.done(ck.q))) return rc;
        HIPCK(hipGetLastError());
    }
    if ((rc = in.fold(0)) || (rc = in.fold(1)) || (rc = mark(s, model_begins))) return rc;
    for (uint32_t first = 0; first < cnt; first += MapStaging::CHUNK)
        launch(d_model + (size_t)first * 3, std::min(MapStaging::CHUNK, cnt - first), (uint32_t)set.file_total + first);
    return SM_OK;
}

// Views (sweeps) per pass over the files: all of them, at most 4096, at most what <key_mb_var> MiB (default 1024, 1..8192: at
// most 2^30 keys per batch) hold at `keys` 8-byte keys per view.  *cull: 0 with <no_cull_var>=1, the splat then tests every block.
inline uint32_t maps_batch(uint32_t views, size_t keys, const char *key_mb_var, const char *no_cull_var, int *cull)
{
    const char *k = std::getenv(key_mb_var);
    *cull = env_is_one(no_cull_var) ? 0 : 1;
    const size_t key_mb = k ? (size_t)std::min(8192L, std::max(1L, std::atol(k))) : 1024;
    return (uint32_t)std::min<uint64_t>(std::min<uint32_t>(views, 4096u), std::max<uint64_t>(1, (key_mb << 20) / (keys * 8)));
}

}  // namespace sm_impl
