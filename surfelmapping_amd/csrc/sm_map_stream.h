// sm_map_stream.h -- private to sm_render_maps.hip, sm_recall.hip and sm_warp.hip: the double-buffered stream of map-file chunks through
// RenderMaps' staging, one object per call.  Chunk c of a pass goes through buffer q = c & 1: read into h_rec[q] (timed into
// read_ms), copied on `copy` into d_rec[q], and the context's stream waits for the copy; the caller then launches its kernels on
// d_rec[q] and says done(q).  fold(q) waits for them and adds the buffer's event times to the caller's tally.  The host reads
// chunk c while chunk c - 1 is on the device: next() waits only for chunk c - 2, the last user of its buffer, and that one wait
// frees both sides (the copy out of h_rec[q] and the kernels that read d_rec[q] precede the event).
#pragma once

#include "sm_ctx.h"
#include "sm_mapfile.h"

namespace sm_impl __attribute__((visibility("hidden"))) {

class MapStream {
public:
    struct Tally { float *read_ms, *copy_ms, *device_ms; };
    struct Chunk { int q; const sm_mapfile::Job *job; const float4 *d_rec; };

    // paths: by Job::file.  The staging exists (maps_ensure_staging) before the first next().
    MapStream(sm_ctx *s, const char *who, const char *const *paths, Tally t) : s_(s), rm_(s->maps), who_(who), paths_(paths), t_(t) {}
    // A stream that goes away with a chunk in flight -- any failed call -- drains `copy` and the context's stream, nothing wider.
    ~MapStream()
    {
        if (!in_flight_[0] && !in_flight_[1]) return;
        (void)hipStreamSynchronize(rm_.copy);
        (void)hipStreamSynchronize(s_->stream);
    }
    // a pass over `jobs` begins (nothing of an earlier pass is in flight: it ended with fold() of both buffers)
    void begin(const std::vector<sm_mapfile::Job> &jobs) { jobs_ = &jobs; c_ = 0; in_.reset(); in_file_ = NO_FILE; }
    bool more() const { return c_ < jobs_->size(); }

    // the next chunk: read, on its way to the device, the context's stream waiting for it, the start of its kernels marked
    int next(Chunk &ck)
    {
        const sm_mapfile::Job &j = (*jobs_)[c_];
        const int q = (int)(c_ & 1u);
        if (int rc = fold(q)) return rc;                 // buffer q is free on both sides
        if (in_file_ != j.file) {
            sm_mapfile::Header h;
            in_ = sm_mapfile::open_checked(paths_[j.file], who_, h, g_err);
            in_file_ = j.file;
            if (!in_) return SM_E_ARG;
        }
        const double t0 = sm_mapfile::now_ms();
        const bool got = sm_mapfile::read_rows(in_.get(), rm_.h_rec[q].get(), j.n);
        *t_.read_ms += (float)(sm_mapfile::now_ms() - t0);
        if (!got) { g_err = sm_mapfile::said(who_, paths_[j.file], " read err!!"); return SM_E_ARG; }
        in_flight_[q] = true;
        HIPCK(hipEventRecord(rm_.ev_copy0[q], rm_.copy));
        HIPCK(hipMemcpyAsync(rm_.d_rec[q], rm_.h_rec[q], (size_t)j.n * sm_mapfile::RECORD_BYTES, hipMemcpyHostToDevice, rm_.copy));
        HIPCK(hipEventRecord(rm_.ev_copied[q], rm_.copy));
        HIPCK(hipStreamWaitEvent(s_->stream, rm_.ev_copied[q], 0));
        HIPCK(hipEventRecord(rm_.ev_k0[q], s_->stream));
        ck = {q, &j, rm_.d_rec[q].get()};
        ++c_;
        return SM_OK;
    }
    // the caller has launched everything that belongs to the chunk in buffer q
    int done(int q)
    {
        HIPCK(hipEventRecord(rm_.ev_k1[q], s_->stream));
        return SM_OK;
    }
    // waits for the chunk in buffer q, if there is one, and folds its times into the tally
    int fold(int q)
    {
        if (!in_flight_[q]) return SM_OK;
        float ms = 0.0f;
        HIPCK(hipEventSynchronize(rm_.ev_k1[q]));
        HIPCK(hipEventElapsedTime(&ms, rm_.ev_copy0[q], rm_.ev_copied[q]));
        *t_.copy_ms += ms;
        HIPCK(hipEventElapsedTime(&ms, rm_.ev_k0[q], rm_.ev_k1[q]));
        *t_.device_ms += ms;
        in_flight_[q] = false;
        return SM_OK;
    }

private:
    static constexpr uint32_t NO_FILE = 0xFFFFFFFFu;
    sm_ctx *s_;
    RenderMaps &rm_;
    const char *who_;
    const char *const *paths_;
    Tally t_;
    const std::vector<sm_mapfile::Job> *jobs_ = nullptr;
    size_t c_ = 0;                     // chunks handed out in this pass
    sm_mapfile::File in_;              // the file being read
    uint32_t in_file_ = NO_FILE;
    bool in_flight_[2] = {false, false};   // the buffer's events have been recorded and not yet folded
};

}  // namespace sm_impl
