// sm_set_call.h -- private to sm_simplify.hip, sm_register.hip, sm_compare.hip, sm_tile.hip, sm_segment.hip, sm_mesh.hip,
// sm_ground.hip, sm_locate.hip, sm_rays.hip and sm_points.hip: the frame of a call that reads a whole map set and computes something from it (DESIGN.md "4w. The frame of a
// map-set call").  The opening of a call on one set (SetCall) and the live model's export; the scratch a call keeps on its context
// (CallScratch, LabelPair: sm_ctx.h holds them, their members are defined here); the drain of device rows to the host in pieces;
// the collect of a labelled pass; the stats getter.  What lies between a call's opening and its commit is the call's own.
#pragma once

#include "sm_voxel.h"

namespace sm_impl __attribute__((visibility("hidden"))) {

// ---- the opening

// the refusal of an output that would replace a file of the set
inline int own_path_taken(const char *who, const std::string &path)
{
    g_err = sm_mapfile::said(who, path, " is a file of the set: the output needs a path of its own");
    return SM_E_ARG;
}
inline int check_own_path(const sm_map_source *src, const char *out, const char *who)
{
    for (uint32_t i = 0; out && i < src->n_paths; ++i)
        if (strcmp(src->paths[i], out) == 0) return own_path_taken(who, out);
    return SM_OK;
}

// the first n live records as rows in the export scratch, enqueued on the context's stream; null without any
inline int maps_export(sm_ctx *s, uint32_t n, const float4 *&d_model)
{
    d_model = nullptr;
    if (!n) return SM_OK;
    if (int rc = ensure_export(s, (size_t)n * 48)) return rc;
    export_aos(s, (float *)s->d_export.get(), 0u, n);
    d_model = (const float4 *)s->d_export.get();
    return SM_OK;
}

// A call on one set, from its first line (t_begin) on.  open(): the whole map, the call's own parameters (check_params()), the
// half-done cull, the source, no output among the set's files, every header, then the device, the model compact, the live surfels
// that take part and the id limit -- each once, in this order.
struct SetCall {
    sm_ctx *s;
    const sm_map_source *src;
    const char *who;
    const double t_begin = sm_mapfile::now_ms();
    sm_mapset::ReadSet set;
    uint32_t cnt = 0;                  // the live surfels that take part
    uint64_t total = 0;                // the set's records: the files', then those
    const float4 *d_model = nullptr;   // their rows once model() has run; null without any
    float copy_ms = 0.0f;              // the chunks' copies: no call's stats hold them

    SetCall(sm_ctx *s_, const sm_map_source *src_, const char *who_) : s(s_), src(src_), who(who_) {}

    template <typename Check>
    int open(Check check_params, std::initializer_list<const char *> outputs = {})
    {
        int rc;
        if ((rc = check_whole_map(s, who)) || (rc = check_params()) || (rc = check_not_mid_cull(s, who)) || (rc = check_map_source(src, who))) return rc;
        for (const char *out : outputs)
            if ((rc = check_own_path(src, out, who))) return rc;
        if (!sm_mapset::open_read_set(src->paths, src->n_paths, MapStaging::CHUNK, who, set, g_err)) return SM_E_ARG;
        const sm_mapset::ReadSet *sets[1] = {&set};
        if ((rc = maps_counts(s, who, 1, &src, sets, &cnt))) return rc;
        total = set.file_total + cnt;
        return SM_OK;
    }
    int model() { return maps_export(s, cnt, d_model); }
    int staging() { return maps_ensure_staging(s); }
    float elapsed_ms() const { return (float)(sm_mapfile::now_ms() - t_begin); }
};

// ---- the scratch of a call

template <int N>
int CallScratch<N>::ensure(size_t tally_words)
{
    if (d_tally) return SM_OK;
    Dev<uint32_t> tally;
    if (int rc = dalloc(tally, tally_words)) return rc;
    HIPCK(hipHostMalloc((void **)h_tally.put(), tally_words * 4, hipHostMallocDefault));
    for (Event &e : ev) HIPCK(hipEventCreate(e.put()));
    words = tally_words;
    d_tally = std::move(tally);
    return SM_OK;
}
template <int N>
int CallScratch<N>::clear(hipStream_t stream) const
{
    HIPCK(hipMemsetAsync(d_tally.get(), 0, words * 4, stream));
    return SM_OK;
}
template <int N>
int CallScratch<N>::read(sm_ctx *s, size_t n) const
{
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(h_tally.get(), d_tally.get(), (n ? n : words) * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

template <typename T>
int LabelPair<T>::ensure()
{
    if (h[1]) return SM_OK;
    Dev<T> dev[2];
    Host<T> host[2];
    for (int q = 0; q < 2; ++q) {
        if (int rc = dalloc(dev[q], MapStaging::CHUNK)) return rc;
        HIPCK(hipHostMalloc((void **)host[q].put(), (size_t)MapStaging::CHUNK * sizeof(T), hipHostMallocDefault));
    }
    for (int q = 0; q < 2; ++q) { d[q] = std::move(dev[q]); h[q] = std::move(host[q]); }
    return SM_OK;
}

// ---- the drain

// `rows` rows of row_bytes at d_src back to the host through the staging's two host buffers, which no reading is using, in pieces
// of a staging buffer: piece p is copied on the context's stream while the host takes piece p - 1 -- take(q, host rows, first row,
// rows), timed into *write_ms, with the wait for the piece's copy if wait_is_write.  ev[q] guards buffer q.  before(q, first row,
// rows) enqueues what goes in front of a piece's copy; d_src null: that leaves the piece in the staging's d_rec[q].
template <typename Take, typename Before>
int drain(sm_ctx *s, const void *d_src, size_t rows, size_t row_bytes, const Event *ev, float *write_ms, bool wait_is_write, Take take, Before before)
{
    MapStaging &st = s->staging;
    const size_t per = (size_t)MapStaging::CHUNK * 48 / row_bytes, pieces = (rows + per - 1) / per;
    const auto finish = [&](size_t pc) -> int {
        const int q = (int)(pc & 1u);
        double t0 = sm_mapfile::now_ms();
        HIPCK(hipEventSynchronize(ev[q]));
        if (!wait_is_write) t0 = sm_mapfile::now_ms();
        const int rc = take(q, (const void *)st.h_rec[q].get(), pc * per, std::min(per, rows - pc * per));
        *write_ms += (float)(sm_mapfile::now_ms() - t0);
        return rc;
    };
    for (size_t pc = 0; pc < pieces; ++pc) {
        const int q = (int)(pc & 1u);
        const size_t first = pc * per, m = std::min(per, rows - first);
        if (int rc = before(q, first, m)) return rc;
        const void *from = d_src ? (const void *)((const uint8_t *)d_src + first * row_bytes) : (const void *)st.d_rec[q].get();
        HIPCK(hipMemcpyAsync(st.h_rec[q].get(), from, m * row_bytes, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipEventRecord(ev[q], s->stream));
        if (pc)
            if (int rc = finish(pc - 1)) return rc;
    }
    return pieces ? finish(pieces - 1) : SM_OK;
}
template <typename Take>
int drain(sm_ctx *s, const void *d_src, size_t rows, size_t row_bytes, const Event *ev, float *write_ms, bool wait_is_write, Take take)
{
    return drain(s, d_src, rows, row_bytes, ev, write_ms, wait_is_write, take, [](int, size_t, size_t) { return SM_OK; });
}

// ---- the collect of a labelled pass (RankedOutput::run's `collect`)

// The chunk of n records in buffer q, ids gid0 ..: its kernels are over; on `stream`, behind one wait: the kept records through the
// staging's host buffer q into the output, the labels (if the caller wants them) through the pinned buffer q to labels + gid0.
template <typename T>
int collect_labelled(RankedOutput &ro, const LabelPair<T> &lp, T *labels, int q, uint32_t n, uint64_t gid0, hipStream_t stream, float *write_ms)
{
    const double t0 = sm_mapfile::now_ms();
    uint32_t m;
    if (int e = ro.stage(q, stream, m)) return e;
    if (labels) HIPCK(hipMemcpyAsync(lp.h[q].get(), lp.d[q].get(), (size_t)n * sizeof(T), hipMemcpyDeviceToHost, stream));
    if (m || labels) HIPCK(hipStreamSynchronize(stream));
    if (labels) memcpy(labels + gid0, lp.h[q].get(), (size_t)n * sizeof(T));
    const int e = ro.write(q, m);
    *write_ms += (float)(sm_mapfile::now_ms() - t0);
    return e;
}

// ---- sm_<name>_stats: the last call's stats, SM_E_ARG before there are any ("<fn>: no <calls> call yet")
#define SM_STATS_GETTER(fn, stats_t, member, calls)                                                   \
    int fn(sm_ctx *s, stats_t *out)                                                                   \
    {                                                                                                 \
        if (!s || !out) { g_err = #fn ": null argument"; return SM_E_ARG; }                          \
        if (!s->member.stats_valid) { g_err = #fn ": no " calls " call yet"; return SM_E_ARG; }      \
        *out = s->member.stats;                                                                       \
        return SM_OK;                                                                                 \
    }

}  // namespace sm_impl
