// sm_tile.hip -- spatial tiling of a map set (sm_tile_maps; DESIGN.md "4s. Spatial tiling"): the records of a set sorted along a
// Morton curve over a world grid and cut into files at tile boundaries.  One reading of the set counts the records per tile; the
// host plans the files and the batches; one reading per batch collects the batch's records in id order, a stable radix sort orders
// their keys, a gather moves the records once and the host cuts the stream into the planned files.  Kernels: sm_k_tile.h; the
// grid, the table's size, the tally's verdict and the ranks of a reading: sm_voxel.h; the call's frame and the drain: sm_set_call.h.
#include "sm_set_call.h"
#include "sm_k_tile.h"

using namespace sm;

namespace {

constexpr uint32_t SORT_RECORDS = 1u << 22, SORT_RECORDS_MAX = 1u << 26;
constexpr int LOOSE_TALLY = SIMP_TALLY_WORDS;            // the second block of tally words: the loose records' running rank
enum { EV_MODEL0 = 0, EV_MODEL1, EV_SORT0, EV_SORT1, EV_GATHER0, EV_GATHER1 = EV_GATHER0 + 2, EV_PIECE = EV_GATHER1 + 2, N_EV = EV_PIECE + 2 };
static_assert(N_EV == decltype(Tile::scratch)::N_EV, "the context holds the events of a call");

// records a batch may hold; SM_TILE_SORT_RECORDS (read per call) overrides it
uint32_t sort_capacity()
{
    const char *e = std::getenv("SM_TILE_SORT_RECORDS");
    if (!e) return SORT_RECORDS;
    return (uint32_t)std::min<long long>(SORT_RECORDS_MAX, std::max<long long>(256, std::atoll(e)));
}

int check_params(const sm_tile_params *p, uint32_t capacity, const char *who)
{
    auto bad = [&](const std::string &what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (!p) return bad("null params");
    if (p->cell_mm < 10 || p->cell_mm > 10000) return bad("cell_mm outside 10..10000");
    if (p->tile_shift < 0 || p->tile_shift > 17) return bad("tile_shift outside 0..17");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k])) return bad("non-finite origin");
    if (p->max_file_records < 256) return bad("max_file_records below 256");
    if (p->max_file_records > capacity) return bad("max_file_records above the sort capacity of " + std::to_string(capacity) + " records");
    if (p->max_tiles == 0) return bad("max_tiles is 0");
    return SM_OK;
}

struct TileCount { unsigned long long tile; uint32_t n; };
struct Batch { unsigned long long lo, hi; uint32_t n; };   // the tiles lo..hi and their records

// the records per file of the placed records: successive whole tiles up to `limit`; a larger tile alone, in pieces of `limit`
std::vector<uint32_t> plan_files(const std::vector<TileCount> &tiles, uint32_t limit)
{
    std::vector<uint32_t> files;
    uint64_t cur = 0;
    for (const TileCount &t : tiles) {
        if (t.n > limit) {
            if (cur) files.push_back((uint32_t)cur);
            cur = 0;
            for (uint32_t left = t.n; left; left -= std::min(left, limit)) files.push_back(std::min(left, limit));
            continue;
        }
        if (cur + t.n > limit) { files.push_back((uint32_t)cur); cur = 0; }
        cur += t.n;
    }
    if (cur) files.push_back((uint32_t)cur);
    return files;
}

// maximal runs of successive whole tiles of at most `capacity` records (no tile has more)
std::vector<Batch> plan_batches(const std::vector<TileCount> &tiles, uint32_t capacity)
{
    std::vector<Batch> batches;
    for (const TileCount &t : tiles) {
        if (batches.empty() || (uint64_t)batches.back().n + t.n > capacity) batches.push_back({t.tile, t.tile, 0u});
        batches.back().hi = t.tile;
        batches.back().n += t.n;
    }
    return batches;
}

// The output: the stream of sorted records cut into the planned files, each written as a temporary; rename() puts all of them in
// place.  Whatever has not been renamed when the call ends is removed.
struct TileFiles {
    static constexpr float INF = __builtin_inff();
    struct Done { std::string tmp, name; float lo[3], hi[3], tmax; bool renamed; };
    const char *who;
    std::string prefix;
    int32_t start_id = 0, end_id = 0;
    std::vector<uint32_t> want;        // records per file, in order
    std::vector<Done> done;            // complete temporaries
    Done cur{};
    uint32_t in_cur = 0;
    sm_mapfile::Writer w;              // (a writer that goes away uncommitted removes its file)

    TileFiles(const char *who_, const char *prefix_) : who(who_), prefix(prefix_) {}
    ~TileFiles()
    {
        for (const Done &d : done)
            if (!d.renamed) std::remove(d.tmp.c_str());
    }
    std::string name(size_t i) const { return sm_mapfile::policy_file(prefix, (uint32_t)i); }

    // the next n records of the stream
    int put(const float *rows, uint32_t n)
    {
        while (n) {
            if (!w.is_open()) {
                if (done.size() >= want.size()) { g_err = std::string(who) + ": internal: more records than the plan has"; return SM_E_HIP; }
                cur = Done{name(done.size()) + ".tile.tmp", name(done.size()), {INF, INF, INF}, {-INF, -INF, -INF}, -INF, false};
                in_cur = 0;
                if (!w.open(cur.tmp, want[done.size()], start_id, end_id, who, g_err)) return SM_E_ARG;
            }
            const uint32_t m = std::min(n, want[done.size()] - in_cur);
            for (uint32_t i = 0; i < m; ++i) {
                const float *r = rows + (size_t)i * 12;
                if (std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]))
                    for (int k = 0; k < 3; ++k) { cur.lo[k] = std::min(cur.lo[k], r[k]); cur.hi[k] = std::max(cur.hi[k], r[k]); }
                if (r[7] == r[7]) cur.tmax = std::max(cur.tmax, r[7]);
            }
            if (!w.append(rows, m, g_err)) return SM_E_ARG;
            in_cur += m; rows += (size_t)m * 12; n -= m;
            if (in_cur == want[done.size()]) {
                if (!w.commit(g_err)) return SM_E_ARG;
                done.push_back(cur);
            }
        }
        return SM_OK;
    }
    // every planned file is complete: all into place, then into the index
    int rename(sm_mapset::FileIndex &index)
    {
        if (w.is_open() || done.size() != want.size()) { g_err = std::string(who) + ": internal: fewer records than the plan has"; return SM_E_HIP; }
        for (Done &d : done) {
            if (std::rename(d.tmp.c_str(), d.name.c_str()) != 0) { g_err = sm_mapfile::said(who, d.name, " saved err!!"); return SM_E_ARG; }
            d.renamed = true;
        }
        for (const Done &d : done) index.note_now(d.name, d.lo, d.hi, d.tmax);
        return SM_OK;
    }
};

// One call's device side: the tile table, the batch buffers, the launches on the context's stream.
struct TileJob {
    sm_ctx *s;
    Tile &tl;
    const Event *ev;
    const char *who;
    SimplifyArgs a{};
    SimplifyTable T{};                 // key and n (the tile's records) only
    int shift3 = 0;
    Dev<uint8_t> table;                // everything below is freed when the call ends
    Dev<unsigned long long> d_tiles, d_key[2];
    Dev<uint32_t> d_counts, d_idx[2], d_hist;
    Dev<float4> d_batch, d_loose;
    uint32_t cap_batch = 0, cap_loose = 0;
    RankedOutput out;                  // (for the ranks of a reading; it opens no file)
    uint32_t launches = 0;

    TileJob(sm_ctx *s_, const char *who_) : s(s_), tl(s_->tile), ev(s_->tile.scratch.ev), who(who_), out(s_, who_) {}

    uint32_t *tally() const { return tl.scratch.d_tally.get(); }

    int open(uint64_t records, const sm_tile_params &p)
    {
        int rc;
        if ((rc = tl.scratch.ensure(2 * SIMP_TALLY_WORDS)) || (!tl.d_bits && (rc = dalloc(tl.d_bits, 2))) || (rc = out.ensure(0, 0))) return rc;
        a = voxel_args(p.cell_mm, 0, p.origin, 0, p.max_tiles);
        shift3 = 3 * p.tile_shift;
        uint64_t S;
        if ((rc = voxel_slots(records, p.max_tiles, who, "the tile table", S))) return rc;
        if ((rc = dalloc(table, (size_t)S * 12))) return rc;
        T.key = (unsigned long long *)table.get();
        T.n = (uint32_t *)(table.get() + (size_t)S * 8);
        T.mask = (uint32_t)(S - 1);
        T.tally = tally();
        HIPCK(hipMemsetAsync(T.key, 0xFF, (size_t)S * 8, s->stream));
        HIPCK(hipMemsetAsync(T.n, 0, (size_t)S * 4, s->stream));
        return tl.scratch.clear(s->stream);
    }
    // pass 1 of n <= CHUNK records
    void count(const float4 *d_rec, uint32_t n)
    {
        hipLaunchKernelGGL(k_tile_count, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, a, shift3, T);
        launches++;
        tl.stats.chunks++;
    }
    // the table's (tile, count) pairs, sorted by tile; `distinct` of them
    int list(uint32_t distinct, std::vector<TileCount> &tiles)
    {
        int rc;
        tiles.assign(distinct, TileCount{});
        if (!distinct) return SM_OK;
        if ((rc = dalloc(d_tiles, distinct)) || (rc = dalloc(d_counts, distinct))) return rc;
        HIPCK(hipMemsetAsync(tally() + SIMP_RUN, 0, 4, s->stream));
        hipLaunchKernelGGL(k_tile_list, dim3(T.mask / 256u + 1u), dim3(256), 0, s->stream, T, distinct, d_tiles.get(), d_counts.get());
        launches++;
        HIPCK(hipGetLastError());
        std::vector<unsigned long long> ids(distinct);
        std::vector<uint32_t> counts(distinct);
        HIPCK(hipMemcpyAsync(ids.data(), d_tiles, (size_t)distinct * 8, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipMemcpyAsync(counts.data(), d_counts, (size_t)distinct * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        for (uint32_t i = 0; i < distinct; ++i) tiles[i] = {ids[i], counts[i]};
        std::sort(tiles.begin(), tiles.end(), [](const TileCount &x, const TileCount &y) { return x.tile < y.tile; });
        table = Dev<uint8_t>();                          // (the table has served)
        d_tiles = Dev<unsigned long long>();
        d_counts = Dev<uint32_t>();
        return SM_OK;
    }
    // the buffers of batches of at most `batch` records and of `loose` loose records
    int ensure_batch(uint32_t batch, uint32_t loose)
    {
        int rc;
        cap_batch = batch;
        cap_loose = loose;
        if (loose && (rc = dalloc(d_loose, (size_t)loose * 3))) return rc;
        if (!batch) return SM_OK;
        if ((rc = dalloc(d_batch, (size_t)batch * 3)) || (rc = dalloc(d_key[0], batch)) || (rc = dalloc(d_key[1], batch)) || (rc = dalloc(d_idx[0], batch)) ||
            (rc = dalloc(d_idx[1], batch)))
            return rc;
        return dalloc(d_hist, pair_sort_hist_words(batch));
    }
    // a batch's reading begins: no rank given, no key seen
    int begin_batch()
    {
        HIPCK(hipMemsetAsync(tally() + SIMP_RUN, 0, 4, s->stream));
        HIPCK(hipMemsetAsync(tl.d_bits.get(), 0, 8, s->stream));
        HIPCK(hipMemsetAsync(tl.d_bits.get() + 1, 0xFF, 8, s->stream));
        return SM_OK;
    }
    // pass 2 of n <= CHUNK records: those of the tiles r into the batch (r.lo > r.hi: none), the loose ones into their buffer
    void select(const float4 *d_rec, uint32_t n, const TileRange &r, bool loose)
    {
        const unsigned nblk = (n + 255) / 256;
        if (r.lo <= r.hi) {
            hipLaunchKernelGGL(k_tile_mark<false>, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, a, r, out.blk_cnt(), tl.d_bits.get());
            out.scan(nblk, tally(), -1, launches);
            hipLaunchKernelGGL(k_tile_select<false>, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, a, r, out.blk_base(), cap_batch, d_batch.get(),
                               d_key[0].get(), d_idx[0].get());
            launches += 2;
        }
        if (loose) {
            hipLaunchKernelGGL(k_tile_mark<true>, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, a, r, out.blk_cnt(), tl.d_bits.get());
            out.scan(nblk, tally() + LOOSE_TALLY, -1, launches);
            hipLaunchKernelGGL(k_tile_select<true>, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, a, r, out.blk_base(), cap_loose, d_loose.get(),
                               (unsigned long long *)nullptr, (uint32_t *)nullptr);
            launches += 2;
        }
        tl.stats.chunks++;
    }
    // the ranks a batch's reading gave and the bits in which its keys differ, once the stream is idle
    int batch_tally(uint32_t &ranks, uint32_t &loose_ranks, unsigned long long &varying)
    {
        const uint32_t *t = tl.scratch.h();
        unsigned long long bits[2];
        HIPCK(hipMemcpyAsync(bits, tl.d_bits, 16, hipMemcpyDeviceToHost, s->stream));
        if (int rc = tl.scratch.read(s)) return rc;
        ranks = t[SIMP_RUN];
        loose_ranks = t[LOOSE_TALLY + SIMP_RUN];
        varying = ranks ? bits[0] ^ bits[1] : 0ull;
        return SM_OK;
    }
    // n (key, idx) pairs of buffer 0 sorted by key, stably (sm_voxel.h's pair sort); which: the buffer that holds them then
    int sort(uint32_t n, unsigned long long varying, int &which)
    {
        int rc;
        if ((rc = mark(s, ev[EV_SORT0]))) return rc;
        unsigned long long *const key[2] = {d_key[0].get(), d_key[1].get()};
        uint32_t *const idx[2] = {d_idx[0].get(), d_idx[1].get()};
        if ((rc = pair_sort(s, key, idx, d_hist.get(), n, varying, which, launches, tl.stats.sort_passes))) return rc;
        if ((rc = mark(s, ev[EV_SORT1])) || (rc = add_marked(&ev[EV_SORT0], &tl.stats.sort_ms))) return rc;
        return SM_OK;
    }
    // n records into the files, a piece of CHUNK at a time (sm_set_call.h's drain): piece p is gathered and copied while the host
    // writes piece p - 1.  d_idx: the records are d_batch[d_idx[i]], gathered into the staging's device buffer; null: d_src[i].
    int to_files(const uint32_t *d_idx_sorted, const float4 *d_src, uint32_t n, TileFiles &files)
    {
        const auto gather = [&](int q, size_t first, size_t m) -> int {
            if (!d_idx_sorted) return SM_OK;
            HIPCK(hipEventRecord(ev[EV_GATHER0 + q], s->stream));
            hipLaunchKernelGGL(k_tile_gather, dim3(((uint32_t)m * 3u + 255u) / 256u), dim3(256), 0, s->stream, (const float4 *)d_batch.get(), d_idx_sorted,
                               (uint32_t)first, (uint32_t)m, cap_batch, s->staging.d_rec[q].get());
            launches++;
            HIPCK(hipGetLastError());
            HIPCK(hipEventRecord(ev[EV_GATHER1 + q], s->stream));
            return SM_OK;
        };
        const auto put = [&](int q, const void *rows, size_t, size_t m) -> int {
            if (d_idx_sorted) {
                float ms = 0.0f;
                HIPCK(hipEventElapsedTime(&ms, ev[EV_GATHER0 + q], ev[EV_GATHER1 + q]));
                tl.stats.device_ms += ms;
            }
            return files.put((const float *)rows, (uint32_t)m);
        };
        return drain(s, d_src, n, 48, &ev[EV_PIECE], &tl.stats.write_ms, false, put, gather);
    }
};

}  // namespace

extern "C" {

int sm_default_tile_params(sm_tile_params *p)
{
    if (!p) { g_err = "sm_default_tile_params: null argument"; return SM_E_ARG; }
    p->cell_mm = 200;
    p->tile_shift = 7;
    p->origin[0] = p->origin[1] = p->origin[2] = 0.0f;
    p->max_file_records = 1u << 20;
    p->max_tiles = 1u << 20;
    return SM_OK;
}

int sm_tile_maps(sm_ctx *s, const sm_map_source *src, const sm_tile_params *p, const char *out_prefix)
{
    const char *who = "sm_tile_maps";
    SetCall call(s, src, who);
    if (!s || !src || !out_prefix) { g_err = std::string(who) + ": null context, source or output prefix"; return SM_E_ARG; }
    int rc;
    const uint32_t capacity = sort_capacity();
    if ((rc = call.open([&] { return check_params(p, capacity, who); }))) return rc;   // (the names come from the plan: their rule is below)
    const sm_mapset::ReadSet &set = call.set;
    const uint32_t cnt = call.cnt;
    Tile &tl = s->tile;
    tl.stats = sm_tile_stats_t{};
    tl.stats_valid = true;
    const uint64_t total = call.total;
    tl.stats.records_in = total;
    if (!total) { tl.stats.total_ms = call.elapsed_ms(); return SM_OK; }      // (an empty set: no file)

    TileJob job(s, who);
    if ((rc = call.staging()) || (rc = job.open(total, *p)) || (rc = call.model())) return rc;
    const float4 *d_model = call.d_model;
    const MapStream::Tally times = {&tl.stats.read_ms, &call.copy_ms, &tl.stats.device_ms};
    const Event *model = &job.ev[EV_MODEL0];

    // ---- pass 1: the records per tile
    if ((rc = maps_feed(s, who, set, src->paths, cnt, d_model, times, model[0], [&](const float4 *d_rec, uint32_t n, uint32_t) { job.count(d_rec, n); })))
        return rc;
    tl.stats.readings = 1;
    const uint32_t *t = tl.scratch.h();
    if ((rc = mark(s, model[1])) || (rc = tl.scratch.read(s, SIMP_TALLY_WORDS)) || (rc = add_marked(model, &tl.stats.device_ms))) return rc;
    if (voxel_check_tally(t, p->max_tiles, who, "tiles")) {
        g_err = std::string(who) + ": more than max_tiles = " + std::to_string(p->max_tiles) + " tiles";
        return SM_E_CAPACITY;
    }
    std::vector<TileCount> tiles;
    if ((rc = job.list(t[SIMP_CELLS], tiles))) return rc;
    const uint64_t loose = t[SIMP_N_LOOSE];
    uint64_t placed = 0;
    uint32_t largest = 0;
    for (const TileCount &tc : tiles) { placed += tc.n; largest = std::max(largest, tc.n); }
    if (placed + loose != total) { g_err = std::string(who) + ": internal: the tiles' counts and the set differ"; return SM_E_HIP; }
    tl.stats.placed = placed;
    tl.stats.loose = loose;
    tl.stats.tiles = (uint32_t)tiles.size();
    tl.stats.largest_tile = largest;
    if (largest > capacity) {
        g_err = std::string(who) + ": a tile holds " + std::to_string(largest) + " records, above the sort capacity of " + std::to_string(capacity) +
                ": lower tile_shift";
        return SM_E_CAPACITY;
    }

    // ---- the plan: files, batches, names
    TileFiles files(who, out_prefix);
    files.want = plan_files(tiles, p->max_file_records);
    if (loose) files.want.push_back((uint32_t)loose);
    frame_range(set, files.start_id, files.end_id);
    for (size_t i = 0; i < files.want.size(); ++i)
        for (uint32_t k = 0; k < src->n_paths; ++k)
            if (files.name(i) == src->paths[k]) return own_path_taken(who, src->paths[k]);
    std::vector<Batch> batches = plan_batches(tiles, capacity);
    uint32_t largest_batch = 0;
    for (const Batch &b : batches) largest_batch = std::max(largest_batch, b.n);
    if (batches.empty()) batches.push_back({1ull, 0ull, 0u});                           // (loose records only: a reading for them)
    if ((rc = job.ensure_batch(largest_batch, (uint32_t)loose))) return rc;

    // ---- pass 2: per batch a reading, the sort, the gather into the files
    for (size_t b = 0; b < batches.size(); ++b) {
        const TileRange r{batches[b].lo, batches[b].hi, job.shift3};
        const bool with_loose = b == 0 && loose;
        if ((rc = job.begin_batch())) return rc;
        if ((rc = maps_feed(s, who, set, src->paths, cnt, d_model, times, model[0],
                            [&](const float4 *d_rec, uint32_t n, uint32_t) { job.select(d_rec, n, r, with_loose); })))
            return rc;
        tl.stats.readings++;
        uint32_t ranks, loose_ranks;
        unsigned long long varying;
        if ((rc = mark(s, model[1])) || (rc = job.batch_tally(ranks, loose_ranks, varying)) || (rc = add_marked(model, &tl.stats.device_ms))) return rc;
        if (ranks != batches[b].n || (with_loose && loose_ranks != loose)) { g_err = std::string(who) + ": the set changed while it was read"; return SM_E_ARG; }
        if (!ranks) continue;
        int which;
        if ((rc = job.sort(ranks, varying, which)) || (rc = job.to_files(job.d_idx[which].get(), nullptr, ranks, files))) return rc;
    }
    if (loose && (rc = job.to_files(nullptr, job.d_loose.get(), (uint32_t)loose, files))) return rc;
    tl.stats.device_ms += tl.stats.sort_ms;
    tl.stats.launches = job.launches;
    if ((rc = files.rename(s->index))) return rc;
    tl.stats.files_written = (uint32_t)files.done.size();
    tl.stats.total_ms = call.elapsed_ms();
    return SM_OK;
}

SM_STATS_GETTER(sm_tile_stats, sm_tile_stats_t, tile, "sm_tile_maps")

}  // extern "C"
