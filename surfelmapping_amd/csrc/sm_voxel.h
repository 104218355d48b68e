// sm_voxel.h -- private to sm_voxel.hip, which defines what is declared here, and to sm_set_call.h, through which the map-set
// analysis calls take it: what the users of a voxel table do alike on the host.  The grid and the table's size from a call's parameters and the
// tally's verdict (all three); the lookup table -- sums finished into one RegCell per slot, with or without a cover table of keys
// -- of registration and change detection; the ranked output -- what a pass keeps of every chunk, in order, in one map file -- of
// simplification and change detection.  Kernels: sm_k_voxel.h.
#pragma once

#include "sm_map_stream.h"
#include "sm_d_register.h"

namespace sm_impl __attribute__((visibility("hidden"))) {

// the grid of cells of voxel_mm << shift millimetres; SM_SIMPLIFY_NO_COMBINE=1 (read per call) switches the in-wave combination off
SimplifyArgs voxel_args(int32_t voxel_mm, int shift, const float origin[3], int split, uint32_t max_cells);
// the slots of a table for `records` records of at most max_cells cells: a power of two, at least twice the cells it may hold;
// SM_E_CAPACITY, "<who>: <what> would need ...", beyond 2^31
int voxel_slots(uint64_t records, uint32_t max_cells, const char *who, const char *what, uint64_t &slots);
// SM_E_CAPACITY, "<who>: more than max_cells = N <what>", if a table's tally t has its error word set
int voxel_check_tally(const uint32_t *t, uint32_t max_cells, const char *who, const std::string &what);

// A lookup table of a call; the caller sets the grids (voxel_args; ac only with a cover table)
struct LookupTable {
    SimplifyArgs a{}, ac{};
    SimplifyTable T{}, TC{};           // T: key, SW, SP, SN; TC: key only, null without a cover table
    RegCell *lut = nullptr;
};
// n tables of `slots` slots, each with a cover table if `cover`, in one allocation `mem`.  The tally words of table i lie at
// d_tally + i * SIMP_TALLY_WORDS, those of the cover tables behind them.
int lut_open(Dev<uint8_t> &mem, LookupTable *t, int n, uint64_t slots, bool cover, uint32_t *d_tally);
// ... initialised on the context's stream: no key, no sums (the tally is the caller's to clear)
int lut_clear(sm_ctx *s, const LookupTable *t, int n);
// n <= CHUNK records into the table's sums, and into its cover table if it has one, in one launch.  keep_class 0: the class taken
// as 0; it is kept only in a table with a cover table (change detection's match_class): registration's tables never keep it
void lut_insert(sm_ctx *s, const LookupTable &t, const float4 *d_rec, uint32_t n, int keep_class, uint32_t &launches);
// the sums become the lookup records
void lut_finish(sm_ctx *s, const LookupTable &t, uint32_t &launches);

// The lean claim table of the ray casts (sm_d_simplify.h: LeanTable, lean_probe): 4 slots per record of the chunk it indexes, at
// least SIMP_MIN_SLOTS, a power of two; 16 bytes a slot.  lean_clear: keys empty, runs zero, on the context's stream.
size_t lean_slots(uint32_t records);
int lean_clear(sm_ctx *s, const sm::LeanTable &t);

// The pair sort of tiling and meshing: n (key, idx) pairs in key[0] / idx[0] sorted by key, stably, by an LSD radix sort of 8 bits a
// pass over the bits 0..55; a pass whose digit no bit of `varying` touches is skipped (every key has the same digit there).
// hist: pair_sort_hist_words(n) words.  which: the buffer that holds the pairs then; passes: those that ran.
size_t pair_sort_hist_words(uint32_t n);
int pair_sort(sm_ctx *s, unsigned long long *const key[2], uint32_t *const idx[2], uint32_t *hist, uint32_t n, unsigned long long varying, int &which,
              uint32_t &launches, uint32_t &passes);

// the frame range a file made of a set's records carries in its header: the one that spans the files' (0, 0 without files)
void frame_range(const sm_mapset::ReadSet &set, int32_t &start_id, int32_t &end_id);

// One call's ranked output on the context's RankScratch.  A chunk's kernels count what they keep per block of 256 (blk_cnt), scan()
// ranks the blocks on top of the call's running rank, the caller's emit kernel writes the kept records to out(q); fetch(q) brings
// the chunk's count to the host, stage(q) and write(q) its records into the file.  Without open() there is no file: sm_simplify's whole output
// stays on the device (out(0), no info), a change detection that only labels writes nothing.  A pass that ranks two things at once
// (segmentation: the kept records and the components' openers) counts the second in plane 1 of the block counts and scans it on
// top of a running rank of its own.
struct RankedOutput {
    sm_ctx *s;
    RankScratch &rs;
    const char *who;
    sm_mapfile::Writer w;              // (a writer that goes away uncommitted removes its file)
    std::string tmp;

    RankedOutput(sm_ctx *s_, const char *who_) : s(s_), rs(s_->ranked), who(who_) {}
    bool writes() const { return !tmp.empty(); }
    uint32_t *blk_cnt(int plane = 0) const { return rs.d_blk_cnt.get() + plane * RankScratch::BLOCKS; }
    const uint32_t *blk_base(int plane = 0) const { return rs.d_blk_base.get() + plane * RankScratch::BLOCKS; }
    const uint2 *info(int q) const { return rs.d_info.get() + q; }
    float4 *out(int q) const { return rs.d_out[q].get(); }

    // the scratch, with out(q) for `records` records
    int ensure(int q, size_t records);
    // ... with both buffers for the largest chunk of `set` and of `cnt` live records, and "<out_path><suffix>" open with the frame
    // range of the set's files
    int open(const char *out_path, const char *suffix, const sm_mapset::ReadSet &set, uint32_t cnt);
    // nblk blocks of a chunk (their counts in `plane`) ranked on top of tally[SIMP_RUN]; q < 0: no info, the output is the whole call's
    void scan(uint32_t nblk, uint32_t *tally, int q, uint32_t &launches, int plane = 0);
    int fetch(int q);
    // the chunk's kept records through the staging's host buffer q (free until chunk c + 2 is read into it): stage() enqueues their
    // copy on `stream` and says how many there are, write() puts them into the file once the caller has waited for `stream`
    int stage(int q, hipStream_t stream, uint32_t &kept);
    int write(int q, uint32_t kept);
    // the file complete and at out_path, if its rows are the `ranks` that were given; rows: how many
    int commit(const char *out_path, uint32_t ranks, uint64_t &rows);

    // The pass that writes: launch(d_rec, n, gid0, q) enqueues the kernels of a chunk in buffer q, collect(q, n, gid0, stream) takes
    // what they left -- the files' chunks while the next is on the device, then the live model's `cnt` records at d_model, whose
    // kernels are timed between the events `pair` into t.device_ms.
    template <typename Launch, typename Collect>
    int run(const sm_mapset::ReadSet &set, const char *const *paths, uint32_t cnt, const float4 *d_model, MapStream::Tally t, const Event *pair,
            Launch launch, Collect collect)
    {
        int rc;
        MapStream in(s, who, paths, t);
        const auto enqueue = [&](MapStream::Chunk &ck) -> int {
            if (int e = in.next(ck)) return e;
            launch(ck.d_rec, ck.job->n, set.id_base[ck.job->file] + ck.job->first, ck.q);
            HIPCK(hipGetLastError());
            if (int e = fetch(ck.q)) return e;
            return in.done(ck.q);
        };
        const auto finish = [&](const MapStream::Chunk &ck) -> int {
            if (int e = in.fold(ck.q)) return e;         // (waits for the chunk's kernels and the copy of its count)
            return collect(ck.q, ck.job->n, set.id_base[ck.job->file] + ck.job->first, s->staging.copy.get());
        };
        if ((rc = sm_mapset::stream_files(in, set.jobs, enqueue, finish))) return rc;
        for (uint32_t first = 0; first < cnt; first += MapStaging::CHUNK) {
            const uint32_t n = std::min(MapStaging::CHUNK, cnt - first);
            if ((rc = mark(s, pair[0]))) return rc;
            launch(d_model + (size_t)first * 3, n, set.file_total + first, 0);
            HIPCK(hipGetLastError());
            if ((rc = fetch(0)) || (rc = mark(s, pair[1])) || (rc = add_marked(pair, t.device_ms))) return rc;
            HIPCK(hipStreamSynchronize(s->stream));
            if ((rc = collect(0, n, set.file_total + first, s->stream.get()))) return rc;
        }
        return SM_OK;
    }
};

}  // namespace sm_impl
