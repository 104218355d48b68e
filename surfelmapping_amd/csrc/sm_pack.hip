// sm_pack.hip -- packed map files (sm_pack_maps, sm_unpack_maps; DESIGN.md "4aa. Packed map files"): the encoder over the chunks
// of a map set, the decoder that the chunk stream runs on every chunk of a packed file (maps_unpack, for every source that reads
// map files) and the staging's packed pair.  Kernels: sm_k_pack.h; the format's host side: sm_mapfile.h; the call's frame:
// sm_set_call.h.
#include "sm_set_call.h"
#include "sm_k_pack.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

constexpr uint32_t CHUNK = MapStaging::CHUNK, CHUNK_BLOCKS = CHUNK / sm_mapfile::PACK_BLOCK;
static_assert(sizeof(PackDirDev) == sizeof(sm_mapfile::PackDir), "the directory entry of the kernels is the file's");
static_assert(PACK_BLOCK == (int)sm_mapfile::PACK_BLOCK && PACK_RAW_FLAG == sm_mapfile::PACK_RAW, "one format");
static_assert(CHUNK_BLOCKS <= 4096, "k_pack_scan scans a chunk's blocks in one workgroup");
enum { EV_MODEL0 = 0, EV_MODEL1 };

int check_params(const sm_pack_params *p, const char *who)
{
    if (!p) { g_err = std::string(who) + ": null params"; return SM_E_ARG; }
    if (p->pos_step_log2 < sm_mapfile::PACK_STEP_MIN || p->pos_step_log2 > sm_mapfile::PACK_STEP_MAX) {
        g_err = std::string(who) + ": pos_step_log2 outside -14..-6";
        return SM_E_ARG;
    }
    return SM_OK;
}

std::string out_name(const char *prefix, uint32_t i, const char *ext)
{
    char name[32];
    snprintf(name, sizeof name, "_%06u.%s", i, ext);
    return std::string(prefix) + name;
}

// The outputs of a call: each written as a temporary, all renamed into place by rename().  Whatever has not been renamed when the
// call ends is removed.
struct OutFiles {
    struct Done { std::string tmp, name; bool renamed; };
    const char *who;
    std::vector<Done> done;
    OutFiles(const char *who_) : who(who_) {}
    ~OutFiles()
    {
        for (const Done &d : done)
            if (!d.renamed) std::remove(d.tmp.c_str());
    }
    int rename(uint64_t &bytes)
    {
        for (Done &d : done) {
            if (std::rename(d.tmp.c_str(), d.name.c_str()) != 0) { g_err = sm_mapfile::said(who, d.name, " saved err!!"); return SM_E_ARG; }
            d.renamed = true;
            sm_mapfile::Header h;
            if (sm_mapfile::stat_of(d.name, h)) bytes += h.size;
        }
        return SM_OK;
    }
};

// One packed file being written: the header, a directory of zeros, the payload appended chunk by chunk, and commit() puts the
// directory in.  A writer that goes away without a successful commit() removes its file.
class PackWriter {
public:
    ~PackWriter() { discard(); }
    bool open(const std::string &path, uint32_t count, int32_t start_id, int32_t end_id, int32_t step, const char *who)
    {
        discard();
        path_ = path; who_ = who; count_ = count; at_ = 0;
        dir_.clear();
        dir_.reserve(blocks());
        f_.reset(fopen(path.c_str(), "wb"));
        if (!f_) { g_err = sm_mapfile::said(who, path, " is not open!"); return false; }
        const uint32_t hdr[8] = {sm_mapfile::PACK_MAGIC, sm_mapfile::PACK_VERSION, count, (uint32_t)start_id, (uint32_t)end_id, (uint32_t)step, blocks(), 0u};
        const std::vector<sm_mapfile::PackDir> zeros(blocks());
        return (fwrite(hdr, 4, 8, f_.get()) == 8 && (zeros.empty() || fwrite(zeros.data(), sizeof zeros[0], zeros.size(), f_.get()) == zeros.size())) || fail();
    }
    // the next blocks: their entries (offsets counted from the file's first block) and their bytes
    bool append(const sm_mapfile::PackDir *dir, size_t nblk, const void *payload, uint64_t bytes)
    {
        if (!f_ || dir_.size() + nblk > blocks() || (nblk && dir[0].offset != at_)) return fail();
        dir_.insert(dir_.end(), dir, dir + nblk);
        if (bytes && fwrite(payload, 1, bytes, f_.get()) != bytes) return fail();
        at_ += bytes;
        return true;
    }
    bool commit()
    {
        if (!f_ || dir_.size() != blocks()) return fail();
        bool ok = dir_.empty() || (fseeko(f_.get(), (off_t)sm_mapfile::PACK_HEADER_BYTES, SEEK_SET) == 0 &&
                                   fwrite(dir_.data(), sizeof dir_[0], dir_.size(), f_.get()) == dir_.size());
        ok = (fclose(f_.release()) == 0) && ok;
        if (!ok) { std::remove(path_.c_str()); return fail(); }
        return true;
    }
    bool is_open() const { return (bool)f_; }
    uint32_t blocks() const { return (uint32_t)(((uint64_t)count_ + sm_mapfile::PACK_BLOCK - 1) / sm_mapfile::PACK_BLOCK); }
    uint32_t blocks_written() const { return (uint32_t)dir_.size(); }

private:
    void discard()
    {
        if (f_) { f_.reset(); std::remove(path_.c_str()); }
    }
    bool fail()
    {
        discard();
        g_err = sm_mapfile::said(who_, path_, " saved err!!");
        return false;
    }
    sm_mapfile::File f_;
    std::string path_;
    const char *who_ = nullptr;
    uint32_t count_ = 0;
    uint64_t at_ = 0;                  // payload bytes written
    std::vector<sm_mapfile::PackDir> dir_;
};

// the refusals both calls share, and the output names against the sources
int check_names(const sm_map_source *src, const char *prefix, uint32_t n_out, const char *ext, const char *who)
{
    for (uint32_t i = 0; i < n_out; ++i) {
        const std::string name = out_name(prefix, i, ext);
        for (uint32_t k = 0; k < src->n_paths; ++k)
            if (name == src->paths[k]) return own_path_taken(who, name);
    }
    return SM_OK;
}

// One call's device side of the encoder: the output buffers of the two chunks in flight, the launches on the context's stream.
struct PackJob {
    sm_ctx *s;
    Pack &pk;
    float up, down;
    Dev<uint8_t> d_out[2];             // a chunk's payload (all RAW: as large as the chunk)
    Dev<PackDirDev> d_dir[2];
    Dev<uint32_t> d_size;
    Dev<unsigned long long> d_run;     // the payload bytes of the file so far

    PackJob(sm_ctx *s_, int32_t step) : s(s_), pk(s_->pack), up(std::ldexp(1.0f, -step)), down(std::ldexp(1.0f, step)) {}
    int open()
    {
        int rc;
        for (int q = 0; q < 2; ++q)
            if ((rc = dalloc(d_out[q], (size_t)CHUNK * sm_mapfile::RECORD_BYTES)) || (rc = dalloc(d_dir[q], CHUNK_BLOCKS))) return rc;
        if ((rc = dalloc(d_size, CHUNK_BLOCKS)) || (rc = dalloc(d_run, 1))) return rc;
        return pk.scratch.ensure(4);
    }
    int begin_file()
    {
        HIPCK(hipMemsetAsync(d_run.get(), 0, 8, s->stream));
        return SM_OK;
    }
    // the chunk of n <= CHUNK records at d_rec into buffer q; its tally follows it to the host
    int encode(const float4 *d_rec, uint32_t n, int q)
    {
        const unsigned nblk = (n + PACK_BLOCK - 1) / PACK_BLOCK;
        uint32_t *tally = pk.scratch.d_tally.get() + 2 * q;
        hipLaunchKernelGGL(k_pack_plan, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, up, down, d_dir[q].get(), d_size.get());
        hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(1024), 0, s->stream, nblk, (const uint32_t *)d_size.get(), d_dir[q].get(), d_run.get(), tally);
        hipLaunchKernelGGL(k_pack_write, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, up, (const PackDirDev *)d_dir[q].get(), (uint32_t *)d_out[q].get());
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(pk.scratch.h_tally.get() + 2 * q, tally, 8, hipMemcpyDeviceToHost, s->stream));
        pk.stats.chunks++;
        return SM_OK;
    }
    // the chunk in buffer q, whose kernels and tally are over, into the file: through the staging's host buffers on the copy stream
    int take(int q, uint32_t n, PackWriter &w)
    {
        MapStaging &st = s->staging;
        const size_t nblk = ((size_t)n + PACK_BLOCK - 1) / PACK_BLOCK;
        const uint32_t bytes = pk.scratch.h()[2 * q], raws = pk.scratch.h()[2 * q + 1];
        if (bytes > (uint64_t)n * sm_mapfile::RECORD_BYTES) { g_err = "sm_pack_maps: internal: a chunk's payload exceeds its records"; return SM_E_HIP; }
        const double t0 = now_ms();
        HIPCK(hipMemcpyAsync(st.h_dir[q].get(), d_dir[q].get(), nblk * sizeof(PackDirDev), hipMemcpyDeviceToHost, st.copy));
        HIPCK(hipMemcpyAsync(st.h_rec[q].get(), d_out[q].get(), bytes, hipMemcpyDeviceToHost, st.copy));
        HIPCK(hipStreamSynchronize(st.copy));
        const bool ok = w.append((const sm_mapfile::PackDir *)st.h_dir[q].get(), nblk, st.h_rec[q].get(), bytes);
        pk.stats.write_ms += (float)(now_ms() - t0);
        pk.stats.blocks += (uint32_t)nblk;
        pk.stats.raw_blocks += raws;
        return ok ? SM_OK : SM_E_ARG;
    }
};

}  // namespace

int sm_impl::maps_ensure_packed(sm_ctx *s)
{
    MapStaging &st = s->staging;
    if (st.ev_u1[1]) return SM_OK;
    Host<uint8_t> h[2];
    Dev<uint8_t> d[2], p[2];
    Event e[4];
    for (int q = 0; q < 2; ++q) {
        HIPCK(hipHostMalloc((void **)h[q].put(), (size_t)CHUNK_BLOCKS * sm_mapfile::PACK_DIR_BYTES, hipHostMallocDefault));
        if (int rc = dalloc(d[q], (size_t)CHUNK_BLOCKS * sm_mapfile::PACK_DIR_BYTES)) return rc;
        if (int rc = dalloc(p[q], (size_t)CHUNK * sm_mapfile::RECORD_BYTES)) return rc;
    }
    for (Event &ev : e) HIPCK(hipEventCreate(ev.put()));
    for (int q = 0; q < 2; ++q) { st.h_dir[q] = std::move(h[q]); st.d_dir[q] = std::move(d[q]); st.d_pk[q] = std::move(p[q]); }
    st.ev_u0[0] = std::move(e[0]); st.ev_u0[1] = std::move(e[1]); st.ev_u1[0] = std::move(e[2]);
    st.ev_u1[1] = std::move(e[3]);                       // last: the pair is whole or absent
    return SM_OK;
}

void sm_impl::maps_unpack(sm_ctx *s, const uint8_t *d_dir, const uint8_t *d_payload, uint32_t n, int32_t pos_step_log2, float4 *d_rec)
{
    hipLaunchKernelGGL(k_unpack, dim3((n + PACK_BLOCK - 1) / PACK_BLOCK), dim3(256), 0, s->stream, (const PackDirDev *)d_dir, (const uint32_t *)d_payload, n,
                       std::ldexp(1.0f, pos_step_log2), d_rec);
}

extern "C" {

int sm_default_pack_params(sm_pack_params *p)
{
    if (!p) { g_err = "sm_default_pack_params: null argument"; return SM_E_ARG; }
    p->pos_step_log2 = sm_mapfile::PACK_STEP_DEFAULT;
    return SM_OK;
}

int sm_pack_maps(sm_ctx *s, const sm_map_source *src, const sm_pack_params *p, const char *out_prefix)
{
    const char *who = "sm_pack_maps";
    SetCall call(s, src, who);
    if (!s || !src || !out_prefix) { g_err = std::string(who) + ": null context, source or output prefix"; return SM_E_ARG; }
    int rc;
    if ((rc = call.open([&] { return check_params(p, who); }))) return rc;
    const sm_mapset::ReadSet &set = call.set;
    const uint32_t cnt = call.cnt, n_files = src->n_paths, n_out = n_files + (src->include_model ? 1u : 0u);
    if ((rc = check_names(src, out_prefix, n_out, "smp", who))) return rc;
    Pack &pk = s->pack;
    pk.stats = sm_pack_stats_t{};
    pk.stats_valid = true;
    pk.stats.records = call.total;
    for (const sm_mapfile::Header &h : set.files) pk.stats.bytes_in += h.size;
    pk.stats.bytes_in += (uint64_t)cnt * sm_mapfile::RECORD_BYTES;

    OutFiles outs(who);
    PackJob job(s, p->pos_step_log2);
    if (call.total && ((rc = call.staging()) || (rc = maps_ensure_packed(s)) || (rc = job.open()))) return rc;
    PackWriter w;
    // output i begins: its temporary with the header
    const auto begin = [&](uint32_t i, uint32_t count, int32_t start_id, int32_t end_id) -> int {
        const std::string name = out_name(out_prefix, i, "smp");
        outs.done.push_back({name + ".pack.tmp", name, false});
        return w.open(outs.done.back().tmp, count, start_id, end_id, p->pos_step_log2, who) ? SM_OK : SM_E_ARG;
    };
    // the files without a record have no chunk: written here, in front
    for (uint32_t i = 0; i < n_files; ++i)
        if (set.files[i].count == 0 && ((rc = begin(i, 0, set.files[i].start_id, set.files[i].end_id)) || (rc = w.commit() ? SM_OK : SM_E_ARG))) return rc;

    // ---- the files, chunk by chunk: the host reads chunk c + 1 while the device encodes chunk c, then writes chunk c
    {
        MapStream in(s, who, src->paths, {&pk.stats.read_ms, &pk.stats.copy_ms, &pk.stats.device_ms});
        const auto enqueue = [&](MapStream::Chunk &ck) -> int {
            if (int e = in.next(ck)) return e;
            if (ck.job->first == 0)
                if (int e = job.begin_file()) return e;
            if (int e = job.encode(ck.d_rec, ck.job->n, ck.q)) return e;
            return in.done(ck.q);
        };
        const auto finish = [&](const MapStream::Chunk &ck) -> int {
            const sm_mapfile::Job &j = *ck.job;
            const sm_mapfile::Header &h = set.files[j.file];
            if (int e = in.fold(ck.q)) return e;
            if (j.first == 0)
                if (int e = begin(j.file, h.count, h.start_id, h.end_id)) return e;
            if (int e = job.take(ck.q, j.n, w)) return e;
            if ((uint64_t)j.first + j.n == h.count && !w.commit()) return SM_E_ARG;
            return SM_OK;
        };
        if ((rc = sm_mapset::stream_files(in, set.jobs, enqueue, finish))) return rc;
        pk.stats.unpack_ms = in.unpack_ms();
    }

    // ---- the live model, as one more file
    if (src->include_model) {
        if ((rc = call.model()) || (rc = begin(n_files, cnt, 0, 0))) return rc;
        if (cnt && (rc = job.begin_file())) return rc;
        for (uint32_t first = 0; first < cnt; first += CHUNK) {
            const uint32_t n = std::min(CHUNK, cnt - first);
            if ((rc = mark(s, pk.scratch.ev[EV_MODEL0])) || (rc = job.encode(call.d_model + (size_t)first * 3, n, 0)) || (rc = mark(s, pk.scratch.ev[EV_MODEL1])) ||
                (rc = add_marked(&pk.scratch.ev[EV_MODEL0], &pk.stats.device_ms)))
                return rc;
            HIPCK(hipStreamSynchronize(s->stream));
            if ((rc = job.take(0, n, w))) return rc;
        }
        if (!w.commit()) return SM_E_ARG;
    }
    const double t0 = now_ms();
    if ((rc = outs.rename(pk.stats.bytes_out))) return rc;
    pk.stats.write_ms += (float)(now_ms() - t0);
    pk.stats.files = (uint32_t)outs.done.size();
    pk.stats.total_ms = call.elapsed_ms();
    return SM_OK;
}

int sm_unpack_maps(sm_ctx *s, const sm_map_source *src, const char *out_prefix)
{
    const char *who = "sm_unpack_maps";
    SetCall call(s, src, who);
    if (!s || !src || !out_prefix) { g_err = std::string(who) + ": null context, source or output prefix"; return SM_E_ARG; }
    int rc;
    if ((rc = call.open([&]() -> int {
            if (src->include_model) { g_err = std::string(who) + ": include_model must be 0"; return SM_E_ARG; }
            return SM_OK;
        })))
        return rc;
    const sm_mapset::ReadSet &set = call.set;
    const uint32_t n_files = src->n_paths;
    if ((rc = check_names(src, out_prefix, n_files, "bin", who))) return rc;
    Pack &pk = s->pack;
    pk.stats = sm_pack_stats_t{};
    pk.stats_valid = true;
    pk.stats.records = set.file_total;

    OutFiles outs(who);
    outs.done.reserve(n_files);
    for (uint32_t i = 0; i < n_files; ++i) {
        const std::string name = out_name(out_prefix, i, "bin");
        outs.done.push_back({name + ".unpack.tmp", name, false});
    }
    // the chunks of the packed files alone go through the device
    std::vector<sm_mapfile::Job> jobs;
    for (const sm_mapfile::Job &j : set.jobs)
        if (set.files[j.file].packed) jobs.push_back(j);
    if (!jobs.empty() && (rc = call.staging())) return rc;

    sm_mapfile::Writer w;
    // ---- a plain file, and a packed one without a record: on the host
    for (uint32_t i = 0; i < n_files; ++i) {
        const sm_mapfile::Header &h = set.files[i];
        pk.stats.bytes_in += h.size;
        if (h.packed) {
            pk.stats.blocks += (uint32_t)h.dir.size();
            for (const sm_mapfile::PackDir &d : h.dir) pk.stats.raw_blocks += d.flags & sm_mapfile::PACK_RAW;
            if (h.count) continue;
        }
        const double t0 = now_ms();
        const bool ok = w.open(outs.done[i].tmp, h.count, h.start_id, h.end_id, who, g_err) && (h.packed || w.append_head_of(src->paths[i], h.count, g_err)) &&
                        w.commit(g_err);
        pk.stats.write_ms += (float)(now_ms() - t0);
        if (!ok) return SM_E_ARG;
    }
    // ---- the packed files, chunk by chunk: decoded by the stream itself; the host writes chunk c while chunk c + 1 is on its way
    {
        MapStaging &st = s->staging;
        MapStream in(s, who, src->paths, {&pk.stats.read_ms, &pk.stats.copy_ms, &pk.stats.device_ms});
        const auto enqueue = [&](MapStream::Chunk &ck) -> int {
            if (int e = in.next(ck)) return e;
            pk.stats.chunks++;
            return in.done(ck.q);
        };
        const auto finish = [&](const MapStream::Chunk &ck) -> int {
            const sm_mapfile::Job &j = *ck.job;
            const sm_mapfile::Header &h = set.files[j.file];
            if (int e = in.fold(ck.q)) return e;
            const double t0 = now_ms();
            HIPCK(hipMemcpyAsync(st.h_rec[ck.q].get(), ck.d_rec, (size_t)j.n * sm_mapfile::RECORD_BYTES, hipMemcpyDeviceToHost, st.copy));
            HIPCK(hipStreamSynchronize(st.copy));
            bool ok = j.first != 0 || w.open(outs.done[j.file].tmp, h.count, h.start_id, h.end_id, who, g_err);
            ok = ok && w.append(st.h_rec[ck.q].get(), j.n, g_err) && ((uint64_t)j.first + j.n != h.count || w.commit(g_err));
            pk.stats.write_ms += (float)(now_ms() - t0);
            return ok ? SM_OK : SM_E_ARG;
        };
        if ((rc = sm_mapset::stream_files(in, jobs, enqueue, finish))) return rc;
        pk.stats.unpack_ms = in.unpack_ms();
    }
    const double t0 = now_ms();
    if ((rc = outs.rename(pk.stats.bytes_out))) return rc;
    pk.stats.write_ms += (float)(now_ms() - t0);
    pk.stats.files = n_files;
    pk.stats.total_ms = call.elapsed_ms();
    return SM_OK;
}

SM_STATS_GETTER(sm_pack_stats, sm_pack_stats_t, pack, "sm_pack_maps / sm_unpack_maps")

}  // extern "C"
