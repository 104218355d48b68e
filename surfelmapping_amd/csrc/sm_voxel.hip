// sm_voxel.hip -- what the users of a voxel table share on the host (sm_voxel.h): the grid, the slot count and the tally's verdict
// of simplification, registration and change detection; the lookup table of the latter two, its layout, initialisation, insert and
// finish; the ranked output of the first and the last; the pair sort of tiling and meshing.  Kernels: sm_k_voxel.h.
#include "sm_voxel.h"
#include "sm_k_voxel.h"

using namespace sm;

static constexpr uint32_t CHUNK = MapStaging::CHUNK;
static_assert(RankScratch::BLOCKS == CHUNK / 256, "a plane of block counts holds a chunk's");
static constexpr size_t LUT_SUM_BYTES = 8 * 7;           // per slot beside the key and the lookup record: SW, SP[3], SN[3]

SimplifyArgs sm_impl::voxel_args(int32_t voxel_mm, int shift, const float origin[3], int split, uint32_t max_cells)
{
    SimplifyArgs a{};
    a.V = (((long long)voxel_mm << shift) * 65536 + 500) / 1000;
    for (int k = 0; k < 3; ++k) a.origin[k] = origin[k];
    a.split = split;
    a.max_cells = max_cells;
    a.combine = env_is_one("SM_SIMPLIFY_NO_COMBINE") ? 0 : 1;
    return a;
}

int sm_impl::voxel_slots(uint64_t records, uint32_t max_cells, const char *who, const char *what, uint64_t &slots)
{
    slots = SIMP_MIN_SLOTS;
    while (slots < 2 * std::min<uint64_t>(records, max_cells)) slots <<= 1;
    if (slots > (1ull << 31)) { g_err = std::string(who) + ": " + what + " would need more than 2^31 slots"; return SM_E_CAPACITY; }
    return SM_OK;
}

int sm_impl::voxel_check_tally(const uint32_t *t, uint32_t max_cells, const char *who, const std::string &what)
{
    if (!t[SIMP_ERR]) return SM_OK;
    g_err = std::string(who) + ": more than max_cells = " + std::to_string(max_cells) + " " + what;
    return SM_E_CAPACITY;
}

// ---- the lookup table: per table the lookup records first (32-byte aligned), then key, SW, SP[3], SN[3], then the cover's keys

int sm_impl::lut_open(Dev<uint8_t> &mem, LookupTable *t, int n, uint64_t slots, bool cover, uint32_t *d_tally)
{
    const size_t S = (size_t)slots, per_table = S * (sizeof(RegCell) + 8 + LUT_SUM_BYTES + (cover ? 8 : 0));
    HIPCK(hipMalloc((void **)mem.put(), per_table * (size_t)n));
    for (int i = 0; i < n; ++i) {
        SimplifyTable &T = t[i].T, &TC = t[i].TC;
        uint8_t *b = mem.get() + per_table * (size_t)i;
        t[i].lut = (RegCell *)b;
        T.key = (unsigned long long *)(b + S * sizeof(RegCell));
        T.SW = T.key + S; T.SP = T.SW + S; T.SN = T.SP + 3 * S;
        T.mask = (uint32_t)(S - 1);
        T.tally = d_tally + i * SIMP_TALLY_WORDS;
        if (!cover) continue;
        TC.key = T.SN + 3 * S;
        TC.mask = T.mask;
        TC.tally = d_tally + (n + i) * SIMP_TALLY_WORDS;
    }
    return SM_OK;
}

int sm_impl::lut_clear(sm_ctx *s, const LookupTable *t, int n)
{
    for (int i = 0; i < n; ++i) {
        const size_t S = (size_t)t[i].T.mask + 1u;
        HIPCK(hipMemsetAsync(t[i].T.key, 0xFF, S * 8, s->stream));
        HIPCK(hipMemsetAsync(t[i].T.SW, 0, S * LUT_SUM_BYTES, s->stream));
        if (t[i].TC.key) HIPCK(hipMemsetAsync(t[i].TC.key, 0xFF, S * 8, s->stream));
    }
    return SM_OK;
}

void sm_impl::lut_insert(sm_ctx *s, const LookupTable &t, const float4 *d_rec, uint32_t n, int keep_class, uint32_t &launches)
{
    // (the switches are template arguments: as a kernel argument keep_class cost the instance without a cover table 12 VGPRs)
    const auto kernel = !t.TC.key ? k_lut_insert<false, false> : keep_class ? k_lut_insert<true, true> : k_lut_insert<true, false>;
    hipLaunchKernelGGL(kernel, dim3((n + 255) / 256), dim3(256), 0, s->stream, d_rec, n, t.a, t.T, t.ac, t.TC);
    launches++;
}

void sm_impl::lut_finish(sm_ctx *s, const LookupTable &t, uint32_t &launches)
{
    hipLaunchKernelGGL(k_lut_finish, dim3(t.T.mask / 256u + 1u), dim3(256), 0, s->stream, t.a, t.T, t.lut);
    launches++;
}

// ---- the lean claim table

size_t sm_impl::lean_slots(uint32_t records)
{
    uint64_t slots = SIMP_MIN_SLOTS;
    while (slots < 4ull * records) slots <<= 1;
    return (size_t)slots;
}

int sm_impl::lean_clear(sm_ctx *s, const LeanTable &t)
{
    const size_t S = (size_t)t.mask + 1u;
    HIPCK(hipMemsetAsync(t.key, 0xFF, S * 8, s->stream));
    HIPCK(hipMemsetAsync(t.run, 0, S * 8, s->stream));
    return SM_OK;
}

// ---- the pair sort

size_t sm_impl::pair_sort_hist_words(uint32_t n) { return (size_t)((n + PAIR_SORT_BLOCK - 1) / PAIR_SORT_BLOCK) * 256; }

int sm_impl::pair_sort(sm_ctx *s, unsigned long long *const key[2], uint32_t *const idx[2], uint32_t *hist, uint32_t n, unsigned long long varying,
                       int &which, uint32_t &launches, uint32_t &passes)
{
    const uint32_t nblk = (n + PAIR_SORT_BLOCK - 1) / PAIR_SORT_BLOCK;
    which = 0;
    for (int shift = 0; shift < 56; shift += 8) {
        if (!((varying >> shift) & 255ull)) continue;                            // (every key has the same digit here)
        hipLaunchKernelGGL(k_pair_sort_hist, dim3(nblk), dim3(256), 0, s->stream, (const unsigned long long *)key[which], n, shift, nblk, hist);
        hipLaunchKernelGGL(k_pair_sort_scan, dim3(1), dim3(1024), 0, s->stream, hist, nblk * 256u);
        hipLaunchKernelGGL(k_pair_sort_scatter, dim3(nblk), dim3(256), 0, s->stream, (const unsigned long long *)key[which], (const uint32_t *)idx[which], n,
                           shift, nblk, (const uint32_t *)hist, key[which ^ 1], idx[which ^ 1]);
        launches += 3;
        passes++;
        which ^= 1;
    }
    HIPCK(hipGetLastError());
    return SM_OK;
}

// ---- the ranked output

void sm_impl::frame_range(const sm_mapset::ReadSet &set, int32_t &start_id, int32_t &end_id)
{
    start_id = end_id = 0;
    for (size_t i = 0; i < set.files.size(); ++i) {
        start_id = i ? std::min(start_id, set.files[i].start_id) : set.files[i].start_id;
        end_id = i ? std::max(end_id, set.files[i].end_id) : set.files[i].end_id;
    }
}

int sm_impl::RankedOutput::ensure(int q, size_t records)
{
    if (!rs.d_info) {
        int rc;
        if ((rc = dalloc(rs.d_blk_cnt, 2 * RankScratch::BLOCKS)) || (rc = dalloc(rs.d_blk_base, 2 * RankScratch::BLOCKS))) return rc;
        HIPCK(hipHostMalloc((void **)rs.h_info.put(), 2 * sizeof(uint2), hipHostMallocDefault));
        if ((rc = dalloc(rs.d_info, 2))) return rc;      // last: it marks the set complete
    }
    if (records <= rs.out_cap[q]) return SM_OK;
    rs.out_cap[q] = 0;
    HIPCK(hipMalloc((void **)rs.d_out[q].put(), std::max<size_t>(records, 1) * 48));
    rs.out_cap[q] = records;
    return SM_OK;
}

int sm_impl::RankedOutput::open(const char *out_path, const char *suffix, const sm_mapset::ReadSet &set, uint32_t cnt)
{
    int rc;
    uint32_t largest_job = std::min(cnt, CHUNK);
    for (const sm_mapfile::Job &j : set.jobs) largest_job = std::max(largest_job, j.n);
    if (largest_job && ((rc = ensure(0, largest_job)) || (rc = ensure(1, largest_job)))) return rc;   // (an empty set: the file alone)
    int32_t start_id, end_id;
    frame_range(set, start_id, end_id);
    tmp = std::string(out_path) + suffix;
    return w.open(tmp, sm_mapfile::Writer::UNKNOWN, start_id, end_id, who, g_err) ? SM_OK : SM_E_ARG;
}

void sm_impl::RankedOutput::scan(uint32_t nblk, uint32_t *tally, int q, uint32_t &launches, int plane)
{
    hipLaunchKernelGGL(k_rank_scan, dim3(1), dim3(1024), 0, s->stream, (const uint32_t *)blk_cnt(plane), nblk, rs.d_blk_base.get() + plane * RankScratch::BLOCKS,
                       tally, q < 0 ? nullptr : rs.d_info.get() + q);
    launches++;
}

int sm_impl::RankedOutput::fetch(int q)
{
    if (writes()) HIPCK(hipMemcpyAsync(rs.h_info.get() + q, rs.d_info.get() + q, sizeof(uint2), hipMemcpyDeviceToHost, s->stream));
    return SM_OK;
}

int sm_impl::RankedOutput::stage(int q, hipStream_t stream, uint32_t &kept)
{
    kept = writes() ? rs.h_info.get()[q].y : 0u;
    if (kept) HIPCK(hipMemcpyAsync(s->staging.h_rec[q], rs.d_out[q], (size_t)kept * 48, hipMemcpyDeviceToHost, stream));
    return SM_OK;
}

int sm_impl::RankedOutput::write(int q, uint32_t kept)
{
    return !kept || w.append(s->staging.h_rec[q].get(), kept, g_err) ? SM_OK : SM_E_ARG;
}

int sm_impl::RankedOutput::commit(const char *out_path, uint32_t ranks, uint64_t &rows)
{
    if (w.rows() != ranks) { g_err = std::string(who) + ": internal: rows written and ranks given differ"; return SM_E_HIP; }
    rows = w.rows();
    if (!w.commit(g_err)) return SM_E_ARG;
    if (std::rename(tmp.c_str(), out_path) != 0) {
        std::remove(tmp.c_str());
        g_err = sm_mapfile::said(who, out_path, " saved err!!");
        return SM_E_ARG;
    }
    return SM_OK;
}
