// sm_points.hip -- point queries into a map set (sm_query_points_maps; DESIGN.md "4y. Point queries"): the set streamed once; per
// chunk the ray casts' voxel index of its records (sm_k_rays.h), every point walked through the cells its reach meets and against
// the wide list, the winners' centre, normal, radius, colour and class resolved while the chunk is on the device; then the keys
// become (d2, id) and every plane asked for goes back with one copy.  Kernels and the superset proof: sm_k_points.h; the call's
// frame: sm_set_call.h.  The points, the planes and the index are allocated per call and freed when it ends.
#include "sm_set_call.h"
#include "sm_k_points.h"

#include <climits>

using namespace sm;
using sm_mapfile::now_ms;

namespace {

constexpr uint32_t CHUNK = MapStaging::CHUNK;
static_assert(sizeof(sm_point) == 16 && sizeof(sm_point) == sizeof(float4), "a point is one float4 load");
static_assert(sizeof(RaysTally) == 32 && sizeof(RaysChunk) == 40, "the headers are copied as they are");

int check_params(const sm_points_params *p, const char *who)
{
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (p->cell_mm < 1 || p->cell_mm > (1 << 24)) return bad("cell_mm outside 1..2^24");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k])) return bad("non-finite origin");
    return SM_OK;
}

size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int sm_default_points_params(sm_points_params *p)
{
    if (!p) { g_err = "sm_default_points_params: null argument"; return SM_E_ARG; }
    *p = sm_points_params{};
    p->cell_mm = 250;
    return SM_OK;
}

int sm_query_points_maps(sm_ctx *s, const sm_map_source *src, const sm_points_params *p, const sm_point *pts, uint32_t n_pts, float *d2, int32_t *id,
                         float *centre3, float *normal3, float *radius, uint8_t *rgb, uint8_t *sem)
{
    const char *who = "sm_query_points_maps";
    SetCall call(s, src, who);
    if (!s || !src || !p) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if (n_pts && (!pts || !d2)) { g_err = std::string(who) + ": null points or d2"; return SM_E_ARG; }
    if (n_pts > SM_POINTS_MAX) { g_err = std::string(who) + ": more than 2^24 points"; return SM_E_ARG; }
    int rc;
    if ((rc = call.open([&] { return check_params(p, who); }))) return rc;
    const sm_mapset::ReadSet &set = call.set;
    const uint32_t cnt = call.cnt;

    sm_points_stats_t st{};
    st.points = n_pts;
    st.records = call.total;
    Points &P = s->points;
    if (!n_pts) {
        st.total_ms = call.elapsed_ms();
        P.stats = st;
        P.stats_valid = true;
        return SM_OK;
    }

    // ---- the plan: the files' chunks, then the live model's
    const uint32_t model_chunks = (cnt + CHUNK - 1) / CHUNK;
    const size_t nchunks = set.jobs.size() + model_chunks;
    uint32_t largest = std::min(cnt, CHUNK);
    for (const sm_mapfile::Job &j : set.jobs) largest = std::max(largest, j.n);
    const size_t slots_max = lean_slots(largest);
    const int no_index = env_is_one("SM_POINTS_NO_INDEX") ? 1 : 0;
    const SimplifyArgs a = voxel_args(p->cell_mm, 0, p->origin, 0, 0u);
    const float min_conf = p->min_conf;

    // ---- one allocation: points | keys | table keys | runs | tally | d2 | id | pairs | wide | headers | flags | the planes that start as zeros:
    // centre | normal | radius | rgb | sem
    const size_t N = n_pts, L = std::max<uint32_t>(largest, 1u);
    size_t off = 0;
    const auto take = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    const size_t o_pts = take(N * 16), o_key = take(N * 8), o_tkey = take(slots_max * 8), o_run = take(slots_max * 8), o_tally = take(sizeof(RaysTally)),
                 o_d2 = take(N * 4), o_id = take(N * 4), o_pairs = take(L * 4 * (size_t)RAYS_MAX_CELLS), o_wide = take(L * 4),
                 o_hdr = take(std::max<size_t>(nchunks, 1) * sizeof(RaysChunk)), o_flag = take(L), o_ctr = take(N * 12), o_nrm = take(N * 12),
                 o_rad = take(N * 4), o_rgb = take(N * 3), o_sem = take(N);
    Dev<uint8_t> mem;
    if ((rc = dalloc(mem, off))) return rc;
    uint8_t *b = mem.get();
    const float4 *d_pts = (const float4 *)(b + o_pts);
    unsigned long long *d_key = (unsigned long long *)(b + o_key);
    unsigned long long *d_tkey = (unsigned long long *)(b + o_tkey);
    uint2 *d_run = (uint2 *)(b + o_run);
    RaysTally *d_tally = (RaysTally *)(b + o_tally);
    float *d_d2 = (float *)(b + o_d2), *d_ctr = centre3 ? (float *)(b + o_ctr) : nullptr, *d_nrm = normal3 ? (float *)(b + o_nrm) : nullptr,
          *d_rad = radius ? (float *)(b + o_rad) : nullptr;
    int32_t *d_id = (int32_t *)(b + o_id);
    uint32_t *d_pairs = (uint32_t *)(b + o_pairs), *d_wide = (uint32_t *)(b + o_wide);
    RaysChunk *d_hdr = (RaysChunk *)(b + o_hdr);
    uint8_t *d_rgb = rgb ? b + o_rgb : nullptr, *d_sem = sem ? b + o_sem : nullptr, *d_flag = b + o_flag;

    std::vector<Event> ev(3 * nchunks + 2);
    for (Event &e : ev) HIPCK(hipEventCreate(e.put()));
    const Event &ev_begin = ev[3 * nchunks], &ev_end = ev[3 * nchunks + 1];
    Event model_begins;
    HIPCK(hipEventCreate(model_begins.put()));

    if ((rc = call.model())) return rc;
    if (!set.jobs.empty() && (rc = call.staging())) return rc;

    std::vector<RaysChunk> hdr(std::max<size_t>(nchunks, 1));
    for (RaysChunk &h : hdr) { h = RaysChunk{}; for (int k = 0; k < 3; ++k) { h.lo[k] = INT_MAX; h.hi[k] = INT_MIN; } }
    HIPCK(hipMemcpyAsync(b + o_pts, pts, N * 16, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(d_hdr, hdr.data(), hdr.size() * sizeof(RaysChunk), hipMemcpyHostToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));              // (the pageable sources are the caller's and this function's)
    if ((rc = mark(s, ev_begin))) return rc;
    HIPCK(hipMemsetAsync(d_tally, 0, sizeof(RaysTally), s->stream));
    HIPCK(hipMemsetAsync(b + o_ctr, 0, off - o_ctr, s->stream));
    fill_keys(s, (uint64_t *)d_key, N);

    const unsigned pblocks = (unsigned)((N + 255) / 256);
    const bool planes = centre3 || normal3 || radius || rgb || sem;
    size_t c = 0;
    uint32_t most = 0;
    size_t most_at = 0;
    int lrc = SM_OK;
    float feed_ms = 0.0f;
    const auto chunk = [&](const float4 *d_rec, uint32_t n, uint32_t gid0) {
        if (!n || lrc || c >= nchunks) return;
        const size_t slots = lean_slots(n);
        const LeanTable T{d_tkey, d_run, (uint32_t)(slots - 1)};
        RaysChunk *h = d_hdr + c;
        const auto ck = [&](hipError_t e) { if (e != hipSuccess && !lrc) { g_err = std::string(who) + ": " + hipGetErrorString(e); lrc = SM_E_HIP; } };
        ck(hipEventRecord(ev[3 * c], s->stream));
        if (!no_index && lean_clear(s, T) != SM_OK && !lrc) lrc = SM_E_HIP;
        const unsigned nblk = (n + 255) / 256;
        hipLaunchKernelGGL(k_rays_count, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, a, min_conf, no_index, T, d_flag, d_wide, h);
        if (!no_index) {
            hipLaunchKernelGGL(k_rays_alloc, dim3((unsigned)(slots / 256)), dim3(256), 0, s->stream, T, h);
            hipLaunchKernelGGL(k_rays_fill, dim3(nblk), dim3(256), 0, s->stream, d_rec, n, a, min_conf, T, (const uint8_t *)d_flag, d_pairs);
        }
        ck(hipEventRecord(ev[3 * c + 1], s->stream));
        if (!no_index)
            hipLaunchKernelGGL(k_points_walk, dim3(pblocks), dim3(256), 0, s->stream, d_pts, n_pts, d_rec, n, gid0, a, T, (const uint32_t *)d_pairs,
                               (const uint8_t *)d_flag, (const RaysChunk *)h, d_key, d_tally);
        hipLaunchKernelGGL(k_points_wide, dim3(pblocks), dim3(256), 0, s->stream, d_pts, n_pts, d_rec, gid0, (const uint32_t *)d_wide, (const RaysChunk *)h,
                           d_key, d_tally);
        if (planes)
            hipLaunchKernelGGL(k_points_resolve, dim3(pblocks), dim3(256), 0, s->stream, d_rec, gid0, n, (const unsigned long long *)d_key, n_pts, d_ctr,
                               d_nrm, d_rad, d_rgb, d_sem);
        ck(hipEventRecord(ev[3 * c + 2], s->stream));
        if (n > most) { most = n; most_at = c; }
        ++c;
    };
    if ((rc = maps_feed(s, who, set, src->paths, cnt, call.d_model, {&st.read_ms, &st.copy_ms, &feed_ms}, model_begins, chunk))) return rc;
    if (lrc) return lrc;
    hipLaunchKernelGGL(k_points_finish, dim3(pblocks), dim3(256), 0, s->stream, d_pts, (const unsigned long long *)d_key, n_pts, d_d2, d_id, d_tally);
    if ((rc = mark(s, ev_end))) return rc;
    HIPCK(hipGetLastError());

    // ---- the tallies, then the planes asked for, one copy each (nothing has been written so far)
    RaysTally tally{};
    HIPCK(hipMemcpyAsync(&tally, d_tally, sizeof tally, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipMemcpyAsync(hdr.data(), d_hdr, hdr.size() * sizeof(RaysChunk), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    HIPCK(hipMemcpyAsync(d2, d_d2, N * 4, hipMemcpyDeviceToHost, s->stream));
    if (id) HIPCK(hipMemcpyAsync(id, d_id, N * 4, hipMemcpyDeviceToHost, s->stream));
    if (centre3) HIPCK(hipMemcpyAsync(centre3, d_ctr, N * 12, hipMemcpyDeviceToHost, s->stream));
    if (normal3) HIPCK(hipMemcpyAsync(normal3, d_nrm, N * 12, hipMemcpyDeviceToHost, s->stream));
    if (radius) HIPCK(hipMemcpyAsync(radius, d_rad, N * 4, hipMemcpyDeviceToHost, s->stream));
    if (rgb) HIPCK(hipMemcpyAsync(rgb, d_rgb, N * 3, hipMemcpyDeviceToHost, s->stream));
    if (sem) HIPCK(hipMemcpyAsync(sem, d_sem, N, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));

    float ms = 0.0f;
    for (size_t i = 0; i < c; ++i) {
        HIPCK(hipEventElapsedTime(&ms, ev[3 * i], ev[3 * i + 1]));
        st.index_ms += ms;
        HIPCK(hipEventElapsedTime(&ms, ev[3 * i + 1], ev[3 * i + 2]));
        st.walk_ms += ms;
        st.wide += hdr[i].wide;
        st.no_slot += hdr[i].no_slot;
    }
    HIPCK(hipEventElapsedTime(&ms, ev_begin, ev_end));
    st.device_ms = ms;
    if (c) { st.pairs = hdr[most_at].pairs; st.cells = hdr[most_at].cells; }
    st.probes = tally.probes;
    st.tests = tally.tests;
    st.gave_up = tally.gave_up;
    st.bad_points = tally.bad;
    st.chunks = (uint32_t)c;
    st.total_ms = call.elapsed_ms();
    P.stats = st;                                        // (a call that fails leaves the last one's)
    P.stats_valid = true;
    return SM_OK;
}

SM_STATS_GETTER(sm_query_points_stats, sm_points_stats_t, points, "sm_query_points_maps")

}  // extern "C"
