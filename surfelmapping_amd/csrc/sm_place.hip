// sm_place.hip -- place recognition (DESIGN.md "4l. Place recognition"): fern codes of frames (sm_fern_encode*), the keyframe
// database (sm_fern_add / _count / _download / _save / _load), the match (sm_fern_match), and the two entry points that take a
// matched place to the geometric machinery (sm_search_pose_at, sm_close_loop_at).  Kernels: sm_k_place.h.  The table's generator
// and the keyframe file are sm_fernfile.h's (host only).
#include "sm_ctx.h"
#include "sm_fernfile.h"
#include "sm_k_place.h"
#include "sm_mapfile.h"

#include <cstdlib>

using namespace sm;

namespace {

constexpr size_t FIRST_CAP = 1024;                       // keyframes the database holds at first; doubled when full

// what every entry point with a context asks first; ferns: the context must have them
int place_check(sm_ctx *s, bool ferns, const char *who)
{
    if (!s) { g_err = std::string(who) + ": null context"; return SM_E_ARG; }
    if (int rc = check_whole_map(s, who)) return rc;
    if (int rc = check_not_mid_cull(s, who)) return rc;
    if (ferns && !s->place.on) { g_err = std::string(who) + ": the context has no ferns (sm_set_ferns)"; return SM_E_ARG; }
    return SM_OK;
}

size_t words_of(const sm_ctx *s) { return sm_fernfile::code_words(s->place.p); }

// room for n keyframes: the codes and times the device holds survive the move
int place_reserve(sm_ctx *s, size_t n)
{
    Place &pl = s->place;
    if (n <= pl.cap) return SM_OK;
    size_t cap = std::max(pl.cap, FIRST_CAP);
    while (cap < n) cap *= 2;
    cap = std::min<size_t>(cap, SM_FERN_MAX_KEYFRAMES);
    const size_t words = words_of(s), have = pl.count();
    Dev<uint32_t> codes;
    Dev<int32_t> times;
    int rc;
    if ((rc = dalloc(codes, cap * words)) || (rc = dalloc(times, cap))) return rc;
    if (have) {
        HIPCK(hipMemcpyAsync(codes, pl.d_codes, have * words * 4, hipMemcpyDeviceToDevice, s->stream));
        HIPCK(hipMemcpyAsync(times, pl.d_times, have * 4, hipMemcpyDeviceToDevice, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
    }
    pl.d_codes = std::move(codes);
    pl.d_times = std::move(times);
    pl.cap = cap;
    return SM_OK;
}

// alignment in bytes (a power of two, at most 16) of every row start of an image at p with `pitch` bytes per row
uint32_t row_alignment(const void *p, size_t pitch)
{
    const uintptr_t v = (uintptr_t)p | (uintptr_t)pitch | 16u;
    return (uint32_t)(v & (~v + 1u));
}

// the code of the images at d_rgb (may be null) / d_depth into d_code, enqueued
int encode_device(sm_ctx *s, const uint8_t *d_rgb, const uint16_t *d_depth)
{
    Place &pl = s->place;
    FernEncodeArgs a;
    a.rgb = d_rgb; a.depth = d_depth; a.table = pl.d_table; a.code = pl.d_code;
    a.W = s->W;
    a.n_words = (uint32_t)words_of(s);
    a.a_rgb = row_alignment(d_rgb, (size_t)s->W * 3);
    a.a_depth = row_alignment(d_depth, (size_t)s->W * 2);
    const dim3 grid((a.n_words + 3u) / 4u), block(256);
    if (pl.timed) HIPCK(hipEventRecord(pl.ev[0], s->stream));
    switch (pl.p.cell) {
    case 4: hipLaunchKernelGGL(k_fern_encode<4>, grid, block, 0, s->stream, a); break;
    case 8: hipLaunchKernelGGL(k_fern_encode<8>, grid, block, 0, s->stream, a); break;
    case 16: hipLaunchKernelGGL(k_fern_encode<16>, grid, block, 0, s->stream, a); break;
    default: hipLaunchKernelGGL(k_fern_encode<32>, grid, block, 0, s->stream, a); break;
    }
    HIPCK(hipGetLastError());
    if (pl.timed) HIPCK(hipEventRecord(pl.ev[1], s->stream));
    return SM_OK;
}

// the database becomes these n keyframes (host planes): into fresh buffers first, so that a failure leaves it as it was
int place_replace(sm_ctx *s, uint32_t n, const int32_t *times, const float *poses, const uint32_t *codes)
{
    Place &pl = s->place;
    size_t cap = FIRST_CAP;
    while (cap < n) cap *= 2;
    const size_t words = words_of(s);
    Dev<uint32_t> d_codes;
    Dev<int32_t> d_times;
    int rc;
    if ((rc = dalloc(d_codes, cap * words)) || (rc = dalloc(d_times, cap))) return rc;
    if (n) {
        HIPCK(hipMemcpyAsync(d_codes, codes, (size_t)n * words * 4, hipMemcpyHostToDevice, s->stream));
        HIPCK(hipMemcpyAsync(d_times, times, (size_t)n * 4, hipMemcpyHostToDevice, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
    }
    std::vector<int32_t> t(times, times + n);
    std::vector<float> p(poses, poses + (size_t)n * 16);
    pl.d_codes = std::move(d_codes);
    pl.d_times = std::move(d_times);
    pl.cap = cap;
    pl.times.swap(t);
    pl.poses.swap(p);
    return SM_OK;
}

// One launch, two answers: keys[0] the best keyframe of (min_time, max_time], keys[1] (two) of every time up to max_time2; the query
// is d_code as it stands.  One read-back of 16 bytes.  OPEN_LO as min_time: no lower end (sm_fern_match's own INT32_MIN is a
// strict bound, as its rule says).
constexpr long long OPEN_LO = (long long)INT32_MIN - 1;
int match_device(sm_ctx *s, long long min_time, int32_t max_time, bool two, int32_t max_time2, uint32_t *d_dis_all, unsigned long long keys[2])
{
    Place &pl = s->place;
    const size_t words = words_of(s);
    FernMatchArgs a;
    a.codes = (const uint4 *)pl.d_codes.get();
    a.times = pl.d_times;
    a.query = (const uint4 *)pl.d_code.get();
    a.count = pl.count();
    a.Q = (uint32_t)(words / 4);
    a.lpk = 1u;
    while (a.lpk * 2u <= std::min(a.Q, 64u)) a.lpk *= 2u;
    a.min_time = min_time; a.max_time = max_time;
    a.min_time2 = OPEN_LO; a.max_time2 = max_time2; a.two = two ? 1 : 0;
    a.dis_all = d_dis_all;
    a.keys = pl.d_keys;
    HIPCK(hipMemsetAsync(pl.d_keys, 0xFF, 16, s->stream));
    if (pl.timed) HIPCK(hipEventRecord(pl.ev[2], s->stream));
    hipLaunchKernelGGL(k_fern_match, dim3((a.count + FERN_MATCH_KPB - 1u) / FERN_MATCH_KPB), dim3(256), 0, s->stream, a);
    HIPCK(hipGetLastError());
    if (pl.timed) HIPCK(hipEventRecord(pl.ev[3], s->stream));
    HIPCK(hipMemcpyAsync(keys, pl.d_keys, 16, hipMemcpyDeviceToHost, s->stream));
    return SM_OK;
}

}  // namespace

int sm_impl::auto_place_after_track(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const sm_track_params *params,
                                    const sm_track_rgb_params *rgb_params, float *pose16_out, int track_status, bool loop_closed)
{
    Place &pl = s->place;
    if (track_status != SM_TRACK_OK || loop_closed) return SM_OK;
    int rc;
    // the tracker's own device copies of this frame's images (an SM_TRACK_OK track has uploaded them)
    if ((rc = encode_device(s, rgb ? s->trk.d_rgb.get() : nullptr, s->trk.d_depth))) return rc;
    pl.stats.encoded++;
    const int64_t T = s->tick;
    const int64_t split64 = std::max<int64_t>(T - 1 - (int64_t)pl.ap.loop.min_age, INT32_MIN);
    const float n_ferns = (float)pl.p.n_ferns;
    unsigned long long keys[2] = {~0ull, ~0ull};
    if (pl.count()) {
        if ((rc = match_device(s, OPEN_LO, INT32_MAX, true, (int32_t)split64, nullptr, keys))) return rc;
        HIPCK(hipStreamSynchronize(s->stream));
    }
    const uint32_t dis_any = (uint32_t)(keys[0] >> 32), dis_old = (uint32_t)(keys[1] >> 32);
    const int32_t k = keys[1] == ~0ull ? -1 : (int32_t)(uint32_t)(keys[1] & 0xFFFFFFFFull);
    pl.stats.last_k = k;
    pl.stats.last_dis = k < 0 ? UINT32_MAX : dis_old;
    const bool matched = k >= 0 && (float)dis_old <= pl.ap.match_below * n_ferns;
    if (matched) pl.stats.matched++;
    if (matched && T % pl.ap.every == 0 && T >= pl.rest_until) {
        float place[16];
        memcpy(place, pl.poses.data() + (size_t)k * 16, sizeof place);
        const double dx = (double)place[12] - (double)pose16_out[12], dy = (double)place[13] - (double)pose16_out[13],
                     dz = (double)place[14] - (double)pose16_out[14];
        if (std::sqrt((dx * dx + dy * dy) + dz * dz) > (double)pl.ap.min_jump) {
            pl.stats.attempts++;
            pl.rest_until = T + pl.ap.rest;                  // whatever the outcome
            // the sources of the auto-loop policy's attempt: its caller's files while it is on, and the retirement policy's
            std::vector<std::string> paths, retired;
            if (s->aloop.on) paths = s->aloop.paths;
            for (uint32_t i = 0; i < s->ret.files; ++i) {
                retired.push_back(sm_mapfile::policy_file(s->ret.prefix, i));
                if (std::find(paths.begin(), paths.end(), retired.back()) == paths.end()) paths.push_back(retired.back());
            }
            if (s->rec.radius > 0.0f && !retired.empty()) {  // the old map around the place, paged in first
                std::vector<const char *> rp(retired.size());
                for (size_t i = 0; i < retired.size(); ++i) rp[i] = retired[i].c_str();
                const sm_map_source rsrc{rp.data(), (uint32_t)rp.size(), 0};
                const sm_recall_params rpar{s->rec.radius};
                uint32_t n = 0;
                if ((rc = sm_recall(s, &rsrc, place, &rpar, SM_RECALL_MOVE, &n))) { pl.stats.failed++; return rc; }
            }
            std::vector<const char *> ptrs(paths.size());
            for (size_t i = 0; i < paths.size(); ++i) ptrs[i] = paths[i].c_str();
            const sm_map_source src{ptrs.data(), (uint32_t)ptrs.size(), 1};
            float tracked[16], corrected[16];
            memcpy(tracked, pose16_out, sizeof tracked);
            sm_loop_info li;
            rc = close_loop(s, rgb, depth_mm, tracked, &src, params, rgb_params, &pl.ap.loop, true, &pl.ap.search, corrected, &li,
                            "sm_close_loop_at", place);
            if (rc) { pl.stats.failed++; return rc; }
            pl.stats.last = li;
            switch (li.status) {
            case SM_LOOP_CLOSED: pl.stats.closed++; memcpy(pose16_out, corrected, 64); break;
            case SM_LOOP_NONE: pl.stats.none++; break;
            case SM_LOOP_REJECTED: pl.stats.rejected++; break;
            case SM_LOOP_NO_OLD_MAP: pl.stats.no_old_map++; break;
            default: pl.stats.failed++; break;
            }
            // (the attempt ran the trackers on this frame's images: d_code still holds this frame's code)
        }
    }
    if (pl.count() == 0 || (float)dis_any > pl.ap.add_above * n_ferns) {
        const size_t kf = pl.count(), words = words_of(s);
        if (kf >= SM_FERN_MAX_KEYFRAMES) { g_err = "sm_set_auto_place: the database holds 2^20 keyframes"; return SM_E_CAPACITY; }
        if ((rc = place_reserve(s, kf + 1))) return rc;
        const int32_t time = (int32_t)T;
        HIPCK(hipMemcpyAsync(pl.d_codes.get() + kf * words, pl.d_code, words * 4, hipMemcpyDeviceToDevice, s->stream));
        HIPCK(hipMemcpyAsync(pl.d_times.get() + kf, &time, 4, hipMemcpyHostToDevice, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        pl.times.push_back(time);
        pl.poses.insert(pl.poses.end(), pose16_out, pose16_out + 16);
        pl.stats.added++;
    }
    return SM_OK;
}

void sm_impl::place_reset(sm_ctx *s)
{
    s->place.times.clear();
    s->place.poses.clear();
}

void sm_impl::place_warp_poses(sm_ctx *s, const std::function<void(float *, int32_t)> &warp_pose)
{
    Place &pl = s->place;
    for (size_t k = 0; k < pl.times.size(); ++k) warp_pose(pl.poses.data() + k * 16, pl.times[k]);
}

extern "C" {

int sm_default_fern_params(const sm_config *c, sm_fern_params *p)
{
    if (!c || !p) { g_err = "sm_default_fern_params: null argument"; return SM_E_ARG; }
    auto mm = [](float clip) {
        const float v = clip * 1000.0f;
        return !(v > 0.0f) ? 0 : v >= 65535.0f ? 65535 : (int32_t)v;
    };
    p->n_ferns = 512;
    p->cell = 8;
    p->seed = 1;
    p->depth_lo_mm = mm(c->near_clip);
    p->depth_hi_mm = mm(c->far_clip);
    return SM_OK;
}

int sm_fern_table(const sm_fern_params *p, int32_t width, int32_t height, sm_fern *out)
{
    const char *who = "sm_fern_table";
    if (!p || !out) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if (const char *why = sm_fernfile::check_params(*p)) { g_err = std::string(who) + ": " + why; return SM_E_ARG; }
    if (width < p->cell || height < p->cell || width > 65535 * p->cell || height > 65535 * p->cell) {
        g_err = std::string(who) + ": the image holds no cell, or more than 65535 of them along an axis";
        return SM_E_ARG;
    }
    sm_fernfile::make_table(*p, width, height, out);
    return SM_OK;
}

int sm_set_ferns(sm_ctx *s, const sm_fern_params *p)
{
    const char *who = "sm_set_ferns";
    int rc;
    if ((rc = place_check(s, false, who))) return rc;
    if (!p) { s->place = Place(); return SM_OK; }
    if (const char *why = sm_fernfile::check_params(*p)) { g_err = std::string(who) + ": " + why; return SM_E_ARG; }
    std::vector<sm_fern> table((size_t)p->n_ferns);
    if ((rc = sm_fern_table(p, s->W, s->H, table.data()))) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    Place pl;
    pl.p = *p;
    std::vector<uint4> packed(table.size());
    for (size_t f = 0; f < table.size(); ++f) {
        const sm_fern &t = table[f];
        packed[f] = make_uint4((uint32_t)t.x | ((uint32_t)t.y << 16), (uint32_t)t.tr | ((uint32_t)t.tg << 16), (uint32_t)t.tb | ((uint32_t)t.td << 16), 0u);
    }
    const size_t P = (size_t)s->P;
    if ((rc = dalloc(pl.d_table, packed.size())) || (rc = dalloc(pl.d_rgb, P * 3)) || (rc = dalloc(pl.d_depth, P)) ||
        (rc = dalloc(pl.d_code, (size_t)p->n_ferns / 8)) || (rc = dalloc(pl.d_keys, 2)))
        return rc;
    const char *te = std::getenv("SM_PLACE_TIMING");
    pl.timed = te && te[0] == '1';
    if (pl.timed)
        for (Event &e : pl.ev) {
            HIPCK(hipEventCreate(e.put()));
            HIPCK(hipEventRecord(e, s->stream));          // (so that a query before the first launch finds recorded events)
        }
    HIPCK(hipMemcpyAsync(pl.d_table, packed.data(), packed.size() * sizeof(uint4), hipMemcpyHostToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    pl.on = true;
    s->place = std::move(pl);
    return SM_OK;
}

// Diagnostic, deliberately not part of include/sm_c_api.h (tools/place_probe.py): device time of the last k_fern_encode and the last
// k_fern_match of a context whose sm_set_ferns ran with SM_PLACE_TIMING=1; -1 each otherwise.  Waits for the stream.
int sm_debug_place_ms(sm_ctx *s, float *encode_ms, float *match_ms)
{
    if (!s || !encode_ms || !match_ms) return SM_E_ARG;
    *encode_ms = *match_ms = -1.0f;
    if (!s->place.on || !s->place.timed) return SM_OK;
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipStreamSynchronize(s->stream));
    HIPCK(hipEventElapsedTime(encode_ms, s->place.ev[0], s->place.ev[1]));
    HIPCK(hipEventElapsedTime(match_ms, s->place.ev[2], s->place.ev[3]));
    return SM_OK;
}

int sm_fern_encode_device(sm_ctx *s, const uint8_t *d_rgb, const uint16_t *d_depth_mm, uint32_t *code)
{
    const char *who = "sm_fern_encode_device";
    int rc;
    if ((rc = place_check(s, true, who))) return rc;
    if (!d_depth_mm || !code || ((uintptr_t)d_depth_mm & 1u)) { g_err = std::string(who) + ": null or misaligned argument"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = encode_device(s, d_rgb, d_depth_mm))) return rc;
    HIPCK(hipMemcpyAsync(code, s->place.d_code, words_of(s) * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

int sm_fern_encode(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, uint32_t *code)
{
    const char *who = "sm_fern_encode";
    int rc;
    if ((rc = place_check(s, true, who))) return rc;
    if (!depth_mm || !code) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    Place &pl = s->place;
    const size_t P = (size_t)s->P;
    if (rgb) HIPCK(hipMemcpyAsync(pl.d_rgb, rgb, P * 3, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(pl.d_depth, depth_mm, P * 2, hipMemcpyHostToDevice, s->stream));
    if ((rc = encode_device(s, rgb ? pl.d_rgb.get() : nullptr, pl.d_depth))) return rc;
    HIPCK(hipMemcpyAsync(code, pl.d_code, words_of(s) * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

int sm_fern_add(sm_ctx *s, const uint32_t *code, const float *pose16, int32_t time, uint32_t *index)
{
    const char *who = "sm_fern_add";
    int rc;
    if ((rc = place_check(s, true, who))) return rc;
    if (!code || !pose16) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    if ((rc = check_pose(pose16, who))) return rc;
    Place &pl = s->place;
    const size_t k = pl.count(), words = words_of(s);
    if (k >= SM_FERN_MAX_KEYFRAMES) { g_err = std::string(who) + ": the database holds 2^20 keyframes"; return SM_E_CAPACITY; }
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = place_reserve(s, k + 1))) return rc;
    HIPCK(hipMemcpyAsync(pl.d_codes.get() + k * words, code, words * 4, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(pl.d_times.get() + k, &time, 4, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    pl.times.push_back(time);
    pl.poses.insert(pl.poses.end(), pose16, pose16 + 16);
    if (index) *index = (uint32_t)k;
    return SM_OK;
}

int sm_fern_count(sm_ctx *s, uint32_t *n)
{
    const char *who = "sm_fern_count";
    if (int rc = place_check(s, true, who)) return rc;
    if (!n) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    *n = s->place.count();
    return SM_OK;
}

int sm_fern_download(sm_ctx *s, uint32_t *codes, float *poses16, int32_t *times)
{
    const char *who = "sm_fern_download";
    if (int rc = place_check(s, true, who)) return rc;
    Place &pl = s->place;
    const size_t n = pl.count();
    if (codes && n) {
        HIPCK(hipSetDevice(s->cfg.device));
        HIPCK(hipMemcpyAsync(codes, pl.d_codes, n * words_of(s) * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
    }
    if (poses16 && n) memcpy(poses16, pl.poses.data(), n * 64);
    if (times && n) memcpy(times, pl.times.data(), n * 4);
    return SM_OK;
}

int sm_fern_save(sm_ctx *s, const char *path)
{
    const char *who = "sm_fern_save";
    int rc;
    if ((rc = place_check(s, true, who))) return rc;
    if (!path) { g_err = std::string(who) + ": null path"; return SM_E_ARG; }
    Place &pl = s->place;
    std::vector<uint32_t> codes((size_t)pl.count() * words_of(s));
    if ((rc = sm_fern_download(s, codes.data(), nullptr, nullptr))) return rc;
    sm_fernfile::Header h;
    h.p = pl.p; h.width = s->W; h.height = s->H; h.count = pl.count();
    std::string err;
    if (!sm_fernfile::write_file(path, h, pl.times.data(), pl.poses.data(), codes.data(), err)) { g_err = std::string(who) + ": " + err; return SM_E_ARG; }
    return SM_OK;
}

int sm_fern_load(sm_ctx *s, const char *path)
{
    const char *who = "sm_fern_load";
    int rc;
    if ((rc = place_check(s, true, who))) return rc;
    if (!path) { g_err = std::string(who) + ": null path"; return SM_E_ARG; }
    Place &pl = s->place;
    sm_fernfile::Header h;
    std::string err;
    sm_fernfile::File f = sm_fernfile::open_checked(path, h, err);
    if (!f) { g_err = std::string(who) + ": " + err; return SM_E_ARG; }
    if (!sm_fernfile::same_params(h.p, pl.p) || h.width != s->W || h.height != s->H) {
        g_err = std::string(who) + ": " + path + " was written with other fern parameters or another image size";
        return SM_E_ARG;
    }
    std::vector<int32_t> times(h.count);
    std::vector<float> poses((size_t)h.count * 16);
    std::vector<uint32_t> codes((size_t)h.count * words_of(s));
    if (!sm_fernfile::read_records(f.get(), h, times.data(), poses.data(), codes.data(), err, path)) { g_err = std::string(who) + ": " + err; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    return place_replace(s, h.count, times.data(), poses.data(), codes.data());
}

int sm_fern_match(sm_ctx *s, const uint32_t *code, int32_t min_time, int32_t max_time, int32_t *index, uint32_t *dis, uint32_t *dis_all)
{
    const char *who = "sm_fern_match";
    int rc;
    if ((rc = place_check(s, true, who))) return rc;
    if (!code || !index || !dis) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    Place &pl = s->place;
    *index = -1;
    *dis = UINT32_MAX;
    const uint32_t n = pl.count();
    if (n == 0) return SM_OK;
    HIPCK(hipSetDevice(s->cfg.device));
    if (dis_all && pl.dis_cap < pl.cap) {
        pl.dis_cap = 0;
        if ((rc = dalloc(pl.d_dis, pl.cap))) return rc;
        pl.dis_cap = pl.cap;
    }
    unsigned long long keys[2];
    HIPCK(hipMemcpyAsync(pl.d_code, code, words_of(s) * 4, hipMemcpyHostToDevice, s->stream));
    if ((rc = match_device(s, min_time, max_time, false, 0, dis_all ? pl.d_dis.get() : nullptr, keys))) return rc;
    if (dis_all) HIPCK(hipMemcpyAsync(dis_all, pl.d_dis, (size_t)n * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    if (keys[0] != ~0ull) {
        *index = (int32_t)(uint32_t)(keys[0] & 0xFFFFFFFFull);
        *dis = (uint32_t)(keys[0] >> 32);
    }
    return SM_OK;
}

int sm_default_auto_place_params(const sm_config *c, sm_auto_place_params *p)
{
    if (!c || !p) { g_err = "sm_default_auto_place_params: null argument"; return SM_E_ARG; }
    p->every = 1;
    p->rest = 10;
    p->add_above = 0.2f;
    p->match_below = 0.3f;
    p->min_jump = 2.0f;
    sm_default_loop_params(c, &p->loop);
    p->loop.max_trans = 50.0f;
    p->loop.max_rot_deg = 45.0f;
    return sm_default_search_params(&p->search);
}

int sm_set_auto_place(sm_ctx *s, const sm_auto_place_params *p)
{
    const char *who = "sm_set_auto_place";
    int rc;
    if (!s) { g_err = std::string(who) + ": null context"; return SM_E_ARG; }
    if ((rc = check_whole_map(s, who))) return rc;
    Place &pl = s->place;
    if (!p) { pl.auto_on = false; return SM_OK; }
    if (!pl.on) { g_err = std::string(who) + ": the context has no ferns (sm_set_ferns)"; return SM_E_ARG; }
    if (p->every < 1 || p->rest < 0) { g_err = std::string(who) + ": every must be at least 1 and rest at least 0"; return SM_E_ARG; }
    const float frac[2] = {p->add_above, p->match_below};
    for (float f : frac)
        if (!(f >= 0.0f && f <= 1.0f)) { g_err = std::string(who) + ": add_above and match_below are fractions in [0, 1]"; return SM_E_ARG; }
    if (!(p->min_jump >= 0.0f) || !std::isfinite(p->min_jump)) { g_err = std::string(who) + ": min_jump is negative or not finite"; return SM_E_ARG; }
    if ((rc = check_loop_params(p->loop, who)) || (rc = check_search_params(p->search, who))) return rc;
    pl.auto_on = true;
    pl.ap = *p;
    pl.rest_until = 0;
    pl.stats = sm_auto_place_stats_t{};
    pl.stats.last_k = -1;
    pl.stats.last_dis = UINT32_MAX;
    return SM_OK;
}

int sm_auto_place_stats(sm_ctx *s, sm_auto_place_stats_t *out)
{
    if (!s || !out) { g_err = "sm_auto_place_stats: null argument"; return SM_E_ARG; }
    if (int rc = check_whole_map(s, "sm_auto_place_stats")) return rc;
    *out = s->place.stats;
    return SM_OK;
}

int sm_search_pose_at(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pred16, const float *centre16,
                      const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_search_params *sp, int32_t min_time,
                      int32_t max_time, float *pose16_out, sm_search_info *info)
{
    const char *who = "sm_search_pose_at";
    if (!s || !pred16) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    int rc;
    if ((rc = check_whole_map(s, who)) || (rc = check_pose(pred16, who))) return rc;
    return search_pose(s, rgb, depth_mm, pred16, centre16, tp, rp, sp, min_time, max_time, pose16_out, info, who);
}

int sm_close_loop_at(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16, const float *place16,
                     const sm_map_source *src, const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_loop_params *lp,
                     const sm_search_params *sp, float *pose16_out, sm_loop_info *info)
{
    const char *who = "sm_close_loop_at";
    if (!s || !place16) { g_err = std::string(who) + ": null argument"; return SM_E_ARG; }
    int rc;
    if ((rc = check_whole_map(s, who)) || (rc = check_pose(place16, who))) return rc;
    return close_loop(s, rgb, depth_mm, pose16, src, tp, rp, lp, true, sp, pose16_out, info, who, place16);
}

}  // extern "C"
