// sm_loop.hip -- closing loops unasked (DESIGN.md "4i. Closing loops unasked"): the per-frame policy of sm_set_auto_loop.  While it
// is on, sm_track_frame / sm_track_frame_rgb track in the young map, count the old surfels the tracked pose sees (sm_old_in_view)
// and, with enough of them, make one sm_close_loop / sm_close_loop_rgb attempt (sm_close_loop_search after sm_set_auto_loop_search).  Both go through the
// internal bodies (track_windowed, close_loop), not the public entry points: the policy is not re-entered.  Host code only: the kernels are the trackers'
// (sm_k_track.h, sm_k_loop.h) and the warp's (sm_k_warp.h).
#include "sm_ctx.h"

using namespace sm;

int sm_impl::auto_loop_track(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params,
                             const sm_track_rgb_params *rgb_params, float *pose16_out, sm_track_info *info, sm_track_rgb_info *rgb_info)
{
    AutoLoop &a = s->aloop;
    if (!depth_mm || !pose16_out) { g_err = std::string(rgb ? "sm_track_frame_rgb" : "sm_track_frame") + ": null argument"; return SM_E_ARG; }
    const int64_t T = s->tick;
    const int64_t split64 = T - 1 - (int64_t)a.p.loop.min_age;
    // (no window yet: the plain prediction, whatever the times are)
    const int32_t split = split64 < 0 ? INT32_MIN : (int32_t)split64;
    sm_track_info inf;
    int rc;
    const TrackWindow young{split, INT32_MAX};
    if ((rc = track_windowed(s, rgb, depth_mm, guess16, params, rgb_params, &young, pose16_out, &inf, rgb_info, nullptr,
                             rgb ? "sm_track_frame_rgb_window" : "sm_track_frame_window")))
        return rc;
    if (info) *info = inf;
    if (inf.status != SM_TRACK_OK || split64 < 0) return SM_OK;
    if (T % a.p.every != 0 || T < a.rest_until) return SM_OK;
    uint32_t n_old = 0;
    if ((rc = sm_old_in_view(s, pose16_out, split, &n_old))) return rc;
    a.stats.checked++;
    a.stats.last_census = n_old;
    if (n_old < a.p.min_old) return SM_OK;

    // one attempt: the model, the caller's files and every file the retirement policy has written so far, each listed once
    std::vector<std::string> paths = a.paths;
    for (uint32_t i = 0; i < s->ret.files; ++i) {
        const std::string f = sm_mapfile::policy_file(s->ret.prefix, i);
        if (std::find(paths.begin(), paths.end(), f) == paths.end()) paths.push_back(f);
    }
    std::vector<const char *> ptrs(paths.size());
    for (size_t i = 0; i < paths.size(); ++i) ptrs[i] = paths[i].c_str();
    const sm_map_source src{ptrs.data(), (uint32_t)ptrs.size(), 1};
    float tracked[16], corrected[16];
    memcpy(tracked, pose16_out, 64);
    sm_loop_info li;
    a.stats.attempts++;
    a.rest_until = T + a.p.rest;                          // whatever the outcome
    rc = close_loop(s, rgb, depth_mm, tracked, &src, params, rgb_params, &a.p.loop, a.search, &a.sp, corrected, &li,
                    a.search ? "sm_close_loop_search" : rgb ? "sm_close_loop_rgb" : "sm_close_loop");
    if (rc) { a.stats.failed++; return rc; }
    a.stats.last = li;
    switch (li.status) {
    case SM_LOOP_CLOSED: a.stats.closed++; memcpy(pose16_out, corrected, 64); break;
    case SM_LOOP_NONE: a.stats.none++; break;
    case SM_LOOP_REJECTED: a.stats.rejected++; break;
    case SM_LOOP_NO_OLD_MAP: a.stats.no_old_map++; break;
    default: a.stats.failed++; break;
    }
    return SM_OK;
}

extern "C" {

int sm_default_auto_loop_params(const sm_config *c, sm_auto_loop_params *p)
{
    if (!c || !p) return SM_E_ARG;
    p->every = 1;
    p->rest = 10;
    p->min_old = 1000;
    return sm_default_loop_params(c, &p->loop);
}

int sm_set_auto_loop(sm_ctx *s, const sm_auto_loop_params *p, const sm_map_source *src)
{
    const char *who = "sm_set_auto_loop";
    if (!s) { g_err = std::string(who) + ": null context"; return SM_E_ARG; }
    if (int rc = check_whole_map(s, who)) return rc;
    AutoLoop &a = s->aloop;
    if (!p) { a.on = false; a.paths.clear(); return SM_OK; }
    if (p->every < 1 || p->rest < 0) { g_err = std::string(who) + ": every must be at least 1 and rest at least 0"; return SM_E_ARG; }
    int rc;
    if ((rc = check_loop_params(p->loop, who))) return rc;
    std::vector<std::string> paths;
    if (src) {
        if ((rc = check_map_source(src, who))) return rc;
        if (!sm_mapset::check_distinct_paths(src->paths, src->n_paths, who, g_err)) return SM_E_ARG;
        paths.assign(src->paths, src->paths + src->n_paths);
    }
    a.on = true;
    a.p = *p;
    a.paths = std::move(paths);
    a.rest_until = 0;
    a.stats = sm_auto_loop_stats_t{};
    return SM_OK;
}

int sm_set_auto_loop_search(sm_ctx *s, const sm_search_params *sp)
{
    const char *who = "sm_set_auto_loop_search";
    if (!s) { g_err = std::string(who) + ": null context"; return SM_E_ARG; }
    if (int rc = check_whole_map(s, who)) return rc;
    AutoLoop &a = s->aloop;
    if (!sp) { a.search = false; return SM_OK; }
    if (int rc = check_search_params(*sp, who)) return rc;
    a.search = true;
    a.sp = *sp;
    return SM_OK;
}

int sm_auto_loop_stats(sm_ctx *s, sm_auto_loop_stats_t *out)
{
    if (!s || !out) return SM_E_ARG;
    *out = s->aloop.stats;
    return SM_OK;
}

}  // extern "C"
