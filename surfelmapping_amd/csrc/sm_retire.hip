// sm_retire.hip -- retirement (sm_retire*, the periodic policy of sm_set_auto_retire): surfels that fusion can no longer reach
// leave the model for a caller's buffer or a map file, and the existing compaction closes the gaps.  Kernels: sm_k_retire.h.
#include "sm_ctx.h"
#include "sm_k_retire.h"
#include "sm_mapfile.h"

#include <cstdlib>

using namespace sm;

namespace {

constexpr uint32_t CHUNK = 1u << 22;             // surfels per staging chunk, as sm_download_model_aos
constexpr uint32_t FILE_CHUNK = 1u << 20;        // ... and per write of the periodic policy's map file (48 MiB of pinned staging)

int grid_tiles(uint32_t slots)
{
    const uint64_t tiles = ((uint64_t)slots + TILE - 1) / TILE;
    return (int)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), MAX_GRID);
}

int tic(sm_ctx *s, int i)
{
    if (s->ret.timed) HIPCK(hipEventRecord(s->ret.ev[i], s->stream));
    return SM_OK;
}

int check_args(sm_ctx *s, const float *pose16, const sm_retire_params *p, const char *who)
{
    if (int rc = check_whole_map(s, who)) return rc;
    if (p && (p->min_age < 0 || !std::isfinite(p->min_distance))) { g_err = std::string(who) + ": bad parameters"; return SM_E_ARG; }
    if (int rc = check_pose(pose16, who)) return rc;
    return check_not_mid_cull(s, who);
}

sm_retire_params params_or_default(sm_ctx *s, const sm_retire_params *params)
{
    sm_retire_params p;
    if (params) p = *params;
    else sm_default_retire_params(&s->cfg, &p);
    return p;
}

int ensure_scratch(sm_ctx *s)
{
    if (s->ret.d_mask) return SM_OK;
    Dev<uint64_t> mask;
    Dev<uint32_t> tile_ret, tile_base, total;
    int rc;
    if ((rc = dalloc(mask, s->alive_words)) || (rc = dalloc(tile_ret, s->dead_tiles)) || (rc = dalloc(tile_base, s->dead_tiles)) ||
        (rc = dalloc(total, 2)))
        return rc;
    const char *e = std::getenv("SM_RETIRE_TIMING");
    if (e && e[0] == '1')
        for (auto &ev : s->ret.ev) HIPCK(hipEventCreate(ev.put()));
    s->ret.d_mask = std::move(mask); s->ret.d_tile_ret = std::move(tile_ret); s->ret.d_tile_base = std::move(tile_base);
    s->ret.d_total = std::move(total);
    return SM_OK;
}

// Steps 1-2: the retired masks, per-tile counts and bases of the model as it stands; *n = how many would be retired.  Waits for
// the frames in flight; changes nothing in the model.
int retire_mark(sm_ctx *s, const float *pose16, const sm_retire_params *params, uint32_t *n)
{
    const sm_retire_params p = params_or_default(s, params);
    const float *pose = pose16 ? pose16 : s->last_pose;
    int rc = ensure_scratch(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;         // flushes a held-back association, completes the last frame's statistics
    s->ret.timed = (bool)s->ret.ev[0];
    s->ret.stats_valid = false;
    RetireArgs ra;
    ra.tick = (float)s->tick;
    ra.min_age = (float)p.min_age;
    ra.cx = pose[12]; ra.cy = pose[13]; ra.cz = pose[14];
    ra.md2 = p.min_distance * p.min_distance;
    ra.use_dist = p.min_distance <= 0.0f ? 0 : 1;
    if ((rc = tic(s, 0))) return rc;
    hipLaunchKernelGGL(k_retire_mark, dim3(grid_tiles(s->h_state->count)), dim3(256), 0, s->stream, s->M, s->d_state, ra, s->d_alive,
                       s->ret.d_mask, s->ret.d_tile_ret);
    if ((rc = tic(s, 1))) return rc;
    hipLaunchKernelGGL(k_retire_scan, dim3(1), dim3(1024), 0, s->stream, s->d_state, s->ret.d_tile_ret, s->ret.d_tile_base, s->ret.d_total);
    HIPCK(hipGetLastError());
    if ((rc = tic(s, 2))) return rc;
    uint32_t tot[2] = {0, 0};
    HIPCK(hipMemcpyAsync(tot, s->ret.d_total, sizeof tot, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    *n = tot[0];
    return SM_OK;
}

void launch_gather(sm_ctx *s, float *d_dst, uint32_t r0, uint32_t r1)
{
    hipLaunchKernelGGL(k_retire_gather, dim3(grid_tiles(s->h_state->count)), dim3(256), 0, s->stream, s->M, s->d_state, s->ret.d_mask,
                       s->ret.d_tile_ret, s->ret.d_tile_base, s->ret.d_total, (float4 *)d_dst, r0, r1);
}

// Step 3 into host memory, one staging chunk at a time
int retire_gather_host(sm_ctx *s, float *dst12, uint32_t n)
{
    int rc = tic(s, 3);
    if (rc) return rc;
    if (n && (rc = ensure_export(s, (size_t)std::min(n, CHUNK) * 48))) return rc;
    if ((rc = drain_export(s, n, CHUNK, dst12, 12, [s](float *d, uint32_t first, uint32_t m) { launch_gather(s, d, first, first + m); }, no_hook)))
        return rc;
    return tic(s, 4);
}

// Step 4: the retired become dead slots, the compaction that exists squeezes them out, and the kept surfels are published as
// an upload of them would be (publish_dense: the state, the compaction schedule, the tile boxes)
int retire_commit(sm_ctx *s, uint32_t n)
{
    int rc = tic(s, 5);
    if (rc) return rc;
    if (n) {
        const uint32_t words = (uint32_t)(((uint64_t)s->h_state->count + TILE - 1) / TILE) * TILE_WORDS;
        hipLaunchKernelGGL(k_retire_clear, dim3(std::min<uint32_t>((words + 255) / 256, MAX_GRID)), dim3(256), 0, s->stream, s->d_state,
                           s->ret.d_mask, s->ret.d_tile_ret, s->ret.d_total, s->d_alive, s->d_tile_dead);
        HIPCK(hipGetLastError());
        s->slots.dead_slots_made();
    }
    if ((rc = ensure_compact(s))) return rc;
    if ((rc = pull_state(s))) return rc;
    if ((rc = tic(s, 6))) return rc;
    if ((rc = publish_dense(s, s->h_state->count, 0))) return rc;
    if ((rc = tic(s, 7))) return rc;
    if (s->ret.timed) { HIPCK(hipStreamSynchronize(s->stream)); s->ret.stats_valid = true; }
    return SM_OK;
}

int retire_common(sm_ctx *s, const float *pose16, const sm_retire_params *params, float *dst, bool device, uint32_t cap, uint32_t *n,
                  const char *who)
{
    if (!s || !n) return SM_E_ARG;
    int rc = check_args(s, pose16, params, who);
    if (rc) return rc;
    if (device && hip_runtime_conflict(who)) return SM_E_HIP;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = retire_mark(s, pose16, params, n))) return rc;
    if (!dst) return SM_OK;                      // dry run
    if (cap < *n) { g_err = std::string(who) + ": destination too small"; return SM_E_CAPACITY; }
    if (device) {
        if ((rc = tic(s, 3))) return rc;
        if (*n) launch_gather(s, dst, 0u, *n);
        HIPCK(hipGetLastError());
        if ((rc = tic(s, 4))) return rc;
    } else if ((rc = retire_gather_host(s, dst, *n))) return rc;
    return retire_commit(s, *n);
}

}  // namespace

// The periodic policy, called by the frame entry points after a frame has been enqueued: nothing but this test on the
// frames that do not retire.
int sm_impl::auto_retire_after_frame(sm_ctx *s)
{
    Retire &r = s->ret;
    if (r.every <= 0 || s->tick <= 0 || s->tick % r.every != 0) return SM_OK;
    uint32_t n = 0;
    int rc = retire_mark(s, nullptr, &r.params, &n);       // at that frame's pose
    if (rc) return rc;
    if ((rc = tic(s, 3))) return rc;
    if (n) {
        // the map file (sm_mapfile.h) is on disk BEFORE the model changes; one chunk at a time through pinned staging, so that a
        // large retirement needs neither a host copy of its own nor gigabytes of staging
        if (!r.h_stage) HIPCK(hipHostMalloc(r.h_stage.put(), (size_t)FILE_CHUNK * sm_mapfile::RECORD_BYTES, hipHostMallocDefault));
        if ((rc = ensure_export(s, (size_t)std::min(n, FILE_CHUNK) * sm_mapfile::RECORD_BYTES))) return rc;
        const std::string path = sm_mapfile::policy_file(r.prefix, r.files);
        // the file index learns the file's box and its largest time now, from the records on the device, so that neither a recall
        // nor a warp has to read the file only to find out where and when it lies
        const float INF = __builtin_inff();
        float lo[3] = {INF, INF, INF}, hi[3] = {-INF, -INF, -INF}, tmax = -INF;
        sm_mapfile::Writer w;                    // (no half-written map file is left behind: a return below removes it)
        if (!w.open(path, n, r.last_tick, s->tick - 1, nullptr, g_err)) return SM_E_ARG;
        rc = drain_export(s, n, FILE_CHUNK, r.h_stage, 0, [s](float *d, uint32_t first, uint32_t m) { launch_gather(s, d, first, first + m); },
                          [&](uint32_t, uint32_t m) -> int {
                              if (int rb = recall_box_of(s, (const float *)s->d_export.get(), m, lo, hi, &tmax)) return rb;
                              return w.append(r.h_stage, m, g_err) ? SM_OK : SM_E_ARG;
                          });
        if (rc) return rc;
        if (!w.commit(g_err)) return SM_E_ARG;
        s->index.note_now(path, lo, hi, tmax);
        r.files++;
        r.surfels += n;
        r.last_tick = s->tick;
    }
    if ((rc = tic(s, 4))) return rc;
    if ((rc = retire_commit(s, n))) return rc;
    return auto_recall_after_retire(s, n != 0);          // sm_set_auto_recall: pages in around the same pose (one test unless it is on)
}

extern "C" {

int sm_default_retire_params(const sm_config *c, sm_retire_params *p)
{
    if (!c || !p) return SM_E_ARG;
    p->min_age = c->time_delta;
    p->min_distance = 1.5f * c->far_clip;
    return SM_OK;
}

int sm_retire(sm_ctx *s, const float *pose16, const sm_retire_params *params, float *dst12, uint32_t cap, uint32_t *n)
{
    return retire_common(s, pose16, params, dst12, false, cap, n, "sm_retire");
}

int sm_retire_device(sm_ctx *s, const float *pose16, const sm_retire_params *params, float *d_dst12, uint32_t cap, uint32_t *n)
{
    if (d_dst12 && ((uintptr_t)d_dst12 & 15u)) { g_err = "sm_retire_device: destination not 16-byte aligned"; return SM_E_ARG; }
    return retire_common(s, pose16, params, d_dst12, true, cap, n, "sm_retire_device");
}

int sm_set_auto_retire(sm_ctx *s, const sm_retire_params *params, int32_t every, const char *path_prefix)
{
    if (!s) return SM_E_ARG;
    const sm_retire_params p = params_or_default(s, params);
    int rc = check_args(s, nullptr, &p, "sm_set_auto_retire");
    if (rc) return rc;
    Retire &r = s->ret;
    if (every <= 0 || !path_prefix) { r.every = 0; r.prefix.clear(); return SM_OK; }
    if (s->rec.radius > 0.0f && (rc = check_recall_policy(s->rec.radius, p, "sm_set_auto_retire"))) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    if ((rc = ensure_scratch(s)) || (rc = recall_ensure_scratch(s))) return rc;     // so that the frame that retires first allocates nothing (the file index's box pass included)
    r.params = p;
    r.every = every;
    r.prefix = path_prefix;
    return SM_OK;
}

int sm_auto_retire_stats(sm_ctx *s, uint32_t *files, uint64_t *surfels)
{
    if (!s) return SM_E_ARG;
    if (files) *files = s->ret.files;
    if (surfels) *surfels = s->ret.surfels;
    return SM_OK;
}

// diagnostic, not part of the C-ABI header: device times in ms of the last retirement made with SM_RETIRE_TIMING=1 in the
// environment when the context retired first -- mark, scan, gather (with the copies of its chunks when the destination is host
// memory), clear + compaction, the publication of the kept surfels (state and tile bounds); -1 each if that call was not timed or ended before the model changed
int sm_debug_retire_stats(sm_ctx *s, float *ms5)
{
    if (!s || !ms5) return SM_E_ARG;
    for (int i = 0; i < 5; ++i) ms5[i] = -1.0f;
    if (!s->ret.timed || !s->ret.stats_valid) return SM_OK;
    HIPCK(hipSetDevice(s->cfg.device));
    const int a[5] = {0, 1, 3, 5, 6}, b[5] = {1, 2, 4, 6, 7};
    for (int i = 0; i < 5; ++i) HIPCK(hipEventElapsedTime(&ms5[i], s->ret.ev[a[i]], s->ret.ev[b[i]]));
    return SM_OK;
}

}  // extern "C"
