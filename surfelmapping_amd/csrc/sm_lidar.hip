// sm_lidar.hip -- lidar sweeps (sm_lidar_sweep, sm_lidar_sweep_maps; DESIGN.md "4k. Lidar sweeps"): the beams of a spherical grid
// against the live model and against map files streamed in chunks through the context's MapStaging, the live model last.  Kernels: sm_k_lidar.h.
#include "sm_map_stream.h"
#include "sm_k_lidar.h"
#include "sm_pose.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

constexpr double PI = 3.14159265358979323846;
const float DEFAULT_EL[16] = {-15, -14, -13, -12, -11, -10, -9, -8, -7, -6, -5, -4, -3, -2, -1, 0};

// the sensor's rules, without a context (SM_E_ARG with g_err set)
int check_sensor(const sm_lidar_sensor *sn, const char *fn)
{
    auto bad = [&](const char *what) { g_err = std::string(fn) + ": " + what; return SM_E_ARG; };
    if (!sn) return bad("null sensor");
    if (sn->n_az < 1 || sn->n_el < 1 || (uint64_t)sn->n_az * (uint64_t)sn->n_el > SM_LIDAR_MAX_BEAMS) return bad("n_az and n_el must be positive, n_az*n_el at most 2^22");
    if (!std::isfinite(sn->az0_deg) || !std::isfinite(sn->az_step_deg) || !(sn->az_step_deg > 0.0f)) return bad("az0 must be finite and the step finite and positive");
    if (!((double)sn->n_az * (double)sn->az_step_deg <= 360.0)) return bad("n_az*step exceeds 360 degrees");
    if (!sn->el_deg) return bad("null elevations");
    for (int32_t i = 0; i < sn->n_el; ++i) {
        const float e = sn->el_deg[i];
        if (!(e > -90.0f && e < 90.0f)) return bad("an elevation outside (-90, 90)");
        if (i && !(e > sn->el_deg[i - 1])) return bad("the elevations must be strictly increasing");
    }
    if (!std::isfinite(sn->min_range) || !std::isfinite(sn->max_range) || !(sn->min_range > 0.0f) || !(sn->min_range <= sn->max_range))
        return bad("0 < min_range <= max_range, both finite");
    return SM_OK;
}

void directions(const sm_lidar_sensor *sn, float *dir3)
{
    std::vector<double> sa(sn->n_az), ca(sn->n_az);
    for (int32_t j = 0; j < sn->n_az; ++j) {
        const double a = ((double)sn->az0_deg + (double)j * (double)sn->az_step_deg) * PI / 180.0;
        sa[j] = std::sin(a); ca[j] = std::cos(a);
    }
    for (int32_t i = 0; i < sn->n_el; ++i) {
        const double e = (double)sn->el_deg[i] * PI / 180.0, se = std::sin(e), ce = std::cos(e);
        float *row = dir3 + (size_t)i * sn->n_az * 3;
        for (int32_t j = 0; j < sn->n_az; ++j) {
            row[3 * j] = (float)(sa[j] * ce);
            row[3 * j + 1] = (float)(-se);
            row[3 * j + 2] = (float)(ca[j] * ce);
        }
    }
}

// the sensor's tables on the device; kept while the calls come with the same grid
int ensure_tables(sm_ctx *s, const sm_lidar_sensor *sn)
{
    Lidar &L = s->lid;
    std::vector<float> key{(float)sn->n_az, (float)sn->n_el, sn->az0_deg, sn->az_step_deg};
    key.insert(key.end(), sn->el_deg, sn->el_deg + sn->n_el);
    if (L.d_dir && key.size() == L.key.size() && !memcmp(key.data(), L.key.data(), key.size() * 4)) return SM_OK;
    L.key.clear();
    const size_t nb = (size_t)sn->n_az * sn->n_el;
    std::vector<float> dir(nb * 3), el(sn->n_el);
    directions(sn, dir.data());
    for (int32_t i = 0; i < sn->n_el; ++i) el[i] = (float)((double)sn->el_deg[i] * PI / 180.0);
    int rc;
    if ((rc = dalloc(L.d_dir, nb * 3)) || (rc = dalloc(L.d_el, (size_t)sn->n_el))) return rc;
    HIPCK(hipMemcpyAsync(L.d_dir, dir.data(), nb * 12, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(L.d_el, el.data(), (size_t)sn->n_el * 4, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));              // (the vectors go away)
    L.key = std::move(key);
    return SM_OK;
}

}  // namespace

// src null: the live model alone (sm_lidar_sweep); scene non-null: its actors after every static source (sm_lidar_sweep_scene)
int sm_impl::lidar_sweep(sm_ctx *s, const sm_map_source *src, const sm_lidar_sensor *sn, const float *poses16, uint32_t n_sweeps, float *range,
                         int32_t *id, uint8_t *rgb, uint8_t *sem, const char *fn, ScenePlan *scene)
{
    const double t_begin = now_ms();
    if (!s || !sn) { g_err = std::string(fn) + ": null context or sensor"; return SM_E_ARG; }
    if (n_sweeps && (!poses16 || !range)) { g_err = std::string(fn) + ": null pose or range"; return SM_E_ARG; }
    int rc;
    if ((rc = check_sensor(sn, fn))) return rc;
    for (uint32_t i = 0; i < n_sweeps; ++i)
        if ((rc = check_pose(poses16 + (size_t)i * 16, fn))) return rc;
    static const sm_map_source model_only{nullptr, 0, 1};
    if (!src) src = &model_only;
    sm_mapset::ReadSet set;
    uint32_t cnt;
    if ((rc = maps_open(s, src, fn, check_whole_map, set, cnt))) return rc;
    const uint64_t file_total = set.file_total;
    Lidar &L = s->lid;
    L.stats = sm_lidar_stats_t{};
    L.stats_valid = true;
    if (scene && (rc = scene_load(s, *scene, file_total + cnt, n_sweeps != 0, fn))) return rc;
    if (n_sweeps == 0) { L.stats.total_ms = (float)(now_ms() - t_begin); return SM_OK; }
    if (file_total && (rc = maps_ensure_staging(s))) return rc;
    if ((rc = ensure_tables(s, sn))) return rc;

    const size_t nb = (size_t)sn->n_az * sn->n_el;
    int cull;
    const uint32_t B = maps_batch(n_sweeps, nb, "SM_LIDAR_KEY_MB", "SM_LIDAR_NO_CULL", &cull);

    LidarGrid g{};
    g.dir = L.d_dir; g.el = L.d_el;
    g.n_az = sn->n_az; g.n_el = sn->n_el;
    double u0 = std::fmod((double)sn->az0_deg + 180.0, 360.0);                   // az0 reduced to [-180, 180)
    if (u0 < 0.0) u0 += 360.0;
    g.u0 = (float)(u0 - 180.0);
    g.step = sn->az_step_deg;
    g.min_range = sn->min_range; g.max_range = sn->max_range; g.min_conf = sn->min_conf;
    g.lane_beams = LIDAR_LANE_BEAMS;
    if (const char *lb = std::getenv("SM_LIDAR_LANE_BEAMS")) g.lane_beams = (uint32_t)std::max(0, std::atoi(lb));

    // the poses of all sweeps and the tally
    std::vector<LidarPose> poses(n_sweeps);
    for (uint32_t i = 0; i < n_sweeps; ++i) {
        double pose[16], inv[16];
        sm_pose::widen(poses16 + (size_t)i * 16, pose);
        sm_pose::rigid_inv_d(pose, inv);
        for (int k = 0; k < 16; ++k) poses[i].tinv[k] = (float)inv[k];
    }
    if ((size_t)n_sweeps > L.pose_cap) {
        L.pose_cap = 0;
        HIPCK(hipMalloc((void **)L.d_poses.put(), (size_t)n_sweeps * sizeof(LidarPose)));
        L.pose_cap = n_sweeps;
    }
    if (!L.d_tally) HIPCK(hipMalloc((void **)L.d_tally.put(), sizeof(LidarTally)));
    if (!L.ev[0]) { HIPCK(hipEventCreate(L.ev[0].put())); HIPCK(hipEventCreate(L.ev[1].put())); }
    LidarTally *d_tally = (LidarTally *)L.d_tally.get();
    const LidarPose *d_poses = (const LidarPose *)L.d_poses.get();
    HIPCK(hipMemcpyAsync(L.d_poses, poses.data(), (size_t)n_sweeps * sizeof(LidarPose), hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemsetAsync(d_tally, 0, sizeof(LidarTally), s->stream));

    // export scratch: keys | range | id | rgb | sem of one pass
    const size_t Bn = (size_t)B * nb;
    const size_t off_range = Bn * 8, off_id = off_range + Bn * 4, off_rgb = off_id + Bn * 4, off_sem = off_rgb + ((Bn * 3 + 255) & ~(size_t)255);
    if ((rc = ensure_export(s, off_sem + Bn))) return rc;
    uint8_t *base = (uint8_t *)s->d_export.get();
    uint64_t *d_key = (uint64_t *)base;
    float *d_range = (float *)(base + off_range);
    int32_t *d_id = (int32_t *)(base + off_id);
    uint8_t *d_rgb = base + off_rgb, *d_sem = base + off_sem;

    const MapsSoA chunk = planes(s->staging);
    const SurfelSet cur = s->M.s[s->h_state->cur];
    MapStream in(s, fn, src->paths, {&L.stats.read_ms, &L.stats.copy_ms, &L.stats.device_ms});

    for (uint32_t v0 = 0; v0 < n_sweeps; v0 += B) {
        const uint32_t b = std::min(B, n_sweeps - v0);
        const size_t bp = (size_t)b * nb;
        const unsigned rblocks = (unsigned)((bp + 255) / 256);
        L.stats.passes++;
        auto resolve = [&](const uint32_t *color, uint32_t first, uint32_t n, int last) {
            hipLaunchKernelGGL(k_lidar_resolve, dim3(rblocks), dim3(256), 0, s->stream, color, first, n, (const uint64_t *)d_key, bp, last, d_range,
                               d_id, d_rgb, d_sem);
        };
        fill_keys(s, d_key, bp);

        // ---- the files, chunk by chunk: the host reads chunk c + 1 while the copy and the kernels of chunk c run
        for (in.begin(set.jobs); in.more();) {
            MapStream::Chunk ck;
            if ((rc = in.next(ck))) return rc;
            const uint32_t n = ck.job->n;
            const unsigned nblk = (n + MAPS_BLOCK - 1) / MAPS_BLOCK;
            maps_intake(s, ck.d_rec, n);
            const uint32_t gid = (uint32_t)(set.id_base[ck.job->file] + ck.job->first);
            hipLaunchKernelGGL(k_lidar_splat_maps, dim3(nblk, b), dim3(256), 0, s->stream, chunk, n, gid, (const float4 *)s->staging.d_box.get(), g,
                               d_poses + v0, d_key, nb, cull, d_tally);
            resolve(chunk.color, gid, n, 0);
            if ((rc = in.done(ck.q))) return rc;
            HIPCK(hipGetLastError());
            L.stats.surfels += n;
            L.stats.chunks++;
        }
        if ((rc = in.fold(0)) || (rc = in.fold(1))) return rc;

        // ---- the live model, then the beams nobody won
        HIPCK(hipEventRecord(L.ev[0], s->stream));
        if (cnt) {
            for (uint32_t i = 0; i < b; ++i)
                hipLaunchKernelGGL(k_lidar_splat, dim3((cnt + 255) / 256), dim3(256), 0, s->stream, s->M, (const DevState *)s->d_state.get(),
                                   (const uint64_t *)s->d_alive.get(), g, poses[v0 + i], d_key + (size_t)i * nb, (uint32_t)file_total, d_tally);
            L.stats.surfels += cnt;
        }
        resolve(cur.color, (uint32_t)file_total, cnt, scene ? 0 : 1);
        HIPCK(hipEventRecord(L.ev[1], s->stream));
        HIPCK(hipGetLastError());
        // ---- the scene's actors, under this batch's poses; their resolve is the pass's last
        if (scene && (rc = scene_draw_lidar(s, *scene, g, d_poses + v0, v0, b, d_key, nb, d_range, d_id, d_rgb, d_sem))) return rc;

        const size_t vp0 = (size_t)v0 * nb;
        HIPCK(hipMemcpyAsync(range + vp0, d_range, bp * 4, hipMemcpyDeviceToHost, s->stream));
        if (id) HIPCK(hipMemcpyAsync(id + vp0, d_id, bp * 4, hipMemcpyDeviceToHost, s->stream));
        if (rgb) HIPCK(hipMemcpyAsync(rgb + vp0 * 3, d_rgb, bp * 3, hipMemcpyDeviceToHost, s->stream));
        if (sem) HIPCK(hipMemcpyAsync(sem + vp0, d_sem, bp, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        float ms = 0.0f;
        HIPCK(hipEventElapsedTime(&ms, L.ev[0], L.ev[1]));
        L.stats.device_ms += ms;
        if (scene && (rc = scene_fold(s))) return rc;
    }
    LidarTally t{};
    HIPCK(hipMemcpy(&t, d_tally, sizeof t, hipMemcpyDeviceToHost));
    L.stats.tests = t.tests; L.stats.wide = t.wide; L.stats.blocks_skipped = t.skipped;
    L.stats.total_ms = (float)(now_ms() - t_begin);
    return scene ? scene_end(s, *scene) : SM_OK;
}

extern "C" {

int sm_default_lidar_sensor(sm_lidar_sensor *p)
{
    if (!p) { g_err = "sm_default_lidar_sensor: null argument"; return SM_E_ARG; }
    p->n_az = 360; p->n_el = 16;
    p->az0_deg = 0.0f; p->az_step_deg = 1.0f;
    p->el_deg = DEFAULT_EL;
    p->min_range = 1.0f; p->max_range = 60.0f;
    p->min_conf = 0.0f;
    return SM_OK;
}

int sm_lidar_directions(const sm_lidar_sensor *sn, float *dir3)
{
    const char *fn = "sm_lidar_directions";
    if (!sn || !dir3) { g_err = std::string(fn) + ": null argument"; return SM_E_ARG; }
    if (int rc = check_sensor(sn, fn)) return rc;
    directions(sn, dir3);
    return SM_OK;
}

int sm_lidar_sweep(sm_ctx *s, const sm_lidar_sensor *sn, const float *pose16, float *range, int32_t *id, uint8_t *rgb, uint8_t *sem)
{
    const char *fn = "sm_lidar_sweep";
    if (!pose16 || !range) { g_err = std::string(fn) + ": null pose or range"; return SM_E_ARG; }
    return lidar_sweep(s, nullptr, sn, pose16, 1, range, id, rgb, sem, fn);
}

int sm_lidar_sweep_maps(sm_ctx *s, const sm_map_source *src, const sm_lidar_sensor *sn, const float *poses16, uint32_t n_sweeps, float *range,
                        int32_t *id, uint8_t *rgb, uint8_t *sem)
{
    const char *fn = "sm_lidar_sweep_maps";
    if (!src) { g_err = std::string(fn) + ": null source"; return SM_E_ARG; }
    return lidar_sweep(s, src, sn, poses16, n_sweeps, range, id, rgb, sem, fn);
}

int sm_lidar_stats(sm_ctx *s, sm_lidar_stats_t *out)
{
    if (!s || !out) { g_err = "sm_lidar_stats: null argument"; return SM_E_ARG; }
    if (!s->lid.stats_valid) { g_err = "sm_lidar_stats: no sm_lidar_sweep / sm_lidar_sweep_maps call yet"; return SM_E_ARG; }
    *out = s->lid.stats;
    return SM_OK;
}

}  // extern "C"
