// sm_scene.hip -- scenes (sm_render_image_scene, sm_lidar_sweep_scene, sm_scene_place_rows, sm_scene_stats; DESIGN.md "4w. Scenes"):
// a map set with moving actors in it.  The static part is the streamed renderer's (sm_render_maps.hip) and the lidar's pass
// (sm_lidar.hip), which call the scene_* functions below where an actor is a source like the others; this file checks the scene,
// keeps the actor files resident for the call and launches their kernels.  Kernels: sm_k_scene.h.
#include "sm_map_stream.h"
#include "sm_k_scene.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

// sm_scene_place_rows' rule for one row, the host twin of warp_apply (sm_d_warp.h); the build's -ffp-contract=off covers it
void place_row(const float *C, const float *m, float *o)
{
    const float x = m[0], y = m[1], z = m[2], nx = m[8], ny = m[9], nz = m[10];
    if (o != m) memcpy(o, m, 48);
    for (int r = 0; r < 3; ++r) {
        const float *c = C + 4 * r;
        o[r] = ((c[0] * x + c[1] * y) + c[2] * z) + c[3];
        o[8 + r] = (c[0] * nx + c[1] * ny) + c[2] * nz;
    }
}

// sm_loop_spread's test of a rotation, in double: within 1e-3 of orthonormal, proper
bool near_rigid(const float *C)
{
    double worst = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double g = ((double)C[i] * (double)C[j] + (double)C[4 + i] * (double)C[4 + j]) + (double)C[8 + i] * (double)C[8 + j];
            worst = std::max(worst, std::fabs(g - (i == j ? 1.0 : 0.0)));
        }
    const double det = ((double)C[0] * ((double)C[5] * C[10] - (double)C[6] * C[9]) - (double)C[1] * ((double)C[4] * C[10] - (double)C[6] * C[8])) +
                       (double)C[2] * ((double)C[4] * C[9] - (double)C[5] * C[8]);
    return worst <= 1e-3 && det > 0.0;
}

// where the call's tables lie in Scene::d_tab
struct TabLayout {
    size_t off_actors, off_poses, off_present, bytes;
    TabLayout(size_t n_actors, size_t n_views)
    {
        off_actors = 32;                                                     // behind the tally
        off_poses = off_actors + n_actors * sizeof(SceneActor);              // (16-byte aligned: 32 + 16 n)
        off_present = off_poses + n_actors * n_views * 48;
        bytes = off_present + n_actors * n_views;
    }
};

SceneDev device_view(const sm_ctx *s, const ScenePlan &plan)
{
    const Scene &sc = s->scene;
    const TabLayout t(plan.scene->n_actors, plan.n_views);
    uint8_t *tab = sc.d_tab.get();
    SceneDev d{};
    d.rows = MapsSoA{sc.d_pos_conf, sc.d_norm_rad, sc.d_color, sc.d_time};
    d.box = sc.d_box;
    d.actors = (const SceneActor *)(tab + t.off_actors);
    d.n_actors = plan.scene->n_actors; d.n_views = plan.n_views;
    d.poses = (const float4 *)(tab + t.off_poses);
    d.present = tab + t.off_present;
    d.tally = (LidarTally *)tab;
    return d;
}

// what both scene entry points do before the static path takes over: the scene's own checks, host only.  *use: the plan to hand
// on, null for a scene without actors
int scene_enter(const sm_scene *scene, uint32_t n_views, const char *fn, ScenePlan &plan, ScenePlan **use)
{
    *use = nullptr;
    if (!scene) return SM_OK;
    if (int rc = scene_check(scene, n_views, fn, plan)) return rc;
    if (scene->n_actors) *use = &plan;
    return SM_OK;
}

// a scene call without actors leaves an empty tally
void note_empty(sm_ctx *s, double t_begin)
{
    s->scene.stats = sm_scene_stats_t{};
    s->scene.stats.total_ms = (float)(now_ms() - t_begin);
    s->scene.stats_valid = true;
}

}  // namespace

int sm_impl::scene_check(const sm_scene *scene, uint32_t n_views, const char *fn, ScenePlan &plan)
{
    auto bad = [&](uint32_t j, const char *what) { g_err = std::string(fn) + ": actor " + std::to_string(j) + ": " + what; return SM_E_ARG; };
    plan = ScenePlan{};
    plan.scene = scene;
    plan.n_views = n_views;
    if (scene->n_actors && !scene->actors) { g_err = std::string(fn) + ": null actors"; return SM_E_ARG; }
    if (scene->n_actors > SM_SCENE_MAX_ACTORS) {
        g_err = std::string(fn) + ": " + std::to_string(scene->n_actors) + " actors, at most " + std::to_string(SM_SCENE_MAX_ACTORS);
        return SM_E_CAPACITY;
    }
    for (uint32_t j = 0; j < scene->n_actors; ++j) {
        const sm_scene_actor &a = scene->actors[j];
        if (!a.path) return bad(j, "null path");
        if (!a.poses12) return bad(j, "null poses12");
        for (uint32_t i = 0; i < n_views; ++i) {
            if (a.present && !a.present[i]) continue;                        // (rows of absent views are not read)
            const float *C = a.poses12 + (size_t)i * 12;
            for (int k = 0; k < 12; ++k)
                if (!std::isfinite(C[k])) return bad(j, "non-finite pose");
            if (!near_rigid(C)) return bad(j, "the rotation part of a pose is not orthonormal to 1e-3, or mirrors");
        }
    }
    // every header against its file's length, each distinct file once
    plan.file_of.resize(scene->n_actors);
    for (uint32_t j = 0; j < scene->n_actors; ++j) {
        const char *path = scene->actors[j].path;
        uint32_t f = 0;
        while (f < plan.files.size() && plan.files[f].path != path) ++f;
        if (f == plan.files.size()) {
            sm_mapfile::Header h;
            // (an actor file is resident as it lies in the file: a packed one is refused by name)
            if (!sm_mapfile::open_checked(path, fn, h, g_err)) return sm_mapfile::looks_packed(path) ? SM_E_UNSUPPORTED : SM_E_ARG;
            plan.files.push_back({path, h.count, (uint32_t)plan.resident, (uint32_t)plan.rows});
            plan.resident += h.count;
            plan.rows += ((uint64_t)h.count + MAPS_BLOCK - 1) / MAPS_BLOCK * MAPS_BLOCK;
            if (plan.resident > SM_SCENE_MAX_RECORDS) {
                g_err = std::string(fn) + ": the actor files hold more than " + std::to_string(SM_SCENE_MAX_RECORDS) + " records";
                return SM_E_CAPACITY;
            }
        }
        plan.file_of[j] = f;
        plan.ids += plan.files[f].count;
    }
    plan.cull = env_is_one("SM_SCENE_NO_CULL") ? 0 : 1;
    return SM_OK;
}

int sm_impl::scene_load(sm_ctx *s, ScenePlan &plan, uint64_t static_total, bool draw, const char *fn)
{
    const double t0 = now_ms();
    Scene &sc = s->scene;
    const uint32_t n_actors = plan.scene->n_actors;
    if (static_total + plan.ids > 0x7FFFFFFFull) {
        g_err = std::string(fn) + ": the scene holds " + std::to_string(static_total + plan.ids) + " surfels, ids end at 2^31 - 1";
        return SM_E_CAPACITY;
    }
    plan.id_base = (uint32_t)static_total;
    sc.stats = sm_scene_stats_t{};
    sc.stats.actors = n_actors;
    sc.stats.files = (uint32_t)plan.files.size();
    sc.stats_valid = true;
    if (!draw) return SM_OK;

    // ---- the buffers, grown on demand
    int rc;
    if (plan.resident > sc.rec_cap) {
        sc.rec_cap = 0;
        if ((rc = dalloc(sc.d_rec, (size_t)plan.resident * 3))) return rc;
        sc.rec_cap = plan.resident;
    }
    if (plan.rows > sc.row_cap) {
        sc.row_cap = 0;
        if ((rc = dalloc(sc.d_pos_conf, (size_t)plan.rows)) || (rc = dalloc(sc.d_norm_rad, (size_t)plan.rows)) || (rc = dalloc(sc.d_color, (size_t)plan.rows)) ||
            (rc = dalloc(sc.d_time, (size_t)plan.rows)) || (rc = dalloc(sc.d_box, 2 * (size_t)(plan.rows / MAPS_BLOCK))))
            return rc;
        sc.row_cap = plan.rows;
    }
    const TabLayout t(n_actors, plan.n_views);
    if (t.bytes > sc.tab_bytes) {
        sc.tab_bytes = 0;
        if ((rc = dalloc(sc.d_tab, t.bytes))) return rc;
        sc.tab_bytes = t.bytes;
    }
    if (!sc.ev[1]) { HIPCK(hipEventCreate(sc.ev[0].put())); HIPCK(hipEventCreate(sc.ev[1].put())); }

    // ---- every distinct file once, through the one reader; then the planes and the boxes by the chunks' own intake
    std::vector<float> rec((size_t)plan.resident * 12);
    for (const ScenePlan::File &f : plan.files) {
        sm_mapfile::Header h;
        sm_mapfile::File in = sm_mapfile::open_checked(f.path, fn, h, g_err);
        if (!in) return SM_E_ARG;
        if (h.count != f.count || !sm_mapfile::read_rows(in.get(), rec.data() + (size_t)f.rec0 * 12, f.count)) {
            g_err = sm_mapfile::said(fn, f.path, " read err!!");
            return SM_E_ARG;
        }
    }
    // ---- the tables: the tally zeroed, the actors, a pose row and a presence byte per (actor, view)
    std::vector<uint8_t> tab(t.bytes, 0);
    SceneActor *act = (SceneActor *)(tab.data() + t.off_actors);
    uint32_t id = plan.id_base, wg = 0;
    uint64_t pairs = 0;
    for (uint32_t j = 0; j < n_actors; ++j) {
        const sm_scene_actor &a = plan.scene->actors[j];
        const ScenePlan::File &f = plan.files[plan.file_of[j]];
        const uint32_t blocks = (f.count + MAPS_BLOCK - 1) / MAPS_BLOCK;
        act[j] = SceneActor{f.row0, f.count, id, wg};
        id += f.count;
        wg += blocks;
        float *poses = (float *)(tab.data() + t.off_poses) + (size_t)j * plan.n_views * 12;
        uint8_t *present = tab.data() + t.off_present + (size_t)j * plan.n_views;
        for (uint32_t i = 0; i < plan.n_views; ++i) {
            present[i] = (!a.present || a.present[i]) ? 1 : 0;
            if (!present[i]) continue;
            memcpy(poses + (size_t)i * 12, a.poses12 + (size_t)i * 12, 48);
            pairs += blocks;
        }
    }
    plan.n_wg = wg;
    HIPCK(hipSetDevice(s->cfg.device));
    if (plan.resident) HIPCK(hipMemcpyAsync(sc.d_rec, rec.data(), (size_t)plan.resident * 48, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(sc.d_tab, tab.data(), t.bytes, hipMemcpyHostToDevice, s->stream));
    const MapsSoA rows{sc.d_pos_conf, sc.d_norm_rad, sc.d_color, sc.d_time};
    for (const ScenePlan::File &f : plan.files) {
        if (!f.count) continue;
        const MapsSoA at{rows.pos_conf + f.row0, rows.norm_rad + f.row0, rows.color + f.row0, rows.time + f.row0};
        maps_intake_to(s, sc.d_rec.get() + (size_t)f.rec0 * 3, f.count, at, sc.d_box.get() + 2 * (size_t)(f.row0 / MAPS_BLOCK));
    }
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(s->stream));              // (the vectors go away; load_ms is the whole of it)
    sc.stats.records = plan.resident;
    sc.stats.bytes = (uint64_t)plan.resident * 48 + plan.rows * 40 + plan.rows / MAPS_BLOCK * 32 + t.bytes;
    sc.stats.pairs_tested = plan.cull ? pairs : 0;
    sc.stats.load_ms = (float)(now_ms() - t0);
    return SM_OK;
}

int sm_impl::scene_draw_image(sm_ctx *s, const ScenePlan &plan, const RenderParams *d_rps, uint32_t v0, uint32_t b, uint64_t *d_key, size_t npix,
                              uint8_t *d_bgr, uint8_t *d_sem)
{
    Scene &sc = s->scene;
    const SceneDev d = device_view(s, plan);
    const size_t bp = (size_t)b * npix;
    HIPCK(hipEventRecord(sc.ev[0], s->stream));
    if (plan.n_wg)
        hipLaunchKernelGGL(k_scene_splat_image, dim3(plan.n_wg, b), dim3(256), 0, s->stream, d, d_rps, v0, d_key, npix, plan.cull);
    if (plan.ids)
        hipLaunchKernelGGL(k_scene_resolve_image, dim3((unsigned)((bp + 255) / 256)), dim3(256), 0, s->stream, d, plan.id_base, (const uint64_t *)d_key, bp,
                           d_bgr, d_sem);
    HIPCK(hipEventRecord(sc.ev[1], s->stream));
    HIPCK(hipGetLastError());
    return SM_OK;
}

int sm_impl::scene_draw_lidar(sm_ctx *s, const ScenePlan &plan, const LidarGrid &g, const LidarPose *d_poses, uint32_t v0, uint32_t b, uint64_t *d_key,
                              size_t nbeams, float *d_range, int32_t *d_id, uint8_t *d_rgb, uint8_t *d_sem)
{
    Scene &sc = s->scene;
    const SceneDev d = device_view(s, plan);
    const size_t bp = (size_t)b * nbeams;
    HIPCK(hipEventRecord(sc.ev[0], s->stream));
    if (plan.n_wg)
        hipLaunchKernelGGL(k_scene_splat_lidar, dim3(plan.n_wg, b), dim3(256), 0, s->stream, d, g, d_poses, v0, d_key, nbeams, plan.cull);
    // (always: the static sources have left the empty beams to this launch)
    hipLaunchKernelGGL(k_scene_resolve_lidar, dim3((unsigned)((bp + 255) / 256)), dim3(256), 0, s->stream, d, plan.id_base, (const uint64_t *)d_key, bp,
                       d_range, d_id, d_rgb, d_sem);
    HIPCK(hipEventRecord(sc.ev[1], s->stream));
    HIPCK(hipGetLastError());
    return SM_OK;
}

int sm_impl::scene_fold(sm_ctx *s) { return add_marked(s->scene.ev, &s->scene.stats.actor_ms); }

int sm_impl::scene_end(sm_ctx *s, const ScenePlan &plan)
{
    if (plan.n_views == 0) return SM_OK;
    LidarTally t{};
    HIPCK(hipMemcpy(&t, s->scene.d_tab.get(), sizeof t, hipMemcpyDeviceToHost));
    s->scene.stats.pairs_skipped = t.skipped;
    return SM_OK;
}

extern "C" {

int sm_render_image_scene(sm_ctx *s, const sm_map_source *src, const sm_scene *scene, const float *views16, uint32_t n_views, int w, int h, float fx,
                          float fy, float cx, float cy, const sm_fill_params *fill, uint8_t *bgr_out, uint8_t *sem_out, uint16_t *depth_mm_out)
{
    const char *fn = "sm_render_image_scene";
    const double t_begin = now_ms();
    ScenePlan plan, *use;
    int rc;
    if ((rc = scene_enter(scene, n_views, fn, plan, &use))) return rc;
    if (s && (rc = check_whole_map(s, fn))) return rc;
    if ((rc = check_fill_params(fill, fn))) return rc;
    if ((rc = render_image_maps(s, src, views16, n_views, w, h, fx, fy, cx, cy, nullptr, fill, bgr_out, sem_out, depth_mm_out, fn, use))) return rc;
    if (!use) note_empty(s, t_begin);
    else s->scene.stats.total_ms = (float)(now_ms() - t_begin);
    return SM_OK;
}

int sm_lidar_sweep_scene(sm_ctx *s, const sm_map_source *src, const sm_scene *scene, const sm_lidar_sensor *sn, const float *poses16, uint32_t n_sweeps,
                         float *range, int32_t *id, uint8_t *rgb, uint8_t *sem)
{
    const char *fn = "sm_lidar_sweep_scene";
    const double t_begin = now_ms();
    ScenePlan plan, *use;
    int rc;
    if ((rc = scene_enter(scene, n_sweeps, fn, plan, &use))) return rc;
    if (!src) { g_err = std::string(fn) + ": null source"; return SM_E_ARG; }
    if ((rc = lidar_sweep(s, src, sn, poses16, n_sweeps, range, id, rgb, sem, fn, use))) return rc;
    if (!use) note_empty(s, t_begin);
    else s->scene.stats.total_ms = (float)(now_ms() - t_begin);
    return SM_OK;
}

int sm_scene_place_rows(const float *pose12, const float *rows_in, uint32_t n, float *rows_out)
{
    if (!pose12 || (n && (!rows_in || !rows_out))) { g_err = "sm_scene_place_rows: null argument"; return SM_E_ARG; }
    for (uint32_t i = 0; i < n; ++i) place_row(pose12, rows_in + (size_t)i * 12, rows_out + (size_t)i * 12);
    return SM_OK;
}

int sm_scene_stats(sm_ctx *s, sm_scene_stats_t *out)
{
    if (!s || !out) { g_err = "sm_scene_stats: null argument"; return SM_E_ARG; }
    if (!s->scene.stats_valid) { g_err = "sm_scene_stats: no sm_render_image_scene / sm_lidar_sweep_scene call yet"; return SM_E_ARG; }
    *out = s->scene.stats;
    return SM_OK;
}

}  // extern "C"
