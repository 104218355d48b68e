"""ctypes binding of the C-ABI in include/sm_c_api.h (libsurfelmapping_hip.so).

This is plumbing only: every call goes straight to the HIP library.  There is NO CPU
fallback -- if the shared library is missing or no GPU is visible, calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SM_HIP_LIB") or os.path.join(_PKG, "libsurfelmapping_hip.so")      # (SM_HIP_LIB: another build of the core, for A/B runs)
API_VERSION = 4                # SM_API_VERSION of include/sm_c_api.h

SM_OK, SM_E_ARG, SM_E_CAPACITY, SM_E_UNSUPPORTED, SM_E_HIP, SM_E_NO_DEVICE = 0, -1, -2, -3, -4, -5
TEX_DEPTH_METRIC, TEX_DEPTH_FILTERED, TEX_LAST = 0, 1, 2

# every extern "C" symbol include/sm_c_api.h declares
SYMBOLS = (
    "sm_api_version", "sm_last_error", "sm_default_config", "sm_create", "sm_destroy",
    "sm_process_frame", "sm_process_frame_device", "sm_process_frame_async",
    "sm_inputs_consumed", "sm_host_alloc", "sm_host_alloc_frame", "sm_host_free", "sm_debug_slow_frames", "sm_debug_squeezes", "sm_sync", "sm_clean_points", "sm_clean_points_ex", "sm_clean_points_cb", "sm_reset",
    "sm_get_counts", "sm_download_model_aos", "sm_upload_model_aos", "sm_save_map", "sm_load_map",
    "sm_download_index_map", "sm_download_raw_cloud", "sm_download_depth", "sm_render_image", "sm_render_model",
    "sm_render_model_device", "sm_render_image_maps", "sm_render_model_maps", "sm_render_maps_stats", "sm_set_frame", "sm_set_tick",
    "sm_stage_conflict", "sm_stage_cull", "sm_stage_splat", "sm_stage_associate_fuse",
    "sm_stage_timings", "sm_read_frame_log", "sm_device_alloc", "sm_device_free", "sm_device_upload",
    "sm_export_model_device", "sm_append_model_aos_device", "sm_device_download",
    "sm_shard_stream_configure", "sm_shard_set_collective", "sm_shard_rccl_unique_id", "sm_shard_rccl_init",
    "sm_shard_rccl_finalize", "sm_shard_rccl_nranks", "sm_shard_frame_device", "sm_shard_frame", "sm_shard_compact", "sm_shard_export_dense_device",
    "sm_gpu_process_count", "sm_rig_configure", "sm_rig_consolidate", "sm_rig_consolidate_step",
    "sm_default_track_params", "sm_track_frame", "sm_track_debug",
    "sm_default_track_rgb_params", "sm_track_frame_rgb", "sm_track_rgb_debug",
    "sm_default_retire_params", "sm_retire", "sm_retire_device", "sm_set_auto_retire", "sm_auto_retire_stats",
    "sm_default_recall_params", "sm_recall", "sm_recall_stats", "sm_set_auto_recall", "sm_auto_recall_stats",
    "sm_warp_by_time", "sm_warp_stats", "sm_loop_spread", "sm_track_frame_old", "sm_track_debug_old",
    "sm_default_loop_params", "sm_close_loop",
    "sm_track_frame_window", "sm_track_debug_window", "sm_track_frame_rgb_window", "sm_track_rgb_debug_window", "sm_close_loop_rgb",
    "sm_old_in_view", "sm_default_auto_loop_params", "sm_set_auto_loop", "sm_auto_loop_stats",
    "sm_default_search_params", "sm_score_poses_window", "sm_search_pose", "sm_close_loop_search", "sm_set_auto_loop_search",
    "sm_default_lidar_sensor", "sm_lidar_directions", "sm_lidar_sweep", "sm_lidar_sweep_maps", "sm_lidar_stats",
    "sm_default_fern_params", "sm_fern_table", "sm_set_ferns", "sm_fern_encode", "sm_fern_encode_device", "sm_fern_add", "sm_fern_count",
    "sm_fern_download", "sm_fern_save", "sm_fern_load", "sm_fern_match", "sm_search_pose_at", "sm_close_loop_at",
    "sm_default_auto_place_params", "sm_set_auto_place", "sm_auto_place_stats",
    "sm_default_stereo_params", "sm_set_stereo", "sm_stereo_depth", "sm_stereo_depth_device", "sm_stereo_download",
    "sm_default_fill_params", "sm_fill_image", "sm_fill_image_device", "sm_render_image_ex", "sm_render_image_maps_ex", "sm_fill_stats",
    "sm_default_blend_params", "sm_render_image_blend", "sm_render_image_maps_blend", "sm_blend_stats",
    "sm_default_simplify_params", "sm_simplify", "sm_simplify_maps", "sm_simplify_stats",
    "sm_default_register_params", "sm_register_maps", "sm_register_debug", "sm_register_stats",
    "sm_default_compare_params", "sm_compare_maps", "sm_compare_stats",
    "sm_default_tile_params", "sm_tile_maps", "sm_tile_stats",
    "sm_default_segment_params", "sm_segment_maps", "sm_segment_stats",
    "sm_default_mesh_params", "sm_mesh_maps", "sm_mesh_stats",
    "sm_default_ground_params", "sm_ground_maps", "sm_ground_stats",
    "sm_render_image_scene", "sm_lidar_sweep_scene", "sm_scene_place_rows", "sm_scene_stats",
    "sm_default_rays_params", "sm_cast_rays_maps", "sm_cast_rays_stats",
)

SM_COLL_SUM, SM_COLL_MIN, SM_COLL_GATHER = 0, 1, 2
# int fn(void *user, const void *send, void *recv, size_t count_u64, int op, void *hip_stream)
COLLECTIVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
# long long fn(void *user, uint32_t local_conflicts)
CAP_FN = C.CFUNCTYPE(C.c_longlong, C.c_void_p, C.c_uint32)


class SmConfig(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("near_clip", C.c_float), ("far_clip", C.c_float), ("fuse_thresh", C.c_float),
        ("max_sqrt_vertices", C.c_int32), ("time_delta", C.c_int32),
        ("stereo_border", C.c_float), ("preprocess", C.c_int32), ("conflict_cap", C.c_int32),
        ("device", C.c_int32), ("enable_timing", C.c_int32), ("disable_tile_bounds", C.c_int32),
        ("compact_period", C.c_int32),
    ]


class SmCounts(C.Structure):
    _fields_ = [
        ("count", C.c_uint32), ("offset", C.c_uint32), ("data_count", C.c_uint32),
        ("conflict_count", C.c_uint32), ("unstable_count", C.c_uint32),
        ("fused_count", C.c_uint32), ("visible_count", C.c_uint32), ("tick", C.c_int32),
    ]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SmTimings(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "preprocess", "conflict", "index_map", "data_association", "concatenate", "run",
        "k_prep", "k_conflict", "k_scan_cull", "k_compact", "k_associate", "k_scan_new",
        "k_append")] + [("frames", C.c_uint32), ("event_overhead", C.c_float), ("k_compact_own", C.c_float),
                        ("k_cull_lazy", C.c_float), ("frames_compact", C.c_uint32)] + [(n, C.c_float) for n in (
        "k_surfel_pass", "k_pass_fixup", "k_conflict_own", "k_associate_direct", "k_associate_own", "k_append_own")] + [
        ("frames_one_pass", C.c_uint32), ("frames_direct", C.c_uint32), ("k_assoc_prep", C.c_float), ("k_prep_own", C.c_float),
        ("frames_merged", C.c_uint32), ("frames_assoc_alone", C.c_uint32), ("k_scan_own", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


FRAME_LOG_LEN = 1024
FRAME_LOG_DTYPE = np.dtype([(n, np.uint32) for n in (
    "tick", "n_before", "n_after_cull", "n_kill", "conflict_count", "visible_count",
    "fused_count", "unstable_count", "n_static", "n_conf_skipped", "n_splat_skipped", "n_slots")])


class SmModelView(C.Structure):
    _fields_ = [
        ("mvp", C.c_float * 16), ("mv_inv", C.c_float * 16), ("threshold", C.c_float), ("color_type", C.c_int32),
        ("draw_unstable", C.c_int32), ("draw_points", C.c_int32), ("draw_window", C.c_int32), ("time", C.c_int32),
        ("time_delta", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("clear_rgba", C.c_uint8 * 4),
    ]


class SmMapSource(C.Structure):
    _fields_ = [("paths", C.POINTER(C.c_char_p)), ("n_paths", C.c_uint32), ("include_model", C.c_int32)]


class SmMapsStats(C.Structure):
    _fields_ = [("surfels_read", C.c_uint64), ("chunks", C.c_uint32), ("passes", C.c_uint32), ("pairs_tested", C.c_uint64),
                ("pairs_skipped", C.c_uint64), ("read_ms", C.c_float), ("copy_ms", C.c_float), ("device_ms", C.c_float),
                ("total_ms", C.c_float)]


def map_source(paths, include_model=True) -> SmMapSource:
    """a map set: the files in drawing order, then (include_model) the live model; keeps the path strings alive"""
    enc = [os.fsencode(p) for p in paths]
    arr = (C.c_char_p * max(len(enc), 1))(*enc)
    src = SmMapSource(C.cast(arr, C.POINTER(C.c_char_p)), len(enc), int(bool(include_model)))
    src._keep = (enc, arr)
    return src


class SmLidarSensor(C.Structure):
    _fields_ = [("n_az", C.c_int32), ("n_el", C.c_int32), ("az0_deg", C.c_float), ("az_step_deg", C.c_float),
                ("el_deg", C.POINTER(C.c_float)), ("min_range", C.c_float), ("max_range", C.c_float), ("min_conf", C.c_float)]


class SmLidarStats(C.Structure):
    _fields_ = [("surfels", C.c_uint64), ("tests", C.c_uint64), ("wide", C.c_uint64), ("blocks_skipped", C.c_uint64),
                ("chunks", C.c_uint32), ("passes", C.c_uint32), ("read_ms", C.c_float), ("copy_ms", C.c_float),
                ("device_ms", C.c_float), ("total_ms", C.c_float)]


LIDAR_MAX_BEAMS = 1 << 22


def lidar_sensor(**over) -> SmLidarSensor:
    """sm_default_lidar_sensor with fields replaced: n_az, n_el, az0_deg, az_step_deg, el_deg (a sequence of n_el elevations; giving
    it sets n_el unless that is given too), min_range, max_range, min_conf.  Keeps the elevation array alive."""
    p = SmLidarSensor()
    load().sm_default_lidar_sensor(C.byref(p))
    el = over.pop("el_deg", None)
    if el is None:
        el = np.array([p.el_deg[i] for i in range(p.n_el)], np.float32)
    el = np.ascontiguousarray(el, np.float32).reshape(-1)
    p.n_el = len(el)
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    p.el_deg = el.ctypes.data_as(C.POINTER(C.c_float))
    p._keep = el
    return p


def lidar_directions(sensor) -> np.ndarray:
    """the sensor's beam directions in its own frame (sm_lidar_directions): float32[n_el][n_az][3]"""
    d = np.zeros((max(sensor.n_el, 0), max(sensor.n_az, 0), 3), np.float32)
    rc = load().sm_lidar_directions(C.byref(sensor), _ptr(d))
    if rc:
        raise SurfelMapError("sm_lidar_directions", rc, load().sm_last_error().decode())
    return d


def lidar_points(range, dirs, rgb=None) -> np.ndarray:
    """the returns of a sweep as KITTI velodyne points: float32[N][4] = (z, -x, -y) of t*d in the sensor frame (x forward, y left,
    z up) and the reflectance -- the luminance of rgb by the colour tracker's weights, ((0.299 r + 0.587 g) + 0.114 b) / 255 in
    float32, or 0 without rgb.  Beams without a return (range 0) are left out; the order is the grid's, row-major."""
    f32 = np.float32
    t = np.ascontiguousarray(range, f32).reshape(-1)
    d = np.ascontiguousarray(dirs, f32).reshape(-1, 3)
    got = t > 0
    p = t[got, None] * d[got]
    out = np.zeros((int(got.sum()), 4), f32)
    out[:, 0], out[:, 1], out[:, 2] = p[:, 2], -p[:, 0], -p[:, 1]
    if rgb is not None:
        c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)[got].astype(f32)
        out[:, 3] = ((f32(0.299) * c[:, 0] + f32(0.587) * c[:, 1]) + f32(0.114) * c[:, 2]) / f32(255.0)
    return out


class SmRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("t_min", C.c_float), ("dir", C.c_float * 3), ("t_max", C.c_float)]


class SmRaysParams(C.Structure):
    _fields_ = [("cell_mm", C.c_int32), ("origin", C.c_float * 3), ("min_conf", C.c_float), ("reserved", C.c_int32 * 3)]


class SmRaysStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("bad_rays", C.c_uint64), ("records", C.c_uint64), ("wide", C.c_uint64), ("pairs", C.c_uint64),
                ("cells", C.c_uint64), ("probes", C.c_uint64), ("tests", C.c_uint64), ("no_slot", C.c_uint64), ("gave_up", C.c_uint64),
                ("chunks", C.c_uint32), ("files_skipped", C.c_uint32),
                ("read_ms", C.c_float), ("copy_ms", C.c_float), ("index_ms", C.c_float), ("cast_ms", C.c_float), ("device_ms", C.c_float),
                ("total_ms", C.c_float)]


RAYS_MAX = 1 << 24


def rays_params(**over) -> SmRaysParams:
    """sm_default_rays_params with fields replaced: cell_mm, origin (three floats), min_conf"""
    p = SmRaysParams()
    load().sm_default_rays_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, (C.c_float * 3)(*[float(x) for x in v]) if k == "origin" else v)
    return p


def lidar_rays(sensor, poses16) -> np.ndarray:
    """The beams of a sweep as rays for SurfelMap.cast_rays: float32[n_el * n_az][8] = (origin, t_min, dir, t_max), row-major over
    the sensor's grid.  poses16: one sensor->world pose (float32[16] column-major or 4x4), or n_az of them, one per column -- the
    sweep of a vehicle that moves while the sensor turns.  The origin is the pose's translation, the direction R * d of
    lidar_directions' table, computed in double ((R0 dx + R1 dy) + R2 dz, terms with a zero coefficient left out) and rounded
    once; t_min / t_max are the sensor's range limits.  Needs no context."""
    d = lidar_directions(sensor).astype(np.float64)                       # [n_el][n_az][3]
    n_el, n_az = d.shape[0], d.shape[1]
    P = np.asarray(poses16, np.float32)
    if P.ndim >= 2 and P.shape[-2:] == (4, 4):
        P = np.swapaxes(P, -1, -2)                                        # (numpy row/col indexing -> column-major)
    P = np.ascontiguousarray(P).reshape(-1, 16)
    if P.shape[0] not in (1, n_az):
        raise ValueError("poses16: one pose, or one per column (n_az)")
    P = np.broadcast_to(P, (n_az, 16))
    R = P.astype(np.float64).reshape(n_az, 4, 4)[:, :3, :3]               # R[j][c][r]: column c, row r of pose j
    # a term whose coefficient is 0 is left out (-0.0 is the sum's neutral element), so an identity rotation returns d bit for bit
    term = [np.where(R[None, :, c, :] != 0.0, R[None, :, c, :] * d[:, :, None, c], -0.0) for c in range(3)]
    dirs = (term[0] + term[1]) + term[2]
    rays = np.zeros((n_el, n_az, 8), np.float32)
    rays[:, :, 0:3] = P[None, :, 12:15]
    rays[:, :, 3] = np.float32(sensor.min_range)
    rays[:, :, 4:7] = dirs.astype(np.float32)
    rays[:, :, 7] = np.float32(sensor.max_range)
    return rays.reshape(n_el * n_az, 8)


class SmSceneActor(C.Structure):
    _fields_ = [("path", C.c_char_p), ("poses12", C.POINTER(C.c_float)), ("present", C.POINTER(C.c_uint8))]


class SmScene(C.Structure):
    _fields_ = [("actors", C.POINTER(SmSceneActor)), ("n_actors", C.c_uint32)]


class SmSceneStats(C.Structure):
    _fields_ = [("actors", C.c_uint32), ("files", C.c_uint32), ("records", C.c_uint64), ("bytes", C.c_uint64),
                ("pairs_tested", C.c_uint64), ("pairs_skipped", C.c_uint64), ("load_ms", C.c_float), ("actor_ms", C.c_float),
                ("total_ms", C.c_float)]


SCENE_MAX_ACTORS, SCENE_MAX_RECORDS = 4096, 1 << 22


def scene_poses12(poses) -> np.ndarray:
    """actor->world poses as the scene calls take them, float32[V][12] ROW-major 3x4 [R|t]: from float32[V][12] as they are, or
    from [V][4][4] matrices (their top three rows)"""
    p = np.asarray(poses, np.float32)
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        p = p[:, :3, :]
    return np.ascontiguousarray(p.reshape(-1, 12))


def scene(actors, n_views=None) -> SmScene:
    """a scene's actors: a list of (path, poses[, present]) -- a map file in the actor's own frame, its poses per view
    (scene_poses12 forms), optionally uint8[V], 0 = not in that view.  n_views: what every actor's arrays must hold (None: not
    checked).  Keeps the strings and arrays alive."""
    keep, arr = [], (SmSceneActor * max(len(actors), 1))()
    for j, a in enumerate(actors):
        path, poses = os.fsencode(a[0]), scene_poses12(a[1])
        present = None if len(a) < 3 or a[2] is None else np.ascontiguousarray(a[2], np.uint8).reshape(-1)
        if n_views is not None and (len(poses) != n_views or (present is not None and len(present) != n_views)):
            raise ValueError(f"actor {j}: {len(poses)} poses for {n_views} views")
        arr[j].path = path
        arr[j].poses12 = poses.ctypes.data_as(C.POINTER(C.c_float))
        arr[j].present = None if present is None else present.ctypes.data_as(C.POINTER(C.c_uint8))
        keep.append((path, poses, present))
    sc = SmScene(C.cast(arr, C.POINTER(SmSceneActor)), len(actors))
    sc._keep = (keep, arr)
    return sc


def scene_place_rows(pose, rows) -> np.ndarray:
    """sm_scene_place_rows: float32[N][12] records under one actor->world pose (float32[12] row-major 3x4, or 4x4) by
    sm_warp_by_time's row rule, on the host"""
    pose = scene_poses12(np.asarray(pose, np.float32).reshape((1, 4, 4) if np.size(pose) == 16 else (1, 12)))
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 12)
    out = np.empty_like(rows)
    rc = load().sm_scene_place_rows(_ptr(pose), _ptr(rows), len(rows), _ptr(out))
    if rc:
        raise SurfelMapError("sm_scene_place_rows", rc, load().sm_last_error().decode())
    return out


SM_TRACK_OK, SM_TRACK_LOST, SM_TRACK_DEGENERATE, SM_TRACK_NO_MODEL = 0, 1, 2, 3
TRACK_STATUS = {SM_TRACK_OK: "OK", SM_TRACK_LOST: "LOST", SM_TRACK_DEGENERATE: "DEGENERATE", SM_TRACK_NO_MODEL: "NO_MODEL"}


class SmTrackParams(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("dist_thresh", C.c_float), ("angle_thresh", C.c_float), ("min_inliers", C.c_int32),
                ("pixel_stride", C.c_int32)]


class SmTrackInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("inliers", C.c_uint32), ("rmse", C.c_float),
                ("guess", C.c_float * 16)]


def track_params(**over) -> SmTrackParams:
    """sm_default_track_params with fields overridden (max_iters, dist_thresh, angle_thresh, min_inliers, pixel_stride)"""
    p = SmTrackParams()
    load().sm_default_track_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class SmTrackRgbParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("iters", C.c_int32 * 6), ("rgb_weight", C.c_float), ("rgb_max_residual", C.c_float)]


class SmTrackRgbInfo(C.Structure):
    _fields_ = [("rgb_inliers", C.c_uint32), ("rgb_rmse", C.c_float), ("pivot_ratio", C.c_double),
                ("level_iterations", C.c_int32 * 6)]


def track_rgb_params(**over) -> SmTrackRgbParams:
    """sm_default_track_rgb_params with fields overridden (levels, iters: a sequence whose index is the level, the levels it
    does not name keep their default; rgb_weight, rgb_max_residual)"""
    p = SmTrackRgbParams()
    load().sm_default_track_rgb_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if k == "iters":
            for l, n in enumerate(v):
                p.iters[l] = int(n)
        else:
            setattr(p, k, v)
    return p


class SmRetireParams(C.Structure):
    _fields_ = [("min_age", C.c_int32), ("min_distance", C.c_float)]


def retire_params(cfg, **over) -> SmRetireParams:
    """sm_default_retire_params of a config (min_age = time_delta, min_distance = 1.5 * far_clip) with fields overridden"""
    p = SmRetireParams()
    load().sm_default_retire_params(C.byref(cfg), C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


SM_RECALL_MOVE, SM_RECALL_COPY, SM_RECALL_COUNT = 0, 1, 2
RECALL_MODE = {"move": SM_RECALL_MOVE, "copy": SM_RECALL_COPY, "count": SM_RECALL_COUNT}


class SmRecallParams(C.Structure):
    _fields_ = [("radius", C.c_float)]


class SmRecallStats(C.Structure):
    _fields_ = [("files_listed", C.c_uint32), ("files_skipped", C.c_uint32), ("files_read", C.c_uint32), ("files_rewritten", C.c_uint32),
                ("records_read", C.c_uint64), ("recalled", C.c_uint64), ("chunks", C.c_uint32), ("read_ms", C.c_float),
                ("copy_ms", C.c_float), ("device_ms", C.c_float), ("write_ms", C.c_float), ("total_ms", C.c_float)]


def recall_params(cfg, **over) -> SmRecallParams:
    """sm_default_recall_params of a config (radius = 1.5 * far_clip) with fields overridden"""
    p = SmRecallParams()
    load().sm_default_recall_params(C.byref(cfg), C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class SmWarpStats(C.Structure):
    _fields_ = [("files_listed", C.c_uint32), ("files_skipped", C.c_uint32), ("files_read", C.c_uint32), ("files_rewritten", C.c_uint32),
                ("records_read", C.c_uint64), ("records_moved", C.c_uint64), ("model_moved", C.c_uint32), ("chunks", C.c_uint32),
                ("read_ms", C.c_float), ("copy_ms", C.c_float), ("device_ms", C.c_float), ("write_ms", C.c_float), ("total_ms", C.c_float)]


SM_LOOP_CLOSED, SM_LOOP_NONE, SM_LOOP_NO_OLD_MAP, SM_LOOP_TRACK_FAILED, SM_LOOP_REJECTED = 0, 1, 2, 3, 4
LOOP_STATUS = {SM_LOOP_CLOSED: "CLOSED", SM_LOOP_NONE: "NONE", SM_LOOP_NO_OLD_MAP: "NO_OLD_MAP", SM_LOOP_TRACK_FAILED: "TRACK_FAILED",
               SM_LOOP_REJECTED: "REJECTED"}


class SmLoopParams(C.Structure):
    _fields_ = [("min_age", C.c_int32), ("min_trans", C.c_float), ("min_rot_deg", C.c_float), ("max_trans", C.c_float),
                ("max_rot_deg", C.c_float)]


class SmLoopInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("track", SmTrackInfo), ("D", C.c_float * 16), ("t_a", C.c_int32), ("t_b", C.c_int32)]


def loop_params(cfg, **over) -> SmLoopParams:
    """sm_default_loop_params of a config (min_age = time_delta; 0.02 m, 0.05 deg; 2 m, 10 deg) with fields overridden"""
    p = SmLoopParams()
    load().sm_default_loop_params(C.byref(cfg), C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class SmAutoLoopParams(C.Structure):
    _fields_ = [("every", C.c_int32), ("rest", C.c_int32), ("min_old", C.c_uint32), ("loop", SmLoopParams)]


class SmAutoLoopStats(C.Structure):
    _fields_ = [("checked", C.c_uint32), ("attempts", C.c_uint32), ("closed", C.c_uint32), ("none", C.c_uint32),
                ("rejected", C.c_uint32), ("failed", C.c_uint32), ("no_old_map", C.c_uint32), ("last_census", C.c_uint32),
                ("last", SmLoopInfo)]


def auto_loop_params(cfg, **over) -> SmAutoLoopParams:
    """sm_default_auto_loop_params of a config (every 1, rest 10, min_old 1000, loop = loop_params(cfg)) with fields overridden;
    the fields of sm_loop_params are given by their own names (min_age, max_trans, ...)"""
    p = SmAutoLoopParams()
    load().sm_default_auto_loop_params(C.byref(cfg), C.byref(p))
    for k, v in over.items():
        if k != "loop" and hasattr(p, k):
            setattr(p, k, v)
        elif hasattr(p.loop, k):
            setattr(p.loop, k, v)
        else:
            raise KeyError(k)
    return p


class SmSearchParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("trans_half", C.c_float * 3), ("trans_step", C.c_float * 3), ("rot_half_deg", C.c_float * 3),
                ("rot_step_deg", C.c_float * 3), ("refine", C.c_int32), ("stride0", C.c_int32), ("top_k", C.c_int32),
                ("colour_thresh", C.c_float)]


class SmSearchInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("levels_run", C.c_int32), ("candidates", C.c_uint32 * 4), ("best_score", C.c_uint32 * 4),
                ("winner_rank", C.c_int32), ("track", SmTrackInfo), ("start", C.c_float * 16), ("anchor_time", C.c_float),
                ("score_ms", C.c_float), ("total_ms", C.c_float)]


SEARCH_MAX_CANDIDATES = 1 << 20


class SmFernParams(C.Structure):
    _fields_ = [("n_ferns", C.c_int32), ("cell", C.c_int32), ("seed", C.c_uint64), ("depth_lo_mm", C.c_int32), ("depth_hi_mm", C.c_int32)]


class SmFern(C.Structure):
    _fields_ = [("x", C.c_uint16), ("y", C.c_uint16), ("tr", C.c_uint16), ("tg", C.c_uint16), ("tb", C.c_uint16), ("td", C.c_uint16)]


FERN_MAX_KEYFRAMES = 1 << 20
FERN_DTYPE = np.dtype([(n, np.uint16) for n, _ in SmFern._fields_])


def fern_params(cfg, **over) -> SmFernParams:
    """sm_default_fern_params (512 ferns, cell 8, seed 1, the config's near and far clip in millimetres) with fields overridden"""
    p = SmFernParams()
    load().sm_default_fern_params(C.byref(cfg), C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def fern_table(params, width, height) -> np.ndarray:
    """sm_fern_table: the ferns of `params` for an image size, a structured array (x, y, tr, tg, tb, td; uint16).  Host only."""
    L = load()
    out = np.zeros(max(int(params.n_ferns), 0), FERN_DTYPE)
    rc = L.sm_fern_table(C.byref(params), int(width), int(height), _ptr(out))
    if rc != SM_OK:
        raise SurfelMapError("sm_fern_table", rc, L.sm_last_error().decode())
    return out


class SmStereoParams(C.Structure):
    _fields_ = [("max_disp", C.c_int32), ("paths", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("uniqueness", C.c_int32),
                ("lr_max_diff", C.c_int32), ("baseline", C.c_float)]


def stereo_params(cfg, **over) -> SmStereoParams:
    """sm_default_stereo_params (D 128, 8 paths, p1 7, p2 86, uniqueness 5 %, lr_max_diff 1, baseline 0.54 m) with fields overridden"""
    p = SmStereoParams()
    load().sm_default_stereo_params(C.byref(cfg), C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


class SmFillParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("depth_tol_256", C.c_int32), ("through_count", C.c_int32), ("prefer_far", C.c_int32),
                ("min_cover_256", C.c_int32)]


class SmFillStats(C.Structure):
    _fields_ = [("valid", C.c_uint64), ("seen_through", C.c_uint64), ("filled", C.c_uint64), ("left_empty", C.c_uint64),
                ("launches", C.c_uint32), ("device_ms", C.c_float)]


def fill_params(**over) -> SmFillParams:
    """sm_default_fill_params (levels 3, depth_tol_256 13, through_count 6, prefer_far 1, min_cover_256 64) with fields overridden"""
    p = SmFillParams()
    load().sm_default_fill_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _fill_arg(fill):
    """what the entry points' `fill` accepts: None (none), True (the defaults), a dict of overrides, or fill_params(...)"""
    if fill is None or fill is False:
        return None
    if fill is True:
        return fill_params()
    return fill if isinstance(fill, SmFillParams) else fill_params(**fill)


class SmBlendParams(C.Structure):
    _fields_ = [("depth_tol_256", C.c_int32), ("falloff", C.c_int32)]


class SmBlendStats(C.Structure):
    _fields_ = [("drawn", C.c_uint64), ("contributions", C.c_uint64), ("changed", C.c_uint64), ("launches", C.c_uint32),
                ("device_ms", C.c_float)]


def blend_params(**over) -> SmBlendParams:
    """sm_default_blend_params (depth_tol_256 13, falloff 2 = quadratic) with fields overridden"""
    p = SmBlendParams()
    load().sm_default_blend_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _blend_arg(blend):
    """what the entry points' `blend` accepts: None (none), True (the defaults), a dict of overrides, or blend_params(...)"""
    if blend is None or blend is False:
        return None
    if blend is True:
        return blend_params()
    return blend if isinstance(blend, SmBlendParams) else blend_params(**blend)


class SmSimplifyParams(C.Structure):
    _fields_ = [("voxel_mm", C.c_int32), ("split_normals", C.c_int32), ("origin", C.c_float * 3), ("max_cells", C.c_uint32)]


class SmSimplifyStats(C.Structure):
    _fields_ = [("records_in", C.c_uint64), ("records_out", C.c_uint64), ("cells_merged", C.c_uint64), ("loose", C.c_uint64),
                ("largest_cell", C.c_uint32), ("chunks", C.c_uint32), ("launches", C.c_uint32), ("device_ms", C.c_float),
                ("read_ms", C.c_float), ("total_ms", C.c_float)]


def default_simplify_params() -> SmSimplifyParams:
    """sm_default_simplify_params: voxel_mm 50, split_normals 1, origin (0, 0, 0), max_cells 1 << 26"""
    p = SmSimplifyParams()
    load().sm_default_simplify_params(C.byref(p))
    return p


def simplify_params(**over) -> SmSimplifyParams:
    """default_simplify_params() with fields overridden; origin takes a sequence of three"""
    p = default_simplify_params()
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if k == "origin":
            p.origin[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


class SmTileParams(C.Structure):
    _fields_ = [("cell_mm", C.c_int32), ("tile_shift", C.c_int32), ("origin", C.c_float * 3), ("max_file_records", C.c_uint32),
                ("max_tiles", C.c_uint32)]


class SmTileStats(C.Structure):
    _fields_ = [("records_in", C.c_uint64), ("placed", C.c_uint64), ("loose", C.c_uint64), ("tiles", C.c_uint32), ("largest_tile", C.c_uint32),
                ("files_written", C.c_uint32), ("readings", C.c_uint32), ("chunks", C.c_uint32), ("launches", C.c_uint32),
                ("sort_passes", C.c_uint32), ("device_ms", C.c_float), ("sort_ms", C.c_float), ("read_ms", C.c_float), ("write_ms", C.c_float),
                ("total_ms", C.c_float)]


def default_tile_params() -> SmTileParams:
    """sm_default_tile_params: cell_mm 200, tile_shift 7, origin (0, 0, 0), max_file_records 1 << 20, max_tiles 1 << 20"""
    p = SmTileParams()
    load().sm_default_tile_params(C.byref(p))
    return p


def tile_params(**over) -> SmTileParams:
    """default_tile_params() with fields overridden; origin takes a sequence of three"""
    p = default_tile_params()
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if k == "origin":
            p.origin[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


SM_SEGMENT_LOOSE, SM_SEGMENT_SMALL, SM_SEGMENT_SKIPPED = 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
SEGMENT_KINDS = ("NUMBERED", "SMALL", "SKIPPED", "LOOSE")                # the bits of write_mask, the entries of info.counts


class SmSegmentParams(C.Structure):
    _fields_ = [("voxel_mm", C.c_int32), ("connectivity", C.c_int32), ("by_class", C.c_int32), ("class_mask", C.c_uint32 * 8),
                ("min_records", C.c_uint32), ("write_mask", C.c_uint32), ("max_cells", C.c_uint32), ("origin", C.c_float * 3)]


class SmSegmentComponent(C.Structure):
    _fields_ = [("first", C.c_uint32), ("records", C.c_uint32), ("cells", C.c_uint32), ("cls", C.c_int32), ("cell_lo", C.c_int32 * 3),
                ("cell_hi", C.c_int32 * 3), ("sum_cell", C.c_uint64 * 3)]


class SmSegmentInfo(C.Structure):
    _fields_ = [("records", C.c_uint64), ("counts", C.c_uint64 * 4), ("written", C.c_uint64), ("cells", C.c_uint32), ("components", C.c_uint32),
                ("small_components", C.c_uint32), ("largest", C.c_uint32)]


class SmSegmentStats(C.Structure):
    _fields_ = [("chunks", C.c_uint32), ("launches", C.c_uint32), ("readings", C.c_uint32), ("read_ms", C.c_float), ("table_ms", C.c_float),
                ("link_ms", C.c_float), ("label_ms", C.c_float), ("write_ms", C.c_float), ("total_ms", C.c_float)]


# a row of the component table as a numpy record: sm_segment_component, 64 bytes
SEGMENT_COMPONENT = np.dtype([("first", "<u4"), ("records", "<u4"), ("cells", "<u4"), ("cls", "<i4"), ("cell_lo", "<i4", 3), ("cell_hi", "<i4", 3),
                              ("sum_cell", "<u8", 3)])
assert SEGMENT_COMPONENT.itemsize == C.sizeof(SmSegmentComponent) == 64


def default_segment_params() -> SmSegmentParams:
    """sm_default_segment_params: voxel_mm 200, connectivity 26, by_class 1, every class, min_records 1, write_mask 1 (the records of
    numbered components), max_cells 1 << 24, origin (0, 0, 0)"""
    p = SmSegmentParams()
    load().sm_default_segment_params(C.byref(p))
    return p


def segment_params(**over) -> SmSegmentParams:
    """default_segment_params() with fields overridden; origin takes a sequence of three, class_mask eight words or an iterable of
    the classes that take part (`classes=` does the latter too)"""
    p = default_segment_params()
    for k, v in over.items():
        if k == "classes":
            p.class_mask[:] = segment_class_mask(v)
        elif not hasattr(p, k):
            raise KeyError(k)
        elif k == "origin":
            p.origin[:] = [float(x) for x in v]
        elif k == "class_mask":
            p.class_mask[:] = [int(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def segment_class_mask(classes) -> list:
    """the eight words of class_mask with the bits of `classes` (0..255) set"""
    words = [0] * 8
    for c in classes:
        if not 0 <= int(c) <= 255:
            raise ValueError(c)
        words[int(c) >> 5] |= 1 << (int(c) & 31)
    return words


def segment_boxes(components, voxel_mm=200, origin=(0.0, 0.0, 0.0)):
    """(lo, hi, centroid), float64[n, 3] each, in metres, of the rows of a component table: the box of a component's cells -- from
    the low face of cell_lo to the high face of cell_hi -- and the mean over its records of their cells' centres"""
    c = np.asarray(components, SEGMENT_COMPONENT).reshape(-1)
    edge = ((int(voxel_mm) * 65536 + 500) // 1000) / 65536.0
    o = np.asarray([np.float32(v) for v in origin], np.float64)
    lo = o + c["cell_lo"].astype(np.float64) * edge
    hi = o + (c["cell_hi"].astype(np.float64) + 1.0) * edge
    mean = c["sum_cell"].astype(np.float64) / np.maximum(c["records"], 1).astype(np.float64)[:, None] - 65536.0 + 0.5
    return lo, hi, o + mean * edge


MESH_KINDS = ("USED", "SKIPPED", "LOOSE", "OUTSIDE")                     # the entries of a mesh's info.counts


class SmMeshParams(C.Structure):
    _fields_ = [("voxel_mm", C.c_int32), ("reach", C.c_int32), ("min_records", C.c_uint32), ("class_mask", C.c_uint32 * 8),
                ("max_cells", C.c_uint32), ("origin", C.c_float * 3)]


class SmMeshVertex(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("normal", C.c_float * 3), ("colour", C.c_uint32)]


class SmMeshInfo(C.Structure):
    _fields_ = [("records", C.c_uint64), ("counts", C.c_uint64 * 4), ("cells", C.c_uint32), ("lattice_points", C.c_uint32), ("cubes", C.c_uint32),
                ("vertices", C.c_uint32), ("faces", C.c_uint32), ("reserved", C.c_uint32)]


class SmMeshStats(C.Structure):
    _fields_ = [("chunks", C.c_uint32), ("launches", C.c_uint32), ("read_ms", C.c_float), ("table_ms", C.c_float), ("field_ms", C.c_float),
                ("sort_ms", C.c_float), ("emit_ms", C.c_float), ("write_ms", C.c_float), ("total_ms", C.c_float)]


# a vertex of a mesh as a numpy record: sm_mesh_vertex, 28 bytes; colour is laid out as a record's colour word
MESH_VERTEX = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("colour", "<u4")])
assert MESH_VERTEX.itemsize == C.sizeof(SmMeshVertex) == 28


def default_mesh_params() -> SmMeshParams:
    """sm_default_mesh_params: voxel_mm 100, reach 2, min_records 1, every class, max_cells 1 << 24, origin (0, 0, 0)"""
    p = SmMeshParams()
    load().sm_default_mesh_params(C.byref(p))
    return p


def mesh_params(**over) -> SmMeshParams:
    """default_mesh_params() with fields overridden; origin takes a sequence of three, class_mask eight words or an iterable of the
    classes that take part (`classes=` does the latter too)"""
    p = default_mesh_params()
    for k, v in over.items():
        if k == "classes":
            p.class_mask[:] = segment_class_mask(v)
        elif not hasattr(p, k):
            raise KeyError(k)
        elif k == "origin":
            p.origin[:] = [float(x) for x in v]
        elif k == "class_mask":
            p.class_mask[:] = [int(x) for x in v]
        else:
            setattr(p, k, v)
    return p


GROUND_KINDS = ("GROUND", "OBSTACLE", "IGNORED", "UNREFERENCED", "OUTSIDE", "LOOSE")   # the entries of a ground map's info.counts
GROUND_STATES = ("UNKNOWN", "FREE", "OBSTACLE", "STEP")                  # the values of its `state` plane, the entries of info.cells
GROUND_NONE = -(1 << 31)                                                 # SM_GROUND_NONE: `ground` of a cell without ground
GROUND_PLANES = ("ground", "top", "state", "cls", "bgr", "clear2")


class SmGroundParams(C.Structure):
    _fields_ = [("cell_mm", C.c_int32), ("up", C.c_int32), ("origin", C.c_float * 3), ("nu", C.c_int32), ("nv", C.c_int32), ("min_up", C.c_int32),
                ("ground_mask", C.c_uint32 * 8), ("band_mm", C.c_int32), ("clear_lo_mm", C.c_int32), ("clear_hi_mm", C.c_int32),
                ("min_obstacle", C.c_uint32), ("fill_cells", C.c_int32), ("step_mm", C.c_int32), ("reach_cells", C.c_int32),
                ("unknown_blocks", C.c_int32), ("normal_sign", C.c_int32)]


class SmGroundInfo(C.Structure):
    _fields_ = [("records", C.c_uint64), ("counts", C.c_uint64 * 6), ("cells", C.c_uint32 * 4)]


class SmGroundStats(C.Structure):
    _fields_ = [("chunks", C.c_uint32), ("launches", C.c_uint32), ("files_skipped", C.c_uint32), ("read_ms", C.c_float), ("ground_ms", C.c_float),
                ("fill_ms", C.c_float), ("accumulate_ms", C.c_float), ("state_ms", C.c_float), ("clear_ms", C.c_float), ("copy_ms", C.c_float),
                ("total_ms", C.c_float)]


def default_ground_params() -> SmGroundParams:
    """sm_default_ground_params: cell_mm 100, up 3 (-y), origin (0, 0, 0), 256 x 256 cells, min_up 11585 (45 degrees), every class,
    band_mm 200, the body band 150..2000 mm, min_obstacle 2, fill_cells 3, step_mm 150, reach_cells 32, unknown_blocks 0, normal_sign -1
    (normals that point into the surface, as the fusion stores them)"""
    p = SmGroundParams()
    load().sm_default_ground_params(C.byref(p))
    return p


def ground_params(**over) -> SmGroundParams:
    """default_ground_params() with fields overridden; origin takes a sequence of three, ground_mask eight words or an iterable of
    the classes that may be ground (`classes=` does the latter too)"""
    p = default_ground_params()
    for k, v in over.items():
        if k == "classes":
            p.ground_mask[:] = segment_class_mask(v)
        elif not hasattr(p, k):
            raise KeyError(k)
        elif k == "origin":
            p.origin[:] = [float(x) for x in v]
        elif k == "ground_mask":
            p.ground_mask[:] = [int(x) for x in v]
        else:
            setattr(p, k, v)
    return p


_PLY_PROPERTIES = ["property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz",
                   "property uchar red", "property uchar green", "property uchar blue", "property uchar class"]


def read_ply(path):
    """(vertices: MESH_VERTEX[n], faces: uint32[m, 3]) of a file sm_mesh_maps wrote -- that layout alone: binary little-endian, per
    vertex x y z nx ny nz as float and red green blue class as uchar, per face `list uchar int vertex_indices` of three.  The colour
    word is put together again: blue, green, red in bytes 0..2, the class in byte 3."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: no PLY header")
    lines = data[:end].decode("ascii").split("\n")
    body = data[end + len(b"end_header\n"):]
    if lines[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    lines = [l for l in lines[2:] if l and not l.startswith("comment")]
    if (len(lines) != 13 or not lines[0].startswith("element vertex ") or lines[1:11] != _PLY_PROPERTIES or not lines[11].startswith("element face ")
            or lines[12] != "property list uchar int vertex_indices"):
        raise ValueError(f"{path}: not the layout sm_mesh_maps writes")
    nv, nf = int(lines[0].split()[2]), int(lines[11].split()[2])
    if len(body) != nv * 28 + nf * 13:
        raise ValueError(f"{path}: {len(body)} bytes after the header, {nv} vertices and {nf} faces need {nv * 28 + nf * 13}")
    raw = np.frombuffer(body, np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("rgbc", "u1", 4)]), nv)
    vertices = np.zeros(nv, MESH_VERTEX)
    vertices["pos"], vertices["normal"] = raw["pos"], raw["normal"]
    c = raw["rgbc"].astype(np.uint32)
    vertices["colour"] = c[:, 3] << 24 | c[:, 0] << 16 | c[:, 1] << 8 | c[:, 2]
    rows = np.frombuffer(body, np.dtype([("n", "u1"), ("v", "<i4", 3)]), nf, nv * 28)
    if nf and (rows["n"] != 3).any():
        raise ValueError(f"{path}: a face that is no triangle")
    return vertices, rows["v"].view(np.uint32).copy().reshape(-1, 3)


SM_REGISTER_OK, SM_REGISTER_LOST, SM_REGISTER_DEGENERATE, SM_REGISTER_NO_TARGET, SM_REGISTER_NO_SOURCE = 0, 1, 2, 3, 4
REGISTER_STATUS = {SM_REGISTER_OK: "OK", SM_REGISTER_LOST: "LOST", SM_REGISTER_DEGENERATE: "DEGENERATE",
                   SM_REGISTER_NO_TARGET: "NO_TARGET", SM_REGISTER_NO_SOURCE: "NO_SOURCE"}
REGISTER_MAX_LEVELS = 4


class SmRegisterParams(C.Structure):
    _fields_ = [("voxel_mm", C.c_int32), ("levels", C.c_int32), ("max_iters", C.c_int32), ("min_inliers", C.c_int32),
                ("angle_thresh", C.c_float), ("reach_cells", C.c_float), ("stride", C.c_uint32), ("max_samples", C.c_uint32),
                ("max_cells", C.c_uint32), ("origin", C.c_float * 3), ("pivot", C.c_float * 3)]


class SmRegisterInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32 * REGISTER_MAX_LEVELS), ("inliers", C.c_uint32), ("rmse", C.c_float),
                ("pivot_ratio", C.c_float), ("samples", C.c_uint32), ("stride", C.c_uint32), ("cells", C.c_uint32 * REGISTER_MAX_LEVELS)]


class SmRegisterStats(C.Structure):
    _fields_ = [("source_records", C.c_uint64), ("target_records", C.c_uint64), ("chunks", C.c_uint32), ("launches", C.c_uint32),
                ("read_ms", C.c_float), ("table_ms", C.c_float), ("iterate_ms", C.c_float), ("total_ms", C.c_float)]


def default_register_params() -> SmRegisterParams:
    """sm_default_register_params: voxel_mm 200, levels 3, max_iters 20, min_inliers 1000, angle_thresh 30, reach_cells 1, stride 0
    (from max_samples = 1 << 22), max_cells 1 << 24, origin and pivot (0, 0, 0)"""
    p = SmRegisterParams()
    load().sm_default_register_params(C.byref(p))
    return p


def register_params(**over) -> SmRegisterParams:
    """default_register_params() with fields overridden; origin and pivot take a sequence of three"""
    p = default_register_params()
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if k in ("origin", "pivot"):
            getattr(p, k)[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


SM_COMPARE_SUPPORTED, SM_COMPARE_CHANGED, SM_COMPARE_OUTSIDE, SM_COMPARE_LOOSE = 0, 1, 2, 3
COMPARE_LABEL = {SM_COMPARE_SUPPORTED: "SUPPORTED", SM_COMPARE_CHANGED: "CHANGED", SM_COMPARE_OUTSIDE: "OUTSIDE", SM_COMPARE_LOOSE: "LOOSE"}


class SmCompareParams(C.Structure):
    _fields_ = [("voxel_mm", C.c_int32), ("cover_shift", C.c_int32), ("reach_cells", C.c_float), ("plane_mm", C.c_int32),
                ("angle_thresh", C.c_float), ("match_class", C.c_int32), ("write_mask", C.c_uint32), ("max_cells", C.c_uint32),
                ("origin", C.c_float * 3)]


class SmCompareInfo(C.Structure):
    _fields_ = [("counts", C.c_uint64 * 4), ("query_records", C.c_uint64), ("reference_records", C.c_uint64),
                ("cells_fine", C.c_uint32), ("cells_cover", C.c_uint32), ("written", C.c_uint64)]


class SmCompareStats(C.Structure):
    _fields_ = [("chunks", C.c_uint32), ("launches", C.c_uint32), ("read_ms", C.c_float), ("table_ms", C.c_float),
                ("classify_ms", C.c_float), ("write_ms", C.c_float), ("total_ms", C.c_float)]


def _map_records(path) -> int:
    """the records a well-formed map file of this length holds (12 bytes of header, 48 per record); 0 where there is no file --
    the call that reads it reports that"""
    try:
        return max(0, (os.path.getsize(path) - 12) // 48)
    except OSError:
        return 0


def default_compare_params() -> SmCompareParams:
    """sm_default_compare_params: voxel_mm 100, cover_shift 3, reach_cells 2, plane_mm 50, angle_thresh 30, match_class 0,
    write_mask 2 (the CHANGED records), max_cells 1 << 24, origin (0, 0, 0)"""
    p = SmCompareParams()
    load().sm_default_compare_params(C.byref(p))
    return p


def compare_params(**over) -> SmCompareParams:
    """default_compare_params() with fields overridden; origin takes a sequence of three"""
    p = default_compare_params()
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if k == "origin":
            p.origin[:] = [float(x) for x in v]
        else:
            setattr(p, k, v)
    return p


def search_params(**over) -> SmSearchParams:
    """sm_default_search_params (2 levels; +-2 m in x and z at 0.25 m, +-3 deg about y at 0.5 deg; refine 4, stride0 8, top_k 4,
    colour_thresh 0.1) with fields overridden; the four per-axis fields take a sequence of three"""
    p = SmSearchParams()
    load().sm_default_search_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if k in ("trans_half", "trans_step", "rot_half_deg", "rot_step_deg"):
            for a, x in enumerate(v):
                getattr(p, k)[a] = float(x)
        else:
            setattr(p, k, v)
    return p


class SmAutoPlaceParams(C.Structure):
    _fields_ = [("every", C.c_int32), ("rest", C.c_int32), ("add_above", C.c_float), ("match_below", C.c_float), ("min_jump", C.c_float),
                ("loop", SmLoopParams), ("search", SmSearchParams)]


class SmAutoPlaceStats(C.Structure):
    _fields_ = [("encoded", C.c_uint32), ("added", C.c_uint32), ("matched", C.c_uint32), ("attempts", C.c_uint32), ("closed", C.c_uint32),
                ("none", C.c_uint32), ("rejected", C.c_uint32), ("failed", C.c_uint32), ("no_old_map", C.c_uint32), ("last_k", C.c_int32),
                ("last_dis", C.c_uint32), ("last", SmLoopInfo)]


def auto_place_params(cfg, **over) -> SmAutoPlaceParams:
    """sm_default_auto_place_params (every 1, rest 10, add_above 0.2, match_below 0.3, min_jump 2 m, loop = loop_params(cfg) with
    max_trans 50 and max_rot_deg 45, search = search_params()) with fields overridden: a field of sm_loop_params by its own name,
    search as a dict of search_params() overrides"""
    p = SmAutoPlaceParams()
    load().sm_default_auto_place_params(C.byref(cfg), C.byref(p))
    for k, v in over.items():
        if k == "search":
            p.search = search_params(**dict(v))
        elif hasattr(p.loop, k):
            setattr(p.loop, k, v)
        elif hasattr(p, k) and k != "loop":
            setattr(p, k, v)
        else:
            raise KeyError(k)
    return p


def _search_arg(search):
    """close_loop(search=...) / set_auto_loop(search=...): None or False = no search, True = the defaults, a dict = overrides"""
    if search is None or search is False:
        return None
    return search_params(**({} if search is True else dict(search)))


INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _track_info_dict(info, rinfo=None, anchor=None) -> dict:
    """SmTrackInfo as the trackers' info dict; rinfo (SmTrackRgbInfo) and anchor (c_float) add their keys when given"""
    d = dict(status=TRACK_STATUS.get(info.status, str(info.status)), status_code=int(info.status), iterations=int(info.iterations),
             inliers=int(info.inliers), rmse=float(info.rmse), guess=np.array(info.guess[:], np.float32).reshape(4, 4).T.copy())
    if rinfo is not None:
        d.update(rgb_inliers=int(rinfo.rgb_inliers), rgb_rmse=float(rinfo.rgb_rmse), pivot_ratio=float(rinfo.pivot_ratio),
                 level_iterations=[int(x) for x in rinfo.level_iterations])
    if anchor is not None:
        d["anchor_time"] = float(anchor.value)
    return d


def _loop_info_dict(info) -> dict:
    return dict(status=LOOP_STATUS.get(info.status, str(info.status)), status_code=int(info.status), track=_track_info_dict(info.track),
                D=np.array(info.D[:], np.float32).reshape(4, 4).T.copy(), t_a=int(info.t_a), t_b=int(info.t_b))


def loop_spread(D, t_a, t_b) -> np.ndarray:
    """sm_loop_spread: the table float32[t_b - t_a + 1][12] (row-major 3x4 [R|t] per tick) that ramps the world->world correction D
    (4x4, numpy row/col indexing, or float32[16] column-major) from nothing at tick t_a to all of it at t_b.  Host only."""
    L = load()
    d = _mat16(D)
    t_a, t_b = int(t_a), int(t_b)
    out = np.zeros((max(t_b - t_a + 1, 1), 12), np.float32)
    rc = L.sm_loop_spread(_ptr(d), t_a, t_b, _ptr(out))
    if rc != SM_OK:
        raise SurfelMapError("sm_loop_spread", rc, L.sm_last_error().decode())
    return out


def _mat16(m):
    """float32[16] column-major; a 4x4 matrix (numpy row/col indexing) is converted"""
    a = np.asarray(m, np.float32)
    if a.shape == (4, 4):
        a = a.T
    a = np.ascontiguousarray(a.reshape(16))
    return a


def model_view(mvp, mv_inv, w, h, threshold=0.0, color_type=0, unstable=True, points=False, window=False, time=0,
               time_delta=0, clear=(0, 0, 0, 0)) -> SmModelView:
    v = SmModelView()
    v.mvp[:] = [float(x) for x in _mat16(mvp)]
    v.mv_inv[:] = [float(x) for x in _mat16(mv_inv)]
    v.threshold = threshold
    v.color_type, v.draw_unstable, v.draw_points, v.draw_window = int(color_type), int(bool(unstable)), int(bool(points)), int(bool(window))
    v.time, v.time_delta, v.width, v.height = int(time), int(time_delta), int(w), int(h)
    v.clear_rgba[:] = [int(c) for c in clear]
    return v


def _lidar_planes(shape) -> dict:
    return dict(range=np.zeros(shape, np.float32), id=np.zeros(shape, np.int32), rgb=np.zeros(tuple(shape) + (3,), np.uint8),
                sem=np.zeros(shape, np.uint8))


class SurfelMapError(RuntimeError):
    def __init__(self, what, rc, detail=""):
        super().__init__(f"{what} failed: rc={rc} {detail}".strip())
        self.rc = rc


_lib = None


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch's ROCm wheels bundle their own libamdhip64.so (soname libamdhip64.so.7) and ask
    for it by the name "libamdhip64.so"; the HIP core asks for "libamdhip64.so.7".  If the core is loaded first, ROCm's copy
    comes in and torch later loads its own as well -- two runtimes, and RCCL (torch's) cannot use the core's device memory
    (sm_create / sm_export_model_device refuse with both paths).  Loading torch's copy first makes either import order work:
    the core's request matches its soname.  No torch, or SM_NO_TORCH_HIP_PRELOAD=1: nothing is done."""
    if os.environ.get("SM_NO_TORCH_HIP_PRELOAD") == "1":
        return
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return                                   # torch's runtime is loaded already
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if not spec or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def _choose_rccl():
    """RCCL for the in-stream sharded mode is bound at run time by the core.  When PyTorch is installed this module has made
    PyTorch's bundled HIP runtime the process's runtime (above); name PyTorch's bundled RCCL too, so that both come from one
    build.  SM_RCCL_LIB set by the user wins; without PyTorch the core takes ROCm's librccl."""
    if os.environ.get("SM_RCCL_LIB") or os.environ.get("SM_NO_TORCH_HIP_PRELOAD") == "1":
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "librccl.so")
        if os.path.exists(cand):
            os.environ["SM_RCCL_LIB"] = cand


def rccl_unique_id() -> bytes:
    """128-byte RCCL id made by one rank and handed to all (sm_shard_rccl_unique_id)"""
    _choose_rccl()
    L = load()
    buf = C.create_string_buffer(128)
    rc = L.sm_shard_rccl_unique_id(buf)
    if rc:
        raise SurfelMapError("sm_shard_rccl_unique_id", rc, L.sm_last_error().decode())
    return buf.raw


def load():
    """dlopen the HIP library (no compute).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C surfelmapping_amd/csrc). surfelmapping_amd has no CPU fallback.")
    _preload_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    vp, u32p = C.c_void_p, C.POINTER(C.c_uint32)
    L.sm_api_version.restype = C.c_int
    if L.sm_api_version() != API_VERSION:     # a stale build: the struct layouts below would not match
        raise ImportError(f"{LIB_PATH} has API version {L.sm_api_version()}, this binding expects {API_VERSION}: rebuild it "
                          "(python -c 'import __graft_entry__ as g; g.build()')")
    L.sm_last_error.restype = C.c_char_p
    L.sm_default_config.argtypes = [C.POINTER(SmConfig), C.c_int, C.c_int] + [C.c_float] * 4
    L.sm_create.restype = vp
    L.sm_create.argtypes = [C.POINTER(SmConfig)]
    L.sm_destroy.restype = None
    L.sm_destroy.argtypes = [vp]
    L.sm_process_frame.argtypes = [vp, vp, vp, vp, vp]
    L.sm_process_frame_device.argtypes = [vp, vp, vp, vp, vp]
    L.sm_process_frame_async.argtypes = [vp, vp, vp, vp, vp]
    L.sm_inputs_consumed.argtypes = [vp]
    L.sm_host_alloc.restype = vp
    L.sm_host_alloc.argtypes = [vp, C.c_size_t]
    L.sm_host_free.argtypes = [vp, vp]
    L.sm_host_alloc_frame.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.sm_debug_slow_frames.argtypes = [vp, u32p]
    L.sm_debug_squeezes.argtypes = [vp, u32p, u32p]
    L.sm_sync.argtypes = [vp]
    L.sm_clean_points.argtypes = [vp, vp, vp, vp]
    L.sm_clean_points_ex.argtypes = [vp, vp, vp, vp, C.c_int]
    L.sm_clean_points_cb.argtypes = [vp, vp, vp, vp, C.c_int, CAP_FN, vp]
    L.sm_reset.argtypes = [vp]
    L.sm_get_counts.argtypes = [vp, C.POINTER(SmCounts)]
    L.sm_download_model_aos.argtypes = [vp, vp, C.c_uint32, u32p]
    L.sm_upload_model_aos.argtypes = [vp, vp, C.c_uint32]
    L.sm_save_map.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32]
    L.sm_load_map.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sm_download_index_map.argtypes = [vp, vp, vp, vp, vp]
    L.sm_download_raw_cloud.argtypes = [vp, vp, C.c_uint32, u32p]
    L.sm_download_depth.argtypes = [vp, C.c_int, vp]
    L.sm_render_image.argtypes = [vp, vp, C.c_int, C.c_int] + [C.c_float] * 4 + [vp, vp]
    L.sm_render_model.argtypes = [vp, C.POINTER(SmModelView), vp, vp, vp]
    L.sm_render_model_device.argtypes = [vp, C.POINTER(SmModelView), vp, vp, vp]
    L.sm_render_image_maps.argtypes = [vp, C.POINTER(SmMapSource), vp, C.c_uint32, C.c_int, C.c_int] + [C.c_float] * 4 + [vp, vp]
    L.sm_render_model_maps.argtypes = [vp, C.POINTER(SmMapSource), C.POINTER(SmModelView), C.c_uint32, vp, vp, vp]
    L.sm_render_maps_stats.argtypes = [vp, C.POINTER(SmMapsStats)]
    L.sm_set_frame.argtypes = [vp, vp, vp, vp]
    L.sm_set_tick.argtypes = [vp, C.c_int32]
    L.sm_stage_conflict.argtypes = [vp, vp, C.c_float, C.c_float, C.c_float, C.c_int]
    L.sm_stage_cull.argtypes = [vp]
    L.sm_stage_splat.argtypes = [vp, vp, C.c_int32, C.c_float, C.c_int32]
    L.sm_stage_associate_fuse.argtypes = [vp, vp, C.c_int32, C.c_float, C.c_float]
    L.sm_stage_timings.argtypes = [vp, C.POINTER(SmTimings)]
    L.sm_read_frame_log.argtypes = [vp, vp, C.c_uint32, u32p]
    L.sm_device_alloc.restype = vp
    L.sm_device_alloc.argtypes = [vp, C.c_size_t]
    L.sm_device_free.argtypes = [vp, vp]
    L.sm_device_upload.argtypes = [vp, vp, vp, C.c_size_t]
    L.sm_export_model_device.argtypes = [vp, C.POINTER(vp), u32p]
    L.sm_append_model_aos_device.argtypes = [vp, vp, C.c_uint32]
    L.sm_device_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.sm_shard_stream_configure.argtypes = [vp, C.c_int, C.c_int]
    L.sm_shard_set_collective.argtypes = [vp, COLLECTIVE_FN, vp]
    L.sm_shard_rccl_unique_id.argtypes = [vp]
    L.sm_shard_rccl_init.argtypes = [vp, vp]
    L.sm_shard_rccl_finalize.argtypes = [vp]
    L.sm_shard_rccl_nranks.argtypes = [vp]
    L.sm_shard_frame_device.argtypes = [vp, vp, vp, vp, vp]
    L.sm_shard_frame.argtypes = [vp, vp, vp, vp, vp]
    L.sm_shard_compact.argtypes = [vp]
    L.sm_shard_export_dense_device.argtypes = [vp, C.POINTER(vp), u32p]
    L.sm_gpu_process_count.argtypes = [vp]
    L.sm_rig_configure.argtypes = [vp, C.c_int, C.c_int]
    L.sm_rig_consolidate.argtypes = [vp, vp, vp, vp, vp, u32p, u32p]
    L.sm_rig_consolidate_step.argtypes = [vp, vp, vp, vp, vp, u32p, u32p]
    L.sm_default_track_params.argtypes = [C.POINTER(SmTrackParams)]
    L.sm_track_frame.argtypes = [vp, vp, vp, C.POINTER(SmTrackParams), vp, C.POINTER(SmTrackInfo)]
    L.sm_track_debug.argtypes = [vp, vp, vp, vp, vp]
    L.sm_default_track_rgb_params.argtypes = [C.POINTER(SmTrackRgbParams)]
    L.sm_track_frame_rgb.argtypes = [vp, vp, vp, vp, C.POINTER(SmTrackParams), C.POINTER(SmTrackRgbParams), vp,
                                     C.POINTER(SmTrackInfo), C.POINTER(SmTrackRgbInfo)]
    L.sm_track_rgb_debug.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp]
    L.sm_default_retire_params.argtypes = [C.POINTER(SmConfig), C.POINTER(SmRetireParams)]
    L.sm_retire.argtypes = [vp, vp, C.POINTER(SmRetireParams), vp, C.c_uint32, u32p]
    L.sm_retire_device.argtypes = [vp, vp, C.POINTER(SmRetireParams), vp, C.c_uint32, u32p]
    L.sm_set_auto_retire.argtypes = [vp, C.POINTER(SmRetireParams), C.c_int32, C.c_char_p]
    L.sm_auto_retire_stats.argtypes = [vp, u32p, C.POINTER(C.c_uint64)]
    L.sm_default_recall_params.argtypes = [C.POINTER(SmConfig), C.POINTER(SmRecallParams)]
    L.sm_recall.argtypes = [vp, C.POINTER(SmMapSource), vp, C.POINTER(SmRecallParams), C.c_int32, u32p]
    L.sm_recall_stats.argtypes = [vp, C.POINTER(SmRecallStats)]
    L.sm_set_auto_recall.argtypes = [vp, C.POINTER(SmRecallParams)]
    L.sm_auto_recall_stats.argtypes = [vp, u32p, C.POINTER(C.c_uint64)]
    L.sm_warp_by_time.argtypes = [vp, C.POINTER(SmMapSource), C.c_int32, C.c_uint32, vp]
    L.sm_warp_stats.argtypes = [vp, C.POINTER(SmWarpStats)]
    L.sm_loop_spread.argtypes = [vp, C.c_int32, C.c_int32, vp]
    L.sm_track_frame_old.argtypes = [vp, vp, vp, C.POINTER(SmTrackParams), C.c_int32, vp, C.POINTER(SmTrackInfo), C.POINTER(C.c_float)]
    L.sm_track_debug_old.argtypes = [vp, vp, vp, C.c_int32, vp, vp]
    L.sm_default_loop_params.argtypes = [C.POINTER(SmConfig), C.POINTER(SmLoopParams)]
    L.sm_close_loop.argtypes = [vp, vp, vp, C.POINTER(SmMapSource), C.POINTER(SmTrackParams), C.POINTER(SmLoopParams), vp,
                                C.POINTER(SmLoopInfo)]
    i32, tpp, rpp, lpp = C.c_int32, C.POINTER(SmTrackParams), C.POINTER(SmTrackRgbParams), C.POINTER(SmLoopParams)
    L.sm_track_frame_window.argtypes = [vp, vp, vp, tpp, i32, i32, vp, C.POINTER(SmTrackInfo), C.POINTER(C.c_float)]
    L.sm_track_debug_window.argtypes = [vp, vp, vp, i32, i32, vp, vp]
    L.sm_track_frame_rgb_window.argtypes = [vp, vp, vp, vp, tpp, rpp, i32, i32, vp, C.POINTER(SmTrackInfo), C.POINTER(SmTrackRgbInfo),
                                            C.POINTER(C.c_float)]
    L.sm_track_rgb_debug_window.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, i32, i32, vp, vp]
    L.sm_close_loop_rgb.argtypes = [vp, vp, vp, vp, C.POINTER(SmMapSource), tpp, rpp, lpp, vp, C.POINTER(SmLoopInfo)]
    L.sm_old_in_view.argtypes = [vp, vp, i32, u32p]
    L.sm_default_auto_loop_params.argtypes = [C.POINTER(SmConfig), C.POINTER(SmAutoLoopParams)]
    L.sm_set_auto_loop.argtypes = [vp, C.POINTER(SmAutoLoopParams), C.POINTER(SmMapSource)]
    L.sm_auto_loop_stats.argtypes = [vp, C.POINTER(SmAutoLoopStats)]
    spp = C.POINTER(SmSearchParams)
    L.sm_default_search_params.argtypes = [spp]
    L.sm_score_poses_window.argtypes = [vp, vp, vp, vp, C.c_uint32, tpp, i32, C.c_float, i32, i32, vp]
    L.sm_search_pose.argtypes = [vp, vp, vp, vp, tpp, rpp, spp, i32, i32, vp, C.POINTER(SmSearchInfo)]
    L.sm_close_loop_search.argtypes = [vp, vp, vp, vp, C.POINTER(SmMapSource), tpp, rpp, lpp, spp, vp, C.POINTER(SmLoopInfo)]
    L.sm_set_auto_loop_search.argtypes = [vp, spp]
    lsp = C.POINTER(SmLidarSensor)
    L.sm_default_lidar_sensor.argtypes = [lsp]
    L.sm_lidar_directions.argtypes = [lsp, vp]
    L.sm_lidar_sweep.argtypes = [vp, lsp, vp, vp, vp, vp, vp]
    L.sm_lidar_sweep_maps.argtypes = [vp, C.POINTER(SmMapSource), lsp, vp, C.c_uint32, vp, vp, vp, vp]
    L.sm_lidar_stats.argtypes = [vp, C.POINTER(SmLidarStats)]
    fpp = C.POINTER(SmFernParams)
    L.sm_default_fern_params.argtypes = [C.POINTER(SmConfig), fpp]
    L.sm_fern_table.argtypes = [fpp, i32, i32, vp]
    L.sm_set_ferns.argtypes = [vp, fpp]
    L.sm_fern_encode.argtypes = [vp, vp, vp, vp]
    L.sm_fern_encode_device.argtypes = [vp, vp, vp, vp]
    L.sm_fern_add.argtypes = [vp, vp, vp, i32, u32p]
    L.sm_fern_count.argtypes = [vp, u32p]
    L.sm_fern_download.argtypes = [vp, vp, vp, vp]
    L.sm_fern_save.argtypes = [vp, C.c_char_p]
    L.sm_fern_load.argtypes = [vp, C.c_char_p]
    L.sm_fern_match.argtypes = [vp, vp, i32, i32, C.POINTER(i32), u32p, vp]
    L.sm_search_pose_at.argtypes = [vp, vp, vp, vp, vp, tpp, rpp, spp, i32, i32, vp, C.POINTER(SmSearchInfo)]
    L.sm_close_loop_at.argtypes = [vp, vp, vp, vp, vp, C.POINTER(SmMapSource), tpp, rpp, lpp, spp, vp, C.POINTER(SmLoopInfo)]
    L.sm_default_auto_place_params.argtypes = [C.POINTER(SmConfig), C.POINTER(SmAutoPlaceParams)]
    L.sm_set_auto_place.argtypes = [vp, C.POINTER(SmAutoPlaceParams)]
    L.sm_auto_place_stats.argtypes = [vp, C.POINTER(SmAutoPlaceStats)]
    L.sm_debug_place_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]     # (a diagnostic, not in the header)
    stp = C.POINTER(SmStereoParams)
    L.sm_default_stereo_params.argtypes = [C.POINTER(SmConfig), stp]
    L.sm_set_stereo.argtypes = [vp, stp]
    L.sm_stereo_depth.argtypes = [vp, vp, vp, vp, vp]
    L.sm_stereo_depth_device.argtypes = [vp, vp, vp, vp, vp]
    L.sm_stereo_download.argtypes = [vp, vp, vp, vp]
    L.sm_debug_stereo_ms.argtypes = [vp, C.POINTER(C.c_float)]                          # (a diagnostic, not in the header)
    flp = C.POINTER(SmFillParams)
    L.sm_default_fill_params.argtypes = [flp]
    L.sm_fill_image.argtypes = [vp, flp, C.c_int, C.c_int, C.c_uint32, vp, vp, vp]
    L.sm_fill_image_device.argtypes = [vp, flp, C.c_int, C.c_int, C.c_uint32, vp, vp, vp]
    L.sm_render_image_ex.argtypes = [vp, vp, C.c_int, C.c_int] + [C.c_float] * 4 + [flp, vp, vp, vp]
    L.sm_render_image_maps_ex.argtypes = [vp, C.POINTER(SmMapSource), vp, C.c_uint32, C.c_int, C.c_int] + [C.c_float] * 4 + [flp, vp, vp, vp]
    L.sm_fill_stats.argtypes = [vp, C.POINTER(SmFillStats)]
    blp = C.POINTER(SmBlendParams)
    L.sm_default_blend_params.argtypes = [blp]
    L.sm_render_image_blend.argtypes = [vp, vp, C.c_int, C.c_int] + [C.c_float] * 4 + [blp, flp, vp, vp, vp]
    L.sm_render_image_maps_blend.argtypes = [vp, C.POINTER(SmMapSource), vp, C.c_uint32, C.c_int, C.c_int] + [C.c_float] * 4 + [blp, flp, vp, vp, vp]
    L.sm_blend_stats.argtypes = [vp, C.POINTER(SmBlendStats)]
    smp = C.POINTER(SmSimplifyParams)
    L.sm_default_simplify_params.argtypes = [smp]
    L.sm_simplify.argtypes = [vp, smp]
    L.sm_simplify_maps.argtypes = [vp, C.POINTER(SmMapSource), smp, C.c_char_p]
    L.sm_simplify_stats.argtypes = [vp, C.POINTER(SmSimplifyStats)]
    rgp, msp = C.POINTER(SmRegisterParams), C.POINTER(SmMapSource)
    L.sm_default_register_params.argtypes = [rgp]
    L.sm_register_maps.argtypes = [vp, msp, msp, C.c_void_p, rgp, C.c_void_p, C.POINTER(SmRegisterInfo)]
    L.sm_register_debug.argtypes = [vp, msp, msp, C.c_void_p, C.c_int32, rgp, C.c_void_p, C.c_void_p]
    L.sm_register_stats.argtypes = [vp, C.POINTER(SmRegisterStats)]
    cpp = C.POINTER(SmCompareParams)
    L.sm_default_compare_params.argtypes = [cpp]
    L.sm_compare_maps.argtypes = [vp, msp, msp, C.c_void_p, cpp, C.c_void_p, C.c_char_p, C.POINTER(SmCompareInfo)]
    L.sm_compare_stats.argtypes = [vp, C.POINTER(SmCompareStats)]
    tpp = C.POINTER(SmTileParams)
    L.sm_default_tile_params.argtypes = [tpp]
    L.sm_tile_maps.argtypes = [vp, msp, tpp, C.c_char_p]
    L.sm_tile_stats.argtypes = [vp, C.POINTER(SmTileStats)]
    spp = C.POINTER(SmSegmentParams)
    L.sm_default_segment_params.argtypes = [spp]
    L.sm_segment_maps.argtypes = [vp, msp, spp, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.POINTER(SmSegmentInfo)]
    L.sm_segment_stats.argtypes = [vp, C.POINTER(SmSegmentStats)]
    mpp = C.POINTER(SmMeshParams)
    L.sm_default_mesh_params.argtypes = [mpp]
    L.sm_mesh_maps.argtypes = [vp, msp, mpp, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, C.POINTER(SmMeshInfo)]
    L.sm_mesh_stats.argtypes = [vp, C.POINTER(SmMeshStats)]
    gpp = C.POINTER(SmGroundParams)
    L.sm_default_ground_params.argtypes = [gpp]
    L.sm_ground_maps.argtypes = [vp, msp, gpp] + [C.c_void_p] * 6 + [C.POINTER(SmGroundInfo)]
    L.sm_ground_stats.argtypes = [vp, C.POINTER(SmGroundStats)]
    L.sm_default_rays_params.argtypes = [C.POINTER(SmRaysParams)]
    L.sm_cast_rays_maps.argtypes = [vp, C.POINTER(SmMapSource), C.POINTER(SmRaysParams), vp, C.c_uint32, vp, vp, vp, vp, vp]
    L.sm_cast_rays_stats.argtypes = [vp, C.POINTER(SmRaysStats)]
    scp = C.POINTER(SmScene)
    L.sm_render_image_scene.argtypes = [vp, msp, scp, vp, C.c_uint32, C.c_int, C.c_int] + [C.c_float] * 4 + [flp, vp, vp, vp]
    L.sm_lidar_sweep_scene.argtypes = [vp, msp, scp, lsp, vp, C.c_uint32, vp, vp, vp, vp]
    L.sm_scene_place_rows.argtypes = [vp, vp, C.c_uint32, vp]
    L.sm_scene_stats.argtypes = [vp, C.POINTER(SmSceneStats)]
    for name in SYMBOLS:
        getattr(L, name)          # AttributeError here = the library does not match the header
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_config(width, height, fx, fy, cx, cy, **over) -> SmConfig:
    c = SmConfig()
    load().sm_default_config(C.byref(c), width, height, fx, fy, cx, cy)
    for k, v in over.items():
        if not hasattr(c, k):
            raise KeyError(k)
        setattr(c, k, v)
    return c


class SurfelMap:
    """Host-side handle mirroring SurfelMapping / GlobalModel / IndexMap of the reference
    (src/SurfelMapping.h:31-96, src/GlobalModel.h:22-120, src/IndexMap.h:34-88)."""

    def __init__(self, cfg: SmConfig):
        self._L = load()
        self.cfg = cfg
        self.W, self.H = cfg.width, cfg.height
        self.P = self.W * self.H
        self._h = self._L.sm_create(C.byref(cfg))
        if not self._h:
            raise SurfelMapError("sm_create", SM_E_NO_DEVICE, self._L.sm_last_error().decode())

    def _chk(self, rc, what, allow=(0,)):
        if rc not in allow:
            raise SurfelMapError(what, rc, self._L.sm_last_error().decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._L.sm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- SurfelMapping
    def process_frame(self, rgb, depth, sem, pose, allow=(0,)):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = None if depth is None else np.ascontiguousarray(depth, np.uint16)
        sem = None if sem is None else np.ascontiguousarray(sem, np.uint8)
        pose = np.ascontiguousarray(pose, np.float32)
        return self._chk(self._L.sm_process_frame(self._h, _ptr(rgb), _ptr(depth), _ptr(sem), _ptr(pose)),
                         "sm_process_frame", allow)

    def process_frame_device(self, d_rgb, d_depth, d_sem, pose):
        pose = np.ascontiguousarray(pose, np.float32)
        return self._chk(self._L.sm_process_frame_device(self._h, d_rgb, d_depth, d_sem, _ptr(pose)),
                         "sm_process_frame_device")

    def process_frame_async(self, rgb, depth, sem, pose):
        """host arrays, no host wait: the copy of this frame overlaps the previous frame (sm_process_frame_async).  Arrays made by
        host_array() (pinned, owned by the context) are read in place until inputs_consumed() / sync(); others are staged inside
        the call."""
        assert rgb.dtype == np.uint8 and rgb.flags.c_contiguous
        pose = np.ascontiguousarray(pose, np.float32)
        return self._chk(self._L.sm_process_frame_async(self._h, _ptr(rgb), _ptr(depth), _ptr(sem), _ptr(pose)), "sm_process_frame_async")

    def host_array(self, shape, dtype) -> np.ndarray:
        """a numpy array in pinned host memory owned by the context (sm_host_alloc): the fastest source for process_frame_async"""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self._L.sm_host_alloc(self._h, n)
        if not p:
            raise SurfelMapError("sm_host_alloc", SM_E_HIP, self._L.sm_last_error().decode())
        buf = (C.c_ubyte * n).from_address(p)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def host_frame(self):
        """(rgb (H, W, 3) u8, depth (H, W) u16, semantic (H, W) u8): numpy views of ONE pinned block (sm_host_alloc_frame) --
        process_frame_async copies such a frame with a single transfer"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self._L.sm_host_alloc_frame(self._h, C.byref(a), C.byref(b), C.byref(c)), "sm_host_alloc_frame")
        H, W = self.H, self.W
        rgb = np.frombuffer((C.c_ubyte * (H * W * 3)).from_address(a.value), dtype=np.uint8).reshape(H, W, 3)
        dep = np.frombuffer((C.c_ubyte * (H * W * 2)).from_address(b.value), dtype=np.uint16).reshape(H, W)
        sem = np.frombuffer((C.c_ubyte * (H * W)).from_address(c.value), dtype=np.uint8).reshape(H, W)
        return rgb, dep, sem

    def debug_slow_frames(self) -> int:
        """frames that took the rare path of the two-launch frame so far (diagnostic; synchronises)"""
        n = C.c_uint32()
        self._chk(self._L.sm_debug_slow_frames(self._h, C.byref(n)), "sm_debug_slow_frames")
        return int(n.value)

    def debug_squeezes(self):
        """(tail, full): the squeezes between a frame's two launches so far that left dead slots below their boundary / that
        squeezed every dead slot (diagnostic; synchronises)"""
        t, f = C.c_uint32(), C.c_uint32()
        self._chk(self._L.sm_debug_squeezes(self._h, C.byref(t), C.byref(f)), "sm_debug_squeezes")
        return int(t.value), int(f.value)

    def inputs_consumed(self):
        self._chk(self._L.sm_inputs_consumed(self._h), "sm_inputs_consumed")

    def sync(self, allow=(0,)):
        return self._chk(self._L.sm_sync(self._h), "sm_sync", allow)

    def clean_points(self, depth, sem, pose):
        depth = np.ascontiguousarray(depth, np.uint16)
        sem = np.ascontiguousarray(sem, np.uint8)
        pose = np.ascontiguousarray(pose, np.float32)
        self._chk(self._L.sm_clean_points(self._h, _ptr(depth), _ptr(sem), _ptr(pose)), "sm_clean_points")

    def clean_points_slice(self, depth, sem, pose, exempt_first: bool, cap_hook=None):
        """cleanPoints on a rig slice (surfelmapping_amd/dist.py): the id-0 exemption only where the slice holds the global surfel
        0; cap_hook(local_conflicts) -> how many of them may take effect (the slice's share of the union's W*H conflict
        records), called between the conflict test and the cull"""
        depth = np.ascontiguousarray(depth, np.uint16)
        sem = np.ascontiguousarray(sem, np.uint8)
        pose = np.ascontiguousarray(pose, np.float32)
        if cap_hook is None:
            self._chk(self._L.sm_clean_points_ex(self._h, _ptr(depth), _ptr(sem), _ptr(pose), 1 if exempt_first else 0), "sm_clean_points_ex")
            return
        err = []

        def tramp(user, local):
            try:
                return int(cap_hook(int(local)))
            except Exception as e:                       # never let an exception cross the C frame
                err.append(e)
                return SM_E_HIP
        cb = CAP_FN(tramp)
        rc = self._L.sm_clean_points_cb(self._h, _ptr(depth), _ptr(sem), _ptr(pose), 1 if exempt_first else 0, cb, None)
        if err:
            raise err[0]
        self._chk(rc, "sm_clean_points_cb")

    def reset(self):
        self._chk(self._L.sm_reset(self._h), "sm_reset")

    # -- tracking (sm_track_frame): what every wrapper of a tracker shares
    _RGB_KEYS = ("levels", "iters", "rgb_weight", "rgb_max_residual")

    def _images(self, depth, rgb=None):
        """depth uint16[H][W] (and rgb uint8[H][W][3], if given) contiguous and of the context's size"""
        depth = np.ascontiguousarray(depth, np.uint16)
        if rgb is None:
            assert depth.size == self.P, depth.shape
            return depth, None
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert depth.size == self.P and rgb.size == self.P * 3, (depth.shape, rgb.shape)
        return depth, rgb

    def _split_params(self, params, colour):
        """**params as (SmTrackParams, SmTrackRgbParams), None where no field is named (the C side's defaults).  colour False:
        every key must be sm_track_params' own."""
        col = {k: v for k, v in params.items() if colour and k in self._RGB_KEYS}
        icp = {k: v for k, v in params.items() if k not in col}
        return track_params(**icp) if icp else None, track_rgb_params(**col) if col else None

    def _track_frame(self, fn, depth, guess, params, rgb=None, window=()):
        """One tracked frame through sm_track_frame* `fn`, whose arguments are (ctx, [rgb,] depth, guess, params, [rgb params,]
        [window...,] pose out, info, [rgb info,] [anchor time]): rgb and window (a tuple of times) say which.  Returns
        (pose 4x4, info dict)."""
        depth, rgb = self._images(depth, rgb)
        g = None if guess is None else _mat16(guess)
        p, q = self._split_params(params, colour=rgb is not None)
        out = np.zeros(16, np.float32)
        info = SmTrackInfo()
        rinfo = None if rgb is None else SmTrackRgbInfo()
        anchor = C.c_float() if window else None
        one = (lambda x: []) if rgb is None else (lambda x: [x])          # an argument of the colour forms only
        args = ([self._h] + one(_ptr(rgb)) + [_ptr(depth), _ptr(g), p] + one(q) + [int(t) for t in window] + [_ptr(out), info] + one(rinfo)
                + ([anchor] if window else []))
        self._chk(getattr(self._L, fn)(*args), fn)
        return out.reshape(4, 4).T.copy(), _track_info_dict(info, rinfo, anchor)

    def _track_debug(self, fn, depth, pose_eval, *mid, rgb=None):
        """One iteration's system through sm_track*_debug* `fn`(ctx, [rgb,] depth, pose_eval, *mid, pred out, sys29 out).
        Returns (pred_slot int32[H][W], sys float64[29])."""
        depth, rgb = self._images(depth, rgb)
        pe = _mat16(pose_eval)
        pred = np.zeros((self.H, self.W), np.int32)
        sys29 = np.zeros(29, np.float64)
        head = [self._h] if rgb is None else [self._h, _ptr(rgb)]
        self._chk(getattr(self._L, fn)(*head, _ptr(depth), _ptr(pe), *[int(v) for v in mid], _ptr(pred), _ptr(sys29)), fn)
        return pred, sys29

    def track(self, depth, guess=None, **params):
        """Track one depth image (uint16[H][W] mm) against the model (sm_track_frame); the model is not changed.  guess: a 4x4
        camera->world matrix (numpy row/col indexing) or float32[16] column-major; None = constant velocity.  params override
        sm_default_track_params.  Returns (pose 4x4 float32, numpy row/col indexing; the guess unless status is "OK",
        info dict: status (name), status_code, iterations, inliers, rmse, guess 4x4)."""
        return self._track_frame("sm_track_frame", depth, guess, params)

    def track_debug(self, depth, pose_eval):
        """sm_track_debug: (pred_slot int32[H][W], model slot or -1, sys float64[29]) -- the prediction of the next track() and one
        iteration's system at pose_eval (4x4 or float32[16] column-major) with the default parameters"""
        return self._track_debug("sm_track_debug", depth, pose_eval)

    def track_stats(self):
        """device times in ms of the last track()/track_debug() call made with SM_TRACK_TIMING=1 (sm_debug_track_stats, not part
        of the C-ABI header): [prediction, vertex stage, reduce_0, solve_0, reduce_1, solve_1, ...], or [] if it was not timed"""
        f = self._L.sm_debug_track_stats
        f.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
        ms, n = (C.c_float * 256)(), C.c_int()
        self._chk(f(self._h, ms, 256, C.byref(n)), "sm_debug_track_stats")
        return [float(x) for x in ms[:n.value]]

    def process_frame_tracked(self, rgb, depth, sem, guess=None, **params):
        """track() the frame, then process_frame() it with the tracked pose (the guess when tracking failed).
        Returns (pose 4x4 float32, info dict) as track()."""
        pose, info = self.track(depth, guess, **params)
        self.process_frame(rgb, depth, sem, _mat16(pose))
        return pose, info

    # -- tracking with the colour term (sm_track_frame_rgb)
    def track_rgb(self, rgb, depth, guess=None, **params):
        """track() with the photometric term, coarse to fine (sm_track_frame_rgb): rgb uint8[H][W][3] as process_frame takes it.
        params override sm_default_track_params and sm_default_track_rgb_params (levels, iters, rgb_weight, rgb_max_residual).
        Returns (pose, info) as track(), info with rgb_inliers, rgb_rmse, pivot_ratio and level_iterations (list of 6) added."""
        return self._track_frame("sm_track_frame_rgb", depth, guess, params, rgb=np.asarray(rgb))

    def track_rgb_debug(self, rgb, depth, pose_eval, level=0, which=0):
        """sm_track_rgb_debug: the system float64[29] of one iteration at pose_eval and `level` with the default parameters;
        which 0 = joint, 1 = the geometric term, 2 = the photometric term (unweighted)"""
        depth, rgb = self._images(depth, np.asarray(rgb))
        pe = _mat16(pose_eval)
        sys29 = np.zeros(29, np.float64)
        self._chk(self._L.sm_track_rgb_debug(self._h, _ptr(rgb), _ptr(depth), _ptr(pe), int(level), int(which), _ptr(sys29)),
                  "sm_track_rgb_debug")
        return sys29

    def track_rgb_stats(self):
        """device times of the last track_rgb()/track_rgb_debug() call made with SM_TRACK_TIMING=1 (sm_debug_track_rgb_stats, not
        part of the C-ABI header): a list of (kind, level, ms), kind one of "prediction", "vertex", "pyramid", "gather",
        "level_vertex", "icp", "photo", "solve"; [] if it was not timed"""
        f = self._L.sm_debug_track_rgb_stats
        f.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
        ms, kind, n = (C.c_float * 512)(), (C.c_int * 512)(), C.c_int()
        self._chk(f(self._h, ms, kind, 512, C.byref(n)), "sm_debug_track_rgb_stats")
        names = ("prediction", "vertex", "pyramid", "gather", "level_vertex", "icp", "photo", "solve")
        return [(names[kind[i] & 15], kind[i] >> 4, float(ms[i])) for i in range(n.value)]

    def process_frame_tracked_rgb(self, rgb, depth, sem, guess=None, **params):
        """track_rgb() the frame, then process_frame() it with the tracked pose (the guess when tracking failed).
        Returns (pose 4x4 float32, info dict) as track_rgb()."""
        pose, info = self.track_rgb(rgb, depth, guess, **params)
        self.process_frame(rgb, depth, sem, _mat16(pose))
        return pose, info

    # -- GlobalModel
    def counts(self) -> dict:
        c = SmCounts()
        self._chk(self._L.sm_get_counts(self._h, C.byref(c)), "sm_get_counts")
        return c.as_dict()

    def download_model(self) -> np.ndarray:
        n = C.c_uint32()
        self._chk(self._L.sm_download_model_aos(self._h, None, 0, C.byref(n)), "sm_download_model_aos")
        out = np.zeros((n.value, 12), np.float32)
        self._chk(self._L.sm_download_model_aos(self._h, _ptr(out), n.value, C.byref(n)), "sm_download_model_aos")
        return out

    def upload_model(self, m):
        m = np.ascontiguousarray(m, np.float32)
        self._chk(self._L.sm_upload_model_aos(self._h, _ptr(m), m.shape[0]), "sm_upload_model_aos")

    def save_map(self, path, start_id=0, end_id=0):
        self._chk(self._L.sm_save_map(self._h, os.fsencode(path), start_id, end_id), "sm_save_map")

    def load_map(self, path):
        a, b = C.c_int32(), C.c_int32()
        self._chk(self._L.sm_load_map(self._h, os.fsencode(path), C.byref(a), C.byref(b)), "sm_load_map")
        return a.value, b.value

    # -- retirement (sm_retire, sm_set_auto_retire)
    def retire(self, pose=None, dry_run=False, **params):
        """Move the surfels that are older than min_age frames and farther than min_distance from the camera centre out of
        the model (sm_retire).  pose: a 4x4 camera->world matrix (numpy row/col indexing) or float32[16] column-major; None =
        the pose of the last processed frame.  params override sm_default_retire_params.  Returns the retired records,
        float32[n][12] in model order -- or, with dry_run, only how many there would be (nothing changes)."""
        g = None if pose is None else _mat16(pose)
        p = retire_params(self.cfg, **params) if params else None
        pp = C.byref(p) if p is not None else None
        n = C.c_uint32()
        self._chk(self._L.sm_retire(self._h, _ptr(g), pp, None, 0, C.byref(n)), "sm_retire")
        if dry_run:
            return int(n.value)
        out = np.zeros((n.value, 12), np.float32)
        # (a destination is always given, also for n = 0: a NULL one would be another dry run)
        dst = out if n.value else np.zeros((1, 12), np.float32)
        self._chk(self._L.sm_retire(self._h, _ptr(g), pp, _ptr(dst), n.value, C.byref(n)), "sm_retire")
        return out

    def set_auto_retire(self, every, prefix, **params):
        """After every frame whose new tick is a multiple of `every`, retire at that frame's pose into the map file
        "<prefix>_%06u.bin" (sm_set_auto_retire; load_map reads such a file).  every <= 0 or prefix None: off."""
        p = retire_params(self.cfg, **params) if params else None
        self._chk(self._L.sm_set_auto_retire(self._h, C.byref(p) if p is not None else None, int(every),
                                             None if prefix is None else os.fsencode(prefix)), "sm_set_auto_retire")

    def auto_retire_stats(self):
        """(map files, surfels) the periodic policy has written so far"""
        f, n = C.c_uint32(), C.c_uint64()
        self._chk(self._L.sm_auto_retire_stats(self._h, C.byref(f), C.byref(n)), "sm_auto_retire_stats")
        return int(f.value), int(n.value)

    def retire_stats(self):
        """device times in ms of the last retirement made with SM_RETIRE_TIMING=1 (sm_debug_retire_stats, not part of the C-ABI
        header): dict(mark, scan, gather, compact, bounds), or None if it was not timed"""
        f = self._L.sm_debug_retire_stats
        f.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        ms = (C.c_float * 5)()
        self._chk(f(self._h, ms), "sm_debug_retire_stats")
        return None if ms[0] < 0 else dict(zip(("mark", "scan", "gather", "compact", "bounds"), [float(x) for x in ms]))

    # -- paging in (sm_recall, sm_set_auto_recall)
    def recall(self, paths, pose=None, mode="move", **params) -> int:
        """Bring the records of the map files `paths` that lie within `radius` of the camera centre back into the model
        (sm_recall): the model becomes concat(download_model(), near rows of the files in the given order).  mode "move" takes
        them out of the files, "copy" leaves the files alone, "count" only counts.  pose: a 4x4 camera->world matrix or
        float32[16] column-major; None = the pose of the last processed frame.  params override sm_default_recall_params.
        Returns how many rows came back (or would)."""
        g = None if pose is None else _mat16(pose)
        p = recall_params(self.cfg, **params) if params else None
        src = map_source(paths, include_model=False)
        n = C.c_uint32()
        self._chk(self._L.sm_recall(self._h, C.byref(src), _ptr(g), C.byref(p) if p is not None else None, RECALL_MODE[mode], C.byref(n)),
                  "sm_recall")
        return int(n.value)

    def recall_stats(self) -> dict:
        """of the last recall (the policy's included): files_listed, files_skipped (by the file index), files_read,
        files_rewritten, records_read, recalled, chunks, read_ms, copy_ms, device_ms, write_ms, total_ms"""
        st = SmRecallStats()
        self._chk(self._L.sm_recall_stats(self._h, C.byref(st)), "sm_recall_stats")
        return {k: getattr(st, k) for k, _ in SmRecallStats._fields_}

    def set_auto_recall(self, **params):
        """While set_auto_retire is on: after every retirement, move back the records of its files within `radius` of that
        frame's pose (sm_set_auto_recall; 0 < radius <= min_distance).  No params or radius <= 0: off."""
        p = SmRecallParams(float(params["radius"])) if params else None
        if params and set(params) != {"radius"}:
            raise KeyError(sorted(set(params) - {"radius"}))
        self._chk(self._L.sm_set_auto_recall(self._h, C.byref(p) if p is not None else None), "sm_set_auto_recall")

    def auto_recall_stats(self):
        """(recalls the policy has made, surfels they brought back)"""
        r, n = C.c_uint32(), C.c_uint64()
        self._chk(self._L.sm_auto_recall_stats(self._h, C.byref(r), C.byref(n)), "sm_auto_recall_stats")
        return int(r.value), int(n.value)

    # -- closing loops (sm_warp_by_time)
    def warp_by_time(self, paths, t0, corr, include_model=True):
        """Move every surfel whose last-update time tau is >= t0 by row min(int(tau - t0), n - 1) of `corr` (float32[n][12], each
        row a row-major 3x4 world->world [R|t]): the records of the map files `paths` (rewritten in place where a row moved)
        and, with include_model, the live model and the context's stored poses (sm_warp_by_time)."""
        corr = np.ascontiguousarray(corr, np.float32).reshape(-1, 12)
        src = map_source(paths, include_model=include_model)
        self._chk(self._L.sm_warp_by_time(self._h, C.byref(src), int(t0), len(corr), _ptr(corr)), "sm_warp_by_time")

    def warp_stats(self) -> dict:
        """of the last warp_by_time: files_listed, files_skipped (by the file index), files_read, files_rewritten, records_read,
        records_moved, model_moved, chunks, read_ms, copy_ms, device_ms, write_ms, total_ms"""
        st = SmWarpStats()
        self._chk(self._L.sm_warp_stats(self._h, C.byref(st)), "sm_warp_stats")
        return {k: getattr(st, k) for k, _ in SmWarpStats._fields_}

    def track_old(self, depth, max_time, guess=None, **params):
        """track() against the map as it was: the prediction holds only surfels last updated at or before max_time
        (sm_track_frame_old).  Returns (pose, info) as track(), with info["anchor_time"] = the newest time the prediction holds
        (-1: none)."""
        return self._track_frame("sm_track_frame_old", depth, guess, params, window=(max_time,))

    def track_debug_old(self, depth, pose_eval, max_time):
        """track_debug() with track_old()'s window (sm_track_debug_old)"""
        return self._track_debug("sm_track_debug_old", depth, pose_eval, max_time)

    def _close_loop(self, rgb, depth, pose, paths, search, params, place=None):
        """close_loop() (rgb None) and close_loop_rgb(): sm_close_loop_at with `place`, sm_close_loop_search with `search`, else
        sm_close_loop / sm_close_loop_rgb"""
        depth, rgb = self._images(depth, rgb)
        loop_keys = {n for n, _ in SmLoopParams._fields_}
        lp = loop_params(self.cfg, **{k: v for k, v in params.items() if k in loop_keys})
        tp, rp = self._split_params({k: v for k, v in params.items() if k not in loop_keys}, colour=rgb is not None)
        src = map_source(paths, include_model=True)
        g = _mat16(pose)
        out = np.zeros(16, np.float32)
        info = SmLoopInfo()
        sp = _search_arg(search)
        if place is not None:
            pl = _mat16(place)
            self._chk(self._L.sm_close_loop_at(self._h, _ptr(rgb), _ptr(depth), _ptr(g), _ptr(pl), src, tp, rp, lp, sp, _ptr(out), info),
                      "sm_close_loop_at")
        elif sp is not None:
            self._chk(self._L.sm_close_loop_search(self._h, _ptr(rgb), _ptr(depth), _ptr(g), src, tp, rp, lp, sp, _ptr(out), info),
                      "sm_close_loop_search")
        elif rgb is not None:
            self._chk(self._L.sm_close_loop_rgb(self._h, _ptr(rgb), _ptr(depth), _ptr(g), src, tp, rp, lp, _ptr(out), info), "sm_close_loop_rgb")
        else:
            self._chk(self._L.sm_close_loop(self._h, _ptr(depth), _ptr(g), src, tp, lp, _ptr(out), info), "sm_close_loop")
        return out.reshape(4, 4).T.copy(), _loop_info_dict(info)

    def close_loop(self, depth, pose, paths=(), search=None, place=None, **params):
        """Notice that the camera is back in mapped territory and pull the map straight (sm_close_loop).  pose: where the caller
        believes the camera is (4x4 camera->world or float32[16] column-major); paths: the map files that move with the model.
        params: fields of sm_loop_params (min_age, min_trans, min_rot_deg, max_trans, max_rot_deg) and of sm_track_params.
        search: True or a dict of search_params() overrides measures the loop by a pose search around `pose` instead of a single
        track from it (sm_close_loop_search), which reaches metres of drift.  place: a pose (a matched keyframe's, fern_match) at
        which the search is centred and its prediction drawn instead (sm_close_loop_at; search then only sets its parameters).
        Returns (pose 4x4: corrected if status is "CLOSED", else as given; info dict: status (name), status_code, track (as
        track()'s info), D 4x4, t_a, t_b)."""
        return self._close_loop(None, depth, pose, paths, search, params, place)

    # -- closing loops unasked (sm_set_auto_loop)
    def old_in_view(self, pose, max_time) -> int:
        """how many live surfels last updated at or before max_time pass the tracker's prediction gates at `pose` (sm_old_in_view)"""
        g = _mat16(pose)
        n = C.c_uint32()
        self._chk(self._L.sm_old_in_view(self._h, _ptr(g), int(max_time), C.byref(n)), "sm_old_in_view")
        return int(n.value)

    def census_ms(self):
        """device time in ms of the census kernel of the last old_in_view() made with SM_TRACK_TIMING=1 (sm_debug_census_ms, not
        part of the C-ABI header); None if it was not timed"""
        f = self._L.sm_debug_census_ms
        f.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        ms = C.c_float()
        self._chk(f(self._h, C.byref(ms)), "sm_debug_census_ms")
        return None if ms.value < 0 else float(ms.value)

    def track_window(self, depth, min_time, max_time, guess=None, **params):
        """track() with the prediction held to surfels with min_time < time <= max_time; INT32_MIN / INT32_MAX leave an end open
        (sm_track_frame_window).  Returns (pose, info) as track_old()."""
        return self._track_frame("sm_track_frame_window", depth, guess, params, window=(min_time, max_time))

    def track_debug_window(self, depth, pose_eval, min_time, max_time):
        """track_debug() with track_window()'s window (sm_track_debug_window)"""
        return self._track_debug("sm_track_debug_window", depth, pose_eval, min_time, max_time)

    def track_rgb_window(self, rgb, depth, min_time, max_time, guess=None, **params):
        """track_rgb() with track_window()'s window (sm_track_frame_rgb_window); info with anchor_time added"""
        return self._track_frame("sm_track_frame_rgb_window", depth, guess, params, rgb=np.asarray(rgb), window=(min_time, max_time))

    def track_rgb_debug_window(self, rgb, depth, pose_eval, min_time, max_time, level=0, which=0):
        """track_rgb_debug() with track_window()'s window (sm_track_rgb_debug_window): (pred_slot int32[H][W], sys float64[29])"""
        return self._track_debug("sm_track_rgb_debug_window", depth, pose_eval, level, which, min_time, max_time, rgb=np.asarray(rgb))

    def close_loop_rgb(self, rgb, depth, pose, paths=(), search=None, place=None, **params):
        """close_loop() with the loop measured by the colour tracker as well (sm_close_loop_rgb): params may also name the fields of
        sm_track_rgb_params.  search as close_loop()'s: the search scores with the colour gate.  Returns (pose, info) as
        close_loop()."""
        return self._close_loop(np.asarray(rgb), depth, pose, paths, search, params, place)

    def set_auto_loop(self, paths=(), search=None, **params):
        """Make track() / track_rgb() (and process_frame_tracked*) close loops by themselves (sm_set_auto_loop): they track in the
        young map, count the old surfels in view and, with at least min_old of them, make one close_loop attempt before the
        frame is fused.  paths: the map files that move with the model (those of set_auto_retire are added).  params override
        auto_loop_params(cfg).  Neither paths nor params: off -- so to switch the policy on with every default and no file
        of the caller's, name one default, e.g. set_auto_loop(every=1).  search: True or a dict of search_params() overrides makes
        the attempt a close_loop(search=...) (sm_set_auto_loop_search); every call without it switches the search off."""
        paths = list(paths)
        sp = _search_arg(search)
        if not params and not paths and sp is None:
            self._chk(self._L.sm_set_auto_loop(self._h, None, None), "sm_set_auto_loop")
        else:
            p = auto_loop_params(self.cfg, **params)
            src = map_source(paths, include_model=True)
            self._chk(self._L.sm_set_auto_loop(self._h, C.byref(p), C.byref(src)), "sm_set_auto_loop")
        self._chk(self._L.sm_set_auto_loop_search(self._h, C.byref(sp) if sp is not None else None), "sm_set_auto_loop_search")

    # -- pose search before the tracker (sm_score_poses_window, sm_search_pose)
    def score_poses(self, depth, cands, rgb=None, stride=1, colour_thresh=0.1, min_time=INT32_MIN, max_time=INT32_MAX, **params):
        """How many grid points of `depth` at `stride` the tracker would call inliers under each candidate pose, against the
        prediction of the window (sm_score_poses_window).  cands: float32[n][16] column-major poses, or [n][4][4] matrices (numpy
        row/col indexing).  rgb given: the colour gate |Y_frame - Y_surfel| <= colour_thresh as well.  params: fields of
        sm_track_params (pixel_stride is not used).  Returns uint32[n]."""
        depth = np.ascontiguousarray(depth, np.uint16)
        assert depth.size == self.P, depth.shape
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, np.uint8)
            assert rgb.size == self.P * 3, rgb.shape
        c = np.asarray(cands, np.float32)
        if c.ndim == 3:
            c = c.transpose(0, 2, 1)
        c = np.ascontiguousarray(c.reshape(-1, 16))
        p = track_params(**params) if params else None
        scores = np.zeros(len(c), np.uint32)
        self._chk(self._L.sm_score_poses_window(self._h, _ptr(rgb), _ptr(depth), _ptr(c), len(c), C.byref(p) if p is not None else None,
                                                int(stride), float(colour_thresh), int(min_time), int(max_time), _ptr(scores)),
                  "sm_score_poses_window")
        return scores

    def search_pose(self, depth, centre, rgb=None, min_time=INT32_MIN, max_time=INT32_MAX, search=None, pred=None, **params):
        """Find the camera within metres of `centre`: score a grid of poses around it, refine the best, track from the winners
        (sm_search_pose).  search: a dict of search_params() overrides; params: fields of sm_track_params and, with rgb, of
        sm_track_rgb_params.  pred: the pose the prediction is drawn at instead of the last processed frame's (sm_search_pose_at).
        Returns (pose 4x4: the centre unless status is "OK"; info dict: status, status_code, levels_run,
        candidates, best_score, winner_rank, track (as track()'s info), start 4x4, anchor_time, score_ms, total_ms)."""
        depth = np.ascontiguousarray(depth, np.uint16)
        assert depth.size == self.P, depth.shape
        if rgb is not None:
            rgb = np.ascontiguousarray(rgb, np.uint8)
            assert rgb.size == self.P * 3, rgb.shape
        icp = {k: v for k, v in params.items() if k not in self._RGB_KEYS}
        col = {k: v for k, v in params.items() if k in self._RGB_KEYS}
        p = track_params(**icp) if icp else None
        q = track_rgb_params(**col) if col else None
        sp = search_params(**dict(search)) if search else None
        g = _mat16(centre)
        out = np.zeros(16, np.float32)
        info = SmSearchInfo()
        tail = (C.byref(p) if p is not None else None, C.byref(q) if q is not None else None, C.byref(sp) if sp is not None else None,
                int(min_time), int(max_time), _ptr(out), C.byref(info))
        if pred is not None:
            at = _mat16(pred)
            self._chk(self._L.sm_search_pose_at(self._h, _ptr(rgb), _ptr(depth), _ptr(at), _ptr(g), *tail), "sm_search_pose_at")
        else:
            self._chk(self._L.sm_search_pose(self._h, _ptr(rgb), _ptr(depth), _ptr(g), *tail), "sm_search_pose")
        n = int(info.levels_run)
        d = dict(status=TRACK_STATUS.get(info.status, str(info.status)), status_code=int(info.status), levels_run=n,
                 candidates=[int(x) for x in info.candidates[:n]], best_score=[int(x) for x in info.best_score[:n]],
                 winner_rank=int(info.winner_rank), track=_track_info_dict(info.track),
                 start=np.array(info.start[:], np.float32).reshape(4, 4).T.copy(), anchor_time=float(info.anchor_time),
                 score_ms=float(info.score_ms), total_ms=float(info.total_ms))
        return out.reshape(4, 4).T.copy(), d

    # -- place recognition (sm_fern_*)
    def set_ferns(self, on=True, **params):
        """Give the context a fern table for its image size and an empty keyframe database (sm_set_ferns); params override
        fern_params(cfg).  on False: free both."""
        p = fern_params(self.cfg, **params) if on else None
        self._chk(self._L.sm_set_ferns(self._h, C.byref(p) if on else None), "sm_set_ferns")
        self._fern = p

    def _fern_words(self):
        if getattr(self, "_fern", None) is None:
            raise SurfelMapError("fern", SM_E_ARG, "the context has no ferns (set_ferns)")
        return self._fern.n_ferns // 8

    def fern_encode(self, depth, rgb=None) -> np.ndarray:
        """the fern code of a frame, uint32[n_ferns / 8] (sm_fern_encode): depth uint16[H][W] mm, rgb uint8[H][W][3] or None (the
        colour bits are 0 then)"""
        depth, rgb = self._images(depth, rgb)
        code = np.zeros(self._fern_words(), np.uint32)
        self._chk(self._L.sm_fern_encode(self._h, _ptr(rgb), _ptr(depth), _ptr(code)), "sm_fern_encode")
        return code

    def fern_encode_device(self, d_depth: int, d_rgb: int = 0) -> np.ndarray:
        """fern_encode() of images in this context's device memory (sm_fern_encode_device)"""
        code = np.zeros(self._fern_words(), np.uint32)
        self._chk(self._L.sm_fern_encode_device(self._h, d_rgb or None, d_depth, _ptr(code)), "sm_fern_encode_device")
        return code

    def fern_add(self, code, pose, time) -> int:
        """append a keyframe (sm_fern_add): its code, its pose (4x4 or float32[16] column-major) and its time; returns its index"""
        code = np.ascontiguousarray(code, np.uint32)
        assert code.size == self._fern_words(), code.shape
        g = _mat16(pose)
        k = C.c_uint32()
        self._chk(self._L.sm_fern_add(self._h, _ptr(code), _ptr(g), int(time), C.byref(k)), "sm_fern_add")
        return int(k.value)

    def fern_count(self) -> int:
        n = C.c_uint32()
        self._chk(self._L.sm_fern_count(self._h, C.byref(n)), "sm_fern_count")
        return int(n.value)

    def fern_match(self, code, min_time=INT32_MIN, max_time=INT32_MAX, dis_all=False):
        """The keyframe nearest to `code` among those with min_time < time <= max_time (sm_fern_match): (index or -1,
        dissimilarity = ferns whose nibbles differ, 2^32 - 1 with none); with dis_all also uint32[count], every keyframe's."""
        code = np.ascontiguousarray(code, np.uint32)
        assert code.size == self._fern_words(), code.shape
        k, d = C.c_int32(), C.c_uint32()
        every = np.zeros(self.fern_count(), np.uint32) if dis_all else None
        self._chk(self._L.sm_fern_match(self._h, _ptr(code), int(min_time), int(max_time), C.byref(k), C.byref(d), _ptr(every)), "sm_fern_match")
        return (int(k.value), int(d.value), every) if dis_all else (int(k.value), int(d.value))

    def fern_keyframes(self) -> dict:
        """the database (sm_fern_download): codes uint32[n][n_ferns / 8], poses float32[n][16] column-major, times int32[n]"""
        n, w = self.fern_count(), self._fern_words()
        codes, poses, times = np.zeros((n, w), np.uint32), np.zeros((n, 16), np.float32), np.zeros(n, np.int32)
        self._chk(self._L.sm_fern_download(self._h, _ptr(codes), _ptr(poses), _ptr(times)), "sm_fern_download")
        return dict(codes=codes, poses=poses, times=times)

    def fern_save(self, path):
        self._chk(self._L.sm_fern_save(self._h, os.fsencode(path)), "sm_fern_save")

    def fern_load(self, path):
        self._chk(self._L.sm_fern_load(self._h, os.fsencode(path)), "sm_fern_load")

    def place_ms(self):
        """device times in ms of the last fern encode and the last fern match kernel of a context whose set_ferns() ran with
        SM_PLACE_TIMING=1 (sm_debug_place_ms, not part of the C-ABI header); (None, None) if it was not timed"""
        e, m = C.c_float(), C.c_float()
        self._chk(self._L.sm_debug_place_ms(self._h, C.byref(e), C.byref(m)), "sm_debug_place_ms")
        return (None, None) if e.value < 0 else (float(e.value), float(m.value))

    def set_auto_place(self, on=True, **params):
        """Make track() / track_rgb() (and process_frame_tracked*) recognise revisited places by themselves (sm_set_auto_place; needs
        set_ferns first): every tracked frame is encoded and matched against the keyframes, a match with an old keyframe far from
        the tracked pose is verified and closed by close_loop(place=) before the frame is fused, and frames unlike every keyframe
        become keyframes.  params override auto_place_params(cfg).  on False: off."""
        p = auto_place_params(self.cfg, **params) if on else None
        self._chk(self._L.sm_set_auto_place(self._h, C.byref(p) if on else None), "sm_set_auto_place")

    def auto_place_stats(self) -> dict:
        """encoded, added, matched, attempts, closed, none, rejected, failed, no_old_map, last_k, last_dis, and last = the last
        attempt's info as close_loop() returns it (sm_auto_place_stats)"""
        st = SmAutoPlaceStats()
        self._chk(self._L.sm_auto_place_stats(self._h, C.byref(st)), "sm_auto_place_stats")
        d = {k: int(getattr(st, k)) for k, _ in SmAutoPlaceStats._fields_ if k != "last"}
        d["last"] = _loop_info_dict(st.last)
        return d

    # -- stereo depth (sm_stereo_*)
    def set_stereo(self, on=True, **params):
        """Give the context the buffers of the stereo matcher (sm_set_stereo); params override stereo_params(cfg).  on False: free
        them."""
        p = stereo_params(self.cfg, **params) if on else None
        self._chk(self._L.sm_set_stereo(self._h, C.byref(p) if on else None), "sm_set_stereo")
        self._stereo = p

    def _stereo_pair(self, rgb_left, rgb_right):
        rgb_left, rgb_right = np.ascontiguousarray(rgb_left, np.uint8), np.ascontiguousarray(rgb_right, np.uint8)
        assert rgb_left.shape == rgb_right.shape == (self.H, self.W, 3), (rgb_left.shape, rgb_right.shape)
        return rgb_left, rgb_right

    def stereo_depth(self, rgb_left, rgb_right):
        """The depth image of a rectified pair (sm_stereo_depth): (depth_mm uint16[H][W], 0 = invalid, as process_frame takes it;
        disp16 uint16[H][W], the disparity in sixteenths of a pixel, 0 = invalid).  rgb_* uint8[H][W][3]."""
        rgb_left, rgb_right = self._stereo_pair(rgb_left, rgb_right)
        depth, disp = np.zeros((self.H, self.W), np.uint16), np.zeros((self.H, self.W), np.uint16)
        self._chk(self._L.sm_stereo_depth(self._h, _ptr(rgb_left), _ptr(rgb_right), _ptr(depth), _ptr(disp)), "sm_stereo_depth")
        return depth, disp

    def stereo_depth_device(self, d_left: int, d_right: int, d_depth: int, d_disp: int = 0):
        """stereo_depth() of images in this context's device memory into device buffers of the caller's (sm_stereo_depth_device):
        enqueued on the context's stream, not waited for"""
        self._chk(self._L.sm_stereo_depth_device(self._h, d_left or None, d_right or None, d_depth or None, d_disp or None),
                  "sm_stereo_depth_device")

    def stereo_debug(self) -> dict:
        """the intermediates of the last stereo call (sm_stereo_download): census_left, census_right uint64[H][W], volume
        uint16[H][W][D]"""
        if getattr(self, "_stereo", None) is None:
            raise SurfelMapError("sm_stereo_download", SM_E_ARG, "the context has no stereo (set_stereo)")
        H, W, D = self.H, self.W, int(self._stereo.max_disp)
        cl, cr, vol = np.zeros((H, W), np.uint64), np.zeros((H, W), np.uint64), np.zeros((H, W, D), np.uint16)
        self._chk(self._L.sm_stereo_download(self._h, _ptr(cl), _ptr(cr), _ptr(vol)), "sm_stereo_download")
        return dict(census_left=cl, census_right=cr, volume=vol)

    def stereo_ms(self):
        """Device times in ms of the kernels of the last stereo call of a context whose set_stereo() ran with SM_STEREO_TIMING=1
        (sm_debug_stereo_ms, not part of the C-ABI header): dict(census, cost, paths=[one per direction], select); None if it was
        not timed."""
        ms = (C.c_float * 11)()
        self._chk(self._L.sm_debug_stereo_ms(self._h, ms), "sm_debug_stereo_ms")
        if ms[0] < 0:
            return None
        return dict(census=float(ms[0]), cost=float(ms[1]), paths=[float(v) for v in ms[2:10] if v >= 0], select=float(ms[10]))

    def process_frame_stereo(self, rgb_left, rgb_right, sem, pose):
        """process_frame() with the depth estimated from the pair: the images are uploaded, sm_stereo_depth_device and
        sm_process_frame_device are enqueued one after the other, and the depth never leaves the device.  sem None: the previous
        class image stays.  The four device images it stages in are allocated by the first call and live as long as the context."""
        rgb_left, rgb_right = self._stereo_pair(rgb_left, rgb_right)
        if getattr(self, "_stereo_dev", None) is None:
            P = self.P
            self._stereo_dev = [self.device_alloc(P * 3), self.device_alloc(P * 3), self.device_alloc(P * 2), self.device_alloc(P)]
        d_left, d_right, d_depth, d_sem = self._stereo_dev
        self.device_upload(d_left, rgb_left)
        self.device_upload(d_right, rgb_right)
        if sem is not None:
            self.device_upload(d_sem, np.ascontiguousarray(sem, np.uint8))
        self.stereo_depth_device(d_left, d_right, d_depth)
        return self.process_frame_device(d_left, d_depth, d_sem if sem is not None else None, pose)

    def auto_loop_stats(self) -> dict:
        """checked, attempts, closed, none, rejected, failed, no_old_map, last_census, and last = the last attempt's info as
        close_loop() returns it (sm_auto_loop_stats)"""
        st = SmAutoLoopStats()
        self._chk(self._L.sm_auto_loop_stats(self._h, C.byref(st)), "sm_auto_loop_stats")
        d = {k: int(getattr(st, k)) for k, _ in SmAutoLoopStats._fields_ if k != "last"}
        d["last"] = _loop_info_dict(st.last)
        return d

    # -- IndexMap
    def download_index_map(self):
        P = self.P
        idx = np.zeros(P, np.int32)
        vc = np.zeros((P, 4), np.float32)
        ct = np.zeros((P, 4), np.float32)
        nr = np.zeros((P, 4), np.float32)
        self._chk(self._L.sm_download_index_map(self._h, _ptr(idx), _ptr(vc), _ptr(ct), _ptr(nr)),
                  "sm_download_index_map")
        return idx, vc, ct, nr

    def download_raw_cloud(self) -> np.ndarray:
        """FeedbackBuffer "RAW": the raw camera-frame surfel cloud of the last processed frame, float32 [n][12]."""
        n = C.c_uint32()
        self._chk(self._L.sm_download_raw_cloud(self._h, None, 0, C.byref(n)), "sm_download_raw_cloud")
        out = np.zeros((n.value, 12), np.float32)
        if n.value:
            self._chk(self._L.sm_download_raw_cloud(self._h, _ptr(out), n.value, C.byref(n)), "sm_download_raw_cloud")
        return out

    def download_depth(self, which=TEX_DEPTH_METRIC):
        out = np.zeros((self.H, self.W), np.float32)
        self._chk(self._L.sm_download_depth(self._h, which, _ptr(out)), "sm_download_depth")
        return out

    def render_image(self, view, w, h, fx, fy, cx, cy, fill=None, depth=False, blend=None):
        """Novel view (GlobalModel::renderImage): (bgr uint8[h][w][3], semantic uint8[h][w] = class + 1).  fill (True, a dict of
        overrides or fill_params(...)): the holes are filled (sm_render_image_ex); depth: depth_mm uint16[h][w] comes third.
        blend (True, a dict of overrides or blend_params(...)): bgr is the blend of the visible layer's discs, not the nearest
        disc's colour (sm_render_image_blend; blend_stats())."""
        view = np.ascontiguousarray(view, np.float32)
        bgr = np.zeros((h, w, 3), np.uint8)
        sem = np.zeros((h, w), np.uint8)
        fp = _fill_arg(fill)
        bp = _blend_arg(blend)
        if bp is not None:
            d = np.zeros((h, w), np.uint16) if depth else None
            self._chk(self._L.sm_render_image_blend(self._h, _ptr(view), w, h, fx, fy, cx, cy, C.byref(bp),
                                                    C.byref(fp) if fp is not None else None, _ptr(bgr), _ptr(sem), _ptr(d)),
                      "sm_render_image_blend")
            return (bgr, sem, d) if depth else (bgr, sem)
        if fp is None and not depth:
            self._chk(self._L.sm_render_image(self._h, _ptr(view), w, h, fx, fy, cx, cy, _ptr(bgr), _ptr(sem)), "sm_render_image")
            return bgr, sem
        d = np.zeros((h, w), np.uint16) if depth else None
        self._chk(self._L.sm_render_image_ex(self._h, _ptr(view), w, h, fx, fy, cx, cy, C.byref(fp) if fp is not None else None,
                                             _ptr(bgr), _ptr(sem), _ptr(d)), "sm_render_image_ex")
        return (bgr, sem, d) if depth else (bgr, sem)

    # -- hole filling (sm_fill_*)
    def fill_image(self, bgr, sem, depth_mm=None, fill=None):
        """The completion of images that are already there (sm_fill_image): bgr uint8[H][W][3] or [N][H][W][3], sem uint8[H][W] or
        [N][H][W], depth_mm uint16 likewise or None (every valid pixel then has depth 0).  fill as render_image's (None: the
        defaults).  Returns new arrays: (bgr, sem) or (bgr, sem, depth_mm)."""
        bgr, sem = np.array(bgr, np.uint8, order="C"), np.array(sem, np.uint8, order="C")
        d = None if depth_mm is None else np.array(depth_mm, np.uint16, order="C")
        if sem.ndim not in (2, 3) or bgr.shape != sem.shape + (3,) or (d is not None and d.shape != sem.shape):
            raise SurfelMapError("sm_fill_image", SM_E_ARG, "bgr [..][H][W][3], sem and depth_mm [..][H][W] of one size are expected")
        n = 1 if sem.ndim == 2 else sem.shape[0]
        h, w = sem.shape[-2:]
        fp = _fill_arg(True if fill is None else fill)
        self._chk(self._L.sm_fill_image(self._h, C.byref(fp), w, h, n, _ptr(bgr), _ptr(sem), _ptr(d)), "sm_fill_image")
        return (bgr, sem) if d is None else (bgr, sem, d)

    def fill_image_device(self, d_bgr: int, d_sem: int, d_depth: int, w, h, n=1, fill=None):
        """fill_image() of n images in this context's device memory, in place (sm_fill_image_device; d_depth 0: no depth): enqueued,
        not waited for"""
        fp = _fill_arg(True if fill is None else fill)
        self._chk(self._L.sm_fill_image_device(self._h, C.byref(fp), w, h, n, d_bgr or None, d_sem or None, d_depth or None),
                  "sm_fill_image_device")

    def fill_stats(self) -> dict:
        """of the last call that filled (sm_fill_stats): valid, seen_through, filled, left_empty (pixels, summed over the images),
        launches, device_ms"""
        st = SmFillStats()
        self._chk(self._L.sm_fill_stats(self._h, C.byref(st)), "sm_fill_stats")
        return {k: getattr(st, k) for k, _ in SmFillStats._fields_}

    def blend_stats(self) -> dict:
        """of the last blended call (sm_blend_stats): drawn, contributions, changed (summed over its views), launches, device_ms"""
        st = SmBlendStats()
        self._chk(self._L.sm_blend_stats(self._h, C.byref(st)), "sm_blend_stats")
        return {k: getattr(st, k) for k, _ in SmBlendStats._fields_}

    def render_model(self, mvp, mv_inv, w, h, threshold=0.0, color_type=0, unstable=True, points=False, window=False,
                     time=0, time_delta=0, clear=(0, 0, 0, 0), depth=False, ids=False):
        """The model view (GlobalModel::renderModel, sm_render_model): mvp / mv_inv column-major float32[16] (or 4x4).
        Returns rgba uint8[h][w][4] in GL row order (row 0 = bottom) and, if asked, depth float32[h][w] (1.0 = empty) and
        ids int32[h][w] (AoS row of download_model(), -1 = empty): rgba, or a tuple (rgba, depth?, ids?)."""
        v = model_view(mvp, mv_inv, w, h, threshold, color_type, unstable, points, window, time, time_delta, clear)
        rgba = np.zeros((h, w, 4), np.uint8)
        d = np.zeros((h, w), np.float32) if depth else None
        i = np.zeros((h, w), np.int32) if ids else None
        self._chk(self._L.sm_render_model(self._h, C.byref(v), _ptr(rgba), _ptr(d), _ptr(i)), "sm_render_model")
        if not depth and not ids:
            return rgba
        return (rgba,) + ((d,) if depth else ()) + ((i,) if ids else ())

    def render_model_device(self, mvp, mv_inv, w, h, d_rgba, d_depth=0, d_id=0, threshold=0.0, color_type=0, unstable=True,
                            points=False, window=False, time=0, time_delta=0, clear=(0, 0, 0, 0)):
        """render_model into device memory (raw pointers, e.g. torch tensors' data_ptr(); 0 = not wanted), enqueued on the
        context's stream without waiting (sm_render_model_device)"""
        v = model_view(mvp, mv_inv, w, h, threshold, color_type, unstable, points, window, time, time_delta, clear)
        self._chk(self._L.sm_render_model_device(self._h, C.byref(v), d_rgba or None, d_depth or None, d_id or None),
                  "sm_render_model_device")

    def render_model_stats(self):
        """diagnostic of the last render_model* call (sm_debug_render_model_stats, not part of the C-ABI header): (surfels on the
        overflow path, [splat, overflow, resolve] ms or None unless SM_RENDER_MODEL_TIMING=1 was set for that call)"""
        f = self._L.sm_debug_render_model_stats
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        n, ms = C.c_uint32(), (C.c_float * 3)()
        self._chk(f(self._h, C.byref(n), ms), "sm_debug_render_model_stats")
        return int(n.value), (None if ms[0] < 0 else [float(x) for x in ms])

    # -- views of a map set (sm_render_image_maps, sm_render_model_maps)
    def render_image_maps(self, paths, views, w, h, fx, fy, cx, cy, include_model=True, fill=None, depth=False, blend=None):
        """Novel views of a map set -- the map files `paths` in that order, then (include_model) the live model -- streamed
        through the device without loading it: every view equals render_image() of a model that is their concatenation.
        views: float32[V][16] camera->world poses (column-major, as render_image takes them).  Returns (bgr uint8[V][h][w][3],
        semantic uint8[V][h][w]).  One call reads every file once per batch of views (render_maps_stats()['passes']).  fill and
        depth as render_image's (sm_render_image_maps_ex): depth_mm uint16[V][h][w] comes third.  blend as render_image's
        (sm_render_image_maps_blend): every file is then read twice per batch."""
        views = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        V = views.shape[0]
        bgr = np.zeros((V, h, w, 3), np.uint8)
        sem = np.zeros((V, h, w), np.uint8)
        src = map_source(paths, include_model)
        fp = _fill_arg(fill)
        bp = _blend_arg(blend)
        if bp is not None:
            d = np.zeros((V, h, w), np.uint16) if depth else None
            self._chk(self._L.sm_render_image_maps_blend(self._h, C.byref(src), _ptr(views), V, w, h, fx, fy, cx, cy, C.byref(bp),
                                                         C.byref(fp) if fp is not None else None, _ptr(bgr), _ptr(sem), _ptr(d)),
                      "sm_render_image_maps_blend")
            return (bgr, sem, d) if depth else (bgr, sem)
        if fp is None and not depth:
            self._chk(self._L.sm_render_image_maps(self._h, C.byref(src), _ptr(views), V, w, h, fx, fy, cx, cy, _ptr(bgr), _ptr(sem)),
                      "sm_render_image_maps")
            return bgr, sem
        d = np.zeros((V, h, w), np.uint16) if depth else None
        self._chk(self._L.sm_render_image_maps_ex(self._h, C.byref(src), _ptr(views), V, w, h, fx, fy, cx, cy,
                                                  C.byref(fp) if fp is not None else None, _ptr(bgr), _ptr(sem), _ptr(d)),
                  "sm_render_image_maps_ex")
        return (bgr, sem, d) if depth else (bgr, sem)

    def render_model_maps(self, paths, views, include_model=True, depth=False, ids=False):
        """Model views of a map set (see render_image_maps): `views` is a list of model_view(...) structs -- the arguments of
        render_model per view -- or of dicts of those arguments; all of one width x height.  Returns rgba uint8[V][h][w][4] in
        GL row order and, if asked, depth float32[V][h][w] and ids int32[V][h][w] (position in the concatenation, -1 = empty):
        rgba, or a tuple (rgba, depth?, ids?)."""
        vs = [v if isinstance(v, SmModelView) else model_view(**v) for v in views]
        V = len(vs)
        arr = (SmModelView * max(V, 1))(*vs)
        w, h = (vs[0].width, vs[0].height) if V else (1, 1)
        rgba = np.zeros((V, h, w, 4), np.uint8)
        d = np.zeros((V, h, w), np.float32) if depth else None
        i = np.zeros((V, h, w), np.int32) if ids else None
        src = map_source(paths, include_model)
        self._chk(self._L.sm_render_model_maps(self._h, C.byref(src), arr, V, _ptr(rgba), _ptr(d), _ptr(i)), "sm_render_model_maps")
        if not depth and not ids:
            return rgba
        return (rgba,) + ((d,) if depth else ()) + ((i,) if ids else ())

    def render_maps_stats(self) -> dict:
        """of the last render_*_maps call: surfels_read, chunks, passes, pairs_tested, pairs_skipped ((block of 256 records,
        view) pairs the view test ran on / found outside), read_ms, copy_ms, device_ms, total_ms"""
        st = SmMapsStats()
        self._chk(self._L.sm_render_maps_stats(self._h, C.byref(st)), "sm_render_maps_stats")
        return {k: getattr(st, k) for k, _ in SmMapsStats._fields_}

    # -- lidar sweeps (sm_lidar_sweep, sm_lidar_sweep_maps)
    def lidar_sweep(self, pose, sensor=None) -> dict:
        """What a lidar at `pose` (sensor->world, float32[16] column-major or 4x4) measures in the live model: a dict of
        range float32[n_el][n_az] (0 = no return), id int32 (row of download_model(), -1), rgb uint8[..][3], sem uint8 (class + 1,
        0).  sensor: lidar_sensor(...); None = the default."""
        sensor = lidar_sensor() if sensor is None else sensor
        pose = _mat16(pose)
        out = _lidar_planes((sensor.n_el, sensor.n_az))
        self._chk(self._L.sm_lidar_sweep(self._h, C.byref(sensor), _ptr(pose), *[_ptr(out[k]) for k in ("range", "id", "rgb", "sem")]),
                  "sm_lidar_sweep")
        return out

    def lidar_sweep_maps(self, paths, poses, sensor=None, include_model=True) -> dict:
        """lidar_sweep of a map set (see render_image_maps) from every pose of `poses` (float32[V][16]): the same dict with a
        leading axis V; ids are positions in the concatenation."""
        sensor = lidar_sensor() if sensor is None else sensor
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        V = poses.shape[0]
        out = _lidar_planes((V, sensor.n_el, sensor.n_az))
        src = map_source(paths, include_model)
        self._chk(self._L.sm_lidar_sweep_maps(self._h, C.byref(src), C.byref(sensor), _ptr(poses), V,
                                              *[_ptr(out[k]) for k in ("range", "id", "rgb", "sem")]), "sm_lidar_sweep_maps")
        return out

    def lidar_stats(self) -> dict:
        """of the last lidar_sweep* call: surfels offered, exact tests, wide (surfel, sweep) pairs, blocks_skipped, chunks, passes,
        read_ms, copy_ms, device_ms, total_ms"""
        st = SmLidarStats()
        self._chk(self._L.sm_lidar_stats(self._h, C.byref(st)), "sm_lidar_stats")
        return {k: getattr(st, k) for k, _ in SmLidarStats._fields_}

    # -- ray casts (sm_cast_rays_maps)
    def cast_rays(self, rays, paths=(), include_model=True, cell_mm=250, origin=None, min_conf=0.0, normal=False) -> dict:
        """What the rays float32[n][8] = (origin, t_min, dir, t_max), world frame, hit in the map set `paths` (then, with
        include_model, the live model): a dict of t float32[n] (in units of |dir|; 0 = no return), id int32 (position in the
        concatenation, -1), rgb uint8[n][3], sem uint8 (class + 1, 0) and, with normal, normal float32[n][3] (the record's stored
        normal).  The nearest hitting record per ray, ties to the lower id (sm_cast_rays_maps; tests/rays_ref.py restates the
        rule).  cell_mm and origin shape the voxel index and change nothing in the answer.  An invalid ray returns the empty values."""
        rays = np.ascontiguousarray(rays, np.float32)
        if rays.ndim != 2 or rays.shape[1] != 8:
            raise ValueError("rays: float32[n][8]")
        n = rays.shape[0]
        p = rays_params(cell_mm=cell_mm, origin=(0.0, 0.0, 0.0) if origin is None else origin, min_conf=min_conf)
        src = map_source(paths, include_model)
        out = dict(t=np.zeros(n, np.float32), id=np.full(n, -1, np.int32), rgb=np.zeros((n, 3), np.uint8), sem=np.zeros(n, np.uint8))
        if normal:
            out["normal"] = np.zeros((n, 3), np.float32)
        self._chk(self._L.sm_cast_rays_maps(self._h, C.byref(src), C.byref(p), _ptr(rays), n, *[_ptr(out[k]) for k in ("t", "id", "rgb", "sem")],
                                            _ptr(out["normal"]) if normal else None), "sm_cast_rays_maps")
        return out

    def cast_rays_stats(self) -> dict:
        """of the last cast_rays: rays, bad_rays, records, wide, pairs and cells (of the largest chunk), probes, tests, no_slot, gave_up, chunks,
        files_skipped (always 0), read_ms, copy_ms, index_ms, cast_ms, device_ms, total_ms"""
        st = SmRaysStats()
        self._chk(self._L.sm_cast_rays_stats(self._h, C.byref(st)), "sm_cast_rays_stats")
        return {k: getattr(st, k) for k, _ in SmRaysStats._fields_}

    # -- scenes (sm_render_image_scene, sm_lidar_sweep_scene)
    def render_scene(self, paths, actors, views, w, h, fx, fy, cx, cy, include_model=True, fill=None, depth=False):
        """render_image_maps of a scene: the map set plus `actors`, a list of (path, poses[, present]) -- map files in the actor's
        own frame, each drawn under its pose of the view (float32[V][12] row-major 3x4 or [V][4][4], actor->world) where it is
        present (uint8[V]; None: everywhere).  Every view equals render_image_maps of the set followed by the present actors' files
        moved by sm_warp_by_time's row rule.  Returns (bgr, sem[, depth_mm]) as render_image_maps."""
        views = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        V = views.shape[0]
        bgr = np.zeros((V, h, w, 3), np.uint8)
        sem = np.zeros((V, h, w), np.uint8)
        d = np.zeros((V, h, w), np.uint16) if depth else None
        src = map_source(paths, include_model)
        sc = scene(actors, V)
        fp = _fill_arg(fill)
        self._chk(self._L.sm_render_image_scene(self._h, C.byref(src), C.byref(sc), _ptr(views), V, w, h, fx, fy, cx, cy,
                                                C.byref(fp) if fp is not None else None, _ptr(bgr), _ptr(sem), _ptr(d)),
                  "sm_render_image_scene")
        return (bgr, sem, d) if depth else (bgr, sem)

    def lidar_sweep_scene(self, paths, actors, poses, sensor=None, include_model=True) -> dict:
        """lidar_sweep_maps of a scene (see render_scene; an actor's poses are per sweep): the same dict.  Row r of actor j has
        the id A + off_j + r -- A the static total, off_j the records of the actors before it, present or not."""
        sensor = lidar_sensor() if sensor is None else sensor
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        V = poses.shape[0]
        out = _lidar_planes((V, sensor.n_el, sensor.n_az))
        src = map_source(paths, include_model)
        sc = scene(actors, V)
        self._chk(self._L.sm_lidar_sweep_scene(self._h, C.byref(src), C.byref(sc), C.byref(sensor), _ptr(poses), V,
                                               *[_ptr(out[k]) for k in ("range", "id", "rgb", "sem")]), "sm_lidar_sweep_scene")
        return out

    def scene_stats(self) -> dict:
        """of the last render_scene / lidar_sweep_scene call (sm_scene_stats): actors, files (distinct), records and bytes
        resident, pairs_tested / pairs_skipped ((actor block of 256, view) pairs), load_ms, actor_ms, total_ms"""
        st = SmSceneStats()
        self._chk(self._L.sm_scene_stats(self._h, C.byref(st)), "sm_scene_stats")
        return {k: getattr(st, k) for k, _ in SmSceneStats._fields_}

    # -- simplification (sm_simplify, sm_simplify_maps)
    def simplify(self, **params) -> dict:
        """The live model merged per voxel cell, in place (sm_simplify): records that share a cell of `voxel_mm`, a class and
        (split_normals) a facing direction become one; download_model() then gives the rows tests/simplify_ref.py computes.
        params: the fields of simplify_params().  Returns simplify_stats()."""
        p = simplify_params(**params)
        self._chk(self._L.sm_simplify(self._h, C.byref(p)), "sm_simplify")
        return self.simplify_stats()

    def simplify_maps(self, paths, out_path, include_model=False, **params) -> dict:
        """The simplification of a map set -- the files `paths` in that order, then (include_model) the live model -- written
        as ONE map file to out_path (sm_simplify_maps); sources and model stay as they are.  Returns simplify_stats()."""
        p = simplify_params(**params)
        src = map_source(paths, include_model)
        self._chk(self._L.sm_simplify_maps(self._h, C.byref(src), C.byref(p), os.fsencode(out_path)), "sm_simplify_maps")
        return self.simplify_stats()

    # -- spatial tiling of a map set (sm_tile_maps)
    def tile_maps(self, paths, out_prefix, include_model=False, **params) -> list:
        """The map set -- the files `paths` in that order, then (include_model) the live model -- rewritten as a new set: the same
        records sorted along a Morton curve over a grid of `cell_mm` and cut into files "<out_prefix>_%06u.bin" at the boundaries
        of tiles of cell_mm << tile_shift (sm_tile_maps; tests/tile_ref.py restates it).  Sources and model stay as they are.
        params: the fields of tile_params().  Returns the files written, in order."""
        p = tile_params(**params)
        src = map_source(paths, include_model)
        self._chk(self._L.sm_tile_maps(self._h, C.byref(src), C.byref(p), os.fsencode(out_prefix)), "sm_tile_maps")
        return ["%s_%06d.bin" % (os.fspath(out_prefix), i) for i in range(self.tile_stats()["files_written"])]

    def tile_stats(self) -> dict:
        """of the last tile_maps: records_in, placed, loose, tiles, largest_tile, files_written, readings, chunks, launches,
        sort_passes, device_ms, sort_ms, read_ms, write_ms, total_ms"""
        st = SmTileStats()
        self._chk(self._L.sm_tile_stats(self._h, C.byref(st)), "sm_tile_stats")
        return {k: getattr(st, k) for k, _ in SmTileStats._fields_}

    # -- registration of one map set against another (sm_register_maps)
    def register_maps(self, source_paths, target_paths, guess=None, source_model=False, target_model=False, apply=False, **params):
        """The rigid transform that takes the map set `source_paths` (then, with source_model, the live model) onto the set
        `target_paths` (target_model likewise): voxel-cell ICP, coarse to fine (sm_register_maps).  guess: a 4x4 source-world to
        target-world matrix or float32[16] column-major, None = identity; params: the fields of register_params() -- pass `pivot`,
        a point inside the overlap.  Nothing is changed, unless `apply`: on status "OK" the source FILES are then moved by the
        pose (warp_by_time with t0 = 0 and one row; the live model stays).  Returns (pose 4x4 float32 -- the guess unless status
        is "OK" --, info dict: status (name), status_code, iterations and cells per level (level 0 the finest), inliers, rmse,
        pivot_ratio, samples, stride, applied)."""
        p = register_params(**params)
        src, tgt = map_source(source_paths, include_model=source_model), map_source(target_paths, include_model=target_model)
        g = None if guess is None else _mat16(guess)
        out = np.zeros(16, np.float32)
        info = SmRegisterInfo()
        self._chk(self._L.sm_register_maps(self._h, C.byref(src), C.byref(tgt), _ptr(g), C.byref(p), _ptr(out), C.byref(info)), "sm_register_maps")
        pose = out.reshape(4, 4).T.copy()
        d = dict(status=REGISTER_STATUS.get(info.status, str(info.status)), status_code=int(info.status),
                 iterations=[int(v) for v in info.iterations[:p.levels]], cells=[int(v) for v in info.cells[:p.levels]],
                 inliers=int(info.inliers), rmse=float(info.rmse), pivot_ratio=float(info.pivot_ratio), samples=int(info.samples),
                 stride=int(info.stride), applied=False)
        if apply and info.status == SM_REGISTER_OK and len(source_paths):
            self.warp_by_time(source_paths, 0, pose[:3, :].reshape(1, 12), include_model=False)
            d["applied"] = True
        return pose, d

    def register_debug(self, source_paths, target_paths, pose_eval, level, source_model=False, target_model=False, **params):
        """ONE system of register_maps at pose_eval on `level` (sm_register_debug).  Returns (sys float64[29] in track_debug()'s
        layout, the number of samples, regular or not)."""
        p = register_params(**params)
        src, tgt = map_source(source_paths, include_model=source_model), map_source(target_paths, include_model=target_model)
        pe = _mat16(pose_eval)
        sys29 = np.zeros(29, np.float64)
        n = C.c_uint32()
        self._chk(self._L.sm_register_debug(self._h, C.byref(src), C.byref(tgt), _ptr(pe), int(level), C.byref(p), _ptr(sys29), C.addressof(n)),
                  "sm_register_debug")
        return sys29, int(n.value)

    def register_stats(self) -> dict:
        """of the last register_maps / register_debug: source_records, target_records, chunks, launches, read_ms, table_ms,
        iterate_ms, total_ms"""
        st = SmRegisterStats()
        self._chk(self._L.sm_register_stats(self._h, C.byref(st)), "sm_register_stats")
        return {k: getattr(st, k) for k, _ in SmRegisterStats._fields_}

    # -- segmentation of a map set into connected voxel components (sm_segment_maps)
    def segment_maps(self, paths, include_model=False, labels=True, max_components=1 << 20, out_path=None, **params) -> dict:
        """The records of the map set `paths` (then, with include_model, the live model) grouped into connected components of
        occupied voxel cells (sm_segment_maps; tests/segment_ref.py restates it).  params: the fields of segment_params().
        out_path: the records whose label kind is in write_mask (default: those of numbered components, which with min_records
        N drops every speck of fewer than N records) as one map file, verbatim and in set order.  Nothing else is changed.
        Returns dict(labels: uint32[records] by global id -- a component's number, or SM_SEGMENT_SMALL / SKIPPED / LOOSE -- or None
        with labels=False; components: SEGMENT_COMPONENT[min(components, max_components)], row i for number i (segment_boxes
        gives them in metres); info: records, counts by kind name, counts_by_kind, written, cells, components, small_components,
        largest)."""
        p = segment_params(**params)
        src = map_source(paths, include_model=include_model)
        info = SmSegmentInfo()
        lab = None
        if labels:
            # the records of the set are known from the headers; the live model's count from the context
            n = sum(_map_records(q) for q in paths)
            if include_model:
                live = C.c_uint32()
                self._chk(self._L.sm_download_model_aos(self._h, None, 0, C.byref(live)), "sm_download_model_aos")
                n += live.value
            lab = np.full(n, 0xFFFFFFFF, np.uint32)
        cap = int(max_components)
        rows = np.zeros(cap, SEGMENT_COMPONENT)
        out = None if out_path is None else os.fsencode(out_path)
        self._chk(self._L.sm_segment_maps(self._h, C.byref(src), C.byref(p), _ptr(lab), _ptr(rows) if cap else None, cap, out, C.byref(info)),
                  "sm_segment_maps")
        counts = [int(v) for v in info.counts]
        d = dict(records=int(info.records), counts=dict(zip(SEGMENT_KINDS, counts)), counts_by_kind=counts, written=int(info.written),
                 cells=int(info.cells), components=int(info.components), small_components=int(info.small_components), largest=int(info.largest))
        if lab is not None and len(lab) != d["records"]:
            raise SurfelMapError("segment_maps", SM_E_ARG, "the set changed while it was segmented")
        return dict(labels=lab, components=rows[:min(cap, d["components"])].copy(), info=d)

    def segment_stats(self) -> dict:
        """of the last segment_maps: chunks, launches, readings, read_ms, table_ms, link_ms, label_ms, write_ms, total_ms"""
        st = SmSegmentStats()
        self._chk(self._L.sm_segment_stats(self._h, C.byref(st)), "sm_segment_stats")
        return {k: getattr(st, k) for k, _ in SmSegmentStats._fields_}

    # -- a map set as a triangle mesh (sm_mesh_maps)
    def mesh_maps(self, paths, include_model=False, ply_path=None, max_vertices=None, max_faces=None, **params) -> dict:
        """The surface the records of the map set `paths` (then, with include_model, the live model) lie on, as an indexed triangle
        mesh: one plane per occupied voxel cell, a signed field at the lattice points, marching tetrahedra (sm_mesh_maps;
        tests/mesh_ref.py restates it).  params: the fields of mesh_params().  ply_path: the mesh as a binary PLY (read_ply reads it
        back).  max_vertices / max_faces: rows to bring back; None: all of them, for which the set is first read once more to
        count them.  Nothing else is changed.  Returns dict(vertices: MESH_VERTEX[..], faces: uint32[.., 3] -- counter-clockwise
        seen from outside, the way the surfel normals point --, info: records, counts by kind name, counts_by_kind, cells,
        lattice_points, cubes, vertices, faces: the totals whatever the caps are)."""
        p = mesh_params(**params)
        src = map_source(paths, include_model=include_model)
        info = SmMeshInfo()
        if max_vertices is None or max_faces is None:
            self._chk(self._L.sm_mesh_maps(self._h, C.byref(src), C.byref(p), None, 0, None, 0, None, C.byref(info)), "sm_mesh_maps")
            max_vertices = info.vertices if max_vertices is None else max_vertices
            max_faces = info.faces if max_faces is None else max_faces
        vcap, fcap = int(max_vertices), int(max_faces)
        vertices, faces = np.zeros(vcap, MESH_VERTEX), np.zeros((fcap, 3), np.uint32)
        out = None if ply_path is None else os.fsencode(ply_path)
        self._chk(self._L.sm_mesh_maps(self._h, C.byref(src), C.byref(p), _ptr(vertices) if vcap else None, vcap, _ptr(faces) if fcap else None, fcap,
                                       out, C.byref(info)), "sm_mesh_maps")
        counts = [int(v) for v in info.counts]
        d = dict(records=int(info.records), counts=dict(zip(MESH_KINDS, counts)), counts_by_kind=counts, cells=int(info.cells),
                 lattice_points=int(info.lattice_points), cubes=int(info.cubes), vertices=int(info.vertices), faces=int(info.faces))
        return dict(vertices=vertices[:min(vcap, d["vertices"])].copy(), faces=faces[:min(fcap, d["faces"])].copy(), info=d)

    def mesh_stats(self) -> dict:
        """of the last mesh_maps: chunks, launches, read_ms, table_ms, field_ms, sort_ms, emit_ms, write_ms, total_ms"""
        st = SmMeshStats()
        self._chk(self._L.sm_mesh_stats(self._h, C.byref(st)), "sm_mesh_stats")
        return {k: getattr(st, k) for k, _ in SmMeshStats._fields_}

    # -- a map set as a planner's ground map (sm_ground_maps)
    def ground_maps(self, paths, include_model=False, planes=GROUND_PLANES, **params) -> dict:
        """A bird's-eye raster of the map set `paths` (then, with include_model, the live model) over the window of nu x nv cells
        of cell_mm at origin (sm_ground_maps; tests/ground_ref.py restates it).  params: the fields of ground_params().  planes:
        those to bring back, the others come as None; without clear2 the distance transform is not run.  Nothing else is changed.
        Returns dict(ground: int32[nv, nu] in 2^-16 m, GROUND_NONE without ground; top: int32[nv, nu], the tallest obstacle above
        the reference height; state: uint8[nv, nu] of GROUND_STATES; cls: uint8[nv, nu], 255 without ground; bgr: uint8[nv, nu, 3];
        clear2: uint32[nv, nu], the squared distance in cells to the nearest blocking cell, at most reach_cells^2; info: records,
        counts by kind name, counts_by_kind, cells by state name, cells_by_state)."""
        p = ground_params(**params)
        unknown = set(planes) - set(GROUND_PLANES)
        if unknown:
            raise KeyError(sorted(unknown))
        src = map_source(paths, include_model=include_model)
        info = SmGroundInfo()
        nu, nv = max(int(p.nu), 0), max(int(p.nv), 0)
        if nu * nv > 1 << 24:                                                 # (refused below: nothing that large is allocated here)
            nu = nv = 0
        kinds = dict(ground=(np.int32, ()), top=(np.int32, ()), state=(np.uint8, ()), cls=(np.uint8, ()), bgr=(np.uint8, (3,)), clear2=(np.uint32, ()))
        out = {k: (np.zeros((nv, nu) + kinds[k][1], kinds[k][0]) if k in planes else None) for k in GROUND_PLANES}
        self._chk(self._L.sm_ground_maps(self._h, C.byref(src), C.byref(p), *[None if out[k] is None else _ptr(out[k]) for k in GROUND_PLANES],
                                         C.byref(info)), "sm_ground_maps")
        counts, cells = [int(v) for v in info.counts], [int(v) for v in info.cells]
        out["info"] = dict(records=int(info.records), counts=dict(zip(GROUND_KINDS, counts)), counts_by_kind=counts,
                           cells=dict(zip(GROUND_STATES, cells)), cells_by_state=cells)
        return out

    def ground_stats(self) -> dict:
        """of the last ground_maps: chunks, launches, files_skipped, read_ms, ground_ms, fill_ms, accumulate_ms, state_ms, clear_ms,
        copy_ms, total_ms"""
        st = SmGroundStats()
        self._chk(self._L.sm_ground_stats(self._h, C.byref(st)), "sm_ground_stats")
        return {k: getattr(st, k) for k, _ in SmGroundStats._fields_}

    # -- change detection between two map sets (sm_compare_maps)
    def compare_maps(self, query_paths, reference_paths, pose=None, query_model=False, reference_model=False, out_path=None, labels=True,
                     **params):
        """Which records of the map set `query_paths` (then, with query_model, the live model) does the set `reference_paths`
        (reference_model likewise) hold the surface of (sm_compare_maps)?  pose: a 4x4 query-world to reference-world matrix or
        float32[16] column-major, None = identity; params: the fields of compare_params().  out_path: the query records whose
        label is in write_mask (default: the CHANGED ones) as one map file, verbatim and in set order.  Nothing else is changed.
        Returns (uint8[query records] of COMPARE_LABEL codes by global id, or None with labels=False; info dict: counts by label
        name, counts_by_code, query_records, reference_records, cells_fine, cells_cover, written)."""
        p = compare_params(**params)
        qry, ref = map_source(query_paths, include_model=query_model), map_source(reference_paths, include_model=reference_model)
        g = None if pose is None else _mat16(pose)
        info = SmCompareInfo()
        lab = None
        if labels:
            # the records of the set are known from the headers; the live model's count from the context
            n = sum(_map_records(q) for q in query_paths)
            if query_model:
                live = C.c_uint32()
                self._chk(self._L.sm_download_model_aos(self._h, None, 0, C.byref(live)), "sm_download_model_aos")
                n += live.value
            lab = np.full(n, 255, np.uint8)
        out = None if out_path is None else os.fsencode(out_path)
        self._chk(self._L.sm_compare_maps(self._h, C.byref(qry), C.byref(ref), _ptr(g), C.byref(p), _ptr(lab), out, C.byref(info)), "sm_compare_maps")
        codes = [int(v) for v in info.counts]
        d = dict(counts={COMPARE_LABEL[l]: codes[l] for l in range(4)}, counts_by_code=codes, query_records=int(info.query_records),
                 reference_records=int(info.reference_records), cells_fine=int(info.cells_fine), cells_cover=int(info.cells_cover),
                 written=int(info.written))
        if lab is not None and len(lab) != d["query_records"]:
            raise SurfelMapError(SM_E_ARG, "compare_maps: the query set changed while it was compared")
        return lab, d

    def diff_maps(self, a_paths, b_paths, pose_a_to_b=None, out_appeared=None, out_vanished=None, **params):
        """What appeared and what vanished between the map sets a (before) and b (after): compare_maps of b against a -- the
        records of b that a does not hold, written to out_appeared -- and of a against b, written to out_vanished.
        pose_a_to_b: a's world to b's (4x4 or float32[16] column-major, None = identity); the first call gets its inverse, taken
        in float64 and rounded to float32.  Returns (info of b against a, info of a against b), each with its `labels`."""
        fwd = None if pose_a_to_b is None else _mat16(pose_a_to_b)
        inv = None if fwd is None else np.linalg.inv(fwd.astype(np.float64).reshape(4, 4).T).astype(np.float32)
        lab_b, appeared = self.compare_maps(b_paths, a_paths, pose=inv, out_path=out_appeared, **params)
        lab_a, vanished = self.compare_maps(a_paths, b_paths, pose=None if fwd is None else fwd, out_path=out_vanished, **params)
        appeared["labels"], vanished["labels"] = lab_b, lab_a
        return appeared, vanished

    def compare_stats(self) -> dict:
        """of the last compare_maps: chunks, launches, read_ms, table_ms, classify_ms, write_ms, total_ms"""
        st = SmCompareStats()
        self._chk(self._L.sm_compare_stats(self._h, C.byref(st)), "sm_compare_stats")
        return {k: getattr(st, k) for k, _ in SmCompareStats._fields_}

    def simplify_stats(self) -> dict:
        """of the last simplify* call: records_in, records_out, cells_merged, loose, largest_cell, chunks, launches, device_ms,
        read_ms, total_ms"""
        st = SmSimplifyStats()
        self._chk(self._L.sm_simplify_stats(self._h, C.byref(st)), "sm_simplify_stats")
        return {k: getattr(st, k) for k, _ in SmSimplifyStats._fields_}

    # -- per-pass entry points
    def set_frame(self, rgb=None, depth_metric=None, sem=None):
        rgb = None if rgb is None else np.ascontiguousarray(rgb, np.uint8)
        dm = None if depth_metric is None else np.ascontiguousarray(depth_metric, np.float32)
        sem = None if sem is None else np.ascontiguousarray(sem, np.uint8)
        self._chk(self._L.sm_set_frame(self._h, _ptr(rgb), _ptr(dm), _ptr(sem)), "sm_set_frame")

    def set_tick(self, tick):
        self._chk(self._L.sm_set_tick(self._h, tick), "sm_set_tick")

    def stage_conflict(self, pose, min_depth, max_depth, fuse_thresh=0.0, is_clean=0):
        pose = np.ascontiguousarray(pose, np.float32)
        self._chk(self._L.sm_stage_conflict(self._h, _ptr(pose), min_depth, max_depth, fuse_thresh, is_clean),
                  "sm_stage_conflict")

    def stage_cull(self):
        self._chk(self._L.sm_stage_cull(self._h), "sm_stage_cull")

    def stage_splat(self, pose, time, depth_cutoff, time_delta):
        pose = np.ascontiguousarray(pose, np.float32)
        self._chk(self._L.sm_stage_splat(self._h, _ptr(pose), time, depth_cutoff, time_delta), "sm_stage_splat")

    def stage_associate_fuse(self, pose, time, dmin, dmax, allow=(0,)):
        pose = np.ascontiguousarray(pose, np.float32)
        return self._chk(self._L.sm_stage_associate_fuse(self._h, _ptr(pose), time, dmin, dmax),
                         "sm_stage_associate_fuse", allow)

    def timings(self) -> dict:
        t = SmTimings()
        self._chk(self._L.sm_stage_timings(self._h, C.byref(t)), "sm_stage_timings")
        return t.as_dict()

    def read_frame_log(self, n: int = FRAME_LOG_LEN) -> np.ndarray:
        """Newest `n` per-frame counter records written by the device (oldest first)."""
        n = min(n, FRAME_LOG_LEN)
        out = np.zeros(n, FRAME_LOG_DTYPE)
        w = C.c_uint32()
        self._chk(self._L.sm_read_frame_log(self._h, _ptr(out), n, C.byref(w)), "sm_read_frame_log")
        return out[:w.value]

    # -- device staging helpers
    def device_alloc(self, nbytes: int) -> int:
        p = self._L.sm_device_alloc(self._h, nbytes)
        if not p:
            raise SurfelMapError("sm_device_alloc", SM_E_HIP, self._L.sm_last_error().decode())
        return p

    def device_free(self, p: int):
        self._chk(self._L.sm_device_free(self._h, p), "sm_device_free")

    def device_upload(self, dst: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._chk(self._L.sm_device_upload(self._h, dst, _ptr(arr), arr.nbytes), "sm_device_upload")

    def export_model_device(self):
        """(device pointer of an AoS float32[n][12] staging copy of the model, n)."""
        p, n = C.c_void_p(), C.c_uint32()
        self._chk(self._L.sm_export_model_device(self._h, C.byref(p), C.byref(n)), "sm_export_model_device")
        return p.value, n.value

    def append_model_device(self, d_ptr: int, n: int):
        self._chk(self._L.sm_append_model_aos_device(self._h, d_ptr, n), "sm_append_model_aos_device")

    def device_download(self, src: int, nbytes: int, dtype=np.uint8) -> np.ndarray:
        out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype)
        self._chk(self._L.sm_device_download(self._h, _ptr(out), src, nbytes), "sm_device_download")
        return out

    # -- ONE stream sharded over several GPUs (slot-addressed; the collectives run on the context's stream; surfelmapping_amd/sharded.py)
    def shard_stream_configure(self, rank, world):
        self._chk(self._L.sm_shard_stream_configure(self._h, rank, world), "sm_shard_stream_configure")

    def shard_set_collective(self, fn):
        """fn(send_ptr, recv_ptr, count_u64, op) -> 0: an all-reduce over the ranks with the meaning of sm_collective_fn"""
        def tramp(user, send, recv, count, op, stream):
            try:
                return int(fn(send, recv, count, op) or 0)
            except Exception as e:                       # never let an exception cross the C frame
                self._coll_error = e
                return SM_E_HIP
        self._coll_cb = COLLECTIVE_FN(tramp)            # keep the trampoline alive as long as the context
        self._chk(self._L.sm_shard_set_collective(self._h, self._coll_cb, None), "sm_shard_set_collective")

    def shard_rccl_init(self, unique_id: bytes):
        _choose_rccl()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self._L.sm_shard_rccl_init(self._h, buf), "sm_shard_rccl_init")

    def shard_rccl_nranks(self) -> int:
        """ranks of this context's RCCL communicator, as RCCL reports them"""
        n = self._L.sm_shard_rccl_nranks(self._h)
        if n < 0:
            raise SurfelMapError("sm_shard_rccl_nranks", n, self._L.sm_last_error().decode())
        return n

    def shard_rccl_finalize(self):
        self._chk(self._L.sm_shard_rccl_finalize(self._h), "sm_shard_rccl_finalize")

    def shard_frame(self, rgb, depth, sem, pose, allow=(0,)):
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = None if depth is None else np.ascontiguousarray(depth, np.uint16)
        sem = None if sem is None else np.ascontiguousarray(sem, np.uint8)
        pose = np.ascontiguousarray(pose, np.float32)
        rc = self._L.sm_shard_frame(self._h, _ptr(rgb), _ptr(depth), _ptr(sem), _ptr(pose))
        if rc and getattr(self, "_coll_error", None) is not None:
            e, self._coll_error = self._coll_error, None
            raise e
        return self._chk(rc, "sm_shard_frame", allow)

    def shard_frame_device(self, d_rgb, d_depth, d_sem, pose):
        pose = np.ascontiguousarray(pose, np.float32)
        return self._chk(self._L.sm_shard_frame_device(self._h, d_rgb, d_depth, d_sem, _ptr(pose)), "sm_shard_frame_device")

    def shard_compact(self):
        self._chk(self._L.sm_shard_compact(self._h), "sm_shard_compact")

    def shard_export_dense_device(self):
        p, n = C.c_void_p(), C.c_uint32()
        self._chk(self._L.sm_shard_export_dense_device(self._h, C.byref(p), C.byref(n)), "sm_shard_export_dense_device")
        return p.value, n.value

    def shard_export_dense(self) -> np.ndarray:
        """this rank's surfels of the compacted union, zeros in the other ranks' slots: (count, 12) float32 (collective)"""
        p, n = self.shard_export_dense_device()
        if n == 0:
            return np.zeros((0, 12), np.float32)
        return self.device_download(p, n * 48, np.float32).reshape(n, 12)

    # -- rig mode (configs[4]): consolidation into a single GlobalModel inside the core
    def rig_configure(self, rank, world):
        self._chk(self._L.sm_rig_configure(self._h, rank, world), "sm_rig_configure")
        self._rig_world = world

    def rig_consolidate(self, depth, sem, pose, sm_global):
        """collective: -> (surfels in the single GlobalModel now appended to `sm_global`, conflicts per view)"""
        depth = np.ascontiguousarray(depth, np.uint16)
        sem = np.ascontiguousarray(sem, np.uint8)
        pose = np.ascontiguousarray(pose, np.float32)
        per_view = (C.c_uint32 * max(getattr(self, "_rig_world", 1), 1))()
        total = C.c_uint32()
        rc = self._L.sm_rig_consolidate(self._h, _ptr(depth), _ptr(sem), _ptr(pose), sm_global._h, per_view, C.byref(total))
        if rc and getattr(self, "_coll_error", None) is not None:
            e, self._coll_error = self._coll_error, None
            raise e
        self._chk(rc, "sm_rig_consolidate")
        return total.value, [int(x) for x in per_view]

    def rig_consolidate_step(self, depth, sem, pose, sm_global):
        """collective, every K frames: -> (new surfels exchanged in this step, surfels in the single GlobalModel `sm_global` after it)"""
        depth = np.ascontiguousarray(depth, np.uint16)
        sem = np.ascontiguousarray(sem, np.uint8)
        pose = np.ascontiguousarray(pose, np.float32)
        new, tot = C.c_uint32(), C.c_uint32()
        rc = self._L.sm_rig_consolidate_step(self._h, _ptr(depth), _ptr(sem), _ptr(pose), sm_global._h, C.byref(new), C.byref(tot))
        if rc and getattr(self, "_coll_error", None) is not None:
            e, self._coll_error = self._coll_error, None
            raise e
        self._chk(rc, "sm_rig_consolidate_step")
        return new.value, tot.value

    def gpu_process_count(self) -> int:
        """processes with compute queues on this context's GPU per the KFD tables (this one included); -1 if unreadable"""
        return self._L.sm_gpu_process_count(self._h)
