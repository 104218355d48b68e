"""ctypes binding of the C-ABI in include/sm_c_api.h (libsurfelmapping_hip.so).

This is plumbing only: every call goes straight to the HIP library.  There is NO CPU
fallback -- if the shared library is missing or no GPU is visible, calls fail loudly.

Three parts, in this order: the header's mirror (constants, structures, record types and ONE table of prototypes), the helpers
(loading, the parameter builders, what the calls share) and SurfelMap.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SM_HIP_LIB") or os.path.join(_PKG, "libsurfelmapping_hip.so")      # (SM_HIP_LIB: another build of the core, for A/B runs)

# =====================================================================================================================
# The header's mirror
# =====================================================================================================================
API_VERSION = 4                # SM_API_VERSION of include/sm_c_api.h

SM_OK, SM_E_ARG, SM_E_CAPACITY, SM_E_UNSUPPORTED, SM_E_HIP, SM_E_NO_DEVICE = 0, -1, -2, -3, -4, -5
TEX_DEPTH_METRIC, TEX_DEPTH_FILTERED, TEX_LAST = 0, 1, 2

SM_COLL_SUM, SM_COLL_MIN, SM_COLL_GATHER = 0, 1, 2
# int fn(void *user, const void *send, void *recv, size_t count_u64, int op, void *hip_stream)
COLLECTIVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
# long long fn(void *user, uint32_t local_conflicts)
CAP_FN = C.CFUNCTYPE(C.c_longlong, C.c_void_p, C.c_uint32)


def _as_dict(st) -> dict:
    """the fields of a structure by name"""
    return {n: getattr(st, n) for n, _ in st._fields_}


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
    as_dict = _as_dict


class SmTimings(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "preprocess", "conflict", "index_map", "data_association", "concatenate", "run",
        "k_prep", "k_conflict", "k_scan_cull", "k_compact", "k_associate", "k_scan_new",
        "k_append")] + [("frames", C.c_uint32), ("event_overhead", C.c_float), ("k_compact_own", C.c_float),
                        ("k_cull_lazy", C.c_float), ("frames_compact", C.c_uint32)] + [(n, C.c_float) for n in (
        "k_surfel_pass", "k_pass_fixup", "k_conflict_own", "k_associate_direct", "k_associate_own", "k_append_own")] + [
        ("frames_one_pass", C.c_uint32), ("frames_direct", C.c_uint32), ("k_assoc_prep", C.c_float), ("k_prep_own", C.c_float),
        ("frames_merged", C.c_uint32), ("frames_assoc_alone", C.c_uint32), ("k_scan_own", C.c_float)]
    as_dict = _as_dict


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


class SmLidarSensor(C.Structure):
    _fields_ = [("n_az", C.c_int32), ("n_el", C.c_int32), ("az0_deg", C.c_float), ("az_step_deg", C.c_float),
                ("el_deg", C.POINTER(C.c_float)), ("min_range", C.c_float), ("max_range", C.c_float), ("min_conf", C.c_float)]


class SmLidarStats(C.Structure):
    _fields_ = [("surfels", C.c_uint64), ("tests", C.c_uint64), ("wide", C.c_uint64), ("blocks_skipped", C.c_uint64),
                ("chunks", C.c_uint32), ("passes", C.c_uint32), ("read_ms", C.c_float), ("copy_ms", C.c_float),
                ("device_ms", C.c_float), ("total_ms", C.c_float)]


LIDAR_MAX_BEAMS = 1 << 22


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


class SmPoint(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("reach", C.c_float)]


class SmPointsParams(C.Structure):
    _fields_ = [("cell_mm", C.c_int32), ("origin", C.c_float * 3), ("min_conf", C.c_float), ("reserved", C.c_int32 * 3)]


class SmPointsStats(C.Structure):
    _fields_ = [("points", C.c_uint64), ("bad_points", C.c_uint64), ("records", C.c_uint64), ("wide", C.c_uint64), ("pairs", C.c_uint64),
                ("cells", C.c_uint64), ("probes", C.c_uint64), ("tests", C.c_uint64), ("no_slot", C.c_uint64), ("gave_up", C.c_uint64),
                ("chunks", C.c_uint32), ("files_skipped", C.c_uint32),
                ("read_ms", C.c_float), ("copy_ms", C.c_float), ("index_ms", C.c_float), ("walk_ms", C.c_float), ("device_ms", C.c_float),
                ("total_ms", C.c_float)]


POINTS_MAX = 1 << 24


class SmSceneActor(C.Structure):
    _fields_ = [("path", C.c_char_p), ("poses12", C.POINTER(C.c_float)), ("present", C.POINTER(C.c_uint8))]


class SmScene(C.Structure):
    _fields_ = [("actors", C.POINTER(SmSceneActor)), ("n_actors", C.c_uint32)]


class SmSceneStats(C.Structure):
    _fields_ = [("actors", C.c_uint32), ("files", C.c_uint32), ("records", C.c_uint64), ("bytes", C.c_uint64),
                ("pairs_tested", C.c_uint64), ("pairs_skipped", C.c_uint64), ("load_ms", C.c_float), ("actor_ms", C.c_float),
                ("total_ms", C.c_float)]


SCENE_MAX_ACTORS, SCENE_MAX_RECORDS = 4096, 1 << 22

SM_TRACK_OK, SM_TRACK_LOST, SM_TRACK_DEGENERATE, SM_TRACK_NO_MODEL = 0, 1, 2, 3
TRACK_STATUS = {SM_TRACK_OK: "OK", SM_TRACK_LOST: "LOST", SM_TRACK_DEGENERATE: "DEGENERATE", SM_TRACK_NO_MODEL: "NO_MODEL"}


class SmTrackParams(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("dist_thresh", C.c_float), ("angle_thresh", C.c_float), ("min_inliers", C.c_int32),
                ("pixel_stride", C.c_int32)]


class SmTrackInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("inliers", C.c_uint32), ("rmse", C.c_float),
                ("guess", C.c_float * 16)]


class SmTrackRgbParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("iters", C.c_int32 * 6), ("rgb_weight", C.c_float), ("rgb_max_residual", C.c_float)]


class SmTrackRgbInfo(C.Structure):
    _fields_ = [("rgb_inliers", C.c_uint32), ("rgb_rmse", C.c_float), ("pivot_ratio", C.c_double),
                ("level_iterations", C.c_int32 * 6)]


class SmRetireParams(C.Structure):
    _fields_ = [("min_age", C.c_int32), ("min_distance", C.c_float)]


SM_RECALL_MOVE, SM_RECALL_COPY, SM_RECALL_COUNT = 0, 1, 2
RECALL_MODE = {"move": SM_RECALL_MOVE, "copy": SM_RECALL_COPY, "count": SM_RECALL_COUNT}


class SmRecallParams(C.Structure):
    _fields_ = [("radius", C.c_float)]


class SmRecallStats(C.Structure):
    _fields_ = [("files_listed", C.c_uint32), ("files_skipped", C.c_uint32), ("files_read", C.c_uint32), ("files_rewritten", C.c_uint32),
                ("records_read", C.c_uint64), ("recalled", C.c_uint64), ("chunks", C.c_uint32), ("read_ms", C.c_float),
                ("copy_ms", C.c_float), ("device_ms", C.c_float), ("write_ms", C.c_float), ("total_ms", C.c_float)]


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


class SmAutoLoopParams(C.Structure):
    _fields_ = [("every", C.c_int32), ("rest", C.c_int32), ("min_old", C.c_uint32), ("loop", SmLoopParams)]


class SmAutoLoopStats(C.Structure):
    _fields_ = [("checked", C.c_uint32), ("attempts", C.c_uint32), ("closed", C.c_uint32), ("none", C.c_uint32),
                ("rejected", C.c_uint32), ("failed", C.c_uint32), ("no_old_map", C.c_uint32), ("last_census", C.c_uint32),
                ("last", SmLoopInfo)]


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


class SmAutoPlaceParams(C.Structure):
    _fields_ = [("every", C.c_int32), ("rest", C.c_int32), ("add_above", C.c_float), ("match_below", C.c_float), ("min_jump", C.c_float),
                ("loop", SmLoopParams), ("search", SmSearchParams)]


class SmAutoPlaceStats(C.Structure):
    _fields_ = [("encoded", C.c_uint32), ("added", C.c_uint32), ("matched", C.c_uint32), ("attempts", C.c_uint32), ("closed", C.c_uint32),
                ("none", C.c_uint32), ("rejected", C.c_uint32), ("failed", C.c_uint32), ("no_old_map", C.c_uint32), ("last_k", C.c_int32),
                ("last_dis", C.c_uint32), ("last", SmLoopInfo)]


class SmStereoParams(C.Structure):
    _fields_ = [("max_disp", C.c_int32), ("paths", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32), ("uniqueness", C.c_int32),
                ("lr_max_diff", C.c_int32), ("baseline", C.c_float)]


class SmLidarDepthParams(C.Structure):
    _fields_ = [("min_z", C.c_float), ("max_z", C.c_float), ("stages", C.c_int32), ("large", C.c_int32), ("tol_256", C.c_int32)]


class SmLidarDepthStats(C.Structure):
    _fields_ = [("points", C.c_uint64), ("landed", C.c_uint64), ("measured", C.c_uint64), ("filled_small", C.c_uint64),
                ("filled_top", C.c_uint64), ("filled_large", C.c_uint64), ("left_empty", C.c_uint64), ("launches", C.c_uint32),
                ("device_ms", C.c_float), ("launch_ms", C.c_float * 12)]


LIDAR_DEPTH_MAX_POINTS = 1 << 24


class SmFillParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("depth_tol_256", C.c_int32), ("through_count", C.c_int32), ("prefer_far", C.c_int32),
                ("min_cover_256", C.c_int32)]


class SmFillStats(C.Structure):
    _fields_ = [("valid", C.c_uint64), ("seen_through", C.c_uint64), ("filled", C.c_uint64), ("left_empty", C.c_uint64),
                ("launches", C.c_uint32), ("device_ms", C.c_float)]


class SmBlendParams(C.Structure):
    _fields_ = [("depth_tol_256", C.c_int32), ("falloff", C.c_int32)]


class SmBlendStats(C.Structure):
    _fields_ = [("drawn", C.c_uint64), ("contributions", C.c_uint64), ("changed", C.c_uint64), ("launches", C.c_uint32),
                ("device_ms", C.c_float)]


class SmSimplifyParams(C.Structure):
    _fields_ = [("voxel_mm", C.c_int32), ("split_normals", C.c_int32), ("origin", C.c_float * 3), ("max_cells", C.c_uint32)]


class SmSimplifyStats(C.Structure):
    _fields_ = [("records_in", C.c_uint64), ("records_out", C.c_uint64), ("cells_merged", C.c_uint64), ("loose", C.c_uint64),
                ("largest_cell", C.c_uint32), ("chunks", C.c_uint32), ("launches", C.c_uint32), ("device_ms", C.c_float),
                ("read_ms", C.c_float), ("total_ms", C.c_float)]


class SmTileParams(C.Structure):
    _fields_ = [("cell_mm", C.c_int32), ("tile_shift", C.c_int32), ("origin", C.c_float * 3), ("max_file_records", C.c_uint32),
                ("max_tiles", C.c_uint32)]


class SmTileStats(C.Structure):
    _fields_ = [("records_in", C.c_uint64), ("placed", C.c_uint64), ("loose", C.c_uint64), ("tiles", C.c_uint32), ("largest_tile", C.c_uint32),
                ("files_written", C.c_uint32), ("readings", C.c_uint32), ("chunks", C.c_uint32), ("launches", C.c_uint32),
                ("sort_passes", C.c_uint32), ("device_ms", C.c_float), ("sort_ms", C.c_float), ("read_ms", C.c_float), ("write_ms", C.c_float),
                ("total_ms", C.c_float)]


class SmPackParams(C.Structure):
    _fields_ = [("pos_step_log2", C.c_int32)]


class SmPackStats(C.Structure):
    _fields_ = [("records", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64), ("files", C.c_uint32), ("blocks", C.c_uint32),
                ("raw_blocks", C.c_uint32), ("chunks", C.c_uint32), ("read_ms", C.c_float), ("copy_ms", C.c_float), ("unpack_ms", C.c_float),
                ("device_ms", C.c_float), ("write_ms", C.c_float), ("total_ms", C.c_float)]


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


ROUTE_NONE = 0xFFFFFFFF                                                  # SM_ROUTE_NONE: `cost` of a cell without a path to a goal
ROUTE_DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))   # (du, dv) of `next` 0..7; 8: a goal, 255: none
ROUTE_PLANES = ("cost", "next")
SM_E_STALL = -6


class SmRouteParams(C.Structure):
    _fields_ = [("nu", C.c_int32), ("nv", C.c_int32), ("body_cells", C.c_int32), ("soft_cells", C.c_int32), ("near_weight", C.c_int32),
                ("unknown_passable", C.c_int32), ("max_steps", C.c_int32), ("rounds_per_check", C.c_int32), ("max_rounds", C.c_int32)]


class SmRouteInfo(C.Structure):
    _fields_ = [("goals_used", C.c_uint32), ("goals_dropped", C.c_uint32), ("reachable", C.c_uint32), ("max_cost", C.c_uint32)]


class SmRouteStats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("launches", C.c_uint32), ("tile_visits", C.c_uint64), ("tile", C.c_uint32), ("sweep_cap", C.c_uint32),
                ("prepare_ms", C.c_float), ("relax_ms", C.c_float), ("next_ms", C.c_float), ("walk_ms", C.c_float), ("copy_ms", C.c_float),
                ("total_ms", C.c_float)]


CAR_MOVES = ("F", "L", "R", "B")                                       # SM_CAR_MOVE_*: `next` 0..3 of route_car; 8: a goal, 255: none


class SmRouteCarParams(C.Structure):
    _fields_ = [("nu", C.c_int32), ("nv", C.c_int32), ("body_cells", C.c_int32), ("soft_cells", C.c_int32), ("near_weight", C.c_int32),
                ("unknown_passable", C.c_int32), ("turn_cells", C.c_int32), ("turn_cost", C.c_int32), ("reverse_weight", C.c_int32),
                ("max_steps", C.c_int32), ("rounds_per_check", C.c_int32), ("max_rounds", C.c_int32)]


class SmRouteCarInfo(C.Structure):
    _fields_ = [("goals_used", C.c_uint32), ("goals_dropped", C.c_uint32), ("reachable_states", C.c_uint32), ("reachable_cells", C.c_uint32),
                ("max_cost", C.c_uint32)]


class SmRouteCarStats(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("launches", C.c_uint32), ("tile_visits", C.c_uint64), ("tile", C.c_uint32), ("sweep_cap", C.c_uint32),
                ("prepare_ms", C.c_float), ("relax_ms", C.c_float), ("next_ms", C.c_float), ("walk_ms", C.c_float), ("copy_ms", C.c_float),
                ("total_ms", C.c_float)]


LOCATE_STATUS =("OK", "AMBIGUOUS", "NONE", "NO_TARGET", "NO_SOURCE")         # SM_LOCATE_*: sm_locate_info.status
LOCATE_KINDS = ("STRUCTURE", "GROUND", "OTHER", "OUTSIDE", "LOOSE")           # the entries of its source_counts / target_counts


class SmLocateParams(C.Structure):
    _fields_ = [("cell_mm", C.c_int32), ("up", C.c_int32), ("origin", C.c_float * 3), ("source_origin", C.c_float * 3), ("nu", C.c_int32),
                ("nv", C.c_int32), ("structure_mask", C.c_uint32 * 8), ("max_up", C.c_int32), ("ground_mask", C.c_uint32 * 8), ("min_up", C.c_int32),
                ("normal_sign", C.c_int32), ("min_records", C.c_uint32), ("dilate", C.c_int32), ("n_yaw", C.c_int32), ("refine", C.c_int32),
                ("sep_yaw", C.c_int32), ("sep_cells", C.c_int32), ("min_ground", C.c_int32), ("min_overlap_256", C.c_int32),
                ("ambiguity_256", C.c_int32), ("max_source_cells", C.c_uint32), ("max_nodes", C.c_uint32)]


class SmLocateInfo(C.Structure):
    _fields_ = [("status", C.c_int32), ("row", C.c_int32), ("du", C.c_int32), ("dv", C.c_int32), ("score", C.c_uint32), ("coarse_k", C.c_int32),
                ("coarse_du", C.c_int32), ("coarse_dv", C.c_int32), ("coarse_score", C.c_uint32), ("runner_up", C.c_uint32), ("n_s", C.c_uint32),
                ("target_cells", C.c_uint32), ("height_pairs", C.c_uint32), ("dh", C.c_int32), ("source_counts", C.c_uint64 * 5),
                ("target_counts", C.c_uint64 * 5)]


class SmLocateStats(C.Structure):
    _fields_ = [("source_records", C.c_uint64), ("target_records", C.c_uint64), ("nodes", C.c_uint64), ("leaves", C.c_uint64), ("chunks", C.c_uint32),
                ("launches", C.c_uint32), ("rounds", C.c_uint32), ("levels", C.c_uint32), ("exhaustive", C.c_uint32), ("range", C.c_uint32),
                ("read_ms", C.c_float), ("raster_ms", C.c_float), ("pyramid_ms", C.c_float), ("search_ms", C.c_float), ("total_ms", C.c_float)]


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


INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

# ---- the prototypes: entry point -> (restype, argtypes), in the header's order.  load() gives every function of the library its row,
# so a NEW ENTRY POINT takes one row here and nothing else; a row reads like the declaration.  An entry point without a row does
# not exist for this module (tests/test_capi_abi.py holds the table against the header: names, parameter counts, return kinds).
P = C.POINTER
vp, cs, sz, ci, cf, i32, u32 = C.c_void_p, C.c_char_p, C.c_size_t, C.c_int, C.c_float, C.c_int32, C.c_uint32
vpp, i32p, u32p, u64p, cfp = P(vp), P(i32), P(u32), P(C.c_uint64), P(cf)
_VIEW = [ci, ci, cf, cf, cf, cf]                                        # w, h, fx, fy, cx, cy
_CFG, _SRC, _TRACK, _RGB, _LOOP, _SEARCH = P(SmConfig), P(SmMapSource), P(SmTrackParams), P(SmTrackRgbParams), P(SmLoopParams), P(SmSearchParams)
_SENSOR, _FILL, _BLEND, _SCENE = P(SmLidarSensor), P(SmFillParams), P(SmBlendParams), P(SmScene)

PROTOTYPES = {
    "sm_api_version": (ci, []),
    "sm_last_error": (cs, []),
    "sm_default_config": (ci, [_CFG] + _VIEW),
    "sm_create": (vp, [_CFG]),
    "sm_destroy": (None, [vp]),
    "sm_process_frame": (ci, [vp, vp, vp, vp, vp]),
    "sm_process_frame_device": (ci, [vp, vp, vp, vp, vp]),
    "sm_process_frame_async": (ci, [vp, vp, vp, vp, vp]),
    "sm_inputs_consumed": (ci, [vp]),
    "sm_host_alloc": (vp, [vp, sz]),
    "sm_host_alloc_frame": (ci, [vp, vpp, vpp, vpp]),
    "sm_host_free": (ci, [vp, vp]),
    "sm_debug_slow_frames": (ci, [vp, u32p]),
    "sm_debug_squeezes": (ci, [vp, u32p, u32p]),
    "sm_sync": (ci, [vp]),
    "sm_clean_points": (ci, [vp, vp, vp, vp]),
    "sm_clean_points_ex": (ci, [vp, vp, vp, vp, ci]),
    "sm_clean_points_cb": (ci, [vp, vp, vp, vp, ci, CAP_FN, vp]),
    "sm_reset": (ci, [vp]),
    "sm_get_counts": (ci, [vp, P(SmCounts)]),
    "sm_download_model_aos": (ci, [vp, vp, u32, u32p]),
    "sm_upload_model_aos": (ci, [vp, vp, u32]),
    "sm_save_map": (ci, [vp, cs, i32, i32]),
    "sm_load_map": (ci, [vp, cs, i32p, i32p]),
    "sm_download_index_map": (ci, [vp, vp, vp, vp, vp]),
    "sm_download_raw_cloud": (ci, [vp, vp, u32, u32p]),
    "sm_download_depth": (ci, [vp, ci, vp]),
    "sm_render_image": (ci, [vp, vp] + _VIEW + [vp, vp]),
    "sm_render_model": (ci, [vp, P(SmModelView), vp, vp, vp]),
    "sm_render_model_device": (ci, [vp, P(SmModelView), vp, vp, vp]),
    "sm_render_image_maps": (ci, [vp, _SRC, vp, u32] + _VIEW + [vp, vp]),
    "sm_render_model_maps": (ci, [vp, _SRC, P(SmModelView), u32, vp, vp, vp]),
    "sm_render_maps_stats": (ci, [vp, P(SmMapsStats)]),
    "sm_set_frame": (ci, [vp, vp, vp, vp]),
    "sm_set_tick": (ci, [vp, i32]),
    "sm_stage_conflict": (ci, [vp, vp, cf, cf, cf, ci]),
    "sm_stage_cull": (ci, [vp]),
    "sm_stage_splat": (ci, [vp, vp, i32, cf, i32]),
    "sm_stage_associate_fuse": (ci, [vp, vp, i32, cf, cf]),
    "sm_stage_timings": (ci, [vp, P(SmTimings)]),
    "sm_read_frame_log": (ci, [vp, vp, u32, u32p]),
    "sm_device_alloc": (vp, [vp, sz]),
    "sm_device_free": (ci, [vp, vp]),
    "sm_device_upload": (ci, [vp, vp, vp, sz]),
    "sm_export_model_device": (ci, [vp, vpp, u32p]),
    "sm_append_model_aos_device": (ci, [vp, vp, u32]),
    "sm_device_download": (ci, [vp, vp, vp, sz]),
    "sm_shard_stream_configure": (ci, [vp, ci, ci]),
    "sm_shard_set_collective": (ci, [vp, COLLECTIVE_FN, vp]),
    "sm_shard_rccl_unique_id": (ci, [vp]),
    "sm_shard_rccl_init": (ci, [vp, vp]),
    "sm_shard_rccl_finalize": (ci, [vp]),
    "sm_shard_rccl_nranks": (ci, [vp]),
    "sm_shard_frame_device": (ci, [vp, vp, vp, vp, vp]),
    "sm_shard_frame": (ci, [vp, vp, vp, vp, vp]),
    "sm_shard_compact": (ci, [vp]),
    "sm_shard_export_dense_device": (ci, [vp, vpp, u32p]),
    "sm_gpu_process_count": (ci, [vp]),
    "sm_rig_configure": (ci, [vp, ci, ci]),
    "sm_rig_consolidate": (ci, [vp, vp, vp, vp, vp, u32p, u32p]),
    "sm_rig_consolidate_step": (ci, [vp, vp, vp, vp, vp, u32p, u32p]),
    "sm_default_track_params": (ci, [_TRACK]),
    "sm_track_frame": (ci, [vp, vp, vp, _TRACK, vp, P(SmTrackInfo)]),
    "sm_track_debug": (ci, [vp, vp, vp, vp, vp]),
    "sm_default_track_rgb_params": (ci, [_RGB]),
    "sm_track_frame_rgb": (ci, [vp, vp, vp, vp, _TRACK, _RGB, vp, P(SmTrackInfo), P(SmTrackRgbInfo)]),
    "sm_track_rgb_debug": (ci, [vp, vp, vp, vp, ci, ci, vp]),
    "sm_default_retire_params": (ci, [_CFG, P(SmRetireParams)]),
    "sm_retire": (ci, [vp, vp, P(SmRetireParams), vp, u32, u32p]),
    "sm_retire_device": (ci, [vp, vp, P(SmRetireParams), vp, u32, u32p]),
    "sm_set_auto_retire": (ci, [vp, P(SmRetireParams), i32, cs]),
    "sm_auto_retire_stats": (ci, [vp, u32p, u64p]),
    "sm_default_recall_params": (ci, [_CFG, P(SmRecallParams)]),
    "sm_recall": (ci, [vp, _SRC, vp, P(SmRecallParams), i32, u32p]),
    "sm_recall_stats": (ci, [vp, P(SmRecallStats)]),
    "sm_set_auto_recall": (ci, [vp, P(SmRecallParams)]),
    "sm_auto_recall_stats": (ci, [vp, u32p, u64p]),
    "sm_warp_by_time": (ci, [vp, _SRC, i32, u32, vp]),
    "sm_warp_stats": (ci, [vp, P(SmWarpStats)]),
    "sm_loop_spread": (ci, [vp, i32, i32, vp]),
    "sm_track_frame_old": (ci, [vp, vp, vp, _TRACK, i32, vp, P(SmTrackInfo), cfp]),
    "sm_track_debug_old": (ci, [vp, vp, vp, i32, vp, vp]),
    "sm_default_loop_params": (ci, [_CFG, _LOOP]),
    "sm_close_loop": (ci, [vp, vp, vp, _SRC, _TRACK, _LOOP, vp, P(SmLoopInfo)]),
    "sm_track_frame_window": (ci, [vp, vp, vp, _TRACK, i32, i32, vp, P(SmTrackInfo), cfp]),
    "sm_track_debug_window": (ci, [vp, vp, vp, i32, i32, vp, vp]),
    "sm_track_frame_rgb_window": (ci, [vp, vp, vp, vp, _TRACK, _RGB, i32, i32, vp, P(SmTrackInfo), P(SmTrackRgbInfo), cfp]),
    "sm_track_rgb_debug_window": (ci, [vp, vp, vp, vp, ci, ci, i32, i32, vp, vp]),
    "sm_close_loop_rgb": (ci, [vp, vp, vp, vp, _SRC, _TRACK, _RGB, _LOOP, vp, P(SmLoopInfo)]),
    "sm_old_in_view": (ci, [vp, vp, i32, u32p]),
    "sm_default_auto_loop_params": (ci, [_CFG, P(SmAutoLoopParams)]),
    "sm_set_auto_loop": (ci, [vp, P(SmAutoLoopParams), _SRC]),
    "sm_auto_loop_stats": (ci, [vp, P(SmAutoLoopStats)]),
    "sm_default_search_params": (ci, [_SEARCH]),
    "sm_score_poses_window": (ci, [vp, vp, vp, vp, u32, _TRACK, i32, cf, i32, i32, vp]),
    "sm_search_pose": (ci, [vp, vp, vp, vp, _TRACK, _RGB, _SEARCH, i32, i32, vp, P(SmSearchInfo)]),
    "sm_close_loop_search": (ci, [vp, vp, vp, vp, _SRC, _TRACK, _RGB, _LOOP, _SEARCH, vp, P(SmLoopInfo)]),
    "sm_set_auto_loop_search": (ci, [vp, _SEARCH]),
    "sm_default_lidar_sensor": (ci, [_SENSOR]),
    "sm_lidar_directions": (ci, [_SENSOR, vp]),
    "sm_lidar_sweep": (ci, [vp, _SENSOR, vp, vp, vp, vp, vp]),
    "sm_lidar_sweep_maps": (ci, [vp, _SRC, _SENSOR, vp, u32, vp, vp, vp, vp]),
    "sm_lidar_stats": (ci, [vp, P(SmLidarStats)]),
    "sm_default_fern_params": (ci, [_CFG, P(SmFernParams)]),
    "sm_fern_table": (ci, [P(SmFernParams), i32, i32, vp]),
    "sm_set_ferns": (ci, [vp, P(SmFernParams)]),
    "sm_fern_encode": (ci, [vp, vp, vp, vp]),
    "sm_fern_encode_device": (ci, [vp, vp, vp, vp]),
    "sm_fern_add": (ci, [vp, vp, vp, i32, u32p]),
    "sm_fern_count": (ci, [vp, u32p]),
    "sm_fern_download": (ci, [vp, vp, vp, vp]),
    "sm_fern_save": (ci, [vp, cs]),
    "sm_fern_load": (ci, [vp, cs]),
    "sm_fern_match": (ci, [vp, vp, i32, i32, i32p, u32p, vp]),
    "sm_search_pose_at": (ci, [vp, vp, vp, vp, vp, _TRACK, _RGB, _SEARCH, i32, i32, vp, P(SmSearchInfo)]),
    "sm_close_loop_at": (ci, [vp, vp, vp, vp, vp, _SRC, _TRACK, _RGB, _LOOP, _SEARCH, vp, P(SmLoopInfo)]),
    "sm_default_auto_place_params": (ci, [_CFG, P(SmAutoPlaceParams)]),
    "sm_set_auto_place": (ci, [vp, P(SmAutoPlaceParams)]),
    "sm_auto_place_stats": (ci, [vp, P(SmAutoPlaceStats)]),
    "sm_default_stereo_params": (ci, [_CFG, P(SmStereoParams)]),
    "sm_set_stereo": (ci, [vp, P(SmStereoParams)]),
    "sm_stereo_depth": (ci, [vp, vp, vp, vp, vp]),
    "sm_stereo_depth_device": (ci, [vp, vp, vp, vp, vp]),
    "sm_stereo_download": (ci, [vp, vp, vp, vp]),
    "sm_default_lidar_depth_params": (ci, [_CFG, P(SmLidarDepthParams)]),
    "sm_set_lidar_depth": (ci, [vp, P(SmLidarDepthParams)]),
    "sm_lidar_depth": (ci, [vp, vp, u32, vp, vp, vp, vp]),
    "sm_lidar_depth_device": (ci, [vp, vp, u32, vp, vp, vp, vp]),
    "sm_lidar_depth_stats": (ci, [vp, P(SmLidarDepthStats)]),
    "sm_default_fill_params": (ci, [_FILL]),
    "sm_fill_image": (ci, [vp, _FILL, ci, ci, u32, vp, vp, vp]),
    "sm_fill_image_device": (ci, [vp, _FILL, ci, ci, u32, vp, vp, vp]),
    "sm_render_image_ex": (ci, [vp, vp] + _VIEW + [_FILL, vp, vp, vp]),
    "sm_render_image_maps_ex": (ci, [vp, _SRC, vp, u32] + _VIEW + [_FILL, vp, vp, vp]),
    "sm_fill_stats": (ci, [vp, P(SmFillStats)]),
    "sm_default_blend_params": (ci, [_BLEND]),
    "sm_render_image_blend": (ci, [vp, vp] + _VIEW + [_BLEND, _FILL, vp, vp, vp]),
    "sm_render_image_maps_blend": (ci, [vp, _SRC, vp, u32] + _VIEW + [_BLEND, _FILL, vp, vp, vp]),
    "sm_blend_stats": (ci, [vp, P(SmBlendStats)]),
    "sm_default_simplify_params": (ci, [P(SmSimplifyParams)]),
    "sm_simplify": (ci, [vp, P(SmSimplifyParams)]),
    "sm_simplify_maps": (ci, [vp, _SRC, P(SmSimplifyParams), cs]),
    "sm_simplify_stats": (ci, [vp, P(SmSimplifyStats)]),
    "sm_default_register_params": (ci, [P(SmRegisterParams)]),
    "sm_register_maps": (ci, [vp, _SRC, _SRC, vp, P(SmRegisterParams), vp, P(SmRegisterInfo)]),
    "sm_register_debug": (ci, [vp, _SRC, _SRC, vp, i32, P(SmRegisterParams), vp, vp]),
    "sm_register_stats": (ci, [vp, P(SmRegisterStats)]),
    "sm_default_compare_params": (ci, [P(SmCompareParams)]),
    "sm_compare_maps": (ci, [vp, _SRC, _SRC, vp, P(SmCompareParams), vp, cs, P(SmCompareInfo)]),
    "sm_compare_stats": (ci, [vp, P(SmCompareStats)]),
    "sm_default_tile_params": (ci, [P(SmTileParams)]),
    "sm_tile_maps": (ci, [vp, _SRC, P(SmTileParams), cs]),
    "sm_tile_stats": (ci, [vp, P(SmTileStats)]),
    "sm_default_pack_params": (ci, [P(SmPackParams)]),
    "sm_pack_maps": (ci, [vp, _SRC, P(SmPackParams), cs]),
    "sm_unpack_maps": (ci, [vp, _SRC, cs]),
    "sm_pack_stats": (ci, [vp, P(SmPackStats)]),
    "sm_default_segment_params": (ci, [P(SmSegmentParams)]),
    "sm_segment_maps": (ci, [vp, _SRC, P(SmSegmentParams), vp, vp, u32, cs, P(SmSegmentInfo)]),
    "sm_segment_stats": (ci, [vp, P(SmSegmentStats)]),
    "sm_default_mesh_params": (ci, [P(SmMeshParams)]),
    "sm_mesh_maps": (ci, [vp, _SRC, P(SmMeshParams), vp, u32, vp, u32, cs, P(SmMeshInfo)]),
    "sm_mesh_stats": (ci, [vp, P(SmMeshStats)]),
    "sm_default_ground_params": (ci, [P(SmGroundParams)]),
    "sm_ground_maps": (ci, [vp, _SRC, P(SmGroundParams)] + [vp] * 6 + [P(SmGroundInfo)]),
    "sm_ground_stats": (ci, [vp, P(SmGroundStats)]),
    "sm_default_route_params": (ci, [P(SmRouteParams)]),
    "sm_route_ground": (ci, [vp, P(SmRouteParams), vp, vp, u32, vp, vp, u32, vp] + [vp] * 5 + [P(SmRouteInfo)]),
    "sm_route_stats": (ci, [vp, P(SmRouteStats)]),
    "sm_default_route_car_params": (ci, [P(SmRouteCarParams)]),
    "sm_route_car": (ci, [vp, P(SmRouteCarParams), vp, vp, u32, vp, vp, u32, vp] + [vp] * 5 + [P(SmRouteCarInfo)]),
    "sm_route_car_stats": (ci, [vp, P(SmRouteCarStats)]),
    "sm_default_locate_params": (ci, [P(SmLocateParams)]),
    "sm_locate_rotations": (ci, [P(SmLocateParams), vp]),
    "sm_locate_maps": (ci, [vp, _SRC, _SRC, P(SmLocateParams), vp, P(SmLocateInfo)]),
    "sm_locate_stats": (ci, [vp, P(SmLocateStats)]),
    "sm_render_image_scene": (ci, [vp, _SRC, _SCENE, vp, u32] + _VIEW + [_FILL, vp, vp, vp]),
    "sm_lidar_sweep_scene": (ci, [vp, _SRC, _SCENE, _SENSOR, vp, u32, vp, vp, vp, vp]),
    "sm_scene_place_rows": (ci, [vp, vp, u32, vp]),
    "sm_scene_stats": (ci, [vp, P(SmSceneStats)]),
    "sm_default_rays_params": (ci, [P(SmRaysParams)]),
    "sm_cast_rays_maps": (ci, [vp, _SRC, P(SmRaysParams), vp, u32, vp, vp, vp, vp, vp]),
    "sm_cast_rays_stats": (ci, [vp, P(SmRaysStats)]),
    "sm_default_points_params": (ci, [P(SmPointsParams)]),
    "sm_query_points_maps": (ci, [vp, _SRC, P(SmPointsParams), vp, u32, vp, vp, vp, vp, vp, vp, vp]),
    "sm_query_points_stats": (ci, [vp, P(SmPointsStats)]),
}
# ---- NOT IN THE HEADER: the diagnostics the library exports beside its C-ABI (timings of the last call of a kind; SurfelMap's
# *_ms / *_stats readers say what each gives).  They are typed and required like the rest, but are no part of SYMBOLS.
DIAGNOSTICS = {
    "sm_debug_track_stats": (ci, [vp, cfp, ci, P(ci)]),
    "sm_debug_track_rgb_stats": (ci, [vp, cfp, P(ci), ci, P(ci)]),
    "sm_debug_retire_stats": (ci, [vp, cfp]),
    "sm_debug_census_ms": (ci, [vp, cfp]),
    "sm_debug_place_ms": (ci, [vp, cfp, cfp]),
    "sm_debug_stereo_ms": (ci, [vp, cfp]),
    "sm_debug_render_model_stats": (ci, [vp, u32p, cfp]),
}
PROTOTYPES.update(DIAGNOSTICS)
SYMBOLS = tuple(k for k in PROTOTYPES if k not in DIAGNOSTICS)    # every extern "C" symbol include/sm_c_api.h declares
del P, vp, cs, sz, ci, cf, i32, u32, vpp, i32p, u32p, u64p, cfp  # (the rows' shorthand is the table's alone)


# =====================================================================================================================
# The helpers
# =====================================================================================================================
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

    def typed(name):
        fn = getattr(L, name)     # AttributeError here = the library does not match the header
        fn.restype, fn.argtypes = PROTOTYPES[name]
        return fn
    if typed("sm_api_version")() != API_VERSION:     # a stale build: the struct layouts above would not match
        raise ImportError(f"{LIB_PATH} has API version {L.sm_api_version()}, this binding expects {API_VERSION}: rebuild it "
                          "(python -c 'import __graft_entry__ as g; g.build()')")
    for name in PROTOTYPES:
        typed(name)
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _mat16(m):
    """float32[16] column-major; a 4x4 matrix (numpy row/col indexing) is converted"""
    a = np.asarray(m, np.float32)
    if a.shape == (4, 4):
        a = a.T
    a = np.ascontiguousarray(a.reshape(16))
    return a


def rccl_unique_id() -> bytes:
    """128-byte RCCL id made by one rank and handed to all (sm_shard_rccl_unique_id)"""
    _choose_rccl()
    L = load()
    buf = C.create_string_buffer(128)
    rc = L.sm_shard_rccl_unique_id(buf)
    if rc:
        raise SurfelMapError("sm_shard_rccl_unique_id", rc, L.sm_last_error().decode())
    return buf.raw


def make_config(width, height, fx, fy, cx, cy, **over) -> SmConfig:
    c = SmConfig()
    load().sm_default_config(C.byref(c), width, height, fx, fy, cx, cy)
    for k, v in over.items():
        if not hasattr(c, k):
            raise KeyError(k)
        setattr(c, k, v)
    return c


# ---- the parameter builders.  _params() is all of them: the defaults of the C side, then the overrides -- a plain field by setattr,
# an unknown key a KeyError, and the keys of the structure's table below (key -> setter(p, key, value)) by their setter.  A NEW
# PARAMETER STRUCTURE takes its public xxx_params() with one call of _params(), and a row of _SPECIAL only if it has such keys.
def _params(struct, default, cfg, over):
    """`struct` filled by the library's `default` function (of the config `cfg`, where it takes one), then overridden by `over`"""
    p = struct()
    getattr(load(), default)(*([] if cfg is None else [C.byref(cfg)]), C.byref(p))
    special = _SPECIAL.get(struct, {})
    for k, v in over.items():
        if k in special:
            special[k](p, k, v)
        elif not hasattr(p, k):
            raise KeyError(k)
        else:
            setattr(p, k, v)
    return p


def _whole(convert):
    """an array field takes a sequence of exactly its length"""
    def set_(p, k, v):
        getattr(p, k)[:] = [convert(x) for x in v]
    return set_


def _leading(convert):
    """an array field takes its leading entries; those the sequence does not name keep their default"""
    def set_(p, k, v):
        a = getattr(p, k)
        for i, x in enumerate(v):
            a[i] = convert(x)
    return set_


def _classes(mask):
    """classes= sets the eight words of the field `mask` from the classes that take part"""
    def set_(p, k, v):
        getattr(p, mask)[:] = segment_class_mask(v)
    return set_


def _inner(field):
    """a field of the nested structure `field`, given by its own name"""
    def set_(p, k, v):
        setattr(getattr(p, field), k, v)
    return set_


def _refused(p, k, v):
    raise KeyError(k)


def _padded3(p, k, v):
    """(rays_params' origin: a shorter sequence is padded with zeros)"""
    setattr(p, k, (C.c_float * 3)(*[float(x) for x in v]))


_ORIGIN = {"origin": _whole(float)}
_SPECIAL = {
    SmRaysParams: {"origin": _padded3},
    SmPointsParams: {"origin": _padded3},
    SmTrackRgbParams: {"iters": _leading(int)},
    SmSearchParams: {k: _leading(float) for k in ("trans_half", "trans_step", "rot_half_deg", "rot_step_deg")},
    SmSimplifyParams: _ORIGIN,
    SmTileParams: _ORIGIN,
    SmCompareParams: _ORIGIN,
    SmRegisterParams: {"origin": _whole(float), "pivot": _whole(float)},
    SmSegmentParams: {"origin": _whole(float), "class_mask": _whole(int), "classes": _classes("class_mask")},
    SmMeshParams: {"origin": _whole(float), "class_mask": _whole(int), "classes": _classes("class_mask")},
    SmGroundParams: {"origin": _whole(float), "ground_mask": _whole(int), "classes": _classes("ground_mask")},
    SmLocateParams: {"origin": _whole(float), "source_origin": _whole(float), "structure_mask": _whole(int), "ground_mask": _whole(int),
                     "structure_classes": _classes("structure_mask"), "ground_classes": _classes("ground_mask")},
    # the fields of sm_loop_params by their own names; `loop` itself is no key
    SmAutoLoopParams: {**{n: _inner("loop") for n, _ in SmLoopParams._fields_}, "loop": _refused},
}
_SPECIAL[SmAutoPlaceParams] = {**_SPECIAL[SmAutoLoopParams], "search": lambda p, k, v: setattr(p, k, search_params(**dict(v)))}


def rays_params(**over) -> SmRaysParams:
    """sm_default_rays_params with fields replaced: cell_mm, origin (three floats), min_conf"""
    return _params(SmRaysParams, "sm_default_rays_params", None, over)


def points_params(**over) -> SmPointsParams:
    """sm_default_points_params with fields replaced: cell_mm, origin (three floats), min_conf"""
    return _params(SmPointsParams, "sm_default_points_params", None, over)


def track_params(**over) -> SmTrackParams:
    """sm_default_track_params with fields overridden (max_iters, dist_thresh, angle_thresh, min_inliers, pixel_stride)"""
    return _params(SmTrackParams, "sm_default_track_params", None, over)


def track_rgb_params(**over) -> SmTrackRgbParams:
    """sm_default_track_rgb_params with fields overridden (levels, iters: a sequence whose index is the level, the levels it
    does not name keep their default; rgb_weight, rgb_max_residual)"""
    return _params(SmTrackRgbParams, "sm_default_track_rgb_params", None, over)


def retire_params(cfg, **over) -> SmRetireParams:
    """sm_default_retire_params of a config (min_age = time_delta, min_distance = 1.5 * far_clip) with fields overridden"""
    return _params(SmRetireParams, "sm_default_retire_params", cfg, over)


def recall_params(cfg, **over) -> SmRecallParams:
    """sm_default_recall_params of a config (radius = 1.5 * far_clip) with fields overridden"""
    return _params(SmRecallParams, "sm_default_recall_params", cfg, over)


def loop_params(cfg, **over) -> SmLoopParams:
    """sm_default_loop_params of a config (min_age = time_delta; 0.02 m, 0.05 deg; 2 m, 10 deg) with fields overridden"""
    return _params(SmLoopParams, "sm_default_loop_params", cfg, over)


def auto_loop_params(cfg, **over) -> SmAutoLoopParams:
    """sm_default_auto_loop_params of a config (every 1, rest 10, min_old 1000, loop = loop_params(cfg)) with fields overridden;
    the fields of sm_loop_params are given by their own names (min_age, max_trans, ...)"""
    return _params(SmAutoLoopParams, "sm_default_auto_loop_params", cfg, over)


def search_params(**over) -> SmSearchParams:
    """sm_default_search_params (2 levels; +-2 m in x and z at 0.25 m, +-3 deg about y at 0.5 deg; refine 4, stride0 8, top_k 4,
    colour_thresh 0.1) with fields overridden; the four per-axis fields take a sequence of three"""
    return _params(SmSearchParams, "sm_default_search_params", None, over)


def auto_place_params(cfg, **over) -> SmAutoPlaceParams:
    """sm_default_auto_place_params (every 1, rest 10, add_above 0.2, match_below 0.3, min_jump 2 m, loop = loop_params(cfg) with
    max_trans 50 and max_rot_deg 45, search = search_params()) with fields overridden: a field of sm_loop_params by its own name,
    search as a dict of search_params() overrides"""
    return _params(SmAutoPlaceParams, "sm_default_auto_place_params", cfg, over)


def fern_params(cfg, **over) -> SmFernParams:
    """sm_default_fern_params (512 ferns, cell 8, seed 1, the config's near and far clip in millimetres) with fields overridden"""
    return _params(SmFernParams, "sm_default_fern_params", cfg, over)


def stereo_params(cfg, **over) -> SmStereoParams:
    """sm_default_stereo_params (D 128, 8 paths, p1 7, p2 86, uniqueness 5 %, lr_max_diff 1, baseline 0.54 m) with fields overridden"""
    return _params(SmStereoParams, "sm_default_stereo_params", cfg, over)


def lidar_depth_params(cfg, **over) -> SmLidarDepthParams:
    """sm_default_lidar_depth_params (min_z 0.5, max_z 65, stages 127, large 31, tol_256 13) with fields overridden"""
    return _params(SmLidarDepthParams, "sm_default_lidar_depth_params", cfg, over)


def fill_params(**over) -> SmFillParams:
    """sm_default_fill_params (levels 3, depth_tol_256 13, through_count 6, prefer_far 1, min_cover_256 64) with fields overridden"""
    return _params(SmFillParams, "sm_default_fill_params", None, over)


def blend_params(**over) -> SmBlendParams:
    """sm_default_blend_params (depth_tol_256 13, falloff 2 = quadratic) with fields overridden"""
    return _params(SmBlendParams, "sm_default_blend_params", None, over)


def default_simplify_params() -> SmSimplifyParams:
    """sm_default_simplify_params: voxel_mm 50, split_normals 1, origin (0, 0, 0), max_cells 1 << 26"""
    return simplify_params()


def simplify_params(**over) -> SmSimplifyParams:
    """default_simplify_params() with fields overridden; origin takes a sequence of three"""
    return _params(SmSimplifyParams, "sm_default_simplify_params", None, over)


def default_tile_params() -> SmTileParams:
    """sm_default_tile_params: cell_mm 200, tile_shift 7, origin (0, 0, 0), max_file_records 1 << 20, max_tiles 1 << 20"""
    return tile_params()


def tile_params(**over) -> SmTileParams:
    """default_tile_params() with fields overridden; origin takes a sequence of three"""
    return _params(SmTileParams, "sm_default_tile_params", None, over)


def pack_params(**over) -> SmPackParams:
    """sm_default_pack_params (pos_step_log2 -10: positions in steps of 2^-10 m) with fields overridden"""
    return _params(SmPackParams, "sm_default_pack_params", None, over)


# the packed map-file format (include/sm_c_api.h "packed map files")
PACK_MAGIC = 0x4B504D53
PACK_DIR = np.dtype([("origin", "<f4", 3), ("time_base", "<f4"), ("init_base", "<f4"), ("flags", "<u4"), ("offset", "<u8")])


def read_packed_map(path):
    """A packed map file decoded on the host, as the GPU decodes it: (rows float32[n, 12], (start_id, end_id), raw bool[n_blocks] --
    the blocks stored verbatim).  ValueError for anything but a whole packed file."""
    data = open(path, "rb").read()
    if len(data) < 32:
        raise ValueError(f"{path} is too short for a packed map file")
    head = np.frombuffer(data, "<u4", 8)
    n, nb, step = int(head[2]), int(head[6]), int(head[5:6].view(np.int32)[0])
    if head[0] != PACK_MAGIC or head[1] != 1 or head[7] != 0 or nb != (n + 255) // 256 or not -14 <= step <= -6 or len(data) < 32 + 32 * nb:
        raise ValueError(f"{path} is not a packed map file")
    d = np.frombuffer(data, PACK_DIR, nb, 32)
    raw = (d["flags"] & 1).astype(bool)
    m = np.minimum(256, n - 256 * np.arange(nb))
    size = np.where(raw, 48, 20) * m
    at = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    if (d["flags"] > 1).any() or (d["offset"] != at[:-1].astype(np.uint64)).any() or len(data) != 32 + 32 * nb + int(at[-1]):
        raise ValueError(f"{path}: the directory of the packed map file and its length disagree")
    rows = np.zeros((n, 12), np.float32)
    down = np.float32(2.0 ** step)
    base = 32 + 32 * nb
    for b in range(nb):
        out = rows[256 * b:256 * b + m[b]]
        if raw[b]:
            out[:] = np.frombuffer(data, "<f4", 12 * int(m[b]), base + int(at[b])).reshape(-1, 12)
            continue
        w = np.frombuffer(data, "<u4", 5 * int(m[b]), base + int(at[b])).reshape(-1, 5)
        q = np.stack([w[:, 0] & 0xFFFF, w[:, 0] >> 16, w[:, 1] & 0xFFFF], axis=1).astype(np.float32)
        out[:, 0:3] = d["origin"][b] + q * down
        out[:, 3] = (w[:, 3] >> 20).astype(np.float32) * np.float32(0.0625)
        out.view(np.uint32)[:, 4] = w[:, 2]
        out[:, 6] = d["init_base"][b] + (w[:, 4] >> 16).astype(np.float32)
        out[:, 7] = d["time_base"][b] + (w[:, 4] & 0xFFFF).astype(np.float32)
        # the normal: the fold in integers on the codes, then one fp32 normalisation
        ui, vi = 2 * (w[:, 3] & 1023).astype(np.int64) - 1023, 2 * ((w[:, 3] >> 10) & 1023).astype(np.int64) - 1023
        zi = 1023 - np.abs(ui) - np.abs(vi)
        t = np.maximum(-zi, 0)
        xi, yi = np.where(ui >= 0, ui - t, ui + t), np.where(vi >= 0, vi - t, vi + t)
        ln = np.sqrt((xi * xi + yi * yi + zi * zi).astype(np.float32))
        out[:, 8], out[:, 9], out[:, 10] = xi.astype(np.float32) / ln, yi.astype(np.float32) / ln, zi.astype(np.float32) / ln
        out[:, 11] = (w[:, 1] >> 16).astype(np.float32) * np.float32(1.0 / 8192)
    return rows, (int(head[3:4].view(np.int32)[0]), int(head[4:5].view(np.int32)[0])), raw


def default_segment_params() -> SmSegmentParams:
    """sm_default_segment_params: voxel_mm 200, connectivity 26, by_class 1, every class, min_records 1, write_mask 1 (the records of
    numbered components), max_cells 1 << 24, origin (0, 0, 0)"""
    return segment_params()


def segment_params(**over) -> SmSegmentParams:
    """default_segment_params() with fields overridden; origin takes a sequence of three, class_mask eight words or an iterable of
    the classes that take part (`classes=` does the latter too)"""
    return _params(SmSegmentParams, "sm_default_segment_params", None, over)


def segment_class_mask(classes) -> list:
    """the eight words of class_mask with the bits of `classes` (0..255) set"""
    words = [0] * 8
    for c in classes:
        if not 0 <= int(c) <= 255:
            raise ValueError(c)
        words[int(c) >> 5] |= 1 << (int(c) & 31)
    return words


def default_mesh_params() -> SmMeshParams:
    """sm_default_mesh_params: voxel_mm 100, reach 2, min_records 1, every class, max_cells 1 << 24, origin (0, 0, 0)"""
    return mesh_params()


def mesh_params(**over) -> SmMeshParams:
    """default_mesh_params() with fields overridden; origin takes a sequence of three, class_mask eight words or an iterable of the
    classes that take part (`classes=` does the latter too)"""
    return _params(SmMeshParams, "sm_default_mesh_params", None, over)


def default_ground_params() -> SmGroundParams:
    """sm_default_ground_params: cell_mm 100, up 3 (-y), origin (0, 0, 0), 256 x 256 cells, min_up 11585 (45 degrees), every class,
    band_mm 200, the body band 150..2000 mm, min_obstacle 2, fill_cells 3, step_mm 150, reach_cells 32, unknown_blocks 0, normal_sign -1
    (normals that point into the surface, as the fusion stores them)"""
    return ground_params()


def locate_params(**over) -> SmLocateParams:
    """sm_default_locate_params with fields overridden; origin and source_origin take a sequence of three, structure_mask and
    ground_mask eight words (`structure_classes=` / `ground_classes=` take an iterable of classes instead)"""
    return _params(SmLocateParams, "sm_default_locate_params", None, over)


def locate_rotations(**over) -> np.ndarray:
    """sm_locate_rotations: int32[n_yaw * refine, 2], row j = (c_j, s_j) in 2^-30 -- the table sm_locate_maps rotates cells with"""
    p = locate_params(**over)
    t = np.zeros((max(int(p.n_yaw), 0) * max(int(p.refine), 0), 2), np.int32)
    rc = load().sm_locate_rotations(C.byref(p), _ptr(t))
    if rc:
        raise SurfelMapError("sm_locate_rotations", rc, load().sm_last_error().decode())
    return t


def ground_params(**over) -> SmGroundParams:
    """default_ground_params() with fields overridden; origin takes a sequence of three, ground_mask eight words or an iterable of
    the classes that may be ground (`classes=` does the latter too)"""
    return _params(SmGroundParams, "sm_default_ground_params", None, over)


def route_params(**over) -> SmRouteParams:
    """sm_default_route_params (256 x 256 cells, body_cells 0, soft_cells 0, near_weight 0, unknown_passable 0, max_steps 4096,
    rounds_per_check 4, max_rounds 65536) with fields overridden"""
    return _params(SmRouteParams, "sm_default_route_params", None, over)


def route_ground(m, ground, goals, starts=None, max_steps=4096, planes=ROUTE_PLANES, **params) -> dict:
    """Cost-to-go fields and paths over a ground map (sm_route_ground; tests/route_ref.py restates it).  m: a SurfelMap, whose stream
    the call runs on.  ground: the dict ground_maps returned, or any dict with `state` uint8[nv, nu] and `clear2` uint32[nv, nu].
    goals: a list of goal sets, each a list of (u, v): one field per set.  starts: (field, u, v) triples whose paths are wanted.
    params: the fields of route_params() (nu and nv are the planes').  planes: which of ROUTE_PLANES to copy back.
    Returns dict(cost: uint32[G, nv, nu], ROUTE_NONE without a path; next: uint8[G, nv, nu], an index of ROUTE_DIRS, 8 at a goal, 255
    without; a plane not asked for is None; info: per field dict(goals_used, goals_dropped, reachable, max_cost); with starts also
    path: uint32[n, max_steps + 1] of cell numbers v * nu + u padded with ROUTE_NONE, path_len, path_cost: uint32[n])."""
    unknown = set(planes) - set(ROUTE_PLANES)
    if unknown:
        raise KeyError(sorted(unknown)[0])
    state = np.ascontiguousarray(ground["state"], np.uint8)
    clear2 = np.ascontiguousarray(ground["clear2"], np.uint32)
    if state.ndim != 2 or clear2.shape != state.shape:
        raise ValueError("route_ground: state and clear2 are planes [nv, nu] of one shape")
    nv, nu = state.shape
    p = route_params(nu=nu, nv=nv, max_steps=max_steps, **params)
    G = len(goals)
    first = np.zeros(G + 1, np.uint32)
    first[1:] = np.cumsum([len(g) for g in goals])
    flat = np.ascontiguousarray([uv for g in goals for uv in g], np.int32).reshape(-1, 2)
    st = np.ascontiguousarray([] if starts is None else starts, np.int32).reshape(-1, 3)
    n = len(st)
    ok = G >= 1 and 1 <= nu * nv and G * nu * nv <= 1 << 26 and 0 <= p.max_steps and n * (p.max_steps + 1) <= 1 << 26   # (else the call refuses)
    out = dict(cost=np.zeros((G, nv, nu), np.uint32) if ok and "cost" in planes else None,
               next=np.zeros((G, nv, nu), np.uint8) if ok and "next" in planes else None)
    if n and ok:
        out.update(path=np.zeros((n, p.max_steps + 1), np.uint32), path_len=np.zeros(n, np.uint32), path_cost=np.zeros(n, np.uint32))
    info = (SmRouteInfo * max(G, 1))()
    m._chk(m._L.sm_route_ground(m._h, C.byref(p), _ptr(state), _ptr(clear2), G, _ptr(first), _ptr(flat) if len(flat) else None, n,
                                _ptr(st) if n else None, _ptr(out["cost"]), _ptr(out["next"]), _ptr(out.get("path")), _ptr(out.get("path_len")),
                                _ptr(out.get("path_cost")), info), "sm_route_ground")
    out["info"] = [_as_dict(info[f]) for f in range(G)]
    return out


def route_stats(m) -> dict:
    """of m's last route_ground: rounds, launches, tile_visits, tile, sweep_cap, prepare_ms, relax_ms, next_ms, walk_ms, copy_ms,
    total_ms (sm_route_stats)"""
    return m._stats(SmRouteStats, "sm_route_stats")


def route_car_params(**over) -> SmRouteCarParams:
    """sm_default_route_car_params (route_params()'s defaults, turn_cells 2, turn_cost 0, reverse_weight 0) with fields overridden"""
    return _params(SmRouteCarParams, "sm_default_route_car_params", None, over)


def route_car(m, ground, goals, starts=None, max_steps=4096, planes=ROUTE_PLANES, **params) -> dict:
    """Cost-to-go over (cell, heading) and paths a car can follow (sm_route_car; tests/car_ref.py restates it).  m, ground, planes: as
    route_ground's.  goals: a list of goal sets, each a list of (u, v, h), h = -1: any heading; one field per set.  starts:
    (field, u, v, h) quadruples whose paths are wanted.  params: the fields of route_car_params() (nu and nv are the planes').
    Returns dict(cost: uint32[G, 8, nv, nu] by heading, ROUTE_NONE without a way to a goal; next: uint8[G, 8, nv, nu], an index of
    CAR_MOVES, 8 at a goal, 255 without; a plane not asked for is None; info: per field dict(goals_used, goals_dropped,
    reachable_states, reachable_cells, max_cost); with starts also path: uint32[n, max_steps + 1] of words (car_path_cells splits
    them) padded with ROUTE_NONE, path_len, path_cost: uint32[n])."""
    unknown = set(planes) - set(ROUTE_PLANES)
    if unknown:
        raise KeyError(sorted(unknown)[0])
    state = np.ascontiguousarray(ground["state"], np.uint8)
    clear2 = np.ascontiguousarray(ground["clear2"], np.uint32)
    if state.ndim != 2 or clear2.shape != state.shape:
        raise ValueError("route_car: state and clear2 are planes [nv, nu] of one shape")
    nv, nu = state.shape
    p = route_car_params(nu=nu, nv=nv, max_steps=max_steps, **params)
    G = len(goals)
    first = np.zeros(G + 1, np.uint32)
    first[1:] = np.cumsum([len(g) for g in goals])
    flat = np.ascontiguousarray([uvh for g in goals for uvh in g], np.int32).reshape(-1, 3)
    st = np.ascontiguousarray([] if starts is None else starts, np.int32).reshape(-1, 4)
    n = len(st)
    ok = G >= 1 and 1 <= nu * nv and G * nu * nv <= 1 << 23 and 0 <= p.max_steps and n * (p.max_steps + 1) <= 1 << 26   # (else the call refuses)
    out = dict(cost=np.zeros((G, 8, nv, nu), np.uint32) if ok and "cost" in planes else None,
               next=np.zeros((G, 8, nv, nu), np.uint8) if ok and "next" in planes else None)
    if n and ok:
        out.update(path=np.zeros((n, p.max_steps + 1), np.uint32), path_len=np.zeros(n, np.uint32), path_cost=np.zeros(n, np.uint32))
    info = (SmRouteCarInfo * max(G, 1))()
    m._chk(m._L.sm_route_car(m._h, C.byref(p), _ptr(state), _ptr(clear2), G, _ptr(first), _ptr(flat) if len(flat) else None, n,
                             _ptr(st) if n else None, _ptr(out["cost"]), _ptr(out["next"]), _ptr(out.get("path")), _ptr(out.get("path_len")),
                             _ptr(out.get("path_cost")), info), "sm_route_car")
    out["info"] = [_as_dict(info[f]) for f in range(G)]
    return out


def route_car_stats(m) -> dict:
    """of m's last route_car: rounds, launches, tile_visits, tile, sweep_cap, prepare_ms, relax_ms, next_ms, walk_ms, copy_ms,
    total_ms (sm_route_car_stats)"""
    return m._stats(SmRouteCarStats, "sm_route_car_stats")


def car_path_cells(path_row):
    """(cell, heading, reverse) of the words of one row of route_car's `path`, the padding dropped: cell = v * nu + u"""
    w = np.asarray(path_row, np.uint32)
    w = w[w != ROUTE_NONE]
    return w & 0x3FFFFF, (w >> 22) & 7, (w >> 25) & 1


def default_register_params() -> SmRegisterParams:
    """sm_default_register_params: voxel_mm 200, levels 3, max_iters 20, min_inliers 1000, angle_thresh 30, reach_cells 1, stride 0
    (from max_samples = 1 << 22), max_cells 1 << 24, origin and pivot (0, 0, 0)"""
    return register_params()


def register_params(**over) -> SmRegisterParams:
    """default_register_params() with fields overridden; origin and pivot take a sequence of three"""
    return _params(SmRegisterParams, "sm_default_register_params", None, over)


def default_compare_params() -> SmCompareParams:
    """sm_default_compare_params: voxel_mm 100, cover_shift 3, reach_cells 2, plane_mm 50, angle_thresh 30, match_class 0,
    write_mask 2 (the CHANGED records), max_cells 1 << 24, origin (0, 0, 0)"""
    return compare_params()


def compare_params(**over) -> SmCompareParams:
    """default_compare_params() with fields overridden; origin takes a sequence of three"""
    return _params(SmCompareParams, "sm_default_compare_params", None, over)


def _fill_arg(fill):
    """what the entry points' `fill` accepts: None (none), True (the defaults), a dict of overrides, or fill_params(...)"""
    if fill is None or fill is False:
        return None
    if fill is True:
        return fill_params()
    return fill if isinstance(fill, SmFillParams) else fill_params(**fill)


def _blend_arg(blend):
    """what the entry points' `blend` accepts: None (none), True (the defaults), a dict of overrides, or blend_params(...)"""
    if blend is None or blend is False:
        return None
    if blend is True:
        return blend_params()
    return blend if isinstance(blend, SmBlendParams) else blend_params(**blend)


def _search_arg(search):
    """close_loop(search=...) / set_auto_loop(search=...): None or False = no search, True = the defaults, a dict = overrides"""
    if search is None or search is False:
        return None
    return search_params(**({} if search is True else dict(search)))


# ---- map sets, sensors, scenes and what else the calls take or give
def map_source(paths, include_model=True) -> SmMapSource:
    """a map set: the files in drawing order, then (include_model) the live model; keeps the path strings alive"""
    enc = [os.fsencode(p) for p in paths]
    arr = (C.c_char_p * max(len(enc), 1))(*enc)
    src = SmMapSource(C.cast(arr, C.POINTER(C.c_char_p)), len(enc), int(bool(include_model)))
    src._keep = (enc, arr)
    return src


def _map_records(path) -> int:
    """the records a well-formed map file of this length holds (12 bytes of header, 48 per record; a packed file: its header's
    count); 0 where there is no file -- the call that reads it reports that"""
    try:
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = np.frombuffer(f.read(12), "<u4")
        if len(head) == 3 and head[0] == PACK_MAGIC and size != 12 + 48 * PACK_MAGIC:
            return int(head[2])
        return max(0, (size - 12) // 48)
    except OSError:
        return 0


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


def sweep_points(range, sensor) -> np.ndarray:
    """The returns of a sweep as a scan for SurfelMap.lidar_depth: float32[N][4] = t*d in the sensor's own frame (the frame of
    lidar_directions' table and of the sweep's pose), one float32 product per component, and a reflectance of 0.  Beams without
    a return (range 0) are left out; the order is the grid's, row-major."""
    t = np.ascontiguousarray(range, np.float32).reshape(-1)
    d = lidar_directions(sensor).reshape(-1, 3)
    if len(t) != len(d):
        raise ValueError("range: not the sensor's grid")
    got = t > 0
    out = np.zeros((int(got.sum()), 4), np.float32)
    out[:, :3] = t[got, None] * d[got]
    return out


def read_velodyne(path) -> np.ndarray:
    """a KITTI velodyne file (float32 x, y, z, reflectance per point, nothing else): float32[N][4]"""
    raw = np.fromfile(path, np.float32)
    if raw.size % 4:
        raise ValueError(f"{path}: not a whole number of 16-byte points")
    return raw.reshape(-1, 4)


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


def body_points(poses16, spheres) -> np.ndarray:
    """A body of spheres under poses as points for SurfelMap.query_points: float32[k * m][4] = (centre, reach), pose-major.  spheres:
    float32[m][4] = (centre in the body frame, radius); poses16: one body->world pose (float32[16] column-major or 4x4) or k of
    them.  Each centre is R * c + t, computed in double (((R0 cx + R1 cy) + R2 cz) + t, terms with a zero coefficient left out, as
    lidar_rays does) and rounded once; the radius is the reach, so id >= 0 in the answer reads "this sphere at this pose touches
    the map".  Needs no context."""
    S = np.asarray(spheres, np.float32)
    if S.ndim != 2 or S.shape[1] != 4:
        raise ValueError("spheres: float32[m][4]")
    P = np.asarray(poses16, np.float32)
    if P.ndim >= 2 and P.shape[-2:] == (4, 4):
        P = np.swapaxes(P, -1, -2)                                        # (numpy row/col indexing -> column-major)
    P = np.ascontiguousarray(P).reshape(-1, 16)
    k, m = P.shape[0], S.shape[0]
    R = P.astype(np.float64).reshape(k, 4, 4)[:, :3, :3]                  # R[j][c][r]: column c, row r of pose j
    c = S[:, 0:3].astype(np.float64)
    term = [np.where(R[:, None, a, :] != 0.0, R[:, None, a, :] * c[None, :, None, a], -0.0) for a in range(3)]
    centre = ((term[0] + term[1]) + term[2]) + P[:, None, 12:15].astype(np.float64)
    out = np.zeros((k, m, 4), np.float32)
    out[:, :, 0:3] = centre.astype(np.float32)
    out[:, :, 3] = S[None, :, 3]
    return out.reshape(k * m, 4)


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


def fern_table(params, width, height) -> np.ndarray:
    """sm_fern_table: the ferns of `params` for an image size, a structured array (x, y, tr, tg, tb, td; uint16).  Host only."""
    L = load()
    out = np.zeros(max(int(params.n_ferns), 0), FERN_DTYPE)
    rc = L.sm_fern_table(C.byref(params), int(width), int(height), _ptr(out))
    if rc != SM_OK:
        raise SurfelMapError("sm_fern_table", rc, L.sm_last_error().decode())
    return out


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


def _view_planes(shape, depth):
    """the outputs of a novel-view call: bgr uint8[shape][3], sem uint8[shape], depth_mm uint16[shape] (None unless depth)"""
    return np.zeros(tuple(shape) + (3,), np.uint8), np.zeros(shape, np.uint8), np.zeros(shape, np.uint16) if depth else None


# =====================================================================================================================
# SurfelMap
# =====================================================================================================================
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

    def _stats(self, struct, getter) -> dict:
        """the fields of a stats structure read through its getter, int getter(ctx, struct *out).  A NEW STATS STRUCTURE takes its
        xxx_stats() with one call of this."""
        st = struct()
        self._chk(getattr(self._L, getter)(self._h, C.byref(st)), getter)
        return _as_dict(st)

    def _row_count(self, fn):
        """how many float32[12] rows the count-then-fetch entry point `fn` holds -- its call without a destination (a c_uint32)"""
        n = C.c_uint32()
        self._chk(getattr(self._L, fn)(self._h, None, 0, C.byref(n)), fn)
        return n

    def _fetch_rows(self, fn, n) -> np.ndarray:
        """... and the n rows themselves"""
        out = np.zeros((n.value, 12), np.float32)
        self._chk(getattr(self._L, fn)(self._h, _ptr(out), n.value, C.byref(n)), fn)
        return out

    def _label_buffer(self, paths, include_model, empty, dtype) -> np.ndarray:
        """the label buffer of a map set, one entry per record, filled with `empty`: the records of the files are known from their
        headers, the live model's count from the context"""
        n = sum(_map_records(q) for q in paths)
        if include_model:
            n += self._row_count("sm_download_model_aos").value
        return np.full(n, empty, dtype)

    def _check_labels(self, lab, records, what, detail):
        """the call has counted the set's records: a label buffer of another length was sized for another set"""
        if lab is not None and len(lab) != records:
            raise SurfelMapError(what, SM_E_ARG, detail)

    def _novel_views(self, stem, head, shape, camera, fill, depth, blend):
        """The novel views of render_image and render_image_maps: the output planes, and the entry point of the family `stem` that
        the arguments ask for -- stem_blend with blend, stem itself with neither fill nor depth, else stem_ex.  head: the arguments
        between the context and camera = (w, h, fx, fy, cx, cy).  Returns (bgr, sem) or (bgr, sem, depth_mm)."""
        bgr, sem, d = _view_planes(shape, depth)
        fp, bp = _fill_arg(fill), _blend_arg(blend)
        fill_ref = C.byref(fp) if fp is not None else None
        if bp is not None:
            fn, tail = stem + "_blend", (C.byref(bp), fill_ref, _ptr(bgr), _ptr(sem), _ptr(d))
        elif fp is None and not depth:
            fn, tail = stem, (_ptr(bgr), _ptr(sem))
        else:
            fn, tail = stem + "_ex", (fill_ref, _ptr(bgr), _ptr(sem), _ptr(d))
        self._chk(getattr(self._L, fn)(self._h, *head, *camera, *tail), fn)
        return (bgr, sem, d) if depth else (bgr, sem)

    def _lidar_sweep(self, fn, shape, *head) -> dict:
        """the sweep calls: the four output planes of `shape`, filled by `fn`(ctx, *head, range, id, rgb, sem)"""
        out = dict(range=np.zeros(shape, np.float32), id=np.zeros(shape, np.int32), rgb=np.zeros(tuple(shape) + (3,), np.uint8),
                   sem=np.zeros(shape, np.uint8))
        self._chk(getattr(self._L, fn)(self._h, *head, *[_ptr(out[k]) for k in ("range", "id", "rgb", "sem")]), fn)
        return out

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
        """process_frame() of images in this context's device memory, enqueued and not waited for (sm_process_frame_device).
        d_depth / d_sem None (or 0): the current image stays, whichever call gave it.  One given here becomes the current image
        in the caller's buffer, without a copy: if a later call passes None for it, the buffer must stay allocated and unchanged
        until another depth (or class) image has been given or the context is closed."""
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
        ms, n = (C.c_float * 256)(), C.c_int()
        self._chk(self._L.sm_debug_track_stats(self._h, ms, 256, C.byref(n)), "sm_debug_track_stats")
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
        ms, kind, n = (C.c_float * 512)(), (C.c_int * 512)(), C.c_int()
        self._chk(self._L.sm_debug_track_rgb_stats(self._h, ms, kind, 512, C.byref(n)), "sm_debug_track_rgb_stats")
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
        return self._fetch_rows("sm_download_model_aos", self._row_count("sm_download_model_aos"))

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
        ms = (C.c_float * 5)()
        self._chk(self._L.sm_debug_retire_stats(self._h, ms), "sm_debug_retire_stats")
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
        return self._stats(SmRecallStats, "sm_recall_stats")

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
        return self._stats(SmWarpStats, "sm_warp_stats")

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
        ms = C.c_float()
        self._chk(self._L.sm_debug_census_ms(self._h, C.byref(ms)), "sm_debug_census_ms")
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
        sm_process_frame_device are enqueued one after the other, and the depth never leaves the device.  sem None: the current
        class image stays, whichever call gave it.  The four device images it stages in are allocated by the first call and live
        as long as the context, so the depth and the class image given here stay readable as the current ones for later calls
        that pass None (a later stereo frame rewrites them in place, on the context's stream: after every frame enqueued so far)."""
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

    # -- lidar depth (sm_lidar_depth*)
    def set_lidar_depth(self, on=True, **params):
        """Give the context the planes of the lidar depth stage (sm_set_lidar_depth); params override lidar_depth_params(cfg).  on
        False: free them."""
        p = lidar_depth_params(self.cfg, **params) if on else None
        self._chk(self._L.sm_set_lidar_depth(self._h, C.byref(p) if on else None), "sm_set_lidar_depth")

    @staticmethod
    def _scan(points, T):
        points = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
        T = np.ascontiguousarray(T, np.float32).reshape(-1)
        assert T.size in (12, 16), T.shape
        return points, np.concatenate([T, np.array([0, 0, 0, 1], np.float32)])[:16]

    def lidar_depth(self, points, T):
        """The depth image of a scan (sm_lidar_depth): (depth_mm uint16[H][W], completed, 0 = empty, as process_frame takes it;
        sparse_mm uint16[H][W], the z-buffered points alone; index int32[H][W], the row of `points` each measured pixel shows,
        -1).  points float32[N][4] (x, y, z, reflectance); T the lidar->camera transform, row-major 4 x 4 or 3 x 4."""
        points, T = self._scan(points, T)
        depth, sparse = np.zeros((self.H, self.W), np.uint16), np.zeros((self.H, self.W), np.uint16)
        index = np.zeros((self.H, self.W), np.int32)
        self._chk(self._L.sm_lidar_depth(self._h, _ptr(points) if len(points) else None, len(points), _ptr(T), _ptr(depth),
                                         _ptr(sparse), _ptr(index)), "sm_lidar_depth")
        return depth, sparse, index

    def lidar_depth_device(self, d_points: int, n: int, T, d_depth: int, d_sparse: int = 0, d_index: int = 0):
        """lidar_depth() of a scan in this context's device memory into device buffers of the caller's (sm_lidar_depth_device):
        enqueued on the context's stream, not waited for.  T is on the host."""
        T = self._scan(np.zeros((0, 4), np.float32), T)[1]
        self._chk(self._L.sm_lidar_depth_device(self._h, d_points or None, n, _ptr(T), d_depth or None, d_sparse or None,
                                                d_index or None), "sm_lidar_depth_device")

    def lidar_depth_stats(self) -> dict:
        """of the last lidar_depth call: points, landed, measured, filled_small, filled_top, filled_large, left_empty, launches,
        device_ms, launch_ms (a list of twelve, of which the default form uses four; -1 unless SM_LIDAR_DEPTH_TIMING=1 was set at
        set_lidar_depth)"""
        d = self._stats(SmLidarDepthStats, "sm_lidar_depth_stats")
        d["launch_ms"] = [float(v) for v in d["launch_ms"]]
        return d

    def process_frame_lidar(self, rgb, points, T, sem, pose):
        """process_frame() with the depth made from the scan: the image and the points are uploaded, sm_lidar_depth_device and
        sm_process_frame_device are enqueued one after the other, and the depth never leaves the device.  sem None: the current
        class image stays, whichever call gave it.  The device buffers it stages in are allocated by the first call and live as
        long as the context, so the depth and the class image given here stay readable as the current ones for later calls that
        pass None; the scan's grows by at least half when a scan has more points than it holds, and the one it replaces is freed."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.shape == (self.H, self.W, 3), rgb.shape
        points, _ = self._scan(points, T)
        if getattr(self, "_ldepth_dev", None) is None:
            P = self.P
            self._ldepth_dev = [self.device_alloc(P * 3), self.device_alloc(P * 2), self.device_alloc(P), 0, 0]
        if len(points) > self._ldepth_dev[4]:
            cap = max(len(points), self._ldepth_dev[4] * 3 // 2)
            if self._ldepth_dev[3]:
                self.device_free(self._ldepth_dev[3])                     # (waits for the calls that still read it)
                self._ldepth_dev[3] = self._ldepth_dev[4] = 0
            self._ldepth_dev[3], self._ldepth_dev[4] = self.device_alloc(cap * 16), cap
        d_rgb, d_depth, d_sem, d_points, _ = self._ldepth_dev
        self.device_upload(d_rgb, rgb)
        if len(points):
            self.device_upload(d_points, points)
        if sem is not None:
            self.device_upload(d_sem, np.ascontiguousarray(sem, np.uint8))
        self.lidar_depth_device(d_points, len(points), T, d_depth)
        return self.process_frame_device(d_rgb, d_depth, d_sem if sem is not None else None, pose)

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
        n = self._row_count("sm_download_raw_cloud")
        return self._fetch_rows("sm_download_raw_cloud", n) if n.value else np.zeros((0, 12), np.float32)

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
        return self._novel_views("sm_render_image", (_ptr(view),), (h, w), (w, h, fx, fy, cx, cy), fill, depth, blend)

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
        return self._stats(SmFillStats, "sm_fill_stats")

    def blend_stats(self) -> dict:
        """of the last blended call (sm_blend_stats): drawn, contributions, changed (summed over its views), launches, device_ms"""
        return self._stats(SmBlendStats, "sm_blend_stats")

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
        n, ms = C.c_uint32(), (C.c_float * 3)()
        self._chk(self._L.sm_debug_render_model_stats(self._h, C.byref(n), ms), "sm_debug_render_model_stats")
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
        src = map_source(paths, include_model)
        return self._novel_views("sm_render_image_maps", (C.byref(src), _ptr(views), V), (V, h, w), (w, h, fx, fy, cx, cy),
                                 fill, depth, blend)

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
        return self._stats(SmMapsStats, "sm_render_maps_stats")

    # -- lidar sweeps (sm_lidar_sweep, sm_lidar_sweep_maps)
    def lidar_sweep(self, pose, sensor=None) -> dict:
        """What a lidar at `pose` (sensor->world, float32[16] column-major or 4x4) measures in the live model: a dict of
        range float32[n_el][n_az] (0 = no return), id int32 (row of download_model(), -1), rgb uint8[..][3], sem uint8 (class + 1,
        0).  sensor: lidar_sensor(...); None = the default."""
        sensor = lidar_sensor() if sensor is None else sensor
        pose = _mat16(pose)
        return self._lidar_sweep("sm_lidar_sweep", (sensor.n_el, sensor.n_az), C.byref(sensor), _ptr(pose))

    def lidar_sweep_maps(self, paths, poses, sensor=None, include_model=True) -> dict:
        """lidar_sweep of a map set (see render_image_maps) from every pose of `poses` (float32[V][16]): the same dict with a
        leading axis V; ids are positions in the concatenation."""
        sensor = lidar_sensor() if sensor is None else sensor
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        V = poses.shape[0]
        src = map_source(paths, include_model)
        return self._lidar_sweep("sm_lidar_sweep_maps", (V, sensor.n_el, sensor.n_az), C.byref(src), C.byref(sensor), _ptr(poses), V)

    def lidar_stats(self) -> dict:
        """of the last lidar_sweep* call: surfels offered, exact tests, wide (surfel, sweep) pairs, blocks_skipped, chunks, passes,
        read_ms, copy_ms, device_ms, total_ms"""
        return self._stats(SmLidarStats, "sm_lidar_stats")

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
        return self._stats(SmRaysStats, "sm_cast_rays_stats")

    # -- point queries (sm_query_points_maps)
    def query_points(self, points, paths=(), include_model=True, cell_mm=250, origin=None, min_conf=0.0,
                     planes=("centre", "normal", "radius", "rgb", "sem")) -> dict:
        """The nearest disc of the map set `paths` (then, with include_model, the live model) to each of the points float32[n][4] =
        (position, reach), world frame, metres, within that reach: a dict of d2 float32[n] (the squared distance; +inf = none),
        dist (its square root), id int32 (position in the concatenation, -1) and the `planes` asked for: centre float32[n][3],
        normal float32[n][3], radius float32[n] (the record's, verbatim), rgb uint8[n][3], sem uint8 (class + 1, 0).  Ties go to the
        lower id (sm_query_points_maps; tests/points_ref.py restates the rule).  cell_mm and origin shape the voxel index and change
        nothing in the answer.  A reach of +inf asks for the nearest disc of the whole set; an invalid point returns the empty values."""
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 4:
            raise ValueError("points: float32[n][4]")
        shapes = dict(centre=((3,), np.float32), normal=((3,), np.float32), radius=((), np.float32), rgb=((3,), np.uint8), sem=((), np.uint8))
        for k in planes:
            if k not in shapes:
                raise KeyError(k)
        n = pts.shape[0]
        p = points_params(cell_mm=cell_mm, origin=(0.0, 0.0, 0.0) if origin is None else origin, min_conf=min_conf)
        src = map_source(paths, include_model)
        out = dict(d2=np.full(n, np.inf, np.float32), id=np.full(n, -1, np.int32))
        for k in planes:
            out[k] = np.zeros((n,) + shapes[k][0], shapes[k][1])
        self._chk(self._L.sm_query_points_maps(self._h, C.byref(src), C.byref(p), _ptr(pts), n, _ptr(out["d2"]), _ptr(out["id"]),
                                               *[_ptr(out[k]) if k in out else None for k in shapes]), "sm_query_points_maps")
        out["dist"] = np.sqrt(out["d2"])
        return out

    def query_points_stats(self) -> dict:
        """of the last query_points: points, bad_points, records, wide, pairs and cells (of the largest chunk), probes, tests, no_slot,
        gave_up, chunks, files_skipped (always 0), read_ms, copy_ms, index_ms, walk_ms, device_ms, total_ms"""
        return self._stats(SmPointsStats, "sm_query_points_stats")

    # -- scenes (sm_render_image_scene, sm_lidar_sweep_scene)
    def render_scene(self, paths, actors, views, w, h, fx, fy, cx, cy, include_model=True, fill=None, depth=False):
        """render_image_maps of a scene: the map set plus `actors`, a list of (path, poses[, present]) -- map files in the actor's
        own frame, each drawn under its pose of the view (float32[V][12] row-major 3x4 or [V][4][4], actor->world) where it is
        present (uint8[V]; None: everywhere).  Every view equals render_image_maps of the set followed by the present actors' files
        moved by sm_warp_by_time's row rule.  Returns (bgr, sem[, depth_mm]) as render_image_maps."""
        views = np.ascontiguousarray(views, np.float32).reshape(-1, 16)
        V = views.shape[0]
        src = map_source(paths, include_model)
        sc = scene(actors, V)
        bgr, sem, d = _view_planes((V, h, w), depth)
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
        src = map_source(paths, include_model)
        sc = scene(actors, V)
        return self._lidar_sweep("sm_lidar_sweep_scene", (V, sensor.n_el, sensor.n_az), C.byref(src), C.byref(sc), C.byref(sensor),
                                 _ptr(poses), V)

    def scene_stats(self) -> dict:
        """of the last render_scene / lidar_sweep_scene call (sm_scene_stats): actors, files (distinct), records and bytes
        resident, pairs_tested / pairs_skipped ((actor block of 256, view) pairs), load_ms, actor_ms, total_ms"""
        return self._stats(SmSceneStats, "sm_scene_stats")

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
        return self._stats(SmTileStats, "sm_tile_stats")

    # -- packed map files (sm_pack_maps, sm_unpack_maps)
    def pack_maps(self, paths, out_prefix, include_model=False, **params) -> list:
        """The files `paths` -- then (include_model) the live model as one more -- written again in the packed format of 20 bytes
        a record, file i as "<out_prefix>_%06u.smp" (sm_pack_maps; tests/pack_ref.py restates the format).  Every call that reads
        a map set takes the packed files in place of the plain ones.  Sources and model stay as they are.  params: the fields of
        pack_params().  Returns the files written, in order."""
        p = pack_params(**params)
        src = map_source(paths, include_model)
        self._chk(self._L.sm_pack_maps(self._h, C.byref(src), C.byref(p), os.fsencode(out_prefix)), "sm_pack_maps")
        return ["%s_%06d.smp" % (os.fspath(out_prefix), i) for i in range(len(paths) + (1 if include_model else 0))]

    def unpack_maps(self, paths, out_prefix) -> list:
        """The files `paths` as plain map files "<out_prefix>_%06u.bin": a packed one decoded, a plain one copied (sm_unpack_maps).
        Returns the files written, in order."""
        src = map_source(paths, include_model=False)
        self._chk(self._L.sm_unpack_maps(self._h, C.byref(src), os.fsencode(out_prefix)), "sm_unpack_maps")
        return ["%s_%06d.bin" % (os.fspath(out_prefix), i) for i in range(len(paths))]

    def pack_stats(self) -> dict:
        """of the last pack_maps or unpack_maps: records, bytes_in, bytes_out, files, blocks, raw_blocks, chunks, read_ms, copy_ms,
        unpack_ms (of copy_ms: the decode of packed sources), device_ms, write_ms, total_ms"""
        return self._stats(SmPackStats, "sm_pack_stats")

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
        return self._stats(SmRegisterStats, "sm_register_stats")

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
        lab = self._label_buffer(paths, include_model, 0xFFFFFFFF, np.uint32) if labels else None
        cap = int(max_components)
        rows = np.zeros(cap, SEGMENT_COMPONENT)
        out = None if out_path is None else os.fsencode(out_path)
        self._chk(self._L.sm_segment_maps(self._h, C.byref(src), C.byref(p), _ptr(lab), _ptr(rows) if cap else None, cap, out, C.byref(info)),
                  "sm_segment_maps")
        counts = [int(v) for v in info.counts]
        d = dict(records=int(info.records), counts=dict(zip(SEGMENT_KINDS, counts)), counts_by_kind=counts, written=int(info.written),
                 cells=int(info.cells), components=int(info.components), small_components=int(info.small_components), largest=int(info.largest))
        self._check_labels(lab, d["records"], "segment_maps", "the set changed while it was segmented")
        return dict(labels=lab, components=rows[:min(cap, d["components"])].copy(), info=d)

    def segment_stats(self) -> dict:
        """of the last segment_maps: chunks, launches, readings, read_ms, table_ms, link_ms, label_ms, write_ms, total_ms"""
        return self._stats(SmSegmentStats, "sm_segment_stats")

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
        return self._stats(SmMeshStats, "sm_mesh_stats")

    # -- one map set located in another without a guess (sm_locate_maps)
    def locate_maps(self, source_paths, target_paths, source_model=False, target_model=False, **params) -> dict:
        """Where the map set `source_paths` (then, with source_model, the live model) lies in the world of the set `target_paths`
        (target_model likewise), without a guess: any yaw about the shared up axis, offsets of thousands of cells, a height
        (sm_locate_maps; tests/locate_ref.py restates it).  params: the fields of locate_params() -- the target window (origin, nu,
        nv, cell_mm) should hold the target's structure, source_origin lie near the source's middle.  Nothing is changed.  Returns
        dict(pose: 4x4 float32 source world -> target world, the identity unless status is "OK" or "AMBIGUOUS" -- pass it as `guess`
        to register_maps --, info: status (name), status_code, row, yaw_deg, du, dv, score, coarse_k, coarse_du, coarse_dv,
        coarse_score, runner_up, n_s, target_cells, height_pairs, dh, source_counts, target_counts (by LOCATE_KINDS))."""
        p = locate_params(**params)
        src, tgt = map_source(source_paths, include_model=source_model), map_source(target_paths, include_model=target_model)
        out = np.zeros(16, np.float32)
        info = SmLocateInfo()
        self._chk(self._L.sm_locate_maps(self._h, C.byref(src), C.byref(tgt), C.byref(p), _ptr(out), C.byref(info)), "sm_locate_maps")
        d = {n: int(getattr(info, n)) for n, _ in SmLocateInfo._fields_ if not n.endswith("_counts")}
        d.update(status=LOCATE_STATUS[info.status], status_code=int(info.status), yaw_deg=360.0 * info.row / (p.n_yaw * p.refine),
                 source_counts=[int(v) for v in info.source_counts], target_counts=[int(v) for v in info.target_counts])
        return dict(pose=out.reshape(4, 4).T.copy(), info=d)

    def locate_stats(self) -> dict:
        """of the last locate_maps: source_records, target_records, nodes, leaves, chunks, launches, rounds, levels, exhaustive,
        range, read_ms, raster_ms, pyramid_ms, search_ms, total_ms"""
        return self._stats(SmLocateStats, "sm_locate_stats")

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
        return self._stats(SmGroundStats, "sm_ground_stats")

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
        lab = self._label_buffer(query_paths, query_model, 255, np.uint8) if labels else None
        out = None if out_path is None else os.fsencode(out_path)
        self._chk(self._L.sm_compare_maps(self._h, C.byref(qry), C.byref(ref), _ptr(g), C.byref(p), _ptr(lab), out, C.byref(info)), "sm_compare_maps")
        codes = [int(v) for v in info.counts]
        d = dict(counts={COMPARE_LABEL[l]: codes[l] for l in range(4)}, counts_by_code=codes, query_records=int(info.query_records),
                 reference_records=int(info.reference_records), cells_fine=int(info.cells_fine), cells_cover=int(info.cells_cover),
                 written=int(info.written))
        self._check_labels(lab, d["query_records"], "compare_maps", "the query set changed while it was compared")
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
        return self._stats(SmCompareStats, "sm_compare_stats")

    def simplify_stats(self) -> dict:
        """of the last simplify* call: records_in, records_out, cells_merged, loose, largest_cell, chunks, launches, device_ms,
        read_ms, total_ms"""
        return self._stats(SmSimplifyStats, "sm_simplify_stats")

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
