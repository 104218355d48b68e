/*
 * sm_c_api.h -- C-ABI of the MI355X-native surfel-fusion core (libsurfelmapping_hip.so).
 *
 * The reference (SUSTech-SLAM-XYZZY/SurfelMapping) has no plugin/FFI layer: its boundary is
 * the C++ class surface build_map.cpp / load_map.cpp / gui/GUI.cpp compile against.  This
 * header is the thin C boundary the drop-in C++ facade (surfelmapping_amd/csrc/facade/) calls;
 * every entry point names the reference interface it replaces (file:line under
 * /root/reference).  Plain pointers and sizes only; no torch / HIP types in signatures.
 *
 * Threading: one sm_ctx = one HIP device + one stream; calls on a ctx are not re-entrant.
 * Host-buffer entry points are synchronous (the reference glFinish()es after every pass,
 * e.g. src/GlobalModel.cpp:341); *_device / *_async entry points only enqueue.
 */
#ifndef SM_C_API_H
#define SM_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SM_API_VERSION 4   /* bumped whenever a struct or an entry point changes (3, 4: round 3 -- asynchronous host path, rig step, sm_timings::k_scan_own, sm_host_alloc_frame; the staged shard entry points are gone).  Purely additive changes keep it: sm_model_view / sm_render_model*, sm_track_* and sm_track_*rgb* were added at 4, as were sm_warp_by_time / sm_loop_spread / sm_track_*_old / sm_close_loop and sm_track_*_window / sm_close_loop_rgb / sm_old_in_view / sm_*auto_loop*, and sm_fern_* / sm_search_pose_at / sm_close_loop_at / sm_*auto_place*, and sm_fill_* / sm_render_image_ex / sm_render_image_maps_ex: no existing struct or entry point changed. */

/* error codes (reference: void returns + CheckGlDieOnError(); bool for map IO) */
enum {
    SM_OK = 0,
    SM_E_ARG = -1,          /* null / inconsistent argument (reference would segfault: src/SurfelMapping.cpp:130) */
    SM_E_CAPACITY = -2,     /* model would exceed MAX_VERTICES (unchecked in src/GlobalModel.cpp:627-629) */
    SM_E_UNSUPPORTED = -3,
    SM_E_HIP = -4,          /* a HIP runtime call failed; see sm_last_error() */
    SM_E_NO_DEVICE = -5,    /* no gfx950 device visible: the product has NO CPU fallback */
    SM_E_STALL = -6         /* an in-kernel hand-off wait hit its spin bound: the in-place compaction needs its whole grid
                               resident, which another job on the same GPU can prevent.  Contexts of one process that
                               share a GPU are safe (they use the ticket-ordered form of the kernel); for several
                               PROCESSES on one GPU set SM_COMPACT_TICKETS=1 in their environment. */
};

/* Config singleton values (src/Config.cpp:32-37) + the magic numbers of the hot path
 * (src/SurfelMapping.cpp:197,261; src/IndexMap.cpp:21). */
typedef struct sm_config {
    int32_t width, height;         /* Config::W(), Config::H() */
    float fx, fy, cx, cy;          /* Config::fx() ... */
    float near_clip;               /* 1.0  Config::nearClip() */
    float far_clip;                /* 30.0 Config::farClip()  */
    float fuse_thresh;             /* 0.0  Config::surfelFuseDistanceThreshFactor() */
    int32_t max_sqrt_vertices;     /* 5000 Config::maxSqrtVertices(); capacity = its square */
    int32_t time_delta;            /* 200  src/SurfelMapping.cpp:197 */
    float stereo_border;           /* 80   src/SurfelMapping.cpp:261 */
    int32_t preprocess;            /* 0: metricise only (p0a); 1: full chain p0a..p0e */
    int32_t conflict_cap;          /* 1: only the first W*H conflicts take effect (conflictVbo size, src/GlobalModel.cpp:54-57) */
    int32_t device;                /* HIP device ordinal */
    int32_t enable_timing;         /* 1: record hipEvents per stage (sm_stage_timings) */
    int32_t disable_tile_bounds;   /* 1: never skip tiles by their bounding box (A/B switch; results are identical) */
    int32_t compact_period;        /* 24: deferred compaction -- a cull only marks the surfels it removes (they keep their slots)
                                      and every 24th cull squeezes the dead slots out in one in-place pass; also whenever dead
                                      slots could make a frame exceed MAX_VERTICES.  0/1: compact at every cull like the
                                      reference.  Counts, ids and the stored model are identical for every period. */
} sm_config;

/* GlobalModel counters (src/GlobalModel.cpp:860-888) + tick (src/SurfelMapping.h:100) */
typedef struct sm_counts {
    uint32_t count;           /* getModel().second    */
    uint32_t offset;          /* getOffset()          */
    uint32_t data_count;      /* getData().second     */
    uint32_t conflict_count;  /* getConflict().second */
    uint32_t unstable_count;  /* getUnstable().second */
    uint32_t fused_count;     /* data entries that update an existing surfel (F) */
    uint32_t visible_count;   /* surfels that passed the index-map view test (V) */
    int32_t tick;
} sm_counts;

/* Stage timings in milliseconds (HIP events on the ctx stream, averaged over the frames since
 * the previous query), labelled with the reference's TICK/TOCK names
 * (src/SurfelMapping.cpp:120-250, src/GlobalModel.cpp:258,350,519,583). */
typedef struct sm_timings {
    float preprocess;         /* "Preprocess": k_prep (+ p0b..p0e)                         */
    float conflict;           /* "Conflict": k_conflict + k_scan_cull + k_compact (p2..p5) */
    float index_map;          /* "indexMap": 0, the splat is fused into k_compact          */
    float data_association;   /* "Data::Association" + "Update::Fuse": k_associate         */
    float concatenate;        /* "Concatenate": k_scan_new + k_append                      */
    float run;                /* "Run": whole frame                                        */
    /* per kernel */
    float k_prep, k_conflict, k_scan_cull, k_compact, k_associate, k_scan_new, k_append;
    uint32_t frames;          /* frames averaged */
    float event_overhead;     /* measured cost of one event record, already subtracted from the k_* fields */
    /* the cull slot by kernel: k_compact above averages over ALL frames; these two over their own frames */
    float k_compact_own;      /* k_compact, averaged over the frames that compacted */
    float k_cull_lazy;        /* k_cull_lazy, averaged over the frames that only marked the dead */
    uint32_t frames_compact;  /* how many of `frames` compacted */
    /* the frame forms of the default path, each kernel averaged over the frames that ran it:
     * one-pass frames (the cull only marks the dead): k_surfel_pass (conflict + cull + splat) and k_pass_fixup (0 where the
     * fixup step rides on the next frame's preparation launch: the two-launch frame of asynchronous streams);
     * direct-append frames: k_associate_direct (association + fuse + append); the other frames run k_conflict
     * (+ k_scan_cull + k_cull_finalize + k_compact) and k_associate + k_append_scan */
    float k_surfel_pass, k_pass_fixup, k_conflict_own;
    float k_associate_direct, k_associate_own, k_append_own;
    uint32_t frames_one_pass, frames_direct;
    /* asynchronous plain streams: frames whose preparation launch also carried the previous frame's association
     * (k_assoc_prep); k_prep_own / k_associate_direct then average only over the frames that launched those kernels alone */
    float k_assoc_prep, k_prep_own;
    uint32_t frames_merged, frames_assoc_alone;
    float k_scan_own;         /* k_scan_cull + k_cull_finalize, averaged over the frames that ran k_conflict */
} sm_timings;

/* Per-frame counters written by the device at the end of every fusing frame (ring of
 * SM_FRAME_LOG_LEN entries) so that an asynchronous run can be audited without host syncs. */
#define SM_FRAME_LOG_LEN 1024
typedef struct sm_frame_log {
    uint32_t tick;            /* time stamp of the frame */
    uint32_t n_before;        /* N  live surfels at frame start */
    uint32_t n_after_cull;    /* N' */
    uint32_t n_kill;
    uint32_t conflict_count;  /* C */
    uint32_t visible_count;   /* V */
    uint32_t fused_count;     /* F */
    uint32_t unstable_count;  /* U */
    uint32_t n_static;        /* surfels the in-place cull did not have to move */
    uint32_t n_conf_skipped;  /* surfels in tiles the conflict pass skipped by their bounding box */
    uint32_t n_splat_skipped; /* surfels in static tiles the index-map splat skipped by their bounding box */
    uint32_t n_slots;         /* model slots scanned by the cull = n_before + slots of surfels killed since the last compaction */
} sm_frame_log;

enum { SM_TEX_DEPTH_METRIC = 0, SM_TEX_DEPTH_FILTERED = 1, SM_TEX_LAST = 2 };

typedef struct sm_ctx sm_ctx;

int sm_api_version(void);
const char *sm_last_error(void);

/* Config::getInstance(fx,fy,cx,cy,rows,cols) defaults: src/Config.cpp:7-38 */
int sm_default_config(sm_config *c, int width, int height, float fx, float fy, float cx, float cy);

/* SurfelMapping::SurfelMapping() (src/SurfelMapping.cpp:12-25): allocates all device buffers. */
sm_ctx *sm_create(const sm_config *c);
/* SurfelMapping::~SurfelMapping() (src/SurfelMapping.cpp:27-49) */
void sm_destroy(sm_ctx *s);

/* SurfelMapping::processFrame (src/SurfelMapping.h:31-34, src/SurfelMapping.cpp:115-251).
 * rgb H*W*3 u8 (R first), depth_mm H*W u16 (0 invalid), semantic H*W u8, pose = column-major
 * 4x4 camera->world (Eigen::Matrix4f storage).  Inputs are borrowed for the call only.
 * depth_mm and semantic may each be null: "keep what is in the texture" (src/SurfelMapping.cpp:122-128).  The context has ONE
 * current depth image and ONE current class image, as the reference has one DEPTH_RAW and one SEMANTIC texture: an image given
 * to ANY entry point -- sm_process_frame, sm_process_frame_async, sm_process_frame_device, sm_clean_points*, sm_set_frame (class
 * only), sm_shard_frame, sm_shard_frame_device -- becomes current, and a null in any of them reads the current one, whichever
 * call gave it.  Before the first one is given the images are zeros (no depth anywhere); sm_reset, sm_upload_model, sm_load_map
 * and the trackers leave them alone. */
int sm_process_frame(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm,
                     const uint8_t *semantic, const float *pose16);
/* Same, inputs already resident in device memory of this ctx's GPU; enqueue only.  Without the depth filter chain the
 * frame's last kernel (association + append) is held back and launched together with the NEXT call's image preparation
 * (one launch less per frame); sm_sync and every entry point that reads the model launch it first, so the only visible
 * effect is that a caller who never calls anything again must call sm_sync to have the last frame finished.
 * SM_DEFER_ASSOC=0 turns this off.  (One bounded exception to "enqueue only": when the model
 * is within one frame of MAX_VERTICES and the host has run ahead of the device, the call waits up to SM_CAPACITY_WAIT_US
 * (default 2000) microseconds for the device's slot count before deciding whether this frame's cull must compact.)
 * A depth or class image given here becomes the current one IN THE CALLER'S BUFFER (no copy is made): if a later call to any
 * entry point passes null for it, the buffer must stay allocated and unchanged until another depth (or class) image has been
 * given or the context is destroyed.  A caller who never passes null may reuse the buffer as soon as the frame has run. */
int sm_process_frame_device(sm_ctx *s, const uint8_t *d_rgb, const uint16_t *d_depth_mm,
                            const uint8_t *d_semantic, const float *pose16);
/* The same for callers whose images live in HOST memory and who do not want to wait (SurfelMapping::processFrame uploads its
 * three images itself, src/SurfelMapping.cpp:122-128): the images are copied on a copy stream into one of three device input
 * sets, so the 2.8 MB host-to-device copy of frame f+1 runs while frame f computes; the call returns once copies and frame are
 * enqueued (it waits for the frame three calls back, which bounds the work in flight).  Images that live in buffers of
 * sm_host_alloc -- pinned memory a reader decodes straight into -- are copied from in place and must stay unchanged until
 * sm_inputs_consumed() or sm_sync() returns; any other pointer is first copied into pinned staging inside the call (one host
 * memcpy) and may be reused at once.  Caller memory is never registered with the runtime. */
int sm_process_frame_async(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16);
int sm_inputs_consumed(sm_ctx *s);                                     /* waits for the copies only, not for the frames */
void *sm_host_alloc(sm_ctx *s, size_t bytes);                          /* hipHostMalloc, owned by the context */
/* The three images of ONE frame in one pinned block (colour | depth | class, each 16-byte aligned): sm_process_frame_async copies
 * such a frame with a single host-to-device transfer -- 58 us for 2.8 MB at 1242 x 375, the PCIe rate, against 87 us for three
 * transfers from separate buffers (tools/h2d_probe.hip).  Free with sm_host_free(s, *rgb). */
int sm_host_alloc_frame(sm_ctx *s, uint8_t **rgb, uint16_t **depth_mm, uint8_t **semantic);
int sm_host_free(sm_ctx *s, void *p);
/* Wait for all enqueued work; refresh counters; returns a sticky device-side error. */
int sm_sync(sm_ctx *s);

/* SurfelMapping::cleanPoints (src/SurfelMapping.cpp:496-532) */
int sm_clean_points(sm_ctx *s, const uint16_t *depth_mm, const uint8_t *semantic,
                    const float *pose16);
/* cleanPoints for a model SLICE of a multi-GPU rig (surfelmapping_amd/dist.py, BASELINE configs[4]): as sm_clean_points,
 * but the "surfel id 0 never conflicts" rule (conflict.geom:15) applies only where exempt_first != 0 -- i.e. on the rank
 * whose slice holds the first surfel of the single GlobalModel; the other slices have no id 0. */
int sm_clean_points_ex(sm_ctx *s, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16, int exempt_first);
/* The same for rigs that stage the exchange outside the core (surfelmapping_amd/dist.py RigMapper.consolidate): between the
 * conflict test -- which changes nothing -- and the cull, `fn` is called with this slice's conflict count and returns how many
 * of them, in surfel order, may take effect: the slice's share of the union's W*H conflict records (src/GlobalModel.cpp:54-57),
 * i.e. W*H minus the conflicts of the slices before it, clamped; a negative return abandons the cull (the model is untouched)
 * and is passed on as the result. */
typedef long long (*sm_cap_fn)(void *user, uint32_t local_conflicts);
int sm_clean_points_cb(sm_ctx *s, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16, int exempt_first,
                       sm_cap_fn fn, void *user);
/* SurfelMapping::reset (src/SurfelMapping.cpp:436-441): empties the model and sets tick = 0; the next processFrame
 * builds the model anew from that frame's raw cloud (GlobalModel::initialize), discarding anything uploaded in between.
 * The index map is left as the last predictIndices drew it. */
int sm_reset(sm_ctx *s);

/* GlobalModel::getModel/getData/getConflict/getUnstable/getOffset counts */
int sm_get_counts(sm_ctx *s, sm_counts *out);
/* GlobalModel::downloadMap payload (src/GlobalModel.cpp:905-911): AoS, 12 floats/surfel */
int sm_download_model_aos(sm_ctx *s, float *dst12, uint32_t cap, uint32_t *n);
/* GlobalModel::uploadMap payload (src/GlobalModel.cpp:995-1002) */
int sm_upload_model_aos(sm_ctx *s, const float *src12, uint32_t n);
/* GlobalModel::downloadMap / uploadMap files (src/GlobalModel.cpp:901-1011) */
int sm_save_map(sm_ctx *s, const char *path, int32_t start_id, int32_t end_id);
int sm_load_map(sm_ctx *s, const char *path, int32_t *start_id, int32_t *end_id);
/* IndexMap::indexTex/vertConfTex/colorTimeTex/normalRadTex read-back (src/IndexMap.h:70-88),
 * row-major H*W; any pointer may be NULL.  Ids are surfel positions in the model at the time of the last
 * predictIndices (a later cleanPoints / reset / upload does not redraw the map, as in the reference); the three
 * attribute planes are re-derived from the surfels those ids address in the model as it is NOW, i.e. they equal the
 * reference's textures only while the model has not changed since. */
int sm_download_index_map(sm_ctx *s, int32_t *id, float *vert_conf4, float *color_time4,
                          float *norm_rad4);
/* FeedbackBuffer "RAW" (SurfelMapping::getFeedbackBuffer(FeedbackBuffer::RAW), src/SurfelMapping.cpp:367-376,
 * src/FeedbackBuffer.cpp:85-145, surfel_feedback.vert:25-63): the raw surfel cloud of the last processed frame -- every
 * checkerboard pixel with 0 < z < farClip as a camera-frame surfel, 12 floats each (pos, 0.9 | colour bits, 0, time, time |
 * normal, radius), in vertex order (x-outer / y-inner).  The reference fills it on every frame after the first; it feeds
 * the GUI's "Draw raw" view (build_map.cpp:177-184) and GlobalModel::initialize after reset().  Computed on demand here.
 * dst12 may be NULL to query the count. */
int sm_download_raw_cloud(sm_ctx *s, float *dst12, uint32_t cap, uint32_t *n);
/* SurfelMapping::getTexture(DEPTH_METRIC / DEPTH_FILTERED / "LAST") read-back, row-major */
int sm_download_depth(sm_ctx *s, int which, float *dst);

/* GlobalModel::setImageSize + renderImage + the two texture downloads of SurfelMapping::acquireImages
 * (src/GlobalModel.cpp:772-833, src/SurfelMapping.cpp:378-434): novel view of the model from camera->world
 * pose `view16`; bgr_out h*w*3 u8 (B,G,R as FragColor = srgb.wzy), sem_out h*w u8 = class + 1, 0 = empty. */
int sm_render_image(sm_ctx *s, const float *view16, int w, int h, float fx, float fy, float cx, float cy,
                    uint8_t *bgr_out, uint8_t *sem_out);

/* The model view: GlobalModel::renderModel's uniforms (src/GlobalModel.cpp:683-758) plus a viewport. */
typedef struct sm_model_view {
    float mvp[16];        /* column-major, pangolin::OpenGlMatrix converted to float (the MVP uniform) */
    float mv_inv[16];     /* column-major, mv.Inverse() as the reference uploads it (the MVINV uniform) */
    float threshold;
    int32_t color_type;   /* 0 shaded, 1 normals, 2 colours, 3 semantic: renderModel's drawNormals ? 1 : drawColors ? 2 : drawSemantic ? 3 : 0 */
    int32_t draw_unstable, draw_points, draw_window, time, time_delta;
    int32_t width, height;
    uint8_t clear_rgba[4];
} sm_model_view;

/* GlobalModel::renderModel (src/GlobalModel.cpp:683-758) into an image instead of the bound framebuffer: surfels as
 * oriented discs (draw_surface.vert / draw_surface_adaptive.geom / draw_surface.frag) or points (draw_feedback.vert/.frag),
 * GL_LESS into a 24-bit depth buffer cleared to 1.0, ties to the lower id (DESIGN.md "Model view").
 * rgba: w*h*4 host bytes (alpha 255 where a surfel is drawn, clear_rgba elsewhere), GL row order (row 0 = bottom, as
 * glReadPixels); depth (w*h float window z, 1.0 = empty) and id (w*h int32, AoS row of sm_download_model_aos, -1 = empty) are
 * optional (NULL).  Waits for the copies.  Changes neither the model nor the frame state; frames in flight are waited for.
 * SM_E_ARG: NULL ctx / view / rgba, w or h <= 0, w*h > 2^28, color_type outside 0..3, or a call between sm_stage_conflict
 * and sm_stage_cull.  SM_E_UNSUPPORTED in a sharded context (a rank holds only its own surfels). */
int sm_render_model(sm_ctx *s, const sm_model_view *v, uint8_t *rgba, float *depth, int32_t *id);
/* the same into device memory (4-byte aligned), enqueued on the context's stream; returns without waiting for the render */
int sm_render_model_device(sm_ctx *s, const sm_model_view *v, uint8_t *d_rgba, float *d_depth, int32_t *d_id);

/* ---- views of a map set (DESIGN.md "4f. Views of a map set") ----
 * A map set is a list of map files (GlobalModel::downloadMap's format: sm_save_map, the files of sm_set_auto_retire), drawn in
 * the given order, optionally followed by the context's live model.  The two calls below draw it without loading it: the
 * files are streamed through the device in chunks, so the set may be larger than the context, larger than device memory, and
 * include what retirement has moved out of the model.
 *   Global id.  A surfel's id is its position in the concatenation of the set: the files in order, each file's records in
 *     file order, then the live model in sm_download_model_aos order.  The id planes carry it.
 *   Output equality.  Per view, every output equals sm_render_image / sm_render_model of a context whose model is that
 *     concatenation, bit for bit (whether or not such a context could exist) -- the clear colour, sem 0, depth 1.0 and id -1 of
 *     an empty pixel included; a depth tie goes to the lower id, so to the source that comes first.  The result depends
 *     neither on the chunking nor on how many views are drawn per pass over the files.
 *   Size limit.  A set of more than 2^31 - 1 surfels: SM_E_CAPACITY, before anything is drawn.
 *   Degenerate sets.  n_paths == 0 with include_model == 1 equals the existing entry point; an empty set gives the cleared images.
 *   Side effects.  The model, the counters, the tick, the frame log and the tracker state are untouched; the forced compaction
 *     that every read-back does is the only side effect, as in sm_render_model.  Frames in flight are waited for.
 *   Files.  The headers of ALL files are read and checked before anything else is done: the record count against the file's
 *     length (12 + 48 * count bytes exactly), the total against the size limit.  A file that is missing, shorter or longer
 *     than its header says: SM_E_ARG, sm_last_error() names it, and the outputs are not written.  That guarantee is
 *     the header check's: a file that shrinks or disappears after it (between the check and a later pass) also gives
 *     SM_E_ARG, but views of earlier passes may already have been written; treat the outputs as undefined then.  Every file
 *     is read once per pass; a pass draws as many views as fit the key budget (1 GiB of 8-byte keys; SM_RENDER_MAPS_KEY_MB overrides it).
 *   Other errors.  SM_E_UNSUPPORTED in a sharded context.  SM_E_ARG: a NULL ctx or source, a call between sm_stage_conflict and
 *     sm_stage_cull, NULL paths with n_paths > 0, NULL views or outputs (bgr_out, sem_out; rgba) with n_views > 0, a view
 *     sm_render_image / sm_render_model would refuse, views of different width x height.  n_views == 0 checks the set and
 *     draws nothing.
 * SM_RENDER_MAPS_NO_CULL=1 turns the per-block view test off (an A/B switch: the images are the same either way). */
typedef struct sm_map_source {
    const char *const *paths; uint32_t n_paths;  /* GlobalModel::downloadMap files, drawn in this order */
    int32_t include_model;                        /* 1: the live model follows the files */
} sm_map_source;

/* what the last sm_render_image_maps / sm_render_model_maps call of the context did */
typedef struct sm_maps_stats {
    uint64_t surfels_read;        /* records read from the files, all passes together (a blended call reads them twice per pass) */
    uint32_t chunks, passes;      /* chunks (at most 2^20 records) copied to the device; passes over the files */
    uint64_t pairs_tested;        /* (block of 256 records, view) pairs the view test ran on (0 with SM_RENDER_MAPS_NO_CULL=1) */
    uint64_t pairs_skipped;       /* ... of them, found outside the view and not drawn */
    float read_ms, copy_ms;       /* in fread; in the host-to-device copies (events) */
    float device_ms;              /* in the kernels (events around each chunk's and the live model's) */
    float total_ms;               /* the whole call (host clock) */
} sm_maps_stats;   /* (not named after the call: a typedef and a function share C's name space) */

/* sm_render_image of a map set from n_views camera->world poses (16 floats each): bgr_out n_views*h*w*3, sem_out n_views*h*w */
int sm_render_image_maps(sm_ctx *s, const sm_map_source *src, const float *views16, uint32_t n_views, int w, int h, float fx,
                         float fy, float cx, float cy, uint8_t *bgr_out, uint8_t *sem_out);
/* sm_render_model of a map set from n_views views of one width x height: rgba n_views*w*h*4; depth and id (n_views*w*h each)
 * are optional (NULL) */
int sm_render_model_maps(sm_ctx *s, const sm_map_source *src, const sm_model_view *views, uint32_t n_views, uint8_t *rgba,
                         float *depth, int32_t *id);
/* SM_E_ARG if the context has made no such call yet */
int sm_render_maps_stats(sm_ctx *s, sm_maps_stats *out);

/* ---- camera tracking (DESIGN.md "4d. Tracking") ----
 * The reference documents processFrame's gtPose as optional ("if provided, we don't attempt to perform tracking",
 * src/SurfelMapping.h:31-34) but has no tracker.  This one is projective frame-to-model point-to-plane ICP against the map:
 *  - Poses are camera->world, column-major float[16], as everywhere in this header.
 *  - Prediction: ONE per tracked frame, at T_prev = the pose of the last processed frame, of the model as it stands after that
 *    frame.  Pixel (u, v) holds the nearest live surfel (alive under the deferred compaction; nothing is compacted) whose centre
 *    has camera z in (near_clip, far_clip) and projects to u = floor(fx*x/z + cx + 0.5), v likewise (ties: lower slot).
 *  - Current frame: metric depth by the metricise rule of the fused frame (mm -> m inside the clip range, 0 left of
 *    stereo_border; no moving-object filter), vertex and normal of every pixel of the pixel_stride grid by the frame's own rule;
 *    a pixel counts if its depth and its four neighbours' are non-zero.
 *  - Association: T*v projected into the prediction camera; a pair is kept iff a surfel is at that pixel, |T*v - p_m| <= dist_thresh
 *    and dot(R*n, n_m) >= cos(angle_thresh).  Residual r = n_m . (T*v - p_m); left-multiplied world twist xi = (rho, phi),
 *    T <- exp(xi) T, Jacobian row [n_m, (T*v) x n_m].  Per-pixel terms fp32, sums fp64 in a fixed order: bit-reproducible.
 *  - Solve: LDLT in double on the device; stop when |phi| < 1e-6 rad and |rho| < 1e-6 m, else after max_iters.  One host
 *    synchronisation per tracked frame.
 *  - Failure returns the guess with a status: SM_TRACK_LOST (fewer than min_inliers inliers in any iteration),
 *    SM_TRACK_DEGENERATE (in the system of the converged or the last iteration, the smallest / largest LDLT pivot is below
 *    SM_TRACK_DEGENERATE_BOUND, the system taken with the rotation about the prediction camera's centre and the rotation columns
 *    scaled so that both 3x3 diagonal blocks have the same trace), SM_TRACK_NO_MODEL (no processed frame, an empty model, or no
 *    surfel in view).
 *  - Guess when none is given: constant velocity T_prev * (T_prev2^-1 * T_prev) from the last two processed poses (in double,
 *    their rotations orthonormalised first, rounded to float); with one processed pose that pose; with none the identity.  The
 *    iterations start from the guess with its rotation orthonormalised (in double). */
enum { SM_TRACK_OK = 0, SM_TRACK_LOST = 1, SM_TRACK_DEGENERATE = 2, SM_TRACK_NO_MODEL = 3 };
#define SM_TRACK_DEGENERATE_BOUND 1e-4
#define SM_TRACK_MAX_ITERS 100        /* max_iters above this is SM_E_ARG */

typedef struct sm_track_params {
    int32_t max_iters;        /* 15 */
    float dist_thresh;        /* 0.3 m */
    float angle_thresh;       /* 30 degrees */
    int32_t min_inliers;      /* 1000 */
    int32_t pixel_stride;     /* 1: every pixel; s: every s-th column of every s-th row */
} sm_track_params;

typedef struct sm_track_info {
    int32_t status;           /* SM_TRACK_* */
    int32_t iterations;       /* Gauss-Newton systems solved (0: none was built) */
    uint32_t inliers;         /* of the last system */
    float rmse;               /* sqrt(sum r^2 / inliers) of the last system, metres */
    float guess[16];          /* the guess the tracker started from */
} sm_track_info;

int sm_default_track_params(sm_track_params *p);
/* Track one depth image (H*W u16 millimetres, host memory) against the model: pose16_out receives the pose (the guess on failure),
 * info (may be NULL) the statistics.  guess16 NULL = constant velocity; params NULL = defaults.  Waits for frames in flight; changes
 * nothing in the model, its counters, the frame log or the compaction schedule.  The tracked frame is NOT fused: pass the pose to
 * sm_process_frame* (which still requires one).  SM_E_ARG: a NULL ctx / depth / output, a parameter out of range, or a call
 * between sm_stage_conflict and sm_stage_cull.  SM_E_UNSUPPORTED in a sharded context (a rank holds only its own surfels). */
int sm_track_frame(sm_ctx *s, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params, float *pose16_out,
                   sm_track_info *info);
/* For tests: the prediction the next sm_track_frame would draw (pred_slot, W*H int32 row-major, model slot or -1; slots equal the
 * rows of sm_download_model_aos once the model is compacted) and the 29-value system of ONE iteration at pose16_eval with the default
 * parameters (sys29: J^T J upper triangle row-major (21), J^T r (6), sum r^2, inliers; double).  Either output may be NULL. */
int sm_track_debug(sm_ctx *s, const uint16_t *depth_mm, const float *pose16_eval, int32_t *pred_slot, double *sys29);

/* ---- camera tracking with the colour term (DESIGN.md "4d. Tracking", "colour term") ----
 * Depth alone cannot see motion along flat ground between flat walls (sm_track_frame reports SM_TRACK_DEGENERATE there).
 * sm_track_frame_rgb adds a photometric term -- the surfels' stored colours against the frame's rgb image -- solved jointly with the
 * geometric one over an image pyramid, coarse to fine.  Everything not restated here is sm_track_frame's rule: the guess, the
 * orthonormalisation, the prediction at T_prev, the frame's depth / vertex / normal rule, the left-multiplied world twist, fp32
 * per-sample terms with fp64 sums in a fixed order (bit-reproducible), the device LDLT, one host synchronisation per frame.
 *  - Luminance: Y = ((0.299f*R + 0.587f*G) + 0.114f*B) / 255.0f; a surfel's from its colour word (sem<<24 | r<<16 | g<<8 | b).
 *  - Pyramid: level 0 is the frame's luminance, level l+1 the mean ((a+b)+(c+d))*0.25f of each 2x2 block (a b the upper row), of size
 *    floor(w/2) x floor(h/2).  Pixel k of level l spans [k*2^l, (k+1)*2^l) in full-resolution coordinates.  No validity mask.
 *  - Levels run from levels-1 down to 0, at most iters[l] Gauss-Newton systems at level l; a level ends early when the step is below
 *    sm_track_frame's stop thresholds; ending level 0 ends the frame.  sum(iters[0..levels-1]) <= SM_TRACK_MAX_ITERS.
 *  - The sample stride at level l is pixel_stride * 2^l for both terms; the geometric term at level l is exactly sm_track_frame's on
 *    that strided grid.
 *  - Photometric samples: one per prediction pixel of the strided grid that holds a surfel, p its world centre, Y_m its luminance.
 *    Under the estimate T = [R|t]: c = R^T (p - t), x = fx*c.x/c.z + cx, y = fy*c.y/c.z + cy (pixel i is centred at i + 0.5).  Kept
 *    iff c.z > 0; 0 <= x < W and 0 <= y < H; the frame's metric depth D at pixel (floor x, floor y) is non-zero and
 *    |D - c.z| <= dist_thresh (occlusion; drops the stereo border too); the four texels of the bilinear sample of level l at
 *    (x/2^l - 0.5, y/2^l - 0.5) lie inside the level image; |r| < rgb_max_residual, r = I_l(bilinear) - Y_m.  (gx, gy) = the
 *    derivative of that interpolant / 2^l; g_c = (gx*fx/c.z, gy*fy/c.z, -(gx*fx*c.x + gy*fy*c.y)/c.z^2), g_w = R g_c; the Jacobian
 *    row is -[g_w, p x g_w].
 *  - System: A = A_icp + rgb_weight * A_rgb, b likewise, added in double after each term's own fixed-order sum.
 *  - Status: SM_TRACK_LOST if in any iteration (geometric inliers) * 4^l < min_inliers; SM_TRACK_DEGENERATE judged on the joint
 *    system of the last level-0 iteration with sm_track_frame's measure and bound; SM_TRACK_NO_MODEL as there.  Failure returns the
 *    guess.
 *  - With levels = 1, iters[0] = max_iters and rgb_weight = 0 the call equals sm_track_frame bit for bit, pose and info.
 *    (sm_track_params::max_iters is range-checked as there and otherwise unused: iters[] is the schedule.) */
typedef struct sm_track_rgb_params {
    int32_t levels;           /* 3 (1..6) */
    int32_t iters[6];         /* index = level: 10, 5, 4, 4, 4, 4 */
    float rgb_weight;         /* 0.01: lambda of the joint system */
    float rgb_max_residual;   /* 0.25 (luminance in 0..1) */
} sm_track_rgb_params;

typedef struct sm_track_rgb_info {
    uint32_t rgb_inliers;     /* photometric samples of the last system */
    float rgb_rmse;           /* sqrt(sum r^2 / rgb_inliers) of the last system, luminance units */
    double pivot_ratio;       /* the degeneracy measure of the last system that was solved (joint) */
    int32_t level_iterations[6];  /* systems solved per level */
} sm_track_rgb_info;

int sm_default_track_rgb_params(sm_track_rgb_params *p);
/* sm_track_frame with the colour term: rgb is the frame's H*W*3 u8 image (host memory), as sm_process_frame takes it.  info and
 * rgb_info may be NULL; sm_track_info's inliers and rmse are the geometric term's.  Synchronous; changes nothing in the model, its
 * counters, the frame log, the pose history or the compaction schedule.  SM_E_ARG / SM_E_UNSUPPORTED as sm_track_frame, and
 * SM_E_ARG for a NULL rgb, levels outside 1..6, iters[l] < 1 for a used level, sum of iters > SM_TRACK_MAX_ITERS, rgb_weight < 0
 * or not finite, rgb_max_residual <= 0, a coarsest level smaller than 8x8, pixel_stride * 2^(levels-1) > min(W, H). */
int sm_track_frame_rgb(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params,
                       const sm_track_rgb_params *rgb_params, float *pose16_out, sm_track_info *info, sm_track_rgb_info *rgb_info);
/* For tests: the 29-value system (layout as sm_track_debug) of ONE iteration at pose16_eval and `level` (0..5) with the default
 * parameters.  which: 0 = joint (values 0..27 = geometric + rgb_weight * photometric, value 28 the geometric inliers), 1 = the
 * geometric term only, 2 = the photometric term only, unweighted (sum r^2 and count are that term's). */
int sm_track_rgb_debug(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16_eval, int level, int which,
                       double *sys29);

/* ---- retirement (DESIGN.md "4e. Retirement") ----
 * The model grows with the distance driven and MAX_VERTICES is fixed; the reference leaves that to a person (build_map.cpp:204
 * draws the capacity bar, :235-254 saves the map, :258-263 resets it, the part under the camera included).  Retirement moves out
 * of the model, in model order, exactly the surfels fusion can no longer reach, and closes the gaps on the GPU.
 * With the context's tick (sm_counts.tick: the time stamp the NEXT frame will carry), the camera centre c = pose16[12..14] and the
 * rows m of sm_download_model_aos, surfel i is retired iff, in fp32 without fused multiply-add and in this order,
 *     age = float(tick) - m[i][7];                      old = age > float(min_age)
 *     dx, dy, dz = m[i][0..2] - c[0..2];                d2  = (dx*dx + dy*dy) + dz*dz
 *     far = min_distance <= 0  ||  d2 > min_distance*min_distance        (the product rounded to fp32 once)
 *     retired = old && far                              (a comparison with a NaN is false; with min_distance <= 0 the
 *                                                        position is not looked at)
 * The records written are m[retired], the model afterwards is m[!retired], both in the old order and bit for bit, whatever
 * compact_period is (slots a deferred-compaction cull has killed are neither).  count = offset = kept; tick, the other counters,
 * the frame log, the tracker's pose history, the frame planes and the depth filter's "last depth" are untouched; the index map is
 * not redrawn (as after sm_clean_points / sm_upload_model_aos); the compaction schedule restarts as after an upload.
 * index_map.vert:45 never draws a surfel whose last update is more than time_delta frames old, so with min_age >= time_delta a
 * retired surfel could never have been associated or fused again; beyond 1.5 * far_clip no pass reaches it at all.  Smaller
 * values are allowed. */
typedef struct sm_retire_params {
    int32_t min_age;          /* frames since the last update, exclusive */
    float min_distance;       /* metres from the camera centre, exclusive; <= 0: the age gate alone */
} sm_retire_params;
/* min_age = c->time_delta; min_distance = 1.5f * c->far_clip (index_map.vert:45 draws nothing beyond maxDepth * 1.5) */
int sm_default_retire_params(const sm_config *c, sm_retire_params *p);
/* pose16 NULL = pose of the last processed frame; params NULL = defaults.  dst12 NULL: *n = how many WOULD be retired, nothing
 * changes.  cap < that number: SM_E_CAPACITY, nothing changes.  Synchronous (waits for frames in flight, flushes a held-back
 * association like every entry point that reads the model).
 * SM_E_ARG: NULL ctx / n, min_age < 0, non-finite min_distance or pose, a call between sm_stage_conflict and sm_stage_cull.
 * SM_E_UNSUPPORTED: a sharded context or a rig context (a rank holds only its own surfels; the rig indexes them by creation
 * time) -- for sm_retire, sm_retire_device and sm_set_auto_retire. */
int sm_retire(sm_ctx *s, const float *pose16, const sm_retire_params *params, float *dst12, uint32_t cap, uint32_t *n);
/* the same into device memory of this context's GPU (48-byte records, 16-byte aligned); *n is still returned, so one wait */
int sm_retire_device(sm_ctx *s, const float *pose16, const sm_retire_params *params, float *d_dst12, uint32_t cap, uint32_t *n);
/* Periodic policy for sm_process_frame / _device / _async: after every frame whose new tick is a multiple of `every`, retire at
 * that frame's pose and write the records as one map file "<prefix>_%06u.bin" in GlobalModel::downloadMap's format
 * (u32 count | i32 startId | i32 endId | count*12 f32, src/GlobalModel.cpp:927-932; startId = tick at the previous retirement that
 * wrote a file or 0, endId = tick - 1), which sm_load_map reads.  An empty retirement writes no file; files are numbered 0,1,2..
 * in writing order.  The file is written BEFORE the model is changed: if it cannot be written the frame call returns SM_E_ARG
 * (sm_last_error names the path) and the model is as the frame left it.  That one frame call in `every` waits for the device; all
 * others are exactly what they are without the policy (no extra launch, copy or wait).  every <= 0 or prefix NULL switches the
 * policy off (the default). */
int sm_set_auto_retire(sm_ctx *s, const sm_retire_params *params, int32_t every, const char *path_prefix);
int sm_auto_retire_stats(sm_ctx *s, uint32_t *files, uint64_t *surfels);     /* written so far */

/* ---- paging in (DESIGN.md "4g. Paging in") ----
 * The reverse of retirement: the records of map files (GlobalModel::downloadMap's format: the files of sm_set_auto_retire,
 * sm_save_map) that lie within `radius` of the camera centre come back into the model, so that a camera that returns finds
 * the surfels it left, and a second drive can localise and work inside a saved map set.
 * With c = pose16[12..14] (camera->world, column-major; NULL = the pose of the last processed frame), row q of a file is near
 * iff, in fp32 without fused multiply-add and in this order,
 *     dx, dy, dz = q[0..2] - c[0..2];                   d2 = (dx*dx + dy*dy) + dz*dz
 *     near = d2 <= radius*radius                        (the product rounded to fp32 once; a comparison with a NaN is false,
 *                                                        an infinite d2 is not near)
 * For finite rows and the same c and distance this is exactly the complement of sm_retire's `far`: a surfel retired because it
 * is far is never recalled in the same round.  R = the concatenation of rows[near]: the files in the given order, each file's
 * rows in file order.  m = the rows sm_download_model_aos would return (slots a deferred-compaction cull has killed are not
 * among them, so nothing below depends on compact_period).
 *   SM_RECALL_COUNT  *n = |R|; nothing changes, nothing is written anywhere.
 *   SM_RECALL_COPY   the model becomes concat(m, R), bit for bit; the files are untouched.
 *   SM_RECALL_MOVE   the model as in COPY; every file that lost a row holds rows[!near] in order afterwards, with its startId
 *                    and endId unchanged and its count updated.  A file that lost nothing is not rewritten (bytes and mtime
 *                    unchanged); a file that lost every row stays as a 12-byte file with count 0, so path lists and the
 *                    retirement policy's numbering stay valid (sm_render_*_maps accept such a file).
 * State afterwards (COPY, MOVE): as after sm_upload_model_aos(concat(m, R)) with the exceptions retirement makes:
 * count = offset = |m| + |R|; the tick, the other counters, the frame log, the tracker's pose history, the frame planes and the
 * depth filter's "last depth" are untouched; the index map is not redrawn; the compaction schedule restarts.  Synchronous.
 * Errors.  |m| + |R| > MAX_VERTICES (COPY, MOVE): SM_E_CAPACITY with *n = |R|, model and files unchanged.  SM_E_ARG: NULL
 * ctx / src / n, include_model != 0, NULL paths with n_paths > 0, a NULL path, a path listed twice in MOVE, a radius that is
 * not finite or <= 0, a non-finite pose, an unknown mode, a call between sm_stage_conflict and sm_stage_cull.
 * SM_E_UNSUPPORTED: a sharded or rig context.  Every file's length is checked against its header (12 + 48 * count bytes
 * exactly) before anything changes: a file that fails gives SM_E_ARG, sm_last_error() names it, nothing has changed.
 * Durability of MOVE.  A file's new contents go to "<path>.recall.tmp" in the same directory; all temporaries are complete
 * before the model changes; then the model is appended; then each temporary is renamed over its file.  A temporary that cannot
 * be written: all temporaries are removed, SM_E_ARG, nothing has changed.  A rename that fails AFTER the append: SM_E_ARG names
 * the file, the other files are still renamed, and that file still holds the rows that are now in the model as well -- the
 * outcome of a failure is duplicates, never loss.
 * File index.  The context remembers size, mtime and the box of the finite centres of every file a recall has read; a listed
 * file whose stat() still matches and whose box lies farther than radius from c is neither opened nor read.  Nothing is written
 * next to the files.  SM_RECALL_NO_INDEX=1 turns the index off (an A/B switch: the results are the same either way). */
enum { SM_RECALL_MOVE = 0, SM_RECALL_COPY = 1, SM_RECALL_COUNT = 2 };
typedef struct sm_recall_params { float radius; } sm_recall_params;   /* metres, > 0, finite */
/* radius = 1.5f * c->far_clip: sm_retire's default distance */
int sm_default_recall_params(const sm_config *c, sm_recall_params *p);
/* params NULL = defaults; src->include_model must be 0 */
int sm_recall(sm_ctx *s, const sm_map_source *src, const float *pose16, const sm_recall_params *params, int32_t mode, uint32_t *n);

/* what the last sm_recall of the context (the policy's included) did */
typedef struct sm_recall_stats_t {
    uint32_t files_listed, files_skipped;   /* paths given; of them, left unopened by the file index */
    uint32_t files_read, files_rewritten;   /* opened and streamed through the device; renamed over (MOVE) */
    uint64_t records_read, recalled;        /* records of the files read; |R| */
    uint32_t chunks;                        /* chunks (at most 2^20 records) copied to the device */
    float read_ms, copy_ms;                 /* in fread; in the host-to-device copies (events) */
    float device_ms, write_ms;              /* in the kernels (events); in writing the temporaries (with their device-to-host copies) and renaming */
    float total_ms;                         /* the whole call (host clock) */
} sm_recall_stats_t;   /* (a typedef and a function share C's name space) */
/* SM_E_ARG if the context has made no such call yet */
int sm_recall_stats(sm_ctx *s, sm_recall_stats_t *out);

/* Periodic policy.  It acts only while sm_set_auto_retire is on: on the one frame in `every` that retires, after the retirement
 * has written its file and changed the model, it does a MOVE recall at that frame's pose from all files the retirement policy
 * has written so far ("<prefix>_%06u.bin", 0 .. files - 1, in number order; the file this round has just written is known to hold
 * no near row, because radius <= min_distance at the same pose, and is not read; the file index learns its box from the
 * retirement itself).  It requires 0 < radius <= min_distance of the
 * retirement parameters and min_distance > 0 (so that what a round retires it does not recall): whichever of the two setters is
 * called second checks this, returns SM_E_ARG and leaves the earlier setting alone.  SM_E_CAPACITY of the recall is returned by
 * the frame call: that frame's retirement stands and nothing is recalled.  Frames that do not retire do exactly what they do
 * without the policy.  params NULL or radius <= 0: off (the default). */
int sm_set_auto_recall(sm_ctx *s, const sm_recall_params *params);
int sm_auto_recall_stats(sm_ctx *s, uint32_t *rounds, uint64_t *surfels);    /* recalls made by the policy; surfels they brought back */

/* ---- closing loops: the map warped by surfel time (DESIGN.md "4h. Closing loops") ----
 * A camera that tracks its own pose drifts; when it returns to a place it has mapped, the error it has gathered since is a
 * world->world correction that is fully due now and not at all when it left.  Every surfel record carries its last-update time
 * (m[7]), so a correction that is a function of that time can be applied to the live model and to map files alike.
 * corr12 is n rows of 12 floats: row k is the ROW-major 3x4 world->world transform [R|t] for tick t0 + k (C[0..3] = the first row
 * of R, then t.x) -- the one exception to "column-major float[16]" in this header.
 * Row rule.  For a record m (a row of sm_download_model_aos, or of a map file), in fp32 without fused multiply-add, in this order:
 *     tau = m[7];  sel = tau >= float(t0)                                  (false on a NaN)
 *     d   = tau - float(t0);  k = d >= float(n-1) ? n-1 : (uint32)d         (truncation; +inf -> n-1)
 *     C   = corr12[k]
 *     m'[0] = ((C[0]*m[0] + C[1]*m[1]) + C[2]*m[2]) + C[3]                  (m'[1] from C[4..7], m'[2] from C[8..11])
 *     m'[8] = ( C[0]*m[8] + C[1]*m[9]) + C[2]*m[10]                         (m'[9], m'[10] likewise: no translation, no renormalisation)
 * Every other field of a selected row and every field of an unselected row is bit-identical afterwards; the order is unchanged.
 * The transform is applied as given: rigidity is the caller's business (sm_loop_spread makes rigid tables).
 * Model (src->include_model == 1).  Warped in place, live surfels only: the result is defined on the rows of sm_download_model_aos
 *   and is the same for every compact_period.  The tile boxes are rebuilt for the whole model; the index map is not redrawn; count,
 *   offset, tick, the other counters, the frame log and the compaction schedule are untouched.  Synchronous: waits for frames in
 *   flight and flushes a held-back association, like sm_retire.  The context's stored poses move with the model: the pose of the
 *   last processed frame (both copies: the one sm_retire / sm_recall default to and the moving-object filter's "last pose") and the
 *   tracker's history (tick - 1 and tick - 2).  A stored pose P of tick T is selected by the row rule with tau = float(T) and becomes
 *   C * P, the product computed in double from the widened floats and rounded to float once -- so the next constant-velocity guess
 *   and the filter's relative pose live in the corrected world.
 * Files.  Each listed file is streamed through the device in chunks, its rows warped there and copied back.  A file with at least
 *   one selected row is rewritten through "<path>.warp.tmp" in the same directory, header (count, startId, endId) unchanged; a
 *   file with none is not rewritten (bytes and mtime unchanged).  Durability, in sm_recall MOVE's order: all temporaries are
 *   complete; then the model is warped; then each temporary is renamed over its file.  A temporary that cannot be written: all
 *   temporaries are removed, SM_E_ARG, nothing has changed.  A rename that fails AFTER the model was warped: SM_E_ARG names the
 *   file, the other files are still renamed, and that file's temporary is LEFT IN PLACE -- it holds the warped rows the model now
 *   agrees with, so an operator finishes the job with one mv "<path>.warp.tmp" "<path>"; until then the file holds the unwarped world.
 * File index.  sm_recall's index also remembers the largest non-NaN m[7] of every file a recall or a warp has read or the
 *   retirement policy has written: a listed file whose stat() still matches and whose largest time is below t0 is neither opened
 *   nor read, so a loop closed late in a long drive touches only the recent files.  A rewritten file's entry is refreshed (size,
 *   mtime, the box of the warped rows).  SM_RECALL_NO_INDEX=1 turns this off too (the results are the same either way).
 * Errors.  SM_E_ARG: NULL ctx / src / corr12, n == 0, a non-finite table entry, NULL paths with n_paths > 0, a NULL path, a path
 *   listed twice, a file whose length disagrees with its header (all files are checked before anything changes), a call between
 *   sm_stage_conflict and sm_stage_cull.  SM_E_UNSUPPORTED: a sharded or rig context.  An empty source is a valid no-op. */
typedef struct sm_warp_stats_t {
    uint32_t files_listed, files_skipped, files_read, files_rewritten;   /* paths given; left unopened by the index; streamed; renamed over */
    uint64_t records_read, records_moved;   /* records of the files read; of them, selected */
    uint32_t model_moved, chunks;           /* live surfels selected; chunks (at most 2^20 records) copied to the device */
    float read_ms, copy_ms, device_ms, write_ms, total_ms;   /* fread; host-to-device copies; kernels (files and model); temporaries and renames; the call */
} sm_warp_stats_t;
int sm_warp_by_time(sm_ctx *s, const sm_map_source *src, int32_t t0, uint32_t n, const float *corr12);
/* of the context's last sm_warp_by_time; SM_E_ARG before the first */
int sm_warp_stats(sm_ctx *s, sm_warp_stats_t *out);

/* The table for a loop closure.  D16 (column-major 4x4, world->world) is the correction that is fully due at tick t_b and not at
 * all at t_a; corr12 receives t_b - t_a + 1 rows.  All in double: phi = log(R_D) (axis-angle), w_k = k / (t_b - t_a),
 * R_k = exp(w_k * phi) by Rodrigues' formula, t_k = w_k * t_D; row k = [R_k | t_k] rounded to float once; row 0 is exactly the
 * identity.  (Rotation and translation are interpolated separately, on purpose: the simplest rule a restatement can pin.)  Host
 * only, no device call.  SM_E_ARG: a NULL argument, t_b <= t_a, a non-finite D, a rotation part farther than 1e-3 from
 * orthonormal (max |R^T R - I|, or det < 0), a rotation angle above pi - 1e-3. */
int sm_loop_spread(const float *D16, int32_t t_a, int32_t t_b, float *corr12);

/* The loop measurement: sm_track_frame in every rule, except that the prediction holds only surfels with m[7] <= float(max_time)
 * (false on a NaN) -- the map as it was before the drift, which index_map.vert:45 no longer draws for fusion but a recall has
 * brought back.  With max_time = INT32_MAX there is no window: pose and info equal sm_track_frame's bit for bit.  anchor_time
 * (may be NULL) receives the largest m[7] among the surfels the prediction holds, or -1 with none.  No surfel of the window in
 * view: SM_TRACK_NO_MODEL.  sm_track_debug_old is sm_track_debug with the same window.  (sm_track_frame_rgb's form: sm_track_frame_rgb_window.) */
int sm_track_frame_old(sm_ctx *s, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params, int32_t max_time,
                       float *pose16_out, sm_track_info *info, float *anchor_time);
int sm_track_debug_old(sm_ctx *s, const uint16_t *depth_mm, const float *pose16_eval, int32_t max_time, int32_t *pred_slot, double *sys29);

/* The policy: notice that the camera is back, measure the error, pull the map straight.  pose16 is where the caller believes the
 * camera is (sm_track_frame's answer, say); src lists the map files that are to move with the model (include_model is taken as 1).
 *   1. max_time = tick - 1 - min_age;  T_old = sm_track_frame_old(depth, guess = pose16, tp, max_time).  SM_TRACK_NO_MODEL gives
 *      SM_LOOP_NO_OLD_MAP, any other failure SM_LOOP_TRACK_FAILED.
 *   2. D = T_old * pose16^-1 (the rigid inverse [R^T | -R^T t]), in double, rounded to float once: info->D.  Its size is judged
 *      at the camera: trans = |centre of T_old - centre of pose16|, rot = the angle of D's rotation.  trans < min_trans and
 *      rot < min_rot_deg: SM_LOOP_NONE.  trans > max_trans or rot > max_rot_deg: SM_LOOP_REJECTED.
 *   3. In every case so far nothing has changed and pose16_out = pose16.  Otherwise t_a = int(anchor_time), t_b = tick - 1, the
 *      table is sm_loop_spread(info->D, t_a, t_b), sm_warp_by_time(src, t_a + 1, t_b - t_a, table + 12) moves model, poses and files
 *      (the table without its identity row: the same row for every surfel newer than the anchor, while the surfels OF the anchor
 *      time keep their bits -- an identity row would still turn a -0.0 into +0.0), and pose16_out = D * pose16 (in double from the
 *      widened floats, rounded once): SM_LOOP_CLOSED.
 * Everything last touched up to the anchor time is the old world and stays put, bit for bit; everything after slides along the ramp.
 * Returns SM_OK with the outcome in info->status (info may not be NULL); SM_E_ARG / SM_E_UNSUPPORTED as sm_track_frame_old and
 * sm_warp_by_time, and SM_E_ARG for min_age < 1 or a negative or non-finite bound.  tp, lp NULL = defaults. */
typedef struct sm_loop_params { int32_t min_age; float min_trans, min_rot_deg, max_trans, max_rot_deg; } sm_loop_params;
     /* defaults: time_delta; 0.02 m, 0.05 deg; 2 m, 10 deg */
typedef struct sm_loop_info { int32_t status; sm_track_info track; float D[16]; int32_t t_a, t_b; } sm_loop_info;
enum { SM_LOOP_CLOSED = 0, SM_LOOP_NONE = 1, SM_LOOP_NO_OLD_MAP = 2, SM_LOOP_TRACK_FAILED = 3, SM_LOOP_REJECTED = 4 };
int sm_default_loop_params(const sm_config *c, sm_loop_params *p);
int sm_close_loop(sm_ctx *s, const uint16_t *depth_mm, const float *pose16, const sm_map_source *src, const sm_track_params *tp,
                  const sm_loop_params *lp, float *pose16_out, sm_loop_info *info);

/* ---- closing loops unasked (DESIGN.md "4i. Closing loops unasked") ----
 * Every frame fused before a loop is closed fuses the drifted world into the old one and culls the old one where the two disagree,
 * so a loop has to be noticed and closed BEFORE the frame that sees it is fused.  Four pieces, each usable by hand:
 * The window.  sm_track_frame_window / sm_track_debug_window / sm_track_frame_rgb_window / sm_track_rgb_debug_window are
 *   sm_track_frame / sm_track_debug / sm_track_frame_rgb / sm_track_rgb_debug in every rule, except that the prediction holds only
 *   surfels with m[7] > float(min_time) && m[7] <= float(max_time) (both comparisons false on a NaN).  min_time = INT32_MIN and
 *   max_time = INT32_MAX leave that end open: no comparison is made for an open end, so a NaN time passes exactly where it passes
 *   in the plain form.  Both ends open equals the plain form bit for bit, pose and info; (INT32_MIN, max_time) equals
 *   sm_track_frame_old / sm_track_debug_old bit for bit.  anchor_time (may be NULL) as sm_track_frame_old's.  The debug forms'
 *   pred_slot (may be NULL) is the windowed prediction.  Arguments and errors as the plain forms'.
 * The measurement with colour.  sm_close_loop_rgb is sm_close_loop in every rule, except that step 1 is
 *   sm_track_frame_rgb_window(rgb, depth, guess = pose16, tp, rp, INT32_MIN, tick - 1 - min_age): a street of flat ground and flat
 *   walls, SM_LOOP_TRACK_FAILED for depth alone, can close.  info->track is that call's sm_track_info; the colour tracker's extra
 *   info is not reported.  rp NULL = defaults; a NULL rgb is SM_E_ARG.
 * The census.  sm_old_in_view counts the slots k below the occupied count with the alive bit set, m[7] <= float(max_time) (false on
 *   a NaN) and, with tinv = [R^T | -R^T t] of pose16 in double rounded to float and c = tinv * centre, sm_track_frame's own
 *   prediction gates: near < c.z < far and the pixel (floor(((fx*c.x)/c.z + cx) + 0.5), floor(((fy*c.y)/c.z + cy) + 0.5)) inside the
 *   image.  It is what sm_track_debug_old's prediction would be offered, before the nearest-per-pixel choice.  Synchronous (waits
 *   for frames in flight); changes nothing.  SM_E_ARG: a NULL argument, a non-finite pose, a call between sm_stage_conflict and
 *   sm_stage_cull.  SM_E_UNSUPPORTED: a sharded or rig context.
 * The policy.  While sm_set_auto_loop is on, sm_track_frame and sm_track_frame_rgb (and so the callers that track first and fuse
 *   second) do the following, with T = tick and split = T - 1 - loop.min_age:
 *   1. The pose is tracked in the young window (split, INT32_MAX) -- while split < 0 in the plain prediction, bit for bit.  A status
 *      other than SM_TRACK_OK returns as without the policy: no census, no attempt.
 *   2. A census is due when split >= 0, T % every == 0 and T >= rest_until (0 at first).  n_old = sm_old_in_view(tracked pose, split);
 *      `checked` counts the censuses.  n_old < min_old: nothing more happens, pose16_out is the tracked pose.
 *   3. Otherwise one attempt: sm_close_loop (from sm_track_frame) or sm_close_loop_rgb (from sm_track_frame_rgb) with pose16 = the
 *      tracked pose, this call's tracker parameters and the policy's `loop`.  The source is the model, the paths of `src` and every
 *      file the retirement policy has written so far ("<prefix>_%06u.bin"), a path in both lists once.  On SM_LOOP_CLOSED
 *      pose16_out is the corrected pose, so the caller fuses in the straightened map; on every other outcome the tracked pose.
 *   4. After every attempt, whatever its outcome: rest_until = T + rest.
 *   sm_track_info is sm_track_frame's own, of the young-window track; the loop's outcome is read from sm_auto_loop_stats.  An error
 *   of the attempt (a map file that cannot be read, say) is returned by the tracker call and counted as `failed`.
 *   With the policy off (the default; p NULL switches it off) every entry point is exactly what it is without it.  src may be NULL
 *   (no files of the caller's); its paths are copied.  Setting the policy clears its tally and rest_until.
 *   SM_E_ARG: a NULL ctx, every < 1, rest < 0, loop as sm_close_loop rejects it, a NULL path, a path listed twice.
 *   SM_E_UNSUPPORTED: a sharded or rig context; sm_shard_stream_configure and sm_rig_configure switch the policy off.
 *   "Bit for bit" above speaks of results: with the policy on and split < 0 the call also computes the anchor time it does not
 *   report (one small kernel and a 4-byte read-back), and a parameter the tracker rejects is named in sm_last_error under
 *   sm_track_frame_window / sm_track_frame_rgb_window, the entry points the policy tracks through. */
int sm_track_frame_window(sm_ctx *s, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params, int32_t min_time,
                          int32_t max_time, float *pose16_out, sm_track_info *info, float *anchor_time);
int sm_track_debug_window(sm_ctx *s, const uint16_t *depth_mm, const float *pose16_eval, int32_t min_time, int32_t max_time,
                          int32_t *pred_slot, double *sys29);
int sm_track_frame_rgb_window(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params,
                              const sm_track_rgb_params *rgb_params, int32_t min_time, int32_t max_time, float *pose16_out,
                              sm_track_info *info, sm_track_rgb_info *rgb_info, float *anchor_time);
int sm_track_rgb_debug_window(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16_eval, int level, int which,
                              int32_t min_time, int32_t max_time, int32_t *pred_slot, double *sys29);
int sm_close_loop_rgb(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16, const sm_map_source *src,
                      const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_loop_params *lp, float *pose16_out,
                      sm_loop_info *info);
int sm_old_in_view(sm_ctx *s, const float *pose16, int32_t max_time, uint32_t *n);
typedef struct sm_auto_loop_params {
    int32_t every, rest;      /* 1: a census on every tick that is a multiple of it; 10: ticks without a census after an attempt */
    uint32_t min_old;         /* 1000 (sm_track_params::min_inliers): old surfels in view below which no attempt is made */
    sm_loop_params loop;      /* sm_default_loop_params */
} sm_auto_loop_params;
typedef struct sm_auto_loop_stats_t {
    uint32_t checked, attempts;                            /* censuses taken; of them, followed by an attempt */
    uint32_t closed, none, rejected, failed, no_old_map;   /* the attempts by outcome (failed: SM_LOOP_TRACK_FAILED or an error) */
    uint32_t last_census;                                  /* n_old of the last census */
    sm_loop_info last;                                     /* of the last attempt that returned SM_OK */
} sm_auto_loop_stats_t;
int sm_default_auto_loop_params(const sm_config *c, sm_auto_loop_params *p);
int sm_set_auto_loop(sm_ctx *s, const sm_auto_loop_params *p, const sm_map_source *src);
int sm_auto_loop_stats(sm_ctx *s, sm_auto_loop_stats_t *out);

/* ---- pose search before the tracker (DESIGN.md "4j. Pose search") ----
 * The trackers converge from a few decimetres; a drive that returns after retirement and recall has drifted by metres.  The search
 * scores a grid of candidate poses against the windowed prediction, refines the best on a finer grid and hands the winners to the
 * trackers.  Three layers, each usable by hand:
 * The score.  sm_score_poses_window takes sm_track_frame_window's prediction (at T_prev, the same window rules and open ends) and
 *   the grid points (0, stride, 2*stride, ...) x (0, stride, ...) of the depth image with the tracker's vertex and normal rule
 *   (tp->pixel_stride is ignored).  scores[i] counts the grid points that pass, under candidate i (cand16 + 16*i, camera->world,
 *   column-major), the tracker's own association tests in the same fp32 expressions: vertex valid, c.z > 0, the pixel inside the
 *   image, a surfel at the pixel, |T v - p_m| <= dist_thresh, dot(R n, n_m) >= cos(angle_thresh) -- and, with rgb non-NULL,
 *   fabsf(Y_f - Y_m) <= colour_thresh, Y_f the luminance of the grid point's own pixel and Y_m that of the surfel's colour word,
 *   both by sm_track_frame_rgb's rule.  With rgb NULL, stride 1 and default tp, scores[i] is value 28 of sm_track_debug_window at the
 *   same pose.  tp NULL = defaults.  Synchronous (waits for frames in flight); changes nothing.  No processed frame or an empty
 *   model: every score is 0.  SM_E_ARG: a NULL argument (rgb aside), n == 0, n > 2^20, stride < 1 or > min(W, H), a non-finite
 *   candidate, colour_thresh < 0 or NaN, tp as the trackers reject it, a call between sm_stage_conflict and sm_stage_cull.
 * The search.  sm_search_pose, with sp NULL = sm_default_search_params:
 *   Axes.  Six axes in the order rot x, rot y, rot z (rot_half_deg / rot_step_deg, about the camera's x right, y down, z forward),
 *     trans x, trans y, trans z (trans_half / trans_step, metres).  An axis is active iff half > 0 and step > 0; it has
 *     n = 2*floor(half/step) + 1 offsets (k - (n-1)/2) * step, k = 0..n-1, in double; an inactive axis the single offset 0.
 *   Level 0.  Nested loops over the six axes in that order, the last fastest.  Delta = [Ry(b) * Rx(a) * Rz(c) | t] in double for
 *     rotation offsets (a, b, c) in degrees and translation t; candidate = centre16 * Delta (column-major rigid product in double,
 *     ((a0*b0 + a1*b1) + a2*b2) + a3), rounded to float once.  More than 2^20 candidates: SM_E_ARG.  Scored at stride0.
 *   Ranking.  Score descending, then index ascending; a candidate is kept only if score * stride^2 >= tp->min_inliers (64-bit);
 *     the first top_k kept go on.  None kept at any level: status SM_TRACK_LOST, pose16_out = centre16.
 *   Level l+1 (levels - 1 of them).  For each kept candidate in rank order, the same nesting with offsets k * step / refine^(l+1),
 *     k = -refine..refine, on the active axes, right-multiplied onto that candidate's float pose widened to double; all of them
 *     scored in one call at stride max(1, stride0 >> (l+1)) and ranked as one list.
 *   Refinement.  Each kept candidate of the last level, in rank order, is the guess of sm_track_frame_rgb_window (rgb given; rp
 *     NULL = defaults) or sm_track_frame_window (rgb NULL) with the caller's tp and window.  The answer is the SM_TRACK_OK result
 *     with the most inliers, ties to the earlier rank.  None OK: the status of rank 0's track, pose16_out = centre16.
 *   No processed frame, an empty model or no surfel of the window in view: SM_TRACK_NO_MODEL, pose16_out = centre16.
 *   info (may be NULL): status; levels_run; candidates[l] and best_score[l] (the largest score) of each level run; winner_rank
 *   (-1: none); track, start (the guess the winner started from) and anchor_time of the winner -- of rank 0's track when none is
 *   OK; score_ms (device time of the scoring kernels) and total_ms (host clock).  The candidates are ranked on the host.
 *   SM_E_ARG: as the score's and the trackers', levels outside 1..4, refine < 1, top_k outside 1..16, stride0 < 1, a negative or
 *   non-finite half, step or colour_thresh, a level with more than 2^20 candidates.
 * The policies.  sm_close_loop_search is sm_close_loop (rgb NULL) / sm_close_loop_rgb in every rule, except that step 1 is
 *   sm_search_pose(centre = pose16, window (INT32_MIN, tick - 1 - min_age)): T_old and the anchor are the winner's, info->track the
 *   winner's sm_track_info.  SM_TRACK_NO_MODEL gives SM_LOOP_NO_OLD_MAP, any other failure SM_LOOP_TRACK_FAILED.  The default box
 *   reaches sqrt(2^2 + 2^2) = 2.8 m, past sm_loop_params' default max_trans = 2: a caller who wants a wider loop raises lp.
 *   sm_set_auto_loop_search(sp): while the auto-loop policy is on, its attempt (step 3) is sm_close_loop_search with these
 *   parameters, with rgb when the call came from sm_track_frame_rgb.  NULL = off (the default): the attempt is what it was.  The
 *   census, the rest and the statistics are unchanged.  May be set before or after sm_set_auto_loop, which leaves it alone.
 * SM_E_UNSUPPORTED, all of them: a sharded or rig context. */
typedef struct sm_search_params {
    int32_t levels;           /* 2 (1..4) */
    float trans_half[3];      /* camera x right, y down, z forward: 2, 0, 2 m */
    float trans_step[3];      /* 0.25 m each */
    float rot_half_deg[3];    /* about camera x, y, z: 0, 3, 0 */
    float rot_step_deg[3];    /* 0.5 each */
    int32_t refine;           /* 4: level l+1 has steps / refine and spans +-1 step of level l on every active axis */
    int32_t stride0;          /* 8: level l scores at max(1, stride0 >> l) */
    int32_t top_k;            /* 4 (1..16) */
    float colour_thresh;      /* 0.1 */
} sm_search_params;
typedef struct sm_search_info {
    int32_t status;           /* SM_TRACK_* */
    int32_t levels_run;
    uint32_t candidates[4];
    uint32_t best_score[4];
    int32_t winner_rank;      /* -1: none */
    sm_track_info track;
    float start[16];
    float anchor_time;
    float score_ms, total_ms;
} sm_search_info;
#define SM_SEARCH_MAX_CANDIDATES (1u << 20)
int sm_default_search_params(sm_search_params *p);
int sm_score_poses_window(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *cand16, uint32_t n,
                          const sm_track_params *tp, int32_t stride, float colour_thresh, int32_t min_time, int32_t max_time,
                          uint32_t *scores);
int sm_search_pose(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *centre16, const sm_track_params *tp,
                   const sm_track_rgb_params *rp, const sm_search_params *sp, int32_t min_time, int32_t max_time, float *pose16_out,
                   sm_search_info *info);
int sm_close_loop_search(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16, const sm_map_source *src,
                         const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_loop_params *lp, const sm_search_params *sp,
                         float *pose16_out, sm_loop_info *info);
int sm_set_auto_loop_search(sm_ctx *s, const sm_search_params *sp);

/* ---- lidar sweeps (DESIGN.md "4k. Lidar sweeps") ----
 * What a spinning lidar at a pose would measure in the map: every beam of a spherical grid against every live surfel as an oriented
 * disc, the nearest return per beam.  The renderers above are pinhole rasterisers and return no range; this is the second sensor.
 * Sensor.  n_el rows x n_az columns.  The sensor frame is the camera's (x right, y down, z forward); pose16 is sensor->world,
 *   column-major.  Azimuth runs from +z towards +x, elevation is positive upwards.
 * Directions.  Beam (row i, column j): a = (az0_deg + j*az_step_deg) * pi/180, e = el_deg[i] * pi/180, pi = 3.14159265358979323846,
 *   d = (sin a cos e, -sin e, cos a cos e), in double from the widened floats, each component rounded to float once.
 *   sm_lidar_directions (host only, no context) writes the table, n_el * n_az * 3 floats, row-major; the sweep uses exactly it.
 * Surfel in the sensor frame.  tinv = [R^T | -R^T t] of pose16 in double, rounded to float.  c = tinv * centre by sm_old_in_view's
 *   rule, each row ((m[r]*x + m[r+4]*y) + m[r+8]*z) + m[r+12]; m = the rotation rows of tinv applied to the stored normal in the same
 *   order, (m[r]*x + m[r+4]*y) + m[r+8]*z, not normalised; r = the stored radius.  Everything fp32, no contraction, as written.
 * Hit.  For a beam d and a surfel (c, m, r):
 *     den = (m.x*d.x + m.y*d.y) + m.z*d.z        num = (m.x*c.x + m.y*c.y) + m.z*c.z        t = num / den        q_i = t*d_i - c_i
 *     hit = t >= min_range && t <= max_range && ((q.x*q.x + q.y*q.y) + q.z*q.z) <= r*r
 *   Every comparison is false on a NaN; a grazing beam (den == 0) gives an infinity or a NaN and no hit: no epsilon.  Discs are
 *   two-sided.  The beam's return is the hitting surfel with the smallest t, ties to the lower id (t > 0: its float bits order).
 * Which surfels, which ids.  The live ones (alive bit set) with conf >= min_conf (false on a NaN).  Ids are the rows of
 *   sm_download_model_aos, exactly as sm_render_model's id plane; the same forced compaction on read-back is the only side effect.
 * Outputs, row-major n_el x n_az (per sweep); any but `range` may be NULL:
 *     range  float   t                                                            empty: 0
 *     id     int32   surfel id                                                    empty: -1
 *     rgb    3 x u8  bytes >>16, >>8, >>0 of the surfel's colour word             empty: 0
 *     sem    u8      class + 1, as sm_render_image's                              empty: 0
 * The calls are synchronous and wait for frames in flight; the model, the counters, the tick, the frame log and the tracker
 *   state are untouched.
 * sm_lidar_sweep_maps is sm_render_image_maps rule for rule: the global id is the position in the concatenation (files in order,
 *   then the live model); every output equals sm_lidar_sweep of a context holding that concatenation, bit for bit; the result
 *   depends neither on the chunking nor on the sweeps per pass; all headers are checked first and a bad file gives SM_E_ARG with the
 *   outputs unwritten; more than 2^31 - 1 surfels: SM_E_CAPACITY; n_sweeps == 0 checks the set only.  poses16: n_sweeps poses,
 *   outputs n_sweeps planes each.  A pass sweeps as many poses as fit the key budget (1 GiB of 8-byte keys; SM_LIDAR_KEY_MB
 *   overrides it).  SM_LIDAR_NO_CULL=1 turns the per-block range test off and SM_LIDAR_LANE_BEAMS sets the beams a lane tests by
 *   itself (A/B switches: the outputs are the same either way).
 * sm_lidar_stats: what the last sweep call of the context did (SM_E_ARG before the first).
 * Errors.  SM_E_ARG: a NULL ctx, sensor, pose or range; a sensor outside the limits in the struct below (non-increasing elevations
 *   included); a non-finite pose; a call between sm_stage_conflict and sm_stage_cull; the file errors of sm_render_image_maps.
 *   SM_E_UNSUPPORTED: a sharded or rig context. */
typedef struct sm_lidar_sensor {
    int32_t n_az, n_el;            /* columns, rows; n_az * n_el <= 2^22 */
    float az0_deg, az_step_deg;    /* column j looks at azimuth az0 + j*step; step > 0; n_az*step <= 360 */
    const float *el_deg;           /* n_el elevations, strictly increasing, each inside (-90, 90) */
    float min_range, max_range;    /* metres, 0 < min_range <= max_range, finite */
    float min_conf;                /* a surfel takes part iff conf >= min_conf (false on a NaN); default 0 */
} sm_lidar_sensor;
typedef struct sm_lidar_stats_t {
    uint64_t surfels;              /* offered: live slots and records read, once per pass and source */
    uint64_t tests;                /* exact tests made */
    uint64_t wide;                 /* (surfel, sweep) pairs whose footprint went to a whole wave */
    uint64_t blocks_skipped;       /* (block of 256 records, sweep) pairs the range test skipped */
    uint32_t chunks, passes;       /* chunks (at most 2^20 records) copied to the device; passes over the files */
    float read_ms, copy_ms;        /* in fread; in the host-to-device copies (events) */
    float device_ms;               /* in the kernels (events) */
    float total_ms;                /* the whole call (host clock) */
} sm_lidar_stats_t;
#define SM_LIDAR_MAX_BEAMS (1u << 22)
/* 360 x 16 at 1 deg from az0 = 0, el = -15..0 step 1 (a static table), 1..60 m, min_conf 0 */
int sm_default_lidar_sensor(sm_lidar_sensor *p);
int sm_lidar_directions(const sm_lidar_sensor *sn, float *dir3);
int sm_lidar_sweep(sm_ctx *s, const sm_lidar_sensor *sn, const float *pose16, float *range, int32_t *id, uint8_t *rgb, uint8_t *sem);
int sm_lidar_sweep_maps(sm_ctx *s, const sm_map_source *src, const sm_lidar_sensor *sn, const float *poses16, uint32_t n_sweeps,
                        float *range, int32_t *id, uint8_t *rgb, uint8_t *sem);
int sm_lidar_stats(sm_ctx *s, sm_lidar_stats_t *out);

/* ---- place recognition (DESIGN.md "4l. Place recognition") ----
 * Everything above starts from the believed pose; after more drift than the pose search's box reaches, none of it finds the place
 * again.  A fern code (Glocker et al., the global loops of ElasticFusion) is a short binary code of a frame, computed from block
 * means of colour and depth; the codes of keyframes live in a database on the device with their poses and times; a new frame is
 * matched against all of them, and the matched keyframe's pose is handed to the geometric machinery, which verifies the match.
 * The table (host only, no context).  sm_fern_params: n_ferns a multiple of 32 in 32..2048, cell one of 4, 8, 16, 32,
 *   0 <= depth_lo_mm < depth_hi_mm <= 65535.  sm_default_fern_params: 512, 8, seed 1, the config's near and far clip in millimetres
 *   ((int32)(clip * 1000.0f), clamped to 0..65535).  sm_fern_table writes n_ferns records.  gw = width / cell, gh = height / cell
 *   (integer division; both must be >= 1; the remainder columns and rows belong to no cell).  The generator is splitmix64 on a
 *   uint64 state that starts at `seed`; one draw is
 *       state += 0x9E3779B97F4A7C15;  z = state;  z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;  z = (z ^ z>>27) * 0x94D049BB133111EB;
 *       z ^= z>>31;  draw(r) = ((z >> 32) * r) >> 32
 *   and a fern takes six draws in this order: x = draw(gw), y = draw(gh), tr = draw(255), tg = draw(255), tb = draw(255),
 *   td = depth_lo_mm + draw(depth_hi_mm - depth_lo_mm).
 * The code.  sm_set_ferns builds the table for the context's image size and creates an empty database; p NULL frees both (the
 *   default).  Setting it again replaces table and database and switches sm_set_auto_place off.  sm_reset empties the database: the map
 *   it indexes is gone.
 *   sm_fern_encode takes host images as sm_track_frame_rgb takes them (rgb H*W*3 u8, R first; depth_mm H*W u16); rgb may be NULL;
 *   code receives n_ferns / 8 uint32.  sm_fern_encode_device takes images resident in this context's device memory (depth 2-byte
 *   aligned) and is synchronous too.  The cell of fern f is columns [x*cell, (x+1)*cell) of rows [y*cell, (y+1)*cell).  Its means:
 *       R, G, B = the sum of the cell^2 bytes of the channel / cell^2                       (integer division)
 *       D       = the sum of the non-zero depth_mm of the cell / their count                 (integer division, 32 bits; 0 with none)
 *   of the raw inputs: no stereo border, no clip, no filter.  The fern's nibble: bit 0 = R > tr, bit 1 = G > tg, bit 2 = B > tb,
 *   bit 3 = D > td; with rgb NULL the three colour bits are 0.  Fern f occupies bits 4*(f&7) .. 4*(f&7)+3 of word f>>3.
 * The database.  Codes are stored keyframe-major on the device, each with an int32 time; the poses (column-major float[16]) stay
 *   on the host; the capacity grows geometrically up to SM_FERN_MAX_KEYFRAMES (beyond: SM_E_CAPACITY).  sm_fern_add appends one
 *   keyframe (index, may be NULL, receives its number); sm_fern_count reports how many there are; sm_fern_download reads them back
 *   in order (codes count * n_ferns/8 uint32, poses16 count * 16, times count; any pointer may be NULL).
 *   sm_fern_save writes one file, little-endian, no padding:
 *       offset 0 u32 magic 0x4E524653 | 4 u32 version 1 | 8 i32 n_ferns | 12 i32 cell | 16 u64 seed | 24 i32 depth_lo_mm |
 *       28 i32 depth_hi_mm | 32 i32 width | 36 i32 height | 40 u32 count | 44 u32 0 | 48 count records, each
 *       i32 time | 16 f32 pose | n_ferns/8 u32 code
 *   through "<path>.tmp" in the same directory, renamed over `path` once complete.  sm_fern_load replaces the database by a file's;
 *   a file that is missing, whose magic, version, parameters or image size differ from the context's, whose count exceeds
 *   SM_FERN_MAX_KEYFRAMES or whose length is not exactly 48 + count * (68 + n_ferns/2): SM_E_ARG, sm_last_error() names it, and
 *   nothing has changed.
 * The match.  dis(k) = the number of ferns whose nibbles differ between `code` and keyframe k.  Among the keyframes with
 *   time > min_time && time <= max_time (integer compares) the answer is the smallest dis, ties to the lower index; none in the
 *   window: index = -1, dis = UINT32_MAX.  dis_all (may be NULL; count entries) receives dis(k) of every keyframe, whatever its time.
 * A prediction somewhere else.  sm_search_pose_at is sm_search_pose in every rule, except that the prediction camera of the score
 *   and of the refining trackers is pred16 (camera->world) instead of T_prev; the trackers' guess and history are untouched.  With
 *   pred16 bit-equal to T_prev it equals sm_search_pose bit for bit, pose and info.  sm_close_loop_at is sm_close_loop_search in
 *   every rule, except that step 1 is sm_search_pose_at(pred = place16, centre = place16, window (INT32_MIN, tick - 1 - min_age)):
 *   D = T_old * pose16^-1, and the judgement against lp, the ramp, the warp and pose16_out are as there.  A matched keyframe's pose
 *   is such a place.
 * Keyframe poses move with the map.  sm_warp_by_time (with include_model) applies to every stored keyframe pose the rule it applies
 *   to the context's other stored poses: a keyframe of time T is selected by the row rule with tau = float(T) and becomes C * P, in
 *   double from the widened floats, rounded once; unselected keyframes keep their bits.
 * All of these are synchronous, change nothing in the model, its counters, the tick, the frame log or the tracker state (the warp
 *   aside), and wait for what they need of the stream only.
 * SM_E_ARG: a NULL argument where none is allowed, parameters outside the rules above, a context without ferns (all but
 *   sm_set_ferns), a non-finite pose, a call between sm_stage_conflict and sm_stage_cull.
 *   SM_E_UNSUPPORTED: a sharded or rig context, checked right after the NULL context and before every other argument. */
typedef struct sm_fern_params {
    int32_t n_ferns;               /* 512 */
    int32_t cell;                  /* 8 */
    uint64_t seed;                 /* 1 */
    int32_t depth_lo_mm, depth_hi_mm;   /* near_clip, far_clip in millimetres */
} sm_fern_params;
typedef struct sm_fern { uint16_t x, y, tr, tg, tb, td; } sm_fern;   /* cell column, cell row, the four thresholds */
#define SM_FERN_MAX_KEYFRAMES (1u << 20)
int sm_default_fern_params(const sm_config *c, sm_fern_params *p);
int sm_fern_table(const sm_fern_params *p, int32_t width, int32_t height, sm_fern *out);
int sm_set_ferns(sm_ctx *s, const sm_fern_params *p);
int sm_fern_encode(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, uint32_t *code);
int sm_fern_encode_device(sm_ctx *s, const uint8_t *d_rgb, const uint16_t *d_depth_mm, uint32_t *code);
int sm_fern_add(sm_ctx *s, const uint32_t *code, const float *pose16, int32_t time, uint32_t *index);
int sm_fern_count(sm_ctx *s, uint32_t *n);
int sm_fern_download(sm_ctx *s, uint32_t *codes, float *poses16, int32_t *times);
int sm_fern_save(sm_ctx *s, const char *path);
int sm_fern_load(sm_ctx *s, const char *path);
int sm_fern_match(sm_ctx *s, const uint32_t *code, int32_t min_time, int32_t max_time, int32_t *index, uint32_t *dis, uint32_t *dis_all);
int sm_search_pose_at(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pred16, const float *centre16,
                      const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_search_params *sp, int32_t min_time,
                      int32_t max_time, float *pose16_out, sm_search_info *info);
int sm_close_loop_at(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16, const float *place16,
                     const sm_map_source *src, const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_loop_params *lp,
                     const sm_search_params *sp, float *pose16_out, sm_loop_info *info);
/* The policy.  sm_set_auto_place needs sm_set_ferns first (SM_E_ARG otherwise; sm_set_ferns(NULL) switches it off with the ferns);
 * p NULL switches it off (the default); setting it clears its tally and rest_until.  While it is on, sm_track_frame and
 * sm_track_frame_rgb do the following after their existing work, the policy of sm_set_auto_loop included:
 *   1. If the track's status is not SM_TRACK_OK, or the auto-loop policy closed a loop on this call: nothing.
 *   2. The frame is encoded from the tracker's device copies of its images (rgb NULL from sm_track_frame): `encoded` counts.
 *      T = tick, split = T - 1 - loop.min_age.
 *   3. One match launch gives the best over all keyframes (dis_any) and the best with time <= split (k, dis_old), neither with a
 *      lower end (a keyframe of time INT32_MIN, which sm_fern_match's strict min_time can never name, takes part): `matched` counts
 *      the frames with k >= 0 and float(dis_old) <= match_below * float(n_ferns) (fp32).
 *   4. An attempt is made if T % every == 0, T >= rest_until, the frame matched, and the centres of P_k and of the tracked pose are
 *      more than min_jump apart (in double from the floats: sqrt((dx*dx + dy*dy) + dz*dz) > min_jump).  If the recall policy is on
 *      and the retirement policy has written files, first one SM_RECALL_MOVE around P_k from those files with that policy's radius.
 *      Then sm_close_loop_at(pose16 = the tracked pose, place16 = P_k, this call's tracker parameters, `loop`, `search`) over the
 *      sources of the auto-loop policy's attempt (its caller's files while it is on, and the retirement policy's).  SM_LOOP_CLOSED
 *      hands back the corrected pose, anything else the tracked pose; rest_until = T + rest whatever the outcome.  An error of the
 *      recall or of the attempt is returned by the tracker call and counted as `failed`.
 *   5. If the database is empty or float(dis_any) > add_above * float(n_ferns), the frame becomes a keyframe: its code, the pose
 *      the call returns and time T -- after step 4, so a corrected pose is what is stored.
 * With the policy off every entry point is exactly what it is without it.
 * SM_E_ARG: a NULL ctx, every < 1, rest < 0, add_above or match_below outside [0, 1] or not finite, min_jump negative or not
 * finite, loop as sm_close_loop rejects it, search as sm_search_pose rejects it.  SM_E_UNSUPPORTED: a sharded or rig context. */
typedef struct sm_auto_place_params {
    int32_t every, rest;           /* 1: a check on every tick that is a multiple of it; 10: ticks without an attempt after one */
    float add_above;               /* 0.2: fraction of n_ferns above which a frame becomes a keyframe */
    float match_below;             /* 0.3: fraction of n_ferns up to which an old keyframe counts as a match */
    float min_jump;                /* 2 m: nearer than this the loop policy of 4i is left to handle it */
    sm_loop_params loop;           /* sm_default_loop_params with max_trans 50 m, max_rot_deg 45 */
    sm_search_params search;       /* sm_default_search_params: the search at the matched place */
} sm_auto_place_params;
typedef struct sm_auto_place_stats_t {
    uint32_t encoded, added, matched, attempts;
    uint32_t closed, none, rejected, failed, no_old_map;   /* the attempts by outcome (failed: SM_LOOP_TRACK_FAILED or an error) */
    int32_t last_k;                /* of the last match: the old keyframe, -1 with none */
    uint32_t last_dis;             /* ... and its dissimilarity (UINT32_MAX with none) */
    sm_loop_info last;             /* of the last attempt that returned SM_OK */
} sm_auto_place_stats_t;
int sm_default_auto_place_params(const sm_config *c, sm_auto_place_params *p);
int sm_set_auto_place(sm_ctx *s, const sm_auto_place_params *p);
int sm_auto_place_stats(sm_ctx *s, sm_auto_place_stats_t *out);

/* ---- stereo depth (DESIGN.md "4m. Stereo depth") ----
 * Everything above takes a dense depth image.  This stage makes one from a rectified stereo pair: semi-global matching
 * (Hirschmueller) over a census transform, all integers up to the final division, no weights.  Inputs: rgb_left and rgb_right of
 * the context's size, each H*W*3 u8, R first.  Parameters (sm_stereo_params): max_disp D one of 64, 128, 192, 256; paths 4 or 8;
 * 1 <= p1 <= p2 <= 1023; uniqueness a percentage in 0..100; lr_max_diff in 0..D; baseline in metres, finite, > 0.
 * sm_default_stereo_params: 128, 8, 7, 86, 5, 1, 0.54.
 *   1. Luminance.  Y = (77*R + 150*G + 29*B + 128) >> 8, a u8 per pixel, for both images.
 *   2. Census.  The window is 9 wide and 7 high, coordinates clamped to the image (the edge is replicated).  code = 0; for dy in
 *      -3..3 (outer loop), dx in -4..4 (inner loop), skipping (0, 0): code = (code << 1) | (Y[y+dy][x+dx] < Y[y][x]).  62 bits in a
 *      uint64.
 *   3. Matching cost.  For d in 0..D-1: C(x, y, d) = popcount(cL(x, y) ^ cR(x-d, y)) if x - d >= 0, otherwise 64.
 *   4. Path cost along direction r = (dx, dy), with p' = p - r.  p' outside the image: L_r(p, d) = C(p, d).  Otherwise, with
 *      m = min_k L_r(p', k):  L_r(p, d) = C(p, d) + min(L_r(p', d), L_r(p', d-1) + p1, L_r(p', d+1) + p1, m + p2) - m, where the terms
 *      with d-1 < 0 or d+1 >= D are absent.  The directions in order: (1,0), (-1,0), (0,1), (0,-1); with paths == 8 also (1,1), (-1,1),
 *      (1,-1), (-1,-1).  S(p, d) is the sum over the directions, a u16: the bounds keep it at most 8 * (64 + 1023).
 *   5. Winner.  d* is the lowest d with the least S(p, d).  Right view: dR(xr, y) is the lowest d with the least S(xr+d, y, d) over
 *      the d with xr + d < W.  A pixel is valid iff d* >= 1, x - d* >= 0, no d with |d - d*| > 1 has
 *      S(p, d) * (100 - uniqueness) < S(p, d*) * 100 (32-bit integers), and |dR(x - d*, y) - d*| <= lr_max_diff.
 *   6. Sub-pixel, in sixteenths.  For 1 <= d* <= D-2: a = S(d*-1) - S(d*), b = S(d*+1) - S(d*), den = a + b; den > 0:
 *      q = 16*d* - 8 + (32*a + den) / (2*den) (non-negative integer division); den == 0: q = 16*d*.  For d* == D-1: q = 16*d*.
 *      Invalid pixels have q = 0.  disp16 is q as a u16.
 *   7. Depth.  On the host, in double: K = ((double)fx * (double)baseline) * 16000.0, fx the context's float.  Per valid pixel, in
 *      double: mm = floor(K / (double)q + 0.5); mm > 65535 gives 0, otherwise depth_mm = (uint16)mm.  Invalid pixels have 0.
 * No stereo border, clip or filter is applied here: the fusion's own stereo_border and preprocess chain do that downstream, as
 * they do for a depth image from a file.
 * sm_set_stereo allocates the two census planes, the cost volume and the volume of S (W*H*D*2 bytes) and the two outputs on the
 *   device; p NULL frees them (the default).  Setting it again replaces them.  If an allocation fails: SM_E_HIP, and the context is
 *   left without stereo.
 * sm_stereo_depth takes host images and waits; either output may be NULL.  sm_stereo_depth_device takes images resident on the
 *   context's GPU and outputs that are device pointers the caller owns (2-byte aligned, either may be NULL); its work is enqueued
 *   on the context's stream and not waited for, so a following sm_process_frame_device(ctx, d_left, d_depth_mm_out, ...) sees
 *   the result.
 * sm_stereo_download returns the intermediates of the last call (zeros before the first): the two census planes (H*W uint64 each)
 *   and the volume of S (row-major y, x, d; H*W*D uint16).  Any pointer may be NULL.  Synchronous.
 * These entry points change nothing in the model, its counters, the tick, the frame log or the tracker state.
 * SM_E_ARG: a NULL context or image, parameters outside the ranges above, a misaligned output, a context without stereo (every call
 *   except sm_set_stereo and the defaults), a call between sm_stage_conflict and sm_stage_cull.
 *   SM_E_UNSUPPORTED: a sharded or rig context, checked right after the NULL context and before every other argument. */
typedef struct sm_stereo_params {
    int32_t max_disp;              /* D: 64, 128, 192 or 256; default 128 */
    int32_t paths;                 /* 4 or 8; default 8 */
    int32_t p1, p2;                /* 1 <= p1 <= p2 <= 1023; defaults 7, 86 */
    int32_t uniqueness;            /* percent, 0..100; default 5 */
    int32_t lr_max_diff;           /* 0..D; default 1 */
    float   baseline;              /* metres, finite, > 0; default 0.54 */
} sm_stereo_params;
int sm_default_stereo_params(const sm_config *c, sm_stereo_params *p);
int sm_set_stereo(sm_ctx *s, const sm_stereo_params *p);
int sm_stereo_depth(sm_ctx *s, const uint8_t *rgb_left, const uint8_t *rgb_right, uint16_t *depth_mm_out, uint16_t *disp16_out);
int sm_stereo_depth_device(sm_ctx *s, const uint8_t *d_left, const uint8_t *d_right, uint16_t *d_depth_mm_out, uint16_t *d_disp16_out);
int sm_stereo_download(sm_ctx *s, uint64_t *census_left, uint64_t *census_right, uint16_t *volume);

/* ---- lidar depth (DESIGN.md "4z. Lidar depth") ----
 * The depth image of a frame from a lidar scan: the points are z-buffered into the camera, and the sparse image is completed to a
 * dense one by a fixed chain of morphological steps, in the manner of IP-Basic (Ku et al. 2018), all in integers.
 * Inputs: points, n x 4 fp32 (x, y, z, reflectance: the layout of a KITTI velodyne file), n <= SM_LIDAR_DEPTH_MAX_POINTS, n = 0
 * allowed; T, 16 floats, row-major 4 x 4, lidar frame to camera frame, of which rows 0..2 are used; fx, fy, cx, cy, W, H the
 * context's.  All float work is fp32, every operation rounded once, in the order written, nothing contracted.
 *   1. Project, per point i.  X = ((T[0]*x + T[1]*y) + T[2]*z) + T[3]; Y with row 1 and Z with row 2 in the same way.  The point
 *      is dropped unless X, Y, Z are finite and min_z <= Z <= max_z.  u = (fx*X)/Z + cx, v = (fy*Y)/Z + cy; dropped unless u and v
 *      are finite, -0.5 <= u < W-0.5 and -0.5 <= v < H-0.5.  px = (int)floorf(u + 0.5f), py likewise,
 *      mm = (int)floorf(Z*1000.0f + 0.5f); dropped unless 1 <= mm <= 65535, px < W and py < H.  Splat: a 64-bit minimum of
 *      key = (uint64)mm << 32 | i per pixel: the nearest point wins, among equal mm the lowest index.  sparse_mm = the winner's
 *      mm, 0 where no point landed; index = the winner's i, or -1.  The reflectance is not used; index lets a caller gather it.
 *   2. Complete, on v = 65536 - mm for measured pixels and v = 0 for empty ones: near is large, and a maximum takes the nearest,
 *      which is also what removes far points the lidar saw past an edge the camera cannot see past.  In every window the taps
 *      outside the image do not exist: they enter neither a maximum nor a minimum.  Each step reads the complete output of the
 *      step before, never its own, and is switched off by clearing its bit in `stages`.
 *      bit 0 DILATE      v <- max over the 13-tap diamond |dx| + |dy| <= 2; every pixel takes it, measured ones included.
 *      bit 1 CLOSE       v <- max over the 5 x 5 box, then v <- min over the 5 x 5 box (empty taps count as 0 in the min).
 *      bit 2 FILL_SMALL  pixels with v = 0 take the max over the 7 x 7 box; others keep v.
 *      bit 3 EXTEND_TOP  in each column the pixels above the topmost pixel with v > 0 take its v; a column without one stays empty.
 *      bit 4 FILL_LARGE  pixels with v = 0 take the max over the large x large box.
 *      bit 5 MEDIAN      a pixel with v > 0 takes the lower median of the taps with v > 0 in its 5 x 5 box: element (n-1)/2 of
 *                        the n values sorted ascending.  Empty pixels stay empty.
 *      bit 6 SMOOTH      a pixel with v > 0 and depth z0 = 65536 - v takes (sum w*v + Wt/2) / Wt in 64-bit integers over the taps
 *                        of its 5 x 5 box that have v > 0 and lie in its layer: max(z, z0)*256 <= min(z, z0)*(256 + tol_256).
 *                        w = b[dy]*b[dx], b = 1, 4, 6, 4, 1; Wt the sum of the weights that counted (the pixel itself always does).
 *      depth_mm = 65536 - v where v > 0, else 0.
 * No stereo border, clip or filter is applied here: the fusion's own rules do that downstream, as for a depth image from a file.
 * Parameters (sm_lidar_depth_params): 0 < min_z <= max_z <= 65.535, both finite; stages in 0..127; large odd, in 3..31; tol_256
 *   in 0..255.  sm_default_lidar_depth_params: 0.5, 65.0, 127, 31, 13.
 * sm_set_lidar_depth allocates the key plane and the work planes on the device; p NULL frees them (the default).  Setting it
 *   again replaces them.  A call that is rejected for its arguments (SM_E_ARG, SM_E_UNSUPPORTED) changes nothing: a context that
 *   had the stage keeps its planes and parameters.  If an allocation fails: SM_E_HIP, and the context is left without the stage.
 * sm_lidar_depth takes host pointers and waits; any output may be NULL.  sm_lidar_depth_device takes a scan resident on the
 *   context's GPU (16-byte aligned) and outputs that are device pointers the caller owns (depth_mm and sparse_mm 2-byte, index
 *   4-byte aligned, any may be NULL); T16 is on the host.  Its work -- four kernel launches, three with FILL_LARGE off -- is
 *   enqueued on the context's stream and not waited for, so a following sm_process_frame_device(ctx, d_rgb, d_depth_mm_out, ...)
 *   sees the result.
 * sm_lidar_depth_stats returns the last call's tally (it waits for that call; a call whose tally nobody asked for before the
 *   next one costs no wait: the next call's tally replaces it).  launch_ms is diagnostic only: what it holds, and how many of
 *   its entries mean anything, may change without a new SM_API_VERSION.  It holds the device time of each launch
 *   (0 the projection, 1 the DILATE..FILL_SMALL chain, 2 FILL_LARGE's row pass, 3 the rest) when SM_LIDAR_DEPTH_TIMING=1 was in
 *   the environment of sm_set_lidar_depth, -1 each otherwise and for a launch that was not made.
 *   A measuring aid: with SM_LIDAR_DEPTH_UNFUSED=1 in the environment of sm_set_lidar_depth every step is a launch of its own,
 *   through planes in global memory -- the same results from up to SM_LIDAR_DEPTH_MAX_LAUNCHES launches (0 the projection, 1 keys to
 *   v, 2 DILATE, 3 and 4 CLOSE, 5 FILL_SMALL, 6 EXTEND_TOP, 7 and 8 FILL_LARGE, 9 MEDIAN, 10 SMOOTH, 11 the output).
 * These entry points change nothing in the model, its counters, the tick, the frame log or the tracker state.
 * SM_E_ARG: a NULL context, NULL points with n > 0, n above the cap, parameters outside the ranges above, a misaligned pointer, a
 *   context without the stage (every call except sm_set_lidar_depth and the defaults), sm_lidar_depth_stats before the first
 *   call, a call between sm_stage_conflict and sm_stage_cull.
 *   SM_E_UNSUPPORTED: a sharded or rig context, checked right after the NULL context and before every other argument. */
#define SM_LIDAR_DEPTH_MAX_POINTS (1u << 24)
#define SM_LIDAR_DEPTH_MAX_LAUNCHES 12
#define SM_LIDAR_DEPTH_DILATE 1
#define SM_LIDAR_DEPTH_CLOSE 2
#define SM_LIDAR_DEPTH_FILL_SMALL 4
#define SM_LIDAR_DEPTH_EXTEND_TOP 8
#define SM_LIDAR_DEPTH_FILL_LARGE 16
#define SM_LIDAR_DEPTH_MEDIAN 32
#define SM_LIDAR_DEPTH_SMOOTH 64
typedef struct sm_lidar_depth_params {
    float   min_z, max_z;          /* metres along the camera's z; defaults 0.5, 65.0 */
    int32_t stages;                /* bits 0..6 as above; default 127 */
    int32_t large;                 /* FILL_LARGE's window: odd, 3..31; default 31 */
    int32_t tol_256;               /* SMOOTH's layer gate, 0..255; default 13 (the fill stage's) */
} sm_lidar_depth_params;
typedef struct sm_lidar_depth_stats_t {
    uint64_t points;               /* given */
    uint64_t landed;               /* ... that reached the splat */
    uint64_t measured;             /* pixels of sparse_mm that are not 0 */
    uint64_t filled_small, filled_top, filled_large;   /* pixels that FILL_SMALL, EXTEND_TOP and FILL_LARGE made non-empty */
    uint64_t left_empty;           /* pixels of depth_mm that are 0 */
    uint32_t launches;             /* kernel launches of the call */
    float    device_ms;            /* from before the first to after the last, by events */
    float    launch_ms[SM_LIDAR_DEPTH_MAX_LAUNCHES];   /* each launch's own (see above) */
} sm_lidar_depth_stats_t;
int sm_default_lidar_depth_params(const sm_config *c, sm_lidar_depth_params *p);
int sm_set_lidar_depth(sm_ctx *s, const sm_lidar_depth_params *p);
int sm_lidar_depth(sm_ctx *s, const float *points4, uint32_t n, const float *T16, uint16_t *depth_mm_out, uint16_t *sparse_mm_out, int32_t *index_out);
int sm_lidar_depth_device(sm_ctx *s, const float *d_points4, uint32_t n, const float *T16, uint16_t *d_depth_mm_out, uint16_t *d_sparse_mm_out, int32_t *d_index_out);
int sm_lidar_depth_stats(sm_ctx *s, sm_lidar_depth_stats_t *out);

/* ---- hole filling (DESIGN.md "4n. Hole filling") ----
 * A novel view (sm_render_image, sm_render_image_maps) is empty (sem 0) between discs and where a near object uncovers what no
 * frame saw, shows far surfels through one-pixel gaps of a near surface, and carries no depth.  This is the screen-space stage
 * that mends the three: the view's depth in millimetres from its key map, and a depth-aware push-pull completion of
 * (bgr, sem, depth_mm) in place.  All arithmetic is in integers; every division is a floor division.
 *   Depth of a novel view.  A drawn pixel's key carries d24 = key >> 32, the window z = Z / 200 m in 24 bits:
 *     zmm = (d24 * 200000 + 8388607) / 16777215 in 64 bits; depth_mm = zmm if zmm <= 65535, else 0 (beyond 65.535 m, as the
 *     stereo stage's).  An empty pixel has depth 0 and sem 0; a drawn pixel beyond range has depth 0 and sem != 0.
 *   Input, per pixel.  valid = (sem != 0), colour c[3], label s = sem, depth z = depth_mm, or z = 65536 where depth_mm == 0.
 *   Output.  depth_mm = z if z < 65536, else 0.  A pixel still invalid is all zeros.
 *   0. See-through (through_count = T > 0).  A valid pixel is made invalid if at least T of its 8 neighbours inside the image
 *      are valid and nearer: z_n * (256 + tol) < z_p * 256.  The test reads the input's validity and depths, never another
 *      pixel's verdict.
 *   1. Pull, level l to l + 1, for l = 0 .. levels - 1; w' = (w + 1) / 2, h' = (h + 1) / 2.  Cell (X, Y) has the children
 *      (2X + dx, 2Y + dy) inside level l, in the order dy outer, dx inner.  No valid child: the cell is invalid.  Otherwise, with
 *      zmin the least child depth: the near set is the valid children with z * 256 <= zmin * (256 + tol), n its size;
 *      c = (sum_near c + n/2) / n per channel; z = (sum_near z + n/2) / n; s = the label of the first child in order with
 *      z == zmin; cnt = the valid level-0 pixels under the cell after step 0.  The cell may fill iff
 *      cnt * 256 >= area * min_cover_256, area the level-0 pixels of the cell inside the image.
 *   2. Push, for l = levels - 1 down to 0, level l + 1 complete first (the top level keeps its invalid cells).  Every pixel
 *      (x, y) of level l that is invalid after the pull takes four taps, in this order and with these weights: (X, Y) 9, with
 *      X = x >> 1, Y = y >> 1; (Xn, Y) 3, Xn = X + 1 if x is odd, else X - 1; (X, Yn) 3, Yn likewise; (Xn, Yn) 1.  A tap counts
 *      if it is inside level l + 1, valid and may fill; if none counts the pixel stays invalid.  The group: with prefer_far the
 *      taps with z * (256 + tol) >= zmax * 256, without it those with z * 256 <= zmin * (256 + tol).  With Wt the sum of the
 *      group's weights: c = (sum w*c + Wt/2) / Wt; z = (sum w*z + Wt/2) / Wt; s = the label of the first tap in tap order among
 *      the group's greatest weight.  The pixel becomes valid and, at levels >= 1, may fill.  Valid pixels of level 0 are never
 *      rewritten.
 *   levels bounds the hole: about 1.5 * 2^levels pixels from the nearest observed pixel, so sky stays empty except for a fringe.
 * sm_fill_image takes n images of w x h in host memory, in place, and waits; depth_mm may be NULL (then every valid pixel has
 *   depth 0).  sm_fill_image_device takes device pointers (depth_mm 2-byte aligned), is enqueued on the context's stream and not
 *   waited for.  Both work in any context and touch no model state.
 * sm_render_image_ex / sm_render_image_maps_ex are sm_render_image / sm_render_image_maps plus: fill (NULL = none) and
 *   depth_mm_out (NULL = not wanted; per view h*w uint16).  With fill == NULL, bgr_out and sem_out equal the plain entry point's
 *   bit for bit.  With fill they are, by definition, the completion applied to the call's own unfilled outputs.
 * sm_fill_stats: of the last call that filled (summed over its images and, for a map set, over its passes); launches counts the
 *   stage's kernel launches, at most levels + 2 per pass however many views it fills; device_ms is the stage's time (events).
 * SM_E_ARG: NULL pointers, w or h <= 0, w*h > 2^28, a parameter outside its range, a misaligned depth_mm, sm_fill_stats before
 *   any call that filled.  The _ex calls otherwise refuse what their plain forms refuse (a call between sm_stage_conflict and
 *   sm_stage_cull, the file checks) and are SM_E_UNSUPPORTED in a sharded or rig context. */
typedef struct sm_fill_params {
    int32_t levels;         /* 0..8 pyramid levels above the image; 0 = no filling                        default 3  */
    int32_t depth_tol_256;  /* 0..255: two depths are one layer if z_far*256 <= z_near*(256+tol)          default 13 */
    int32_t through_count;  /* 0 = off, 1..8: nearer neighbours that make a pixel "seen through"          default 6  */
    int32_t prefer_far;     /* push takes the farthest layer among its taps (1) or the nearest (0)        default 1  */
    int32_t min_cover_256;  /* 0..256: share of a cell's pixels that must be observed before it may fill  default 64 */
} sm_fill_params;
typedef struct sm_fill_stats_t {
    uint64_t valid;               /* input pixels with sem != 0 */
    uint64_t seen_through;        /* ... of them, removed by step 0 */
    uint64_t filled;              /* pixels the level-0 push filled */
    uint64_t left_empty;          /* pixels invalid in the output */
    uint32_t launches;
    float device_ms;
} sm_fill_stats_t;
int sm_default_fill_params(sm_fill_params *p);               /* pure, no context */
int sm_fill_image(sm_ctx *s, const sm_fill_params *p, int w, int h, uint32_t n, uint8_t *bgr, uint8_t *sem, uint16_t *depth_mm);
int sm_fill_image_device(sm_ctx *s, const sm_fill_params *p, int w, int h, uint32_t n, uint8_t *d_bgr, uint8_t *d_sem,
                         uint16_t *d_depth_mm);
int sm_render_image_ex(sm_ctx *s, const float *view16, int w, int h, float fx, float fy, float cx, float cy,
                       const sm_fill_params *fill, uint8_t *bgr_out, uint8_t *sem_out, uint16_t *depth_mm_out);
int sm_render_image_maps_ex(sm_ctx *s, const sm_map_source *src, const float *views16, uint32_t n_views, int w, int h, float fx,
                            float fy, float cx, float cy, const sm_fill_params *fill, uint8_t *bgr_out, uint8_t *sem_out,
                            uint16_t *depth_mm_out);
int sm_fill_stats(sm_ctx *s, sm_fill_stats_t *out);

/* ---- blended views (DESIGN.md "4o. Blended views") ----
 * sm_render_image gives every pixel to exactly one surfel, the nearest; where the discs of one surface overlap the image shows
 * patches of each disc's own colour.  The blended view draws the visible layer instead: a visibility pass, a weighted sum of the
 * fragments within a depth band behind the front, a normalisation.  Everything is integer arithmetic on the renderer's own
 * fragments, so the result is defined bit for bit and depends neither on the order of the surfels, nor on the chunking of a map
 * set, nor on the views per pass.
 *   A fragment is a (surfel, pixel) pair that the novel-view rasteriser accepts: the same quad, the same 24.8 fixed-point vertices,
 *   edge functions and fill rule, the same float32 tx, ty, zw, and the same tests: tx*tx + ty*ty <= 1, 0 <= zw <= 1,
 *   d24 < 16777215.  The fill rule gives a surfel at most one fragment per pixel.  A fragment carries d24, its 24-bit window
 *   depth; q = tx*tx + ty*ty, the float32 value the circle test compares; and the surfel's colour word.
 *   1. Visibility: the key map of sm_render_image, unchanged; front = key >> 32 on a drawn pixel.  sem_out and depth_mm_out come
 *      from it exactly as in sm_render_image_ex: labels and depth are never blended.
 *   2. Accumulate: a fragment contributes to its pixel iff (uint64)d24 * 256 <= (uint64)front * (256 + depth_tol_256); the winner
 *      always does.  With i = min(255, (int32)(q * 256.0f)) its weight wt is 256 (falloff 0), 256 - i (falloff 1) or
 *      ((256 - i) * (256 - i) + 255) >> 8 (falloff 2): always in 1..256.  Per pixel SW += wt and SC[c] += wt * colour[c] for
 *      B, G, R.  The sums are exact for any set below 2^31 surfels (up to 2^47): the accumulators are 64 bits wide, four per
 *      pixel, and a map set counts their 32 bytes in the key budget of a batch (SM_RENDER_MAPS_KEY_MB) next to the keys.
 *   3. Normalise: on a drawn pixel bgr[c] = (SC[c] + SW / 2) / SW by floor division; an empty pixel stays 0, 0, 0.  A pixel with
 *      one contributor has exactly that surfel's colour.
 *   4. Fill, if asked, is applied afterwards to (bgr, sem, depth_mm) by the stage of sm_render_image_ex, unchanged.
 * blend == NULL is the _ex call, bit for bit.  Over a map set the accumulation needs the finished key map, so every file is read
 * twice per batch of views: sm_render_maps_stats then counts both readings in surfels_read, chunks and pairs_tested; passes keeps
 * its meaning (batches).
 * sm_blend_stats: of the last blended call, summed over its views and batches; launches counts the stage's kernels, device_ms
 * their time (events; over a map set the second reading's kernels included).
 * Errors follow the _ex forms: SM_E_ARG for NULLs, sizes, a parameter out of range, a call between sm_stage_conflict and
 * sm_stage_cull and the file checks, SM_E_UNSUPPORTED in a sharded or rig context; sm_blend_stats before any blended call is
 * SM_E_ARG.  The model view (sm_render_model) is not blended: it reproduces the reference's draw. */
typedef struct sm_blend_params {
    int32_t depth_tol_256;   /* 0..255: the band behind the front, in 1/256 of its depth (fill's layer test)  default 13 */
    int32_t falloff;         /* 0 box, 1 linear, 2 quadratic in q                                              default 2  */
} sm_blend_params;
typedef struct sm_blend_stats_t {
    uint64_t drawn;          /* pixels with sem != 0 */
    uint64_t contributions;  /* fragments that passed the band test */
    uint64_t changed;        /* drawn pixels whose colour differs from the nearest surfel's */
    uint32_t launches;
    float device_ms;
} sm_blend_stats_t;
int sm_default_blend_params(sm_blend_params *p);             /* pure, no context */
int sm_render_image_blend(sm_ctx *s, const float *view16, int w, int h, float fx, float fy, float cx, float cy,
                          const sm_blend_params *blend, const sm_fill_params *fill, uint8_t *bgr_out, uint8_t *sem_out,
                          uint16_t *depth_mm_out);
int sm_render_image_maps_blend(sm_ctx *s, const sm_map_source *src, const float *views16, uint32_t n_views, int w, int h, float fx,
                               float fy, float cx, float cy, const sm_blend_params *blend, const sm_fill_params *fill,
                               uint8_t *bgr_out, uint8_t *sem_out, uint16_t *depth_mm_out);
int sm_blend_stats(sm_ctx *s, sm_blend_stats_t *out);

/* ---- simplification (DESIGN.md "4p. Simplification") ----
 * With the reference's defaults almost nothing fuses, and every frame stores the surface it sees again.  This pass makes a model
 * or a map set smaller: the records that share a cell of a world grid, a class and (split_normals) a facing direction become one.
 * It is specified in integers: the result is defined bit for bit and is a function of the multiset of (global id, record) pairs
 * alone -- not of the order the device meets them in, of the chunking of a set, or of how the set is split into files.
 *   A record is the map file's: x y z conf | colour word, standby, init_time, time | nx ny nz radius, the colour word
 *   class << 24 | r << 16 | g << 8 | b.  A set is an sm_map_source with the global ids of the map-set calls: the files in list
 *   order, each in file order, then the live model.
 *   V = (voxel_mm * 65536 + 500) / 1000 (integer division): the cell edge in units of 2^-16 m.
 *   Regular records.  x, y, z finite with |(double)p[k] - (double)origin[k]| < 2^24; conf finite and > 0; init_time and time
 *     finite and >= 0; radius finite, 0 <= radius < 32768; the normal finite and not (0, 0, 0); the cell (below) within
 *     [-65536, 65535] on every axis.  Every other record is loose.
 *   Position.  X[k] = (int64)floor(((double)p[k] - (double)origin[k]) * 65536.0), cell[k] = floor_div(X[k], V),
 *     off[k] = X[k] - cell[k] * V in [0, V).
 *   Face.  split_normals: a = the axis of the largest |n[k]| (a tie goes to the lower axis), face = 2a + (n[a] < 0); else 0.
 *   Key.  (cell x, cell y, cell z, face, class): 17 + 17 + 17 + 3 + 8 = 62 bits.
 *   Contribution of a regular record to its key's cell, with t = conf * 16.0f (float32) and w = 255 if t >= 255, else
 *     max(1, (int32)t):  n += 1;  SW += w;  SP[k] += w * off[k];  SN[k] += w * ni[k] with ni[k] = (int32)clamp(floorf(n[k] *
 *     16384.0f + 0.5f), -2^22, 2^22) (a unit normal gives at most 2^14);  SC[c] += w * channel[c] for b, g, r;  lo[k] =
 *     min(off[k]), hi[k] = max(off[k]);  Rmax = max(RI), RI = (int64)floor((double)radius * 65536.0);  conf_max, time_max,
 *     init_time_min on the floats' bit patterns as unsigned words (for non-negative values they order like the values);
 *     first = min(global id).  With 2^31 contributors SP stays below 2^59, SN below 2^61, SC below 2^47: 64-bit sums are exact.
 *   Output.  One record per loose record, verbatim, and one per cell, in ascending order of the loose record's id / the cell's
 *     `first`: the output is in set order of its representatives.  A cell with n == 1 gives its record verbatim, so a map whose
 *     surfels are all alone in their cells comes back unchanged.  A cell with n >= 2 gives
 *       pos[k] = (float)((double)origin[k] + (double)(cell[k] * V + (SP[k] + SW / 2) / SW) * 2^-16)   (floor division; fp64)
 *       conf = conf_max;  colour word = class << 24 | the channels (SC[c] + SW / 2) / SW;  standby = 0;
 *       init_time = init_time_min;  time = time_max;
 *       normal: s = max(0, bit_length(max |SN[k]|) - 24), f[k] = (float)(SN[k] >> s) (arithmetic shift; exact), len =
 *         sqrtf((f0 * f0 + f1 * f1) + f2 * f2), n[k] = f[k] / len -- single float32 operations, no contraction, correctly
 *         rounded / and sqrt.  All three f zero: the normal of the record `first`.
 *       radius = (float)((double)R * 2^-16), R = max(Rmax, (isqrt(ex * ex + ey * ey + ez * ez) + 1) / 2), e = hi - lo, isqrt the
 *         integer square root: the merged disc reaches as far as any disc it replaces and spans the box of their centres.
 *   Capacity.  More distinct cells than max_cells: SM_E_CAPACITY, nothing written, the model unchanged.
 * sm_simplify replaces the live model by the simplification of sm_download_model_aos's rows (ids = rows), on the device.  Frames
 *   in flight are waited for; the tick, the stored poses, the fern keyframes and the tracker's state stay; sm_get_counts reports
 *   the new count.
 * sm_simplify_maps writes ONE map file, the set's simplification, to out_path (through "<out_path>.simplify.tmp" and a rename; its
 *   header's frame range spans the files').  The source files and the live model stay as they are; include_model = 1: the
 *   model's records take part.  Every file is read twice.  The header and set checks and the limit of 2^31 - 1 records are those
 *   of sm_render_image_maps.  SM_SIMPLIFY_NO_COMBINE=1 (read per call) switches off the in-wave combination of equal keys ahead
 *   of the atomics: the result is the same.
 * sm_simplify_stats: of the context's last call of either.
 * Errors.  SM_E_ARG: NULLs, voxel_mm outside 10..10000, split_normals not 0 or 1, a non-finite origin, max_cells == 0, out_path
 *   equal to a source path, a call between sm_stage_conflict and sm_stage_cull, the file checks, sm_simplify_stats before any
 *   call.  SM_E_UNSUPPORTED: a sharded or rig context.  SM_E_CAPACITY as above. */
typedef struct sm_simplify_params {
    int32_t voxel_mm;        /* 10..10000                                                                      default 50 */
    int32_t split_normals;   /* 0 / 1                                                                          default 1  */
    float origin[3];         /* of the grid, metres                                                            default 0  */
    uint32_t max_cells;      /* distinct cells the call may make                                               default 1 << 26 */
} sm_simplify_params;
typedef struct sm_simplify_stats_t {
    uint64_t records_in, records_out;
    uint64_t cells_merged;   /* cells with two or more contributors */
    uint64_t loose;
    uint32_t largest_cell;   /* contributors of the fullest cell */
    uint32_t chunks;         /* pieces of at most 2^20 records, both passes together */
    uint32_t launches;
    float device_ms, read_ms, total_ms;
} sm_simplify_stats_t;
int sm_default_simplify_params(sm_simplify_params *p);       /* pure, no context */
int sm_simplify(sm_ctx *s, const sm_simplify_params *p);
int sm_simplify_maps(sm_ctx *s, const sm_map_source *src, const sm_simplify_params *p, const char *out_path);
int sm_simplify_stats(sm_ctx *s, sm_simplify_stats_t *out);

/* ---- registration of one map set against another (DESIGN.md "4q. Registration") ----
 * Two drives of one street, a drive resumed after a restart, yesterday's map and today's: each set has its own world frame.
 * sm_register_maps measures the rigid transform T (column-major float[16]) that takes the SOURCE set's world to the TARGET set's:
 * point-to-plane ICP of a sample of the source records against one representative per occupied cell of a voxel grid over the
 * target, coarse to fine.  A set is an sm_map_source as in the simplification (files in list order, each in file order, then the
 * live model; global ids in that order); either may include the live model.  Nothing is modified: files, model, tick, stored
 * poses, fern keyframes and tracker state stay; frames in flight are waited for.  Whatever is decided is decided in integers or
 * in single, stated fp64 / fp32 operations (no contraction), so that tests/register_ref.py restates it value for value.
 *   Levels.  Level l = 0 .. levels - 1 has the cell edge V_l = ((voxel_mm << l) * 65536 + 500) / 1000 in units of 2^-16 m
 *     (the simplification's V of voxel_mm << l).  Iterations run on level levels - 1 first and on level 0 last.
 *   1. Target table of a level.  The simplification's regular-record test, X, cell, off, face (always split), weight w and
 *     normal integers ni, all with V_l and `origin`; the key is its key with the class taken as 0.  Per key the exact sums SW,
 *     SP[3], SN[3].  A key's representative c has the simplification's merged position, pos[k] = (float)((double)origin[k] +
 *     (double)(cell[k] * V_l + (SP[k] + SW / 2) / SW) * 2^-16), and its merged normal n_c (f[k] = (float)(SN[k] >> s), n_c = f /
 *     sqrtf((f0 * f0 + f1 * f1) + f2 * f2)) -- for a key with one record as well.  All three f zero: n_c = (0, 0, 0), which no
 *     sample pairs with (angle_thresh < 90).  The table is a function of the multiset of target records alone: not of their
 *     order, the chunking or the split into files.  More than max_cells keys at a level: SM_E_CAPACITY.  One pass over the
 *     target set fills all levels.
 *   2. Samples.  stride = the parameter, or if that is 0 max(1, ceil(records of the source set / max_samples)), known from the
 *     headers before anything is streamed.  The source records with global id % stride == 0 are the samples, sample i the record
 *     i * stride; there are ceil(records / stride) of them (more than 2^28: SM_E_CAPACITY; a stride that leaves more than
 *     max_samples: SM_E_ARG).  A sample is regular if its record passes the simplification's tests of its fields (everything
 *     but the cell range, which is applied to the moved point below); the others never pair.  The source set is read once.
 *   3. Pair of a regular sample (p, n) at the pose T (fp64, column-major) and level l.  With p and n widened to double:
 *     q[r] = ((T[r] * p0 + T[4 + r] * p1) + T[8 + r] * p2) + T[12 + r],  nq[r] = (T[r] * n0 + T[4 + r] * n1) + T[8 + r] * n2.
 *     d[k] = q[k] - (double)origin[k]; no pair unless |d[k]| < 2^24 on every axis.  X, cell, off of q as in the simplification
 *     with V_l; no pair unless every cell[k] is in [-65536, 65535].  face = the simplification's face of nq (compared in
 *     double).  Candidates: the 2 x 2 x 2 cells made per axis of cell[k] and its neighbour towards q -- cell[k] + 1 if
 *     2 * off[k] >= V_l, else cell[k] - 1; a neighbour outside the cell range is no candidate -- with that face and class 0,
 *     those of them that the table holds.  With e[k] = q[k] - (double)pos[k] and d2 = (e0 * e0 + e1 * e1) + e2 * e2 the
 *     candidate with the smallest d2 is kept, of equal ones that of the lower key.  The pair counts iff sqrt(d2) <= reach_l =
 *     (double)reach_cells * ((double)V_l * 2^-16) and (nq0 * n_c0 + nq1 * n_c1) + nq2 * n_c2 >= cos((double)angle_thresh * (pi /
 *     180)).  Then, in double rounded to float32 once: r = (n_c0 * e0 + n_c1 * e1) + n_c2 * e2 and, with u[k] = q[k] -
 *     (double)pivot[k], the row J = [n_c, u x n_c] (u x n = (u1 * n2 - u2 * n1, u2 * n0 - u0 * n2, u0 * n1 - u1 * n0)).  The 28
 *     products J[a] * J[b] (a <= b), J[a] * r, r * r are single float32 multiplications and are added in fp64, in an order
 *     that depends on the number of samples alone: the system is sm_track_debug's 29 values, value 28 the count.
 *   4. Step.  The trackers' solve (LDLT without pivoting, two substitutions, exp of the twist xi = (rho, phi)), the twist taken
 *     about `pivot`: T <- Tr(pivot) * exp(xi) * Tr(-pivot) * T, that is with exp(xi) = [R | t]: t' [r] = (t[r] + pivot[r]) -
 *     ((R[r][0] * pivot0 + R[r][1] * pivot1) + R[r][2] * pivot2), T's columns rotated by R ((R[r][0] * T[c * 4] + R[r][1] *
 *     T[c * 4 + 1]) + R[r][2] * T[c * 4 + 2]) and t' added to the last.  A far pivot makes the rotation and the translation of a
 *     step nearly the same motion of the overlap: pass a point inside it.  The start is guess16 (NULL: the identity) widened,
 *     its rotation made orthonormal as the trackers make their guess.  A level ends when |rho| < 1e-6 and |phi| < 1e-6 or after
 *     max_iters iterations; the next finer level starts from its result.
 *   5. info->status.  SM_REGISTER_OK; _LOST: a system had fewer than min_inliers (or than 6) pairs; _DEGENERATE: a system was
 *     not positive definite, or the trackers' pivot ratio of the last system of level 0, taken about `pivot`, is below
 *     SM_TRACK_DEGENERATE_BOUND; _NO_TARGET: a level without a key (nothing is iterated); _NO_SOURCE: no regular sample.  On
 *     anything but OK pose16_out is guess16 as given (the identity for NULL) and the call still returns SM_OK.
 *   The iterations are enqueued whole -- levels * max_iters pairs of launches, those after the end returning at once -- and the
 *   host waits once, after the last.
 * sm_register_debug: the tables and samples as above, then ONE system at pose16_eval (widened, as given) and `level` into sys29;
 *   *n_samples = the samples, regular or not.
 * sm_register_stats: of the context's last sm_register_maps or sm_register_debug.
 * Errors.  SM_E_ARG: NULLs (guess16 aside), a parameter outside the ranges below, a non-finite guess, origin or pivot, level
 *   outside 0 .. levels - 1, the header and set checks of sm_render_image_maps for both sets (every header of both before any
 *   work), a path that is in both sets, a call between sm_stage_conflict and sm_stage_cull, sm_register_stats before any call.
 *   SM_E_UNSUPPORTED: a sharded or rig context.  SM_E_CAPACITY as above, and for a set of more than 2^31 - 1 records. */
#define SM_REGISTER_OK 0
#define SM_REGISTER_LOST 1
#define SM_REGISTER_DEGENERATE 2
#define SM_REGISTER_NO_TARGET 3
#define SM_REGISTER_NO_SOURCE 4
#define SM_REGISTER_MAX_LEVELS 4
typedef struct sm_register_params {
    int32_t voxel_mm;        /* cell edge of level 0, 10..10000                                                default 200 */
    int32_t levels;          /* 1..4                                                                           default 3 */
    int32_t max_iters;       /* per level, 1..SM_TRACK_MAX_ITERS                                               default 20 */
    int32_t min_inliers;     /* >= 0                                                                           default 1000 */
    float angle_thresh;      /* degrees, in (0, 90)                                                            default 30 */
    float reach_cells;       /* a pair is kept up to reach_cells * the level's cell edge; finite, > 0          default 1.0 */
    uint32_t stride;         /* 0 = from max_samples                                                           default 0 */
    uint32_t max_samples;    /* 1..2^28                                                                        default 1 << 22 */
    uint32_t max_cells;      /* keys a level may hold, >= 1                                                    default 1 << 24 */
    float origin[3];         /* of the grids, metres                                                           default 0 */
    float pivot[3];          /* the point the twist is taken about, in the target's world: inside the overlap  default 0 */
} sm_register_params;
typedef struct sm_register_info {
    int32_t status;
    int32_t iterations[SM_REGISTER_MAX_LEVELS];   /* by level (level levels - 1 ran first) */
    uint32_t inliers;        /* of the last system summed */
    float rmse;              /* of the last system */
    float pivot_ratio;       /* of the last system that was judged */
    uint32_t samples;        /* regular samples */
    uint32_t stride;
    uint32_t cells[SM_REGISTER_MAX_LEVELS];       /* keys per level */
} sm_register_info;
typedef struct sm_register_stats_t {
    uint64_t source_records, target_records;
    uint32_t chunks;         /* pieces of at most 2^20 records, both sets together */
    uint32_t launches;
    float read_ms;           /* host: reading the files */
    float table_ms;          /* device: the tables' initialisation (two memsets per level), inserts, representatives and samples */
    float iterate_ms;        /* device: the iterations */
    float total_ms;
} sm_register_stats_t;
int sm_default_register_params(sm_register_params *p);       /* pure, no context */
int sm_register_maps(sm_ctx *s, const sm_map_source *source, const sm_map_source *target, const float *guess16,
                     const sm_register_params *p, float *pose16_out, sm_register_info *info);
int sm_register_debug(sm_ctx *s, const sm_map_source *source, const sm_map_source *target, const float *pose16_eval, int32_t level,
                      const sm_register_params *p, double *sys29, uint32_t *n_samples);
int sm_register_stats(sm_ctx *s, sm_register_stats_t *out);

/* ---- change detection between two map sets (DESIGN.md "4r. Change detection") ----
 * Once yesterday's map and today's share a frame (sm_register_maps), sm_compare_maps says of every record of the QUERY set
 * whether the REFERENCE set holds its surface: a label per record, and the records with the labels asked for as one map file that
 * every map-set call can draw, sweep or recall.  Which records of today's map are new: query = today, reference = yesterday;
 * which have vanished: the other way round.  Sets and global ids are registration's (files in list order, each in file order,
 * then the live model); either set may include the model.  pose16 (column-major, NULL = the identity) takes the query's world to
 * the reference's and is widened to fp64 as given, as sm_register_debug's.  Neither set is modified, nor the model, tick, stored
 * poses, fern keyframes or tracker state; frames in flight are waited for.  Whatever is decided is decided in integers or in
 * single, stated fp64 / fp32 operations (no contraction): tests/compare_ref.py restates it and the labels agree bit for bit.
 *   V0 = (voxel_mm * 65536 + 500) / 1000 and V1 = ((voxel_mm << cover_shift) * 65536 + 500) / 1000: the edges of a fine and of a
 *   cover cell in units of 2^-16 m.
 *   1. Fine table of the reference.  Registration's step 1 with V0: the simplification's regular-record test, X, cell, off, face
 *     (always split), weight and normal integers; the key is its key with the class kept iff match_class, else taken as 0.  Per
 *     key the exact sums SW, SP[3], SN[3]; a key's representative (pos, n_c) has the simplification's merged position and merged
 *     normal ((0, 0, 0) where all three f vanish: it supports nothing).  The table is a function of the multiset of reference
 *     records alone.
 *   2. Cover table of the reference.  The key is the cell alone, with V1, face 0 and class 0: present iff a reference record that
 *     is regular with V1 (the simplification's test with that edge) lies in the cell.  No sums.
 *     One pass over the reference set fills both tables.  More than max_cells keys in either: SM_E_CAPACITY, nothing is written
 *     (no label, no file).
 *   3. Label of a query record (p, n, class), the first rule that applies:
 *     LOOSE      it fails the simplification's tests of its fields (everything but the cell range).
 *     Otherwise q and nq as in registration's step 3: q[r] = ((T[r] * p0 + T[4 + r] * p1) + T[8 + r] * p2) + T[12 + r],
 *       nq[r] = (T[r] * n0 + T[4 + r] * n1) + T[8 + r] * n2, in double.
 *     OUTSIDE    by range: |q[k] - (double)origin[k]| >= 2^24 (or not a number) on an axis, or the fine cell (X, cell of q with
 *       V0, as in the simplification) or the cover cell (with V1) of q outside [-65536, 65535] on an axis.
 *     Candidate faces.  m = max |nq[k]| (double); the face (a, nq[a] < 0), that is 2a + (nq[a] < 0), is a candidate for every
 *       axis a with 4.0 * |nq[a]| >= m: one to three faces, the simplification's face of nq among them.  (Within angle_thresh of
 *       a normal near the 45 degree tie of two axes lie normals of the other dominant axis; with the primary face alone every
 *       such wall would read as changed.)
 *     Candidate cells.  Registration's 2 x 2 x 2 with V0: per axis cell[k] and its neighbour towards q -- cell[k] + 1 if
 *       2 * off[k] >= V0, else cell[k] - 1; a neighbour outside the cell range is dropped.
 *     Candidate keys.  cells x faces with class 0, or the record's class (colour word >> 24) if match_class; those the fine table
 *       holds: at most 24.  For one with the representative (pos, n_c): e[k] = q[k] - (double)pos[k], d2 = (e0 * e0 + e1 * e1) +
 *       e2 * e2, r = (n_c0 * e0 + n_c1 * e1) + n_c2 * e2 (n_c widened).  It passes iff
 *         sqrt(d2) <= (double)reach_cells * ((double)V0 * 2^-16)  and
 *         (nq0 * n_c0 + nq1 * n_c1) + nq2 * n_c2 >= cos((double)angle_thresh * (pi / 180))  and
 *         fabs(r) <= (double)plane_mm / 1000.0.
 *     SUPPORTED  iff any candidate passes: there is no nearest one, hence no tie and no order.
 *     CHANGED    otherwise, iff the cover table holds one of the 2 x 2 x 2 cover cells of q (cell and neighbour towards q per
 *       axis with V1, neighbours outside the range dropped): the reference mapped this neighbourhood, but not this surface.
 *     OUTSIDE    otherwise: the reference has nothing near -- not mapped there, no statement.
 *   4. Outputs.  labels[g] for every query id g (if labels is given); info->counts by label; with out_path ONE map file, written
 *     as sm_simplify_maps writes its own (through "<out_path>.compare.tmp" and a rename; the header's frame range spans the query
 *     files'), of the query records whose label l has bit l of write_mask set -- verbatim, NOT moved by the pose (sm_warp_by_time
 *     does that), in set order.  No such record: a valid empty file.  info->written is that file's record count.
 * sm_compare_stats: of the context's last sm_compare_maps.
 * Errors.  SM_E_ARG: NULLs other than pose16, labels and out_path; a parameter outside the ranges below; write_mask outside
 *   1..15 when out_path is given; a non-finite pose or origin; the header and set checks of sm_render_image_maps for both sets
 *   (every header of both before any work); a path that is in both sets; out_path equal to a path of either set; a call between
 *   sm_stage_conflict and sm_stage_cull; sm_compare_stats before any call.  SM_E_UNSUPPORTED: a sharded or rig context.
 *   SM_E_CAPACITY as above, and for a set of more than 2^31 - 1 records. */
#define SM_COMPARE_SUPPORTED 0   /* the reference holds this surface */
#define SM_COMPARE_CHANGED   1   /* the reference mapped this neighbourhood, but not this surface */
#define SM_COMPARE_OUTSIDE   2   /* the reference has nothing near: not mapped there, no statement */
#define SM_COMPARE_LOOSE     3   /* an irregular record */
typedef struct sm_compare_params {
    int32_t voxel_mm;        /* edge of a fine cell, 10..10000                                                 default 100 */
    int32_t cover_shift;     /* 1..6: cover cell edge = voxel_mm << cover_shift                                default 3 */
    float reach_cells;       /* lateral reach in fine cell edges; finite, > 0                                  default 2.0 */
    int32_t plane_mm;        /* 1..10000: largest point-to-plane distance that is still the same surface       default 50 */
    float angle_thresh;      /* degrees, in (0, 90): largest angle between the normals                         default 30 */
    int32_t match_class;     /* 0 / 1; 1: a supporting cell must hold records of the query record's class      default 0 */
    uint32_t write_mask;     /* bit l = label l, 1..15; read only if out_path is given                         default 2 */
    uint32_t max_cells;      /* keys either table may hold, >= 1                                               default 1 << 24 */
    float origin[3];         /* of the grids, metres                                                           default 0 */
} sm_compare_params;
typedef struct sm_compare_info {
    uint64_t counts[4];      /* query records by label */
    uint64_t query_records, reference_records;
    uint32_t cells_fine, cells_cover;             /* keys of the two tables */
    uint64_t written;        /* records of the file at out_path (0 without one) */
} sm_compare_info;
typedef struct sm_compare_stats_t {
    uint32_t chunks;         /* pieces of at most 2^20 records, both sets together */
    uint32_t launches;
    float read_ms;           /* host: reading the files */
    float table_ms;          /* device: the tables' initialisation (four memsets), inserts and representatives */
    float classify_ms;       /* device: labels, ranks and kept records of the query's chunks */
    float write_ms;          /* host: labels and kept records back from the device and into the file */
    float total_ms;
} sm_compare_stats_t;
int sm_default_compare_params(sm_compare_params *p);         /* pure, no context */
int sm_compare_maps(sm_ctx *s, const sm_map_source *query, const sm_map_source *reference, const float *pose16,
                    const sm_compare_params *p, uint8_t *labels /* query records, by global id; may be NULL */,
                    const char *out_path /* may be NULL */, sm_compare_info *info);
int sm_compare_stats(sm_ctx *s, sm_compare_stats_t *out);

/* ---- tiling: a map set sorted in space (DESIGN.md "4s. Spatial tiling") ----
 * sm_tile_maps rewrites a map set -- an sm_map_source with the global ids of the map-set calls: the files in list order, each in
 * file order, then (include_model) the live model -- as a NEW set: the same records, verbatim (48 bytes each), sorted along a 3-D
 * Morton curve over a world grid and cut into files at tile boundaries.  Sources and model stay as they are.  Nothing calls it
 * unasked.  The boxes every map-set call skips by (one per block of 256 consecutive records in the streamed renderers and the lidar,
 * one per file in sm_recall and the warp) are tight on its output whatever order the sources were written in.
 *   Definition, in integers (restated by tests/tile_ref.py):
 *   Grid.  The simplification's: V = (cell_mm * 65536 + 500) / 1000 (integer division), X[k] = (int64)floor(((double)p[k] -
 *     (double)origin[k]) * 65536.0), cell[k] = floor_div(X[k], V).
 *   Placed.  A record is placed if x, y, z are finite, |(double)p[k] - (double)origin[k]| < 2^24 and every cell[k] lies in
 *     [-65536, 65535]; every other record is loose.  Only the position is examined: a record with conf <= 0, a NaN normal or a
 *     negative radius is placed (this is not the simplification's "regular").
 *   Key.  u[k] = cell[k] + 65536 in [0, 2^17); bit 3 i + k of M is bit i of u[k] (x lowest): 51 bits.
 *   Tile.  M >> (3 * tile_shift): an aligned cube of 2^tile_shift cells per axis.
 *   Order.  The placed records in ascending (M, global id), then the loose ones in ascending global id.
 *   Files.  The tiles are walked in ascending tile id; a file takes successive whole tiles while its count stays <=
 *     max_file_records; a tile with more records than that is written alone, as consecutive files of max_file_records records, the
 *     last of them shorter; the loose records, if any, form one last file.  Names: "<out_prefix>_%06u.bin", 0, 1, ...  Each header
 *     carries the frame range that spans the sources' (0, 0 without files).  An empty set writes no file.
 *   The result is a function of the multiset of (global id, record) pairs alone: the chunking, the split into source files, the
 *     device's order and the sort capacity do not change a byte.  Tiling the output again with the same parameters, files in
 *     order, reproduces it byte for byte.
 *   Example, cell_mm 1000 (V = 65536), origin 0: centres F (-0.5, .5, .5), A (.5, .5, .5), G (-0.0, .5, .5), B (1.5, .5, .5),
 *     C (.5, 1.5, .5), D (.5, .5, 1.5), E (2.5, .5, .5) have M = 0x6249249249249, 0x7000000000000, 0x7000000000000,
 *     0x7000000000001, ..2, ..4, ..8: the order is F, A and G by id, B, C, D, E; with tile_shift 1 A, G, B, C, D share a tile, E
 *     and F have one each.  cell_mm 100: V = 6554; 200: 13107; 10: 655 (the grid then ends at +-429 m).
 *   Cost.  1 + the number of batches readings of the set: one that counts the records per tile, then one per batch -- a maximal
 *     run of successive whole tiles whose total stays <= the sort capacity, 1 << 22 records (SM_TILE_SORT_RECORDS, read per call,
 *     256 .. 1 << 26, overrides it; the result does not depend on it).  Loose records are collected by the first batch's reading
 *     (by a reading of their own if nothing is placed) and held on the device until they are written.
 *   Writing.  Every file is written as "<name>.tile.tmp"; all are renamed into place only after the last one is complete.  On any
 *     error nothing is renamed and no temporary is left.  Files an earlier call left under higher numbers of the same prefix are
 *     not removed.  After the renames each file is noted in the context's file index with the box of its finite centres and its
 *     largest time: an sm_recall that follows skips files out of reach without opening them.
 *   A tiled set no longer has time-ordered files: sm_warp_by_time (closing a loop) will open every one of them, so tile once the
 *     drive is closed.
 * Errors.  SM_E_ARG: NULLs; a parameter outside the ranges below; a non-finite origin; max_file_records above the sort capacity; an
 *   output name equal to a source path (every name of the plan is checked before anything is written); a call between
 *   sm_stage_conflict and sm_stage_cull; the file checks of sm_render_image_maps; sm_tile_stats before any call.
 *   SM_E_UNSUPPORTED: a sharded or rig context.  SM_E_CAPACITY: more than max_tiles tiles; a single tile above the sort capacity
 *   (lower tile_shift); a set of more than 2^31 - 1 records.  Nothing is written in any of these cases. */
typedef struct sm_tile_params {
    int32_t cell_mm;            /* 10..10000                               default 200 */
    int32_t tile_shift;         /* 0..17: tile edge = cell << shift        default 7 (25.6 m) */
    float origin[3];            /*                                         default 0 */
    uint32_t max_file_records;  /* 256..sort capacity                      default 1 << 20 */
    uint32_t max_tiles;         /* distinct tiles the call may meet, >= 1  default 1 << 20 */
} sm_tile_params;
typedef struct sm_tile_stats_t {
    uint64_t records_in, placed, loose;
    uint32_t tiles;             /* distinct tiles */
    uint32_t largest_tile;      /* records in the fullest */
    uint32_t files_written;
    uint32_t readings;          /* passes over the set */
    uint32_t chunks;            /* of at most 2^20 records, over all readings */
    uint32_t launches;
    uint32_t sort_passes;       /* radix passes run, over all batches: a pass whose digit is the same in all keys is skipped */
    float device_ms;            /* kernels of the readings, the sort and the gather */
    float sort_ms;              /* ... of which the sort */
    float read_ms;              /* host: reading the files */
    float write_ms;             /* host: writing the files */
    float total_ms;
} sm_tile_stats_t;
int sm_default_tile_params(sm_tile_params *p);               /* pure, no context */
int sm_tile_maps(sm_ctx *s, const sm_map_source *src, const sm_tile_params *p, const char *out_prefix);
int sm_tile_stats(sm_ctx *s, sm_tile_stats_t *out);

/* ---- segmentation: the records of a map set grouped into objects (DESIGN.md "4t. Segmentation") ----
 * sm_segment_maps groups the records of a map set -- an sm_map_source with the global ids of the map-set calls: the files in list
 * order, each in file order, then (include_model) the live model -- into connected components of occupied voxel cells: a label per
 * record, a row per component, and with out_path the records of the label kinds asked for as ONE map file.  A component of fewer
 * than min_records records is a speck: write_mask 1 with min_records N writes the set without its specks.  Sources, model, tick,
 * stored poses, fern keyframes and tracker state are untouched; frames in flight are waited for.
 *   Definition, in integers (restated by tests/segment_ref.py):
 *   Grid.  The simplification's: V = (voxel_mm * 65536 + 500) / 1000 (integer division), X[k] = (int64)floor(((double)p[k] -
 *     (double)origin[k]) * 65536.0), cell[k] = floor_div(X[k], V), and its regular-record test: every field finite, conf > 0, both
 *     times >= 0, 0 <= radius < 32768, a normal that is not (0, 0, 0), |(double)p[k] - (double)origin[k]| < 2^24 and every cell[k]
 *     in [-65536, 65535].  The class c of a record is its colour word >> 24.
 *   Label of a record, the first rule that applies:
 *     1. LOOSE    it is not regular.
 *     2. SKIPPED  bit c & 31 of class_mask[c >> 5] is clear.
 *     3. Otherwise it belongs to the node (cell, kc), kc = c with by_class, else 0.  (The node's key is the simplification's key
 *        with face 0 and class kc.)
 *   Edges.  Two nodes are joined iff they have the same kc and their cells differ by a d in {-1, 0, 1}^3 \ {0} with |d|_1 <= 1
 *     (connectivity 6), <= 2 (18) or <= 3 (26).  A neighbour cell outside [-65536, 65535] on any axis does not exist (it is
 *     dropped before a key is made of it: cell 65535 and cell -65536 of an axis are not neighbours).
 *   Components.  The connected components of that graph.  records: the records in its nodes; cells: its nodes; first: the smallest
 *     global id among its records; cell_lo / cell_hi: the box of its cells; sum_cell[k]: the sum over its records of cell[k] +
 *     65536 (the centroid in cells is sum_cell[k] / records - 65536 + 1/2).
 *   Small.  A component with records < min_records is small: its records are labelled SMALL, it gets no number and no row and
 *     counts in info->small_components.
 *   Numbering.  The other components are numbered 0, 1, ... in ascending `first` -- in set order of first appearance.  Their
 *     records are labelled with that number; row i of `components` describes component i.  Rows i >= cap are not written;
 *     info->components is the total whatever cap is.  info->largest: the largest `records` of any component, small ones included
 *     (0 without a component).  info->counts: records labelled with a number, SMALL, SKIPPED, LOOSE; info->cells: all nodes.
 *   The result is a function of the multiset of (global id, record) pairs alone: the chunking, the split into files, the table's
 *     size and hash order and the device's order do not change a bit of it.
 *   Example, voxel_mm 1000 (V = 65536), origin 0, one class: centres A (.5, .5, .5), B (1.5, .5, .5), C (2.5, 1.5, .5),
 *     D (3.5, 2.5, 1.5), E (5.5, .5, .5) with the ids 0..4 lie in the cells (0,0,0) (1,0,0) (2,1,0) (3,2,1) (5,0,0).  B-C differ by
 *     (1,1,0), C-D by (1,1,1).  Connectivity 6: {A,B} {C} {D} {E}; 18: {A,B,C} {D} {E}; 26: {A,B,C,D} {E}.  With 26 and
 *     min_records 2, E is SMALL and there is one row: first 0, records 4, cells 4, cell_lo (0,0,0), cell_hi (3,2,1), sum_cell
 *     (4 * 65536 + 6, 4 * 65536 + 3, 4 * 65536 + 1).
 *   out_path.  One map file, written as sm_compare_maps writes its own (through "<out_path>.segment.tmp" and a rename; the header's
 *     frame range spans the files'), of the records whose label kind -- bit 0 a number, 1 SMALL, 2 SKIPPED, 3 LOOSE -- has its bit
 *     in write_mask, verbatim and in set order.  No such record: a valid empty file.  info->written is its record count.
 *   Cost.  Two readings of the set.  The first claims every node in an open-addressing table (key, records, smallest id); one
 *     launch over the table's slots then unites every node with the neighbours of the forward half of its neighbourhood (3, 9 or
 *     13 keys) by a lock-free union-find -- only roots are hooked, the larger slot under the smaller, by compare-and-swap --, one
 *     flattens the trees, one sums the components at their roots (SM_SEGMENT_NO_COMBINE=1, read per call, switches the in-wave
 *     combination of that step off; the result is the same).  The second reading labels.  Every device loop is bounded by the
 *     table's size: a bound reached is SM_E_STALL, never a hang.
 * sm_segment_stats: of the context's last sm_segment_maps.
 * Errors.  SM_E_ARG: NULLs other than labels, components and out_path; components == NULL with cap != 0; a parameter outside the
 *   ranges below; write_mask outside 1..15 when out_path is given; a non-finite origin; out_path equal to a source path; the
 *   header and set checks of sm_render_image_maps (every header before any work); a call between sm_stage_conflict and
 *   sm_stage_cull; sm_segment_stats before any call.  SM_E_UNSUPPORTED: a sharded or rig context.  SM_E_CAPACITY: more than
 *   max_cells nodes; a set of more than 2^31 - 1 records; a table of more than 2^31 slots.  SM_E_STALL as above.  In the last two
 *   cases no label, no row and no file is written. */
#define SM_SEGMENT_LOOSE   0xFFFFFFFEu   /* an irregular record */
#define SM_SEGMENT_SMALL   0xFFFFFFFDu   /* its component has fewer than min_records records */
#define SM_SEGMENT_SKIPPED 0xFFFFFFFCu   /* its class is not in class_mask */
typedef struct sm_segment_params {
    int32_t  voxel_mm;        /* edge of a cell, 10..10000                                            default 200 */
    int32_t  connectivity;    /* 6, 18 or 26                                                          default 26 */
    int32_t  by_class;        /* 0 / 1; 1: only cells of one class connect                            default 1 */
    uint32_t class_mask[8];   /* bit c & 31 of word c >> 5: class c takes part                        default all ones */
    uint32_t min_records;     /* >= 1: a component of fewer records is small                          default 1 */
    uint32_t write_mask;      /* bit 0 numbered components, 1 SMALL, 2 SKIPPED, 3 LOOSE; 1..15; read only if out_path is given; default 1 */
    uint32_t max_cells;       /* nodes the table may hold, >= 1                                       default 1 << 24 */
    float    origin[3];       /* of the grid, metres                                                  default 0 */
} sm_segment_params;
typedef struct sm_segment_component {   /* 64 bytes */
    uint32_t first;           /* smallest global id among its records */
    uint32_t records, cells;
    int32_t  cls;             /* the class with by_class, else -1 */
    int32_t  cell_lo[3], cell_hi[3];
    uint64_t sum_cell[3];     /* sum over its records of cell[k] + 65536 */
} sm_segment_component;
typedef struct sm_segment_info {
    uint64_t records;         /* of the set */
    uint64_t counts[4];       /* records labelled with a number, SMALL, SKIPPED, LOOSE */
    uint64_t written;         /* records of the file at out_path (0 without one) */
    uint32_t cells;           /* nodes */
    uint32_t components;      /* numbered components, whatever cap is */
    uint32_t small_components;
    uint32_t largest;         /* records of the largest component */
} sm_segment_info;
typedef struct sm_segment_stats_t {
    uint32_t chunks;          /* pieces of at most 2^20 records, both readings together */
    uint32_t launches;
    uint32_t readings;        /* passes over the set: 2 */
    float read_ms;            /* host: reading the files */
    float table_ms;           /* device: the table's initialisation and reading 1's inserts */
    float link_ms;            /* device: link, flatten and reduce */
    float label_ms;           /* device: reading 2's marks, ranks, rows, labels and kept records */
    float write_ms;           /* host: labels and kept records back from the device and into the file */
    float total_ms;
} sm_segment_stats_t;
int sm_default_segment_params(sm_segment_params *p);         /* pure, no context */
int sm_segment_maps(sm_ctx *s, const sm_map_source *src, const sm_segment_params *p,
                    uint32_t *labels /* by global id; may be NULL */,
                    sm_segment_component *components, uint32_t cap /* rows at components; NULL needs 0 */,
                    const char *out_path /* may be NULL */, sm_segment_info *info);
int sm_segment_stats(sm_ctx *s, sm_segment_stats_t *out);

/* ---- meshing: the records of a map set turned into a triangle mesh (DESIGN.md "4u. Meshing") ----
 * sm_mesh_maps reads a map set ONCE -- an sm_map_source with the global ids of the map-set calls: the files in list order, each in
 * file order, then (include_model) the live model -- and gives the surface its surfels lie on as an indexed triangle mesh: one
 * plane per occupied voxel cell, a signed field sampled at the grid's lattice points, marching tetrahedra over the cubes between
 * them.  Sources, model, tick, stored poses, fern keyframes and tracker state are untouched; frames in flight are waited for.
 *   Definition, in integers and stated fp64 operations, none contracted (restated by tests/mesh_ref.py):
 *   Grid.  The simplification's V, X, cell and off (off[k] = X[k] - cell[k] * V) and its regular-record test, with voxel_mm and
 *     origin.  A record that is not regular is LOOSE.  A regular record whose class c (colour word >> 24) has bit c & 31 of
 *     class_mask[c >> 5] clear is SKIPPED.  Otherwise it is OUTSIDE if some cell[k] lies outside [-65536 + reach, 65535 - reach]
 *     (decided before a key is packed: every lattice point a record can reach is on the grid).  Every other record is USED.
 *   Cells.  Per cell, of its USED records (no face and no class in the key): n; the simplification's SW, SP[3], SN[3], SC[3]; cmin,
 *     the minimum of ((uint64)global id << 8) | c.  A cell with n < min_records does not exist anywhere below.  Its plane:
 *     mp[k] = (SP[k] + SW / 2) / SW, an integer offset in the cell, and n_c = the simplification's merged normal of SN; if that
 *     fails (all three components vanish) the cell has no plane: it exists, but adds nothing to F.
 *   Lattice points.  l is an integer triple at position l * V.  Its inner cells are the 2 x 2 x 2 cells l - b, b in {0, 1}^3, its
 *     outer cells the 4 x 4 x 4 cells c with l - 2 <= c <= l + 1.  reach 1: l is sampled iff an inner cell exists.  reach 2: iff
 *     an outer cell exists.  Its contributors are the inner cells that exist; if none does (reach 2), all outer cells that exist.
 *     Over the contributors in ascending lexicographic order of c - l, in fp64, beginning with 0.0:
 *       F += (double)SW_c * ((n0 * e0 + n1 * e1) + n2 * e2),  e[k] = (double)((l[k] - c[k]) * V - mp_c[k]),  n_c widened from float
 *     (a cell without a plane is left out of F only); W, NS[3], CS[3] are the integer sums of SW_c, SN_c, SC_c and cmin the minimum
 *     of cmin_c over all contributors (so W >= 1).  l is inside iff F < 0.
 *   Cubes.  The cube at l has the corners l + b.  It is meshed iff all eight are sampled.  It is cut into six Kuhn tetrahedra, one
 *     per permutation (a, b, c) of the axes in lexicographic order: t0 = l, t1 = l + e_a, t2 = l + e_a + e_b, t3 = l + (1, 1, 1);
 *     for an odd permutation t2 and t3 are exchanged, so that every tetrahedron is positively oriented.
 *   Faces of a tetrahedron, by which corners are inside.  None with 0 or 4.  One corner i unlike the other three: take those in
 *     ascending order j < k < l and exchange k and l if (i, j, k, l) is an odd permutation of (0, 1, 2, 3) (i odd); the triangle is
 *     (v_ij, v_ik, v_il), its first and last exchanged if the lone corner is the outside one.  Two inside i < j, two outside
 *     k < l: exchange k and l if (i, j, k, l) is odd; the triangles are (v_ik, v_il, v_jl), then (v_ik, v_jl, v_jk).  The
 *     orientation is combinatorial, never from computed coordinates: face normals point from inside to outside, the way the
 *     surfel normals point.  Each triangle's indices are then rotated so that the smallest comes first.
 *   Vertices.  v_ab lies on the edge from lattice point a to b = a + d, d in {0, 1}^3 \ {0}; a owns it; its kind is d0 + 2 d1 +
 *     4 d2 (every edge of a Kuhn tetrahedron is such an edge).  It exists iff a face refers to it.
 *       t = A / (A - B), A = F_a * (double)W_b, B = F_b * (double)W_a   (one end is inside: 0 <= t <= 1, never 0 / 0)
 *       pos[k] = (float)((double)origin[k] + ((double)(a[k] * V) + t * (double)(d[k] * V)) * (1.0 / 65536.0))
 *       normal = the merged normal of NS_a + NS_b, or (0, 0, 0) if that fails
 *       colour channel k = ((CS_a + CS_b)[k] + (W_a + W_b) / 2) / (W_a + W_b);  class = the low byte of min(cmin_a, cmin_b)
 *     Zero-area triangles (t = 0) may occur and are kept.
 *   Order.  Vertices ascending by (key of the owner, kind), the key the simplification's packing of l + 65536: lexicographic, x
 *     major.  Faces ascending by (key of the cube's l, tetrahedron, triangle).
 *   The result is a function of the multiset of (global id, record) pairs alone: the chunking, the split into files, the tables'
 *     sizes and hash order and the device's order do not change a byte of it.
 *   Example, voxel_mm 1000 (V = 65536), origin 0: one record at (.5, .5, .5) with normal +z.  Cell (0, 0, 0), mp = (32768, 32768,
 *     32768); F(l) = w (l_z * 65536 - 32768): inside iff l_z <= 0, t = 1/2 on every cut edge.  reach 1: 8 lattice points, 1 cube,
 *     9 vertices (on the 4 upright edges, the 4 upright face diagonals, the body diagonal), 8 faces, all at z = 0.5 exactly, every
 *     face normal +z.  reach 2: 64 lattice points, 27 cubes, the 9 of the layer l_z = 0 cut: 49 vertices, 72 faces.
 *   Output.  vertices: row i < vcap of the vertex list; faces: row i < fcap of the face list; rows beyond a cap are not written;
 *     info carries the totals whatever the caps are.  vertices, faces and ply_path may each be NULL (NULL needs cap 0).
 *   ply_path.  A binary little-endian PLY written through "<ply_path>.mesh.tmp" and a rename: per vertex x y z nx ny nz as float,
 *     red green blue as uchar -- bytes 2, 1, 0 of the colour word, as the renderers map them -- and a uchar `class`; per face
 *     `list uchar int vertex_indices`.  An empty mesh is a valid empty file.
 *   Cost.  One reading into an open-addressing table of cells (in-wave combination of runs, 64-bit atomicCAS claims, integer
 *     atomics).  The lanes of a wave then claim each of its cells' 8 or 64 lattice points in a second table sized from the cell
 *     count (doubled and claimed again should it prove too small: sparse cells share few points); one launch sums the field
 *     per lattice point; one classifies the cubes, counts their faces and marks the used edges at their owners; the owners of a
 *     vertex or face are sorted by key (the tiling's radix sort), ranked, and two launches write vertices and faces, which come
 *     back in pieces while the host writes the file.
 * sm_mesh_stats: of the context's last sm_mesh_maps that succeeded (a call that fails leaves them as they were).
 * Errors.  SM_E_ARG: NULLs other than vertices, faces and ply_path; a NULL buffer with a cap != 0; a parameter outside the ranges
 *   below; a non-finite origin; ply_path equal to a source path; the header and set checks of sm_render_image_maps (every header
 *   before any work); a call between sm_stage_conflict and sm_stage_cull; sm_mesh_stats before any call has succeeded.  SM_E_UNSUPPORTED: a
 *   sharded or rig context.  SM_E_CAPACITY: more than max_cells cells in the table (whatever min_records is); more than 2^32 - 1
 *   vertices or faces; a table of more than 2^31 slots; a set of more than 2^31 - 1 records.  Then nothing is written: no row, no
 *   file, not info. */
#define SM_MESH_USED    0
#define SM_MESH_SKIPPED 1
#define SM_MESH_LOOSE   2
#define SM_MESH_OUTSIDE 3
typedef struct sm_mesh_params {
    int32_t  voxel_mm;        /* edge of a cell, 10..10000                                            default 100 */
    int32_t  reach;           /* 1 or 2: the cells around a lattice point that make it sampled        default 2 */
    uint32_t min_records;     /* >= 1: a cell of fewer records does not exist                         default 1 */
    uint32_t class_mask[8];   /* bit c & 31 of word c >> 5: class c takes part                        default all ones */
    uint32_t max_cells;       /* cells the table may hold, >= 1                                       default 1 << 24 */
    float    origin[3];       /* of the grid, metres                                                  default 0 */
} sm_mesh_params;
typedef struct sm_mesh_vertex {         /* 28 bytes */
    float    pos[3];
    float    normal[3];
    uint32_t colour;          /* laid out as a record's colour word: channels in bytes 0..2, the class in byte 3 */
} sm_mesh_vertex;
typedef struct sm_mesh_info {
    uint64_t records;         /* of the set */
    uint64_t counts[4];       /* records USED, SKIPPED, LOOSE, OUTSIDE */
    uint32_t cells;           /* cells that exist (n >= min_records) */
    uint32_t lattice_points;  /* sampled */
    uint32_t cubes;           /* meshed */
    uint32_t vertices, faces; /* the totals, whatever the caps are */
    uint32_t reserved;
} sm_mesh_info;
typedef struct sm_mesh_stats_t {
    uint32_t chunks;          /* pieces of at most 2^20 records read */
    uint32_t launches;
    float read_ms;            /* host: reading the files */
    float table_ms;           /* device: the cell table's initialisation and inserts */
    float field_ms;           /* device: lattice claim, field, cubes */
    float sort_ms;            /* device: the owners listed, sorted and ranked */
    float emit_ms;            /* device: vertices and faces written */
    float write_ms;           /* host: rows back from the device, into the caller's buffers and the file */
    float total_ms;
} sm_mesh_stats_t;
int sm_default_mesh_params(sm_mesh_params *p);               /* pure, no context */
int sm_mesh_maps(sm_ctx *s, const sm_map_source *src, const sm_mesh_params *p,
                 sm_mesh_vertex *vertices, uint32_t vcap /* rows at vertices; NULL needs 0 */,
                 uint32_t *faces /* three indices a row */, uint32_t fcap /* rows at faces; NULL needs 0 */,
                 const char *ply_path /* may be NULL */, sm_mesh_info *info);
int sm_mesh_stats(sm_ctx *s, sm_mesh_stats_t *out);

/* ---- ground map: a map set as a planner's bird's-eye raster (DESIGN.md "4v. Ground map") ----
 * sm_ground_maps reads a map set TWICE -- an sm_map_source with the global ids of the map-set calls: the files in list order, each
 * in file order, then (include_model) the live model -- and gives, over a stated window of nu x nv square cells in the world frame,
 * per cell: the ground height, the state FREE / OBSTACLE / STEP / UNKNOWN, the ground's colour and class (a top-down ortho image of
 * the driving surface), the height of the tallest obstacle and the exact squared distance, in cells, to the nearest blocking cell.
 * Sources, model, tick, stored poses, fern keyframes and tracker state are untouched; frames in flight are waited for.
 *   Definition, in integers (restated by tests/ground_ref.py):
 *   Units.  Q(mm) = (mm * 65536 + 500) / 1000 by integer division: lengths are in 2^-16 m.  C = Q(cell_mm), B = Q(band_mm),
 *     L = Q(clear_lo_mm), Hi = Q(clear_hi_mm), S = Q(step_mm).
 *   Axes.  a = up >> 1, sgn = (up & 1) ? -1 : +1: axis a points up, negated if the low bit is set.  The horizontal axes are the
 *     other two in ascending order, ua < va: for a = 1, u = x and v = z.  The default, 3, is -y: a camera-frame world with y down.
 *   Record quantities.  The simplification's: its regular-record test on the fields and |(double)p[k] - (double)origin[k]| < 2^24;
 *     X[k] = floor(((double)p[k] - (double)origin[k]) * 65536.0); the quantised normal ni[k]; the weight w; the class c = colour
 *     word >> 24.  (Not its cell range: the window bounds the cells here.)  A record that fails the test is LOOSE.
 *   Placement.  cu = floor_div(X[ua], C), cv = floor_div(X[va], C), H = sgn * X[a].  A regular record with cu outside [0, nu), cv
 *     outside [0, nv) or |H| >= 2^30 is OUTSIDE; the rest lie in cell (cu, cv).  origin is the window's low corner on the two
 *     horizontal axes and height zero on the up axis.
 *   Ground-like.  The record's class has its bit in ground_mask and normal_sign * sgn * ni[a] >= min_up.  normal_sign is +1 for
 *     normals that point out of the surface, towards the viewer, and -1 for normals that point into it, away from the camera that
 *     saw it: the fusion stores the latter (a road seen from above has a normal that points down), so -1 is the default.
 *   Reading 1.  Z[cell] = the minimum H of the cell's ground-like records; a cell that has one "has ground".
 *   Reference height R[cell].  Z[cell] if the cell has ground; otherwise Z of the cell (u', v') with ground that minimises
 *     (du^2 + dv^2, v', u') lexicographically among the cells of the window with |du| <= fill_cells and |dv| <= fill_cells;
 *     otherwise none.
 *   Reading 2.  For every record in the window, with d = H - R[cell], the first rule that applies:
 *     1. no R: UNREFERENCED.
 *     2. GROUND: the record is ground-like, its cell has ground and 0 <= d <= B.  SW += w, SH += w * d, SC[ch] += w * channel[ch]
 *        (ch = 0, 1, 2: bytes 0, 1, 2 of the colour word, b g r), best = max(best, w << 40 | (0x7FFFFFFF - id) << 8 | c).
 *     3. OBSTACLE: L < d < Hi.  n_obst += 1, top = max(top, d).
 *     4. IGNORED: overhangs above the body band (bridges, canopies), anything below the reference, the slab between the ground
 *        band and clear_lo.
 *   Planes.  A cell with ground: ground = Z + (SH + SW / 2) / SW, bgr[ch] = (SC[ch] + SW / 2) / SW, cls = best & 255 (the class
 *     of the heaviest ground record, the smallest id among equals).  A cell without: ground = SM_GROUND_NONE, bgr = 0, cls = 255.
 *     top = the cell's largest obstacle d, 0 when it has none.  Heights are in 2^-16 m above origin[a] along the up direction.
 *   State.  The first rule that applies: OBSTACLE (2) n_obst >= min_obstacle; UNKNOWN (0) no ground; STEP (3) step_mm > 0 and a
 *     4-neighbour inside the window has ground with |ground - ground'| > S; FREE (1).
 *   Clearance.  clear2 = min(reach_cells^2, min over blocking cells of du^2 + dv^2).  Blocking: OBSTACLE, STEP, and UNKNOWN when
 *     unknown_blocks is set.  A blocking cell has 0.  Cells outside the window do not block.
 *   Info.  records: of the set.  counts: records GROUND, OBSTACLE, IGNORED, UNREFERENCED, OUTSIDE, LOOSE.  cells: by state.
 *   The result is a function of the multiset of (global id, record) pairs alone: the chunking, the split into files and the
 *     device's order do not change a bit of it.  The 64-bit sums cannot overflow: w <= 255, d <= Q(10000) and fewer than 2^31
 *     records keep SH below 2^59.
 *   Example, cell_mm 1000 (C = 65536), up 3, origin 0, nu 5, nv 1, normal_sign +1 (the normals below point out of the surface),
 *     the other parameters at their defaults (B = 13107, L = 9830,
 *     Hi = 131072, S = 9830); seven records of conf 1 (w = 16), ids 0..6: (0.5, 1, 0.5) normal (0, -1, 0) class 0;
 *     (1.5, 1, 0.5) (0, -1, 0) class 0; (1.5, 0.875, 0.5) (0, -1, 0) class 1; (2.5, 0, 0.5) (-1, 0, 0); (2.5, -0.5, 0.5) (-1, 0, 0);
 *     (3.5, 1, 0.5) (0, -1, 0); (4.5, 0.5, 0.5) (0, -1, 0).  Z = -65536, -65536, none, -65536, -32768.  Cell 1: ground = -65536 +
 *     (16 * 8192 + 16) / 32 = -61440, class 0 (the weights tie: the lower id wins).  Cell 2 borrows R = -65536 from cell 1 (cells 1
 *     and 3 are equally near: the lower u wins); its records have d = 65536 and 98304: OBSTACLE, top = 98304.  Cells 3 and 4
 *     differ by 32768 > S: both STEP.  state = 1 1 2 3 3, clear2 = 4 1 0 0 0, counts = 5 2 0 0 0 0.
 *   Output.  Planes are row-major, row = cell v, column = cell u, nu * nv entries each (bgr: three bytes a cell).  Every plane may
 *     be NULL; clear2 == NULL skips the distance transform.  A failing call writes no plane and not info.
 *   File skipping.  A file is read in neither reading when the box of its valid entry in the context's file index misses the
 *     window's horizontal extent (the box is grown by nothing: a record's cell depends on its centre only).  Its header is still
 *     checked and counts towards the ids; its records count as OUTSIDE.  SM_RECALL_NO_INDEX=1 turns the lookups off.
 *   Cost.  Reading 1: one atomicMin per run of ground-like records of one cell among neighbouring lanes of a wave.  One launch
 *     over the cells fills R from an LDS tile with a halo of fill_cells.  Reading 2: a record's contribution combined in the wave
 *     per run of equal cells, then integer atomics without return value.  Two launches finish the planes and the states (a
 *     4-neighbour stencil), two make the capped Euclidean distance transform: columns (the 1-D distance, capped), then rows (the
 *     minimum of du^2 + g(u')^2 over |du| <= reach_cells, from LDS).  SM_GROUND_NO_COMBINE=1, read per call, switches the in-wave
 *     combination off in both readings; the result is the same.  Device memory: 64 bytes a cell of accumulators plus the planes,
 *     allocated per call and freed when it ends.
 * sm_ground_stats: of the context's last sm_ground_maps that succeeded (a call that fails leaves them as they were).
 * Errors.  SM_E_ARG: NULLs other than the planes; a parameter outside the ranges below; nu * nv > 2^24; a non-finite origin; the
 *   header and set checks of sm_render_image_maps (every header before any work); a call between sm_stage_conflict and
 *   sm_stage_cull; sm_ground_stats before any call has succeeded.  SM_E_UNSUPPORTED: a sharded or rig context.  SM_E_CAPACITY: a
 *   set of more than 2^31 - 1 records. */
#define SM_GROUND_NONE     INT32_MIN     /* `ground` of a cell without ground */
#define SM_GROUND_UNKNOWN  0
#define SM_GROUND_FREE     1
#define SM_GROUND_OBSTACLE 2
#define SM_GROUND_STEP     3
typedef struct sm_ground_params {
    int32_t  cell_mm;         /* edge of a cell, 10..10000                                            default 100 */
    int32_t  up;              /* 2 * axis + negated, 0..5                                             default 3 (-y) */
    float    origin[3];       /* metres: the window's low corner; height zero on the up axis          default 0 */
    int32_t  nu, nv;          /* cells, 1..8192 each, nu * nv <= 2^24                                 default 256 each */
    int32_t  min_up;          /* least up-component of a ground-like normal in 2^-14, 0..16384        default 11585 (45 degrees) */
    uint32_t ground_mask[8];  /* bit c & 31 of word c >> 5: class c may be ground                     default all ones */
    int32_t  band_mm;         /* ground band above a cell's lowest ground-like record, 0..10000       default 200 */
    int32_t  clear_lo_mm;     /* the body band above the reference height:                            default 150 */
    int32_t  clear_hi_mm;     /*   0 <= clear_lo_mm < clear_hi_mm <= 100000                           default 2000 */
    uint32_t min_obstacle;    /* >= 1: records in the body band that make a cell an obstacle          default 2 */
    int32_t  fill_cells;      /* how far a cell without ground looks for a neighbour's, 0..16         default 3 */
    int32_t  step_mm;         /* height step between 4-neighbours that blocks, 0..10000; 0: off       default 150 */
    int32_t  reach_cells;     /* the clearance saturates here, 1..255                                 default 32 */
    int32_t  unknown_blocks;  /* 0 / 1: UNKNOWN cells count as blocking                               default 0 */
    int32_t  normal_sign;     /* +1: normals point out of the surface; -1: into it, as stored         default -1 */
} sm_ground_params;
typedef struct sm_ground_info {
    uint64_t records;         /* of the set */
    uint64_t counts[6];       /* records GROUND, OBSTACLE, IGNORED, UNREFERENCED, OUTSIDE, LOOSE */
    uint32_t cells[4];        /* by state: UNKNOWN, FREE, OBSTACLE, STEP */
} sm_ground_info;
typedef struct sm_ground_stats_t {
    uint32_t chunks;          /* pieces of at most 2^20 records, both readings together */
    uint32_t launches;
    uint32_t files_skipped;   /* by the file index */
    float read_ms;            /* host: reading the files */
    float ground_ms;          /* device: the planes' initialisation and reading 1 */
    float fill_ms;            /* device: the reference heights */
    float accumulate_ms;      /* device: reading 2 */
    float state_ms;           /* device: planes, states, steps */
    float clear_ms;           /* device: the distance transform */
    float copy_ms;            /* the planes back to the caller */
    float total_ms;
} sm_ground_stats_t;
int sm_default_ground_params(sm_ground_params *p);           /* pure, no context */
int sm_ground_maps(sm_ctx *s, const sm_map_source *src, const sm_ground_params *p,
                   int32_t *ground, int32_t *top, uint8_t *state, uint8_t *cls, uint8_t *bgr /* three bytes a cell */,
                   uint32_t *clear2, sm_ground_info *info);   /* every plane may be NULL; info may not */
int sm_ground_stats(sm_ctx *s, sm_ground_stats_t *out);      /* SM_E_ARG before the first call */

/* ---- routes over the ground map: cost-to-go fields and paths (DESIGN.md "4ac. Routes") ----
 * sm_route_ground takes the `state` and `clear2` planes sm_ground_maps returned and, for each of n_fields goal sets, computes over the
 * same nu x nv window the least cost of an 8-connected path from every cell to any goal of the set (`cost`), the direction of the
 * first step of such a path (`next`), and for a list of starts the cells of the path that follows `next`.  It reads nothing of the
 * model and of no file and changes nothing in the context but its own stats; it runs on the context's stream, behind frames in
 * flight, and works on any context.
 *   Definition, in integers (restated by tests/route_ref.py):
 *   Window.  nu, nv in 1..4096, nu * nv <= 2^22.  Planes are row-major, row = cell v, column = cell u, as sm_ground_maps writes them.
 *   Passable.  A cell is passable when state == FREE, or state == UNKNOWN and unknown_passable is set; and clear2 >= body_cells^2.
 *     body_cells is the vehicle's radius.  clear2 saturates at the ground map's reach_cells^2: the caller must have asked the ground
 *     map for reach_cells >= body_cells (and >= soft_cells for the multiplier to see that far); this call cannot check it.
 *   Multiplier.  S2 = soft_cells^2.  m = 1 when soft_cells == 0, otherwise m = 1 + (near_weight * (S2 - min(clear2, S2))) / S2 by
 *     integer division: 1..15, cells near obstacles cost more.
 *   Directions.  k = 0..7 is (du, dv) = (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1).  L_k = 12 for even k, 17 for odd k
 *     (17 / 12 is within 0.2 % of sqrt 2).
 *   Edges.  The edge p -> q = p + dir_k exists when p and q are both in the window and passable; for odd k the cells (pu + du, pv)
 *     and (pu, pv + dv) must be passable too: no path cuts a corner.  Its cost is L_k * (m[p] + m[q]).  Edges are symmetric, so the
 *     field from the goals is the cost to them.
 *   Goals.  Field f's goals are the pairs (u, v) goals[2 i], goals[2 i + 1] for goal_first[f] <= i < goal_first[f + 1];
 *     goal_first[0] = 0.  n_fields >= 1, n_fields * nu * nv <= 2^26.  A passable goal has cost 0; an impassable goal contributes
 *     nothing and is counted in info.
 *   cost.  uint32[n_fields][nv][nu]: the shortest-path distance in that graph, SM_ROUTE_NONE where there is no path: unique.  A
 *     shortest path visits a cell at most once and an edge costs at most 17 * 30 = 510, so cost < 510 * 2^22 < 2^31: no overflow.
 *   next.  uint8[n_fields][nv][nu].  The first rule that applies: 8 at a cell of cost 0; 255 at an impassable or unreachable cell;
 *     otherwise the smallest k whose edge exists and has cost[q] + w == cost[p].  A pure function of cost.
 *   Paths.  Start i is the triple (field, u, v) starts[3 i ..].  A start whose cost is NONE has path_len 0 and path_cost NONE.
 *     Otherwise the path is the start, then `next` repeatedly until a cell with next == 8 (cost falls strictly along it: no cycle);
 *     path_len = min(cells on it, max_steps + 1), path_cost = cost[start] whether truncated or not.  path is
 *     uint32[n_starts][max_steps + 1] of cell numbers v * nu + u, padded with 0xFFFFFFFF.
 *   Info, per field: goals used and dropped, reachable cells (the goals among them), the largest cost (0 with none reachable).
 *   Output.  cost, next, path, path_len and path_cost may each be NULL: a caller who only wants paths copies nothing else back.  A
 *     failing call writes none of them and not info.
 *   Example 1.  nu = nv = 3, all FREE but the centre (OBSTACLE), body_cells = soft_cells = 0, one goal (0, 0).  cost by rows is
 *     0 24 48 / 24 NONE 72 / 48 72 96: (2, 1) is 72 and not 24 + 34, the diagonal from (1, 0) would cut the corner of the centre.
 *     next at (2, 2) is 4: directions 4 and 6 both reach 96, the smaller wins.
 *   Example 2.  nu = 4, nv = 1, all FREE, clear2 = 4 1 2 4, soft_cells = 2, near_weight = 8, goal u = 3.  m = 1 7 5 1,
 *     cost = 312 216 72 0.
 *   Cost.  One launch writes a byte m and a byte of edge bits per cell, shared by all fields.  The relaxation is tiled: a workgroup
 *     takes one (field, tile of 32 x 32 cells) whose flag is up, relaxes it in LDS until a sweep changes nothing, writes it back and
 *     raises the flags of the neighbouring tiles whose facing border changed.  A round is a launch; the host reads one counter of
 *     raised flags from pinned memory every rounds_per_check rounds and stops when it is 0.  No workgroup waits for another, and the
 *     result does not depend on the order of anything.  SM_ROUTE_TILE=16|32|64 and SM_ROUTE_SWEEPS=n (the cap on the sweeps of one
 *     visit, default half the tile's cells; 1 is the plain global relaxation), read per call, change the schedule and not a bit of the result.
 *     Device memory: 4 bytes a cell and field for cost, 1 for next, 7 a cell shared, allocated per call and freed when it ends.
 * sm_route_stats: of the context's last sm_route_ground that succeeded (a call that fails leaves them as they were).
 * Errors.  SM_E_ARG: NULLs other than the outputs named above (goals with no goal and starts with no start may be NULL); a parameter
 *   outside the ranges below; nu * nv > 2^22, n_fields * nu * nv > 2^26 or n_starts * (max_steps + 1) > 2^26 (all refused before
 *   anything is allocated); goal_first that does not start at 0 or falls; a goal or a start outside the window, a start's field
 *   outside 0..n_fields - 1; SM_ROUTE_TILE or SM_ROUTE_SWEEPS set to something else; sm_route_stats before any call has succeeded.
 *   SM_E_STALL: flags still up after max_rounds rounds (termination is a theorem -- costs are integers that only fall -- the bound
 *   is there for bugs). */
#define SM_ROUTE_NONE 0xFFFFFFFFu     /* `cost` of a cell no path leaves towards a goal; `path_cost` of such a start */
typedef struct sm_route_params {
    int32_t nu, nv;             /* cells, 1..4096 each, nu * nv <= 2^22: the planes' window              default 256 each */
    int32_t body_cells;         /* the vehicle's radius in cells, 0..255                                 default 0 */
    int32_t soft_cells;         /* how far from an obstacle a cell costs more, 0..255; 0: nowhere        default 0 */
    int32_t near_weight;        /* the multiplier beside an obstacle is 1 + near_weight, 0..14           default 0 */
    int32_t unknown_passable;   /* 0 / 1: UNKNOWN cells may be driven on                                 default 0 */
    int32_t max_steps;          /* a path holds at most max_steps + 1 cells, 0..2^22                     default 4096 */
    int32_t rounds_per_check;   /* rounds enqueued between two looks at the counter, 1..64               default 4 */
    int32_t max_rounds;         /* >= 1: SM_E_STALL beyond                                               default 65536 */
} sm_route_params;
typedef struct sm_route_info {
    uint32_t goals_used;        /* passable goals of the field */
    uint32_t goals_dropped;     /* impassable ones */
    uint32_t reachable;         /* cells with a cost */
    uint32_t max_cost;          /* the largest of them */
} sm_route_info;
typedef struct sm_route_stats_t {
    uint32_t rounds;            /* relaxation launches that found a flag up */
    uint32_t launches;          /* every kernel launch of the call, the rounds over lowered flags included */
    uint64_t tile_visits;       /* (field, tile) pairs relaxed, over all rounds */
    uint32_t tile;              /* the tile edge used */
    uint32_t sweep_cap;         /* the cap on the sweeps of one visit used */
    float prepare_ms;           /* device: the planes' way up, the multipliers and edges, the goals */
    float relax_ms;             /* device and the host's looks at the counter: the rounds */
    float next_ms;              /* device: next and the info */
    float walk_ms;              /* device: the paths */
    float copy_ms;              /* the outputs back to the caller */
    float total_ms;
} sm_route_stats_t;
int sm_default_route_params(sm_route_params *p);              /* pure, no context */
int sm_route_ground(sm_ctx *s, const sm_route_params *p, const uint8_t *state, const uint32_t *clear2,
                    uint32_t n_fields, const uint32_t *goal_first, const int32_t *goals /* pairs u, v */,
                    uint32_t n_starts, const int32_t *starts /* triples field, u, v */,
                    uint32_t *cost, uint8_t *next, uint32_t *path, uint32_t *path_len, uint32_t *path_cost,
                    sm_route_info *info /* [n_fields] */);
int sm_route_stats(sm_ctx *s, sm_route_stats_t *out);         /* SM_E_ARG before the first call */

/* ---- routes a car can follow: cost-to-go over (cell, heading) with a turning radius (DESIGN.md "4ad. Routes for a car") ----
 * sm_route_ground's path belongs to a point that turns on the spot.  sm_route_car searches over states (cell, heading) with moves a
 * car can make -- a step ahead, a turn to either side that takes turn_cells cells ahead and as many along the new heading, and
 * (if allowed) a step back -- over the same `state` and `clear2` planes, per goal set.  Like sm_route_ground it reads nothing of the
 * model and of no file, changes nothing in the context but its own stats, runs on the context's stream and works on any context.
 *   Definition, in integers (restated by tests/car_ref.py):
 *   Cells.  The window and its limits, Passable, the Multiplier m, the Directions k = 0..7 with L_k, and the unit edge p -> p + dir_k
 *     with its existence rule (corner rule included) and its cost e_k(p) = L_k * (m[p] + m[q]) are sm_route_ground's, above, word for
 *     word; body_cells, soft_cells, near_weight, unknown_passable, max_steps, rounds_per_check and max_rounds mean what they mean there.
 *   States.  (u, v, h): the cell and the heading h = 0..7, which is direction k = h.  Plane index (h * nv + v) * nu + u.
 *   Parameters.  turn_cells = n in 1..16; turn_cost in 0..4095; reverse_weight in 0..15, 0: the car cannot reverse.
 *   Moves out of (p, h), by code:
 *     0 F  to (p + d_h, h); exists when the unit edge p -> p + d_h exists; weight e_h(p).
 *     1 L (s = +1), 2 R (s = -1)  h' = (h + s) & 7; the cells c_0 = p, c_i = c_(i-1) + d_h for i = 1..n, c_(n+j) = c_(n+j-1) + d_h'
 *          for j = 1..n; exists when all 2 n unit edges along that polyline exist; weight = the sum of their costs + turn_cost;
 *          to (c_2n, h').
 *     3 B  only with reverse_weight > 0: to (p - d_h, h); exists when the unit edge in direction (h + 4) & 7 exists; weight
 *          reverse_weight * e_((h+4)&7)(p).
 *     Every weight is at most 32 * 510 + 4095 = 20 415 < 2^15.
 *   Turning radius.  The graph is directed.  Two turns to the same side are separated by a straight run of at least 2 n cells (a
 *     turn ends with n cells along h', the next begins with n cells along h'), so a half turn -- four turns of 45 degrees -- is
 *     6 n cells wide (Example 2) and the turning radius is about 3 * turn_cells cells.  Derived from the moves, not measured.
 *   Goals.  Field f's goals are the triples (u, v, h) goals[3 i ..] for goal_first[f] <= i < goal_first[f + 1], goal_first as in
 *     sm_route_ground; h = -1 means any heading and seeds all 8 states of the cell.  A goal in an impassable cell contributes
 *     nothing and is counted in info.  n_fields >= 1, n_fields * nu * nv <= 2^23.
 *   cost.  uint32[n_fields][8][nv][nu]: the least total weight of a sequence of moves from the state to a goal state of the field,
 *     0 at goal states, SM_ROUTE_NONE where there is none (or none cheaper than 2^31, below).
 *   Range.  A candidate cost[target] + w >= 2^31 is never stored.  The result is therefore the true least cost where that is
 *     < 2^31 and SM_ROUTE_NONE otherwise: weights are >= 0, so every state on a least-cost sequence has a true cost no larger than
 *     the start's, and a sequence through a state whose true cost is >= 2^31 costs >= 2^31 -- dropping such candidates removes no
 *     sequence cheaper than 2^31 and keeps every one that is.  With cq < 2^31 and w < 2^15 the sum cq + w never wraps a uint32.
 *   next.  uint8, the shape of cost: 8 at cost 0; 255 at SM_ROUTE_NONE; otherwise the smallest move code whose move exists with
 *     cost[target] + w == cost[state].  A pure function of cost.
 *   Paths.  Start i is the quadruple (field, u, v, h) starts[4 i ..].  path is uint32[n_starts][max_steps + 1] of words
 *     cell | heading << 22 | reverse << 25 with cell = v * nu + u < 2^22.  The first word is the start state with reverse 0; then
 *     EVERY unit cell passed, move after move along `next` until a state with next == 8: F one cell with heading h; L or R its 2 n
 *     cells, the first n with heading h, the next n with h'; B one cell with heading h and reverse 1.  A start whose cost is NONE
 *     has path_len 0 and path_cost NONE; otherwise path_len = min(words on it, max_steps + 1) (a turn may be cut in the middle),
 *     path_cost = cost[start] whether truncated or not; padded with 0xFFFFFFFF.
 *   Info, per field: goals used and dropped, reachable states, reachable cells (a cost at any heading), the largest cost.
 *   Output.  cost, next, path, path_len and path_cost may each be NULL.  A failing call writes none of them and not info.
 *   Example 1.  nu = 5, nv = 3, all FREE, m = 1, n = 1, turn_cost 0, no reverse, goal (4, 1, -1).  cost at (0, 1) for h = 0..7 is
 *     96 116 NONE NONE NONE NONE NONE 116: 96 is four steps of 24; the 116 at h = 1 is R (to (1, 2) for 34, to (2, 2) for 24, now
 *     h = 0), then R again (to (3, 2) for 24, to (4, 1) for 34).  With reverse_weight = 2: 96 116 290 464 192 464 290 116.  With the
 *     goal (4, 1, 0) and turn_cost = 5 only h = 0 has a cost, 96.
 *   Example 2.  nu = nv = 7, all FREE, n = 1, no reverse, goal (0, 6, 4).  From (3, 0, h 0) the cost is 304: four turns of 58 that
 *     end at (3, 6, h 4), then three steps of 24; with turn_cost = 9 it is 340.  From (2, 0, h 0) it is 280; from (4, 0, h 0) NONE:
 *     the half turn needs three cells to the side.
 *   Example 3.  nu = 4, nv = 1, m = 1 7 5 1 (sm_route_ground's Example 2), goal (3, 0, -1), reverse_weight = 3.  cost at h = 0 is
 *     312 216 72 0, at h = 4 it is 936 648 216 0.
 *   Cost.  One launch writes m and the edge bits per cell as sm_route_ground does, a second the weights of the four moves of every
 *     state (16 bits each, 0xFFFF: the move does not exist), shared by all fields.  The relaxation is sm_route_ground's in shape: a
 *     workgroup per (field, tile of 32 x 32 cells x 8 headings) whose flag is up, the tile's 8192 costs in LDS; what the tile's
 *     states reach outside it (a move's target lies up to 2 n cells away) is folded once per visit into one value per state, the
 *     sweeps run over the targets inside.  Changed states go back, and the flags of the neighbouring tiles within 2 n cells of a
 *     changed cell are raised.  Rounds are launches, the host reads one counter every rounds_per_check rounds.  SM_CAR_TILE=16|32
 *     (16 refused with turn_cells > 8: a tile is at least 2 n cells wide) and SM_CAR_SWEEPS=n, read per call, change the schedule
 *     and not a bit of the result.  Device memory: 32 bytes a cell and field for cost, 8 for next, 71 a cell shared.
 * sm_route_car_stats: of the context's last sm_route_car that succeeded.
 * Errors.  SM_E_ARG: as sm_route_ground's, with n_fields * nu * nv > 2^23 and n_starts * (max_steps + 1) > 2^26 refused before
 *   anything is allocated; turn_cells, turn_cost or reverse_weight outside their ranges; a goal's heading outside -1..7, a start's
 *   outside 0..7; SM_CAR_TILE or SM_CAR_SWEEPS set to something else.  SM_E_STALL: flags still up after max_rounds rounds. */
#define SM_CAR_MOVE_F 0
#define SM_CAR_MOVE_L 1
#define SM_CAR_MOVE_R 2
#define SM_CAR_MOVE_B 3
typedef struct sm_route_car_params {
    int32_t nu, nv;             /* as sm_route_params                                                    default 256 each */
    int32_t body_cells;         /* as sm_route_params                                                    default 0 */
    int32_t soft_cells;         /* as sm_route_params                                                    default 0 */
    int32_t near_weight;        /* as sm_route_params                                                    default 0 */
    int32_t unknown_passable;   /* as sm_route_params                                                    default 0 */
    int32_t turn_cells;         /* n: a turn of 45 degrees runs n cells ahead and n along the new heading, 1..16   default 2 */
    int32_t turn_cost;          /* added to a turn's weight, 0..4095                                     default 0 */
    int32_t reverse_weight;     /* a step back costs this many times the edge, 0..15; 0: no reverse      default 0 */
    int32_t max_steps;          /* a path holds at most max_steps + 1 words, 0..2^22                     default 4096 */
    int32_t rounds_per_check;   /* as sm_route_params                                                    default 4 */
    int32_t max_rounds;         /* as sm_route_params                                                    default 65536 */
} sm_route_car_params;
typedef struct sm_route_car_info {
    uint32_t goals_used;        /* goals of the field in passable cells */
    uint32_t goals_dropped;     /* those in impassable ones */
    uint32_t reachable_states;  /* states with a cost */
    uint32_t reachable_cells;   /* cells with a cost at any heading */
    uint32_t max_cost;          /* the largest cost (0 with none) */
} sm_route_car_info;
typedef struct sm_route_car_stats_t {
    uint32_t rounds;            /* relaxation launches that found a flag up */
    uint32_t launches;          /* every kernel launch of the call */
    uint64_t tile_visits;       /* (field, tile) pairs relaxed, over all rounds */
    uint32_t tile;              /* the tile edge used */
    uint32_t sweep_cap;         /* the cap on the sweeps of one visit used */
    float prepare_ms;           /* device: the planes' way up, multipliers, edges, the moves' weights, the goals */
    float relax_ms;             /* device and the host's looks at the counter: the rounds */
    float next_ms;              /* device: next and the info */
    float walk_ms;              /* device: the paths */
    float copy_ms;              /* the outputs back to the caller */
    float total_ms;
} sm_route_car_stats_t;
int sm_default_route_car_params(sm_route_car_params *p);      /* pure, no context */
int sm_route_car(sm_ctx *s, const sm_route_car_params *p, const uint8_t *state, const uint32_t *clear2,
                 uint32_t n_fields, const uint32_t *goal_first, const int32_t *goals /* triples u, v, h */,
                 uint32_t n_starts, const int32_t *starts /* quadruples field, u, v, h */,
                 uint32_t *cost, uint8_t *next, uint32_t *path, uint32_t *path_len, uint32_t *path_cost,
                 sm_route_car_info *info /* [n_fields] */);
int sm_route_car_stats(sm_ctx *s, sm_route_car_stats_t *out);  /* SM_E_ARG before the first call */

/* ---- scenes: a map set with moving actors in it (DESIGN.md "4w. Scenes") ----
 * Everything above replays a static world.  A scene is a map set plus actors: an actor is a map file whose records are in the
 * actor's OWN frame, with one actor->world pose per view (or sweep).  The actor files are read once per call and stay on the
 * device; every view draws each actor under that view's pose into the key planes the static set is drawn into.  No file is
 * copied, warped or rewritten, and the static set is read once per batch of views, not once per view.
 *   Two calls draw scenes: the novel view with sm_render_image_maps_ex's extras (sm_render_image_scene) and the lidar sweep
 *   (sm_lidar_sweep_scene).  The model view (sm_render_model_maps) and the blended view (sm_render_image_maps_blend) draw no scenes.
 * Placed row.  Row m of actor j in view i becomes m' by sm_warp_by_time's row rule with C = poses12 row i of actor j (ROW-major
 *   3x4 [R|t], corr12's layout), applied to every row whatever its time:
 *     m'[0] = ((C[0]*m[0] + C[1]*m[1]) + C[2]*m[2]) + C[3],   m'[1], m'[2] likewise with C[4..7], C[8..11];
 *     m'[8] = (C[0]*m[8] + C[1]*m[9]) + C[2]*m[10],           m'[9], m'[10] likewise; no translation, no renormalisation;
 *   fp32, no contraction; every other field bit-identical.  sm_scene_place_rows is that rule on the host (no context; n rows of 12
 *   floats from rows_in to rows_out, which may be the same array), so the definition is executable from C.
 * Scene of view i.  S_i = the files of `src` in order, then (include_model) the live model's rows, then for every actor present
 *   in view i, in list order, its placed rows in file order.
 * Equality.  For every view i, sm_render_image_scene writes bgr, sem and depth_mm that equal sm_render_image_ex of a context
 *   holding S_i, bit for bit, the fill included; sm_lidar_sweep_scene writes range, rgb and sem that equal sm_lidar_sweep of that
 *   context, bit for bit.  A depth or range tie goes to the earlier source: static beats actor, an earlier actor a later one.
 * Ids (the lidar's id plane).  Static ids are sm_lidar_sweep_maps'.  Row r of actor j has id A + off_j + r: A is the static total
 *   (files and live model), off_j the sum of the record counts of actors 0..j-1, PRESENT OR NOT, so an id does not depend on the
 *   view; with every actor present it is the concatenation's id.  More than 2^31 - 1 ids in all: SM_E_CAPACITY before anything is drawn.
 * Independence.  The result depends neither on the chunking, nor on the views per pass, nor on the key budget
 *   (SM_RENDER_MAPS_KEY_MB, SM_LIDAR_KEY_MB), nor on the culling switches, nor on whether two actors name the same file.
 * Degenerate scenes.  scene == NULL or n_actors == 0 equals sm_render_image_maps_ex / sm_lidar_sweep_maps bit for bit (and
 *   enqueues exactly what they enqueue); an actor file of 0 records is valid and takes no ids; n_views == 0 checks the set and the
 *   actors and draws nothing.
 * Limits.  At most SM_SCENE_MAX_ACTORS actors; at most SM_SCENE_MAX_RECORDS records summed over the DISTINCT actor files (two
 *   actors whose paths compare equal share one resident copy).  Beyond either: SM_E_CAPACITY.
 * Errors.  The scene's arguments and every actor's header are checked first, then the set's, before any work; every error leaves
 *   the outputs unwritten.  SM_E_ARG: a NULL actor list with n_actors > 0, a NULL path or NULL poses12; a non-finite entry in a
 *   pose row of a view where the actor is present; a rotation part farther than 1e-3 from orthonormal (largest entry of
 *   |R^T R - I|, in double) or with det <= 0 (sm_loop_spread's test: the culling proof needs near-rigid poses; rows of views the actor is
 *   absent from are not read); an actor file that is missing or whose length disagrees with its header; the argument errors of
 *   sm_render_image_maps_ex / sm_lidar_sweep_maps.  SM_E_UNSUPPORTED: a sharded or rig context.
 * Side effects.  Those of the _maps calls and no more: actor files are read, never written; the model, the tick, the poses and
 *   the frame log are untouched.  sm_render_maps_stats / sm_lidar_stats / sm_fill_stats tell of the static part exactly as after the
 *   _maps calls; sm_scene_stats tells of the actors.
 * SM_SCENE_NO_CULL=1 (read per call) turns the per-(actor block, view) test off (an A/B switch: the outputs are the same). */
#define SM_SCENE_MAX_ACTORS  4096u
#define SM_SCENE_MAX_RECORDS (1u << 22)
typedef struct sm_scene_actor {
    const char    *path;      /* a map file (sm_save_map's format); its records are in the actor's own frame */
    const float   *poses12;   /* n_views rows of 12 floats: ROW-major 3x4 [R|t], actor -> world -- corr12's layout */
    const uint8_t *present;   /* n_views bytes, 0 = the actor is not in that view; NULL = in every view */
} sm_scene_actor;
typedef struct sm_scene { const sm_scene_actor *actors; uint32_t n_actors; } sm_scene;
/* what the last scene call of the context did with its actors */
typedef struct sm_scene_stats_t {
    uint32_t actors, files;        /* actors listed; distinct files among them */
    uint64_t records, bytes;       /* resident: records of the distinct files; device bytes of their planes, boxes and tables */
    uint64_t pairs_tested;         /* (actor block of 256 records, view) pairs with the actor present that the box test ran on (0 with SM_SCENE_NO_CULL=1) */
    uint64_t pairs_skipped;        /* ... of them, found outside the view or out of range and not drawn */
    float load_ms;                 /* reading the actor files, uploading and unpacking them (host clock) */
    float actor_ms;                /* device: the actors' splat and resolve launches (events), all batches together */
    float total_ms;                /* the whole call (host clock) */
} sm_scene_stats_t;
int sm_render_image_scene(sm_ctx *s, const sm_map_source *src, const sm_scene *scene, const float *views16, uint32_t n_views,
                          int w, int h, float fx, float fy, float cx, float cy, const sm_fill_params *fill /* NULL: none */,
                          uint8_t *bgr_out, uint8_t *sem_out, uint16_t *depth_mm_out /* NULL: not wanted */);
int sm_lidar_sweep_scene(sm_ctx *s, const sm_map_source *src, const sm_scene *scene, const sm_lidar_sensor *sn,
                         const float *poses16, uint32_t n_sweeps, float *range, int32_t *id, uint8_t *rgb, uint8_t *sem);
int sm_scene_place_rows(const float *pose12, const float *rows_in, uint32_t n, float *rows_out);   /* host only, no context */
int sm_scene_stats(sm_ctx *s, sm_scene_stats_t *out);        /* SM_E_ARG before the first scene call */

/* ---- ray casts: what a list of rays hits in a map set (DESIGN.md "4x. Ray casts") ----
 * sm_cast_rays_maps casts n_rays arbitrary rays into a map set -- an sm_map_source with the global ids of the map-set calls: the
 * files in list order, each in file order, then (include_model) the live model; no paths and include_model = 1: the live model
 * alone.  Ids are sm_lidar_sweep_maps' ids.  The set is read ONCE per call, whatever n_rays.
 * The rule (fp32, in the order written, no contraction).  For a ray (o, d, t_min, t_max) and a record with centre p, stored normal
 *   n (not normalised) and stored radius r:
 *     c_i = p_i - o_i
 *     den = (n.x*d.x + n.y*d.y) + n.z*d.z
 *     num = (n.x*c.x + n.y*c.y) + n.z*c.z
 *     t   = num / den
 *     q_i = t*d_i - c_i
 *     hit = t >= t_min && t <= t_max && ((q.x*q.x + q.y*q.y) + q.z*q.z) <= r*r
 *   Every comparison is false on a NaN; there is no epsilon; discs are two-sided; dir is used as given, so t is in units of its
 *   length.  A record takes part iff conf >= min_conf (in the live model: the occupied slots after the compaction every map-set
 *   call begins with -- dead slots are gone).  The return of a ray is the hitting record with the smallest t, ties to the lower
 *   id: the least key (bits(t + 0.0f) << 32) | id under a 64-bit atomicMin (the + 0.0f makes a t of -0 order as 0), and t + 0.0f is
 *   the t returned.
 * Rays.  A ray is valid iff its eight floats are finite, t_min >= 0, t_max >= t_min and dir is not all zeros.  An invalid ray
 *   returns the empty values and counts in stats.bad_rays; it is no error.
 * Outputs, one entry per ray; any but t may be NULL.  Empty values: t 0, id -1, rgb 0 0 0, sem 0, normal3 0 0 0.  rgb (3 bytes) and
 *   sem (class + 1) are made of the record's colour word exactly as sm_lidar_sweep makes them; normal3 is the returned record's
 *   stored normal, verbatim.
 * Independence.  The answer is defined by the rule alone: it depends neither on cell_mm, nor on origin, nor on the chunking, nor
 *   on the split of the set into files, nor on the order of work.  The voxel index only leaves out (ray, record) pairs that are
 *   proven to fail the test (csrc/sm_k_rays.h states the proof).  SM_RAYS_NO_INDEX=1 (read per call) tests every record against
 *   every ray (an A/B switch: the outputs are the same).
 * Lidar equality.  Under a pose whose rotation is the identity the lidar's c is p - o bit for bit, so a cast of
 *   sm_lidar_directions' table from that origin with [min_range, max_range] equals sm_lidar_sweep / sm_lidar_sweep_maps in all
 *   four planes, bit for bit.
 * Side effects: none on the model, the counters, the tick, the frame log or the trackers.  Synchronous.
 * Errors.  Everything is checked, every file's header included, before an output is written.  SM_E_ARG: a NULL ctx, source or
 *   params; NULL rays or t with n_rays > 0; cell_mm < 1 or above 2^24; a non-finite origin; n_rays > SM_RAYS_MAX; a
 *   call between sm_stage_conflict and sm_stage_cull; a missing file or one whose length disagrees with its header;
 *   sm_cast_rays_stats before any call has succeeded.  SM_E_UNSUPPORTED: a sharded or rig context.  n_rays == 0 checks the set only.
 * Files are never skipped: the file index bounds the centres of a file, not its radii, so no file is proven out of reach. */
#define SM_RAYS_MAX (1u << 24)
typedef struct sm_ray { float origin[3]; float t_min; float dir[3]; float t_max; } sm_ray;   /* 32 bytes, world frame */
typedef struct sm_rays_params {
    int32_t cell_mm;          /* the index grid's cell edge, 1..2^24 (speed only)                     default 250 */
    float   origin[3];        /* the index grid's origin (speed only)                                 default 0 0 0 */
    float   min_conf;         /* a record takes part iff conf >= min_conf (a NaN: none does)          default 0 */
    int32_t reserved[3];
} sm_rays_params;
typedef struct sm_rays_stats_t {
    uint64_t rays, bad_rays;  /* rays given; invalid ones among them */
    uint64_t records;         /* of the set */
    uint64_t wide;            /* records every ray tests directly: a cube over more than 8 cells, loose to the grid, a radius that
                                 is not finite, no slot in the table (or all taking part with SM_RAYS_NO_INDEX=1) */
    uint64_t pairs, cells;    /* (cell, record) pairs and distinct cells of the largest chunk */
    uint64_t probes, tests;   /* table probes (slots read) and exact tests, all rays and chunks */
    uint64_t no_slot;         /* of `wide`: regular records whose cells found no slot in an overfull table */
    uint64_t gave_up;         /* (ray, chunk) walks that visited more than 64 + n / 8 cells of a chunk of n records and tested its
                                 regular records one by one instead: at most n tests per ray and chunk */
    uint32_t chunks;          /* pieces of at most 2^20 records */
    uint32_t files_skipped;   /* always 0: see above */
    float read_ms;            /* host: reading the files */
    float copy_ms;            /* device: the chunks' copies */
    float index_ms;           /* device: building the chunks' indices */
    float cast_ms;            /* device: traversal, wide lists, resolve */
    float device_ms;          /* device: everything between the upload of the rays and the planes' copies back */
    float total_ms;
} sm_rays_stats_t;
int sm_default_rays_params(sm_rays_params *p);               /* pure, no context */
int sm_cast_rays_maps(sm_ctx *s, const sm_map_source *src, const sm_rays_params *p, const sm_ray *rays, uint32_t n_rays,
                      float *t, int32_t *id, uint8_t *rgb, uint8_t *sem, float *normal3);
int sm_cast_rays_stats(sm_ctx *s, sm_rays_stats_t *out);     /* SM_E_ARG before the first call */

/* ---- point queries: the nearest disc of a map set to arbitrary points (DESIGN.md "4y. Point queries") ----
 * sm_query_points_maps takes n_pts points, each with a reach of its own, and returns per point the nearest DISC of a map set within
 * that reach -- an sm_map_source with the global ids of the map-set calls: the files in list order, each in file order, then
 * (include_model) the live model; no paths and include_model = 1: the live model alone.  Ids are sm_cast_rays_maps' ids.  The set is
 * read ONCE per call, whatever n_pts.
 * The rule (fp32, in the order written, no contraction; / and sqrt correctly rounded).  For a point x with reach R and a record with
 *   centre p, stored normal n (not normalised) and stored radius r:
 *     c_i  = x_i - p_i
 *     nn   = (n.x*n.x + n.y*n.y) + n.z*n.z
 *     h    = (n.x*c.x + n.y*c.y) + n.z*c.z
 *     h2   = (h*h) / nn                       squared distance to the disc's plane
 *     cc   = (c.x*c.x + c.y*c.y) + c.z*c.z
 *     rho2 = cc - h2;            if !(rho2 > 0) rho2 = 0
 *     e    = sqrt(rho2) - |r|;   if !(e > 0)    e = 0        distance past the rim, in the plane
 *     dd   = h2 + e*e                         squared distance to the disc
 *     near = dd <= R*R  &&  dd < +inf
 *   Every comparison is false on a NaN; there is no epsilon.  A record takes part iff conf >= min_conf (in the live model: the
 *   occupied slots after the compaction every map-set call begins with -- dead slots are gone), none of its centre, normal and
 *   radius is a NaN, and nn > 0 and nn is finite: a zero normal takes no part, just as no ray can hit it; an infinite radius is
 *   the whole plane and takes part.  The answer for a point is the near record that takes part with the smallest dd, ties to the
 *   lower id: the least key (bits(dd + 0.0f) << 32) | id under a 64-bit atomicMin, and dd + 0.0f is the d2 returned.
 * Points.  A point is valid iff its three coordinates are finite and R >= 0; R = +inf is valid and asks for the nearest disc of the
 *   whole set (so does an R whose square overflows).  An invalid point returns the empty values and counts in stats.bad_points; it
 *   is no error.
 * Outputs, one entry per point; any but d2 may be NULL.  Empty values: d2 +inf, id -1, centre3 0 0 0, normal3 0 0 0, radius 0,
 *   rgb 0 0 0, sem 0.  centre3, normal3 and radius are the returned record's, verbatim; rgb (3 bytes) and sem (class + 1) are made
 *   of its colour word exactly as sm_cast_rays_maps makes them.
 * Independence.  The answer is defined by the rule alone: it depends neither on cell_mm, nor on origin, nor on the chunking, nor
 *   on the split of the set into files, nor on the order of work.  The voxel index -- the ray casts' -- only leaves out (point,
 *   record) pairs that are proven not to be near or not to win (csrc/sm_k_points.h states the proof).  SM_POINTS_NO_INDEX=1 (read
 *   per call) tests every record against every point (an A/B switch: the outputs are the same).
 * Side effects: none on the model, the counters, the tick, the frame log or the trackers.  Synchronous.
 * Errors.  Everything is checked, every file's header included, before an output is written.  SM_E_ARG: a NULL ctx, source or
 *   params; NULL points or d2 with n_pts > 0; cell_mm < 1 or above 2^24; a non-finite origin; n_pts > SM_POINTS_MAX; a
 *   call between sm_stage_conflict and sm_stage_cull; a missing file or one whose length disagrees with its header;
 *   sm_query_points_stats before any call has succeeded.  SM_E_UNSUPPORTED: a sharded or rig context.  n_pts == 0 checks the set only.
 * Files are never skipped: the file index bounds the centres of a file, not its radii, so no file is proven out of reach. */
#define SM_POINTS_MAX (1u << 24)
typedef struct sm_point { float pos[3]; float reach; } sm_point;   /* 16 bytes, world frame, metres */
typedef struct sm_points_params {
    int32_t cell_mm;          /* the index grid's cell edge, 1..2^24 (speed only)                     default 250 */
    float   origin[3];        /* the index grid's origin (speed only)                                 default 0 0 0 */
    float   min_conf;         /* a record takes part iff conf >= min_conf (a NaN: none does)          default 0 */
    int32_t reserved[3];
} sm_points_params;
typedef struct sm_points_stats_t {
    uint64_t points, bad_points;  /* points given; invalid ones among them */
    uint64_t records;         /* of the set */
    uint64_t wide;            /* records every point tests directly: a cube over more than 8 cells, loose to the grid, a radius that
                                 is not finite, no slot in the table (or all that pass the gate with SM_POINTS_NO_INDEX=1) */
    uint64_t pairs, cells;    /* (cell, record) pairs and distinct cells of the largest chunk */
    uint64_t probes, tests;   /* table probes (slots read) and exact tests, all points and chunks */
    uint64_t no_slot;         /* of `wide`: regular records whose cells found no slot in an overfull table */
    uint64_t gave_up;         /* (point, chunk) walks whose cube met more than 64 + n / 8 cells of a chunk of n records and tested its
                                 regular records one by one instead: at most n tests per point and chunk */
    uint32_t chunks;          /* pieces of at most 2^20 records */
    uint32_t files_skipped;   /* always 0: see above */
    float read_ms;            /* host: reading the files */
    float copy_ms;            /* device: the chunks' copies */
    float index_ms;           /* device: building the chunks' indices */
    float walk_ms;            /* device: walks, wide lists, resolve */
    float device_ms;          /* device: everything between the upload of the points and the planes' copies back */
    float total_ms;
} sm_points_stats_t;
int sm_default_points_params(sm_points_params *p);           /* pure, no context */
int sm_query_points_maps(sm_ctx *s, const sm_map_source *src, const sm_points_params *p, const sm_point *pts, uint32_t n_pts,
                         float *d2, int32_t *id, float *centre3, float *normal3, float *radius, uint8_t *rgb, uint8_t *sem);
int sm_query_points_stats(sm_ctx *s, sm_points_stats_t *out); /* SM_E_ARG before the first call */

/* ---- packed map files: 20-byte records that every map-set call reads (DESIGN.md "4aa. Packed map files") ----
 * A map file (u32 count | i32 startId | i32 endId | count x 12 fp32, 48 bytes a record) carries far less than 48 bytes of
 * information per record.  sm_pack_maps writes the files of a map set in a packed format of 20 bytes a record; every call that
 * READS a map set -- an sm_map_source -- takes plain and packed files, mixed in one list, and decodes a packed chunk on the GPU as
 * it lands.  A record's id stays its position in the set.  sm_unpack_maps makes plain files again.  Nothing calls either unasked.
 *   The file, little-endian:
 *     header, 32 bytes: u32 magic "SMPK" (0x4B504D53) | u32 version = 1 | u32 count | i32 startId | i32 endId | i32 pos_step_log2
 *       (s, -14..-6) | u32 n_blocks = ceil(count / 256) | u32 0.
 *     directory, n_blocks entries of 32 bytes, one per 256 consecutive records (the last block may be shorter): float origin[3] |
 *       float time_base | float init_base | u32 flags (bit 0 = RAW, the others 0) | u64 offset of the block in the payload.
 *     payload, block after block without gaps: a packed block of m records is m x 20 bytes, a RAW block its m x 48 bytes verbatim.
 *     The offsets are the prefix sums of the blocks' sizes, and the file's length is exactly 32 + 32 * n_blocks + their sum; a file
 *     that fails either is refused (SM_E_ARG, sm_last_error() names it) by every call, before anything is computed.  A file that
 *     begins with the magic is a packed one unless it has the very length of a plain file of 0x4B504D53 records (60 GB).
 *   A packed record m[0..11] = x y z conf | colour 0 init_time time | nx ny nz radius, five u32:
 *     w0 = qx | qy << 16      w1 = qz | qr << 16      w2 = the bits of m[4]      w3 = ou | ov << 10 | qc << 20      w4 = dt | di << 16
 *   All arithmetic is IEEE fp32, one operation at a time in the written order (no fused multiply-add), U = 2^-s, D = 2^s:
 *     origin[k] = floor(min over the block of m[k] * U) * D + 0;   q = floor((m[k] - origin[k]) * U + 0.5);   decoded origin[k] + (float)q * D
 *     qr = floor(radius * 8192 + 0.5), decoded qr / 8192;   qc = floor(conf * 16 + 0.5) in 12 bits, decoded qc / 16
 *     time_base, init_base = the block's minima of m[7], m[6];   dt = m[7] - time_base, di = m[6] - init_base, decoded base + (float)d
 *     normal, octahedral: a = (|nx| + |ny|) + |nz|, p = (nx / a, ny / a); if nz < 0: p = ((1 - |py|) * sgn(px), (1 - |px|) * sgn(py))
 *       with sgn(v) = v >= 0 ? 1 : -1; ou = clamp(floor((px * 0.5 + 0.5) * 1023 + 0.5), 0, 1023), ov likewise.  Decoded in integers:
 *       ui = 2 ou - 1023, vi = 2 ov - 1023, zi = 1023 - |ui| - |vi|, t = max(-zi, 0), xi = ui >= 0 ? ui - t : ui + t, yi likewise, then
 *       (xi, yi, zi) / sqrt((float)(xi^2 + yi^2 + zi^2)): decode(encode(decode(c))) == decode(c) for every one of the 2^20 codes.
 *     m[5] decodes to +0.
 *   A block is packed if and only if every one of its records has: every field but the colour word finite; |x|, |y|, |z| < 8192;
 *     every q <= 65535 (at the default step of 2^-10 m: an extent below 64 m); radius >= 0 and qr <= 65535; conf >= 0 and qc <=
 *     4095; m[5] = +0; both times integers in [+0, 2^24) with dt, di <= 65535; | |n|^2 - 1 | <= 2^-10 with |n|^2 = (nx nx + ny ny) +
 *     nz nz.  Every other block is RAW, and its directory entry holds zeros beside the flag and the offset.  RAW is what makes the
 *     format safe for NaN rows, for a tiled file that jumps across the map and for anything a caller has written into a file.
 *   Errors of a packed block against its source: position <= D / 2 plus one fp32 ulp of the coordinate, radius <= 2^-14 m, conf <=
 *     1 / 32, normal <= 0.25 degrees (worst case seen 0.235); colour, times and order exact.  unpack(pack(unpack(P))) ==
 *     unpack(P) byte for byte.
 * sm_pack_maps: file i of the source becomes "<out_prefix>_%06u.smp" with i's frame range; with include_model the live model
 *   follows as the next number, frame range 0, 0.  An empty file becomes a packed file of no block, so the lists stay parallel.  A
 *   packed source is packed again from its decoded records.  Sources and model stay as they are.  Every output is written as
 *   "<name>.pack.tmp"; all are renamed into place only after the last one is complete, and on any error none is and no temporary
 *   is left.  SM_E_ARG: NULLs, pos_step_log2 outside -14..-6, an output name equal to a source path (checked before anything is
 *   written), the file checks of sm_render_image_maps; SM_E_UNSUPPORTED: a sharded or rig context.
 * sm_unpack_maps: file i becomes "<out_prefix>_%06u.bin", a plain file: a packed source decoded, a plain one copied through
 *   verbatim.  include_model must be 0.  Written and refused as above (temporaries "<name>.unpack.tmp").
 * sm_pack_stats: what the context's last sm_pack_maps or sm_unpack_maps did (SM_E_ARG before the first).
 * What does NOT take a packed file: sm_load_map and a scene's actor files ("<path> is a packed map file; sm_unpack_maps makes a
 *   plain one": SM_E_ARG, for an actor file SM_E_UNSUPPORTED), and the calls that rewrite the files they are given -- sm_recall in
 *   SM_RECALL_MOVE, sm_warp_by_time and through it the loop closures: SM_E_UNSUPPORTED naming the file, before anything changes
 *   (a file the context's file index lets them skip unopened is not examined).  SM_RECALL_COUNT and SM_RECALL_COPY read packed
 *   files like plain ones.  Retirement writes plain files. */
typedef struct sm_pack_params {
    int32_t pos_step_log2;      /* -14..-6: the position step is 2^pos_step_log2 m      default -10 (0.977 mm) */
} sm_pack_params;
typedef struct sm_pack_stats_t {
    uint64_t records;           /* of all sources */
    uint64_t bytes_in;          /* the source files' sizes, plus 48 per record of the live model */
    uint64_t bytes_out;         /* the output files' sizes */
    uint32_t files;             /* written */
    uint32_t blocks;            /* of 256 records in the packed files (written by sm_pack_maps, read by sm_unpack_maps) */
    uint32_t raw_blocks;        /* ... of which RAW */
    uint32_t chunks;            /* of at most 2^20 records through the device */
    float read_ms;              /* host: reading the files */
    float copy_ms;              /* device: the chunks' copies in (and the decode of packed sources) */
    float unpack_ms;            /* ... of which the decode of packed sources (k_unpack) */
    float device_ms;            /* device: the encoder's kernels (sm_unpack_maps: 0, the decode is part of copy_ms) */
    float write_ms;             /* host: the copies back and writing the files */
    float total_ms;
} sm_pack_stats_t;
int sm_default_pack_params(sm_pack_params *p);               /* pure, no context */
int sm_pack_maps(sm_ctx *s, const sm_map_source *src, const sm_pack_params *p, const char *out_prefix);
int sm_unpack_maps(sm_ctx *s, const sm_map_source *src, const char *out_prefix);
int sm_pack_stats(sm_ctx *s, sm_pack_stats_t *out);

/* ---- locating one map set in another without a guess (DESIGN.md "4ab. Locating") ----
 * sm_register_maps needs a guess inside its basin (0.8 m, a few degrees).  sm_locate_maps finds that guess for two sets whose
 * worlds share their up axis and differ by ANY yaw, by offsets of up to thousands of cells and by a height: the vertical structure
 * of both sets is rasterised top-down (as sm_ground_maps rasterises), the SOURCE's occupied cells are correlated with the TARGET's
 * occupancy over every yaw of a table and every offset of a range, and the ground heights give the fourth unknown.  The result is
 * defined as an exact argmax of integer counts; tests/locate_ref.py restates every operation below and the GPU path is pinned to it
 * bit for bit.  pose16_out (column-major, source world -> target world) is meant to be passed as guess16 to sm_register_maps.
 *   Units and axes.  Q(mm) = (mm * 65536 + 500) / 1000 in integers, C = Q(cell_mm) (cell_mm 50..4000: C <= 2^18).  a = up >> 1 is the
 *     up axis, sgn = up & 1 ? -1 : +1, ua < va are the two horizontal axes.
 *   Record quantities.  sm_ground_maps' regular-record test, X[k] = floor(((double)p[k] - (double)o[k]) * 65536), ni[k], class c; cu =
 *     floor_div(X[ua], C), cv = floor_div(X[va], C), H = sgn * X[a]; o = origin for the target set, source_origin for the source set.
 *     A record that fails the test is LOOSE.  OUTSIDE: |H| >= 2^30; in the target cu outside [0, nu) or cv outside [0, nv); in the
 *     source |cu| > 4095 or |cv| > 4095.
 *   Kinds.  Structure-like: c has its bit in structure_mask and |ni[a]| <= max_up.  Ground-like: c has its bit in ground_mask and
 *     normal_sign * sgn * ni[a] >= min_up.  A record may be both (it then takes part in both rasters) or neither.  It is counted
 *     once: STRUCTURE if structure-like, else GROUND if ground-like, else OTHER.
 *   Target raster, over the window of nu x nv cells (each 1..4096) whose low corner is origin: n_t[cell] = the cell's structure-like
 *     records; occ0 = n_t >= min_records; occ = occ0 dilated by `dilate` cells (0..2, Chebyshev), clipped to the window; Zt[cell] =
 *     the minimum H of the cell's ground-like records.
 *   Source cells.  S = the cells with at least min_records structure-like records, in (cv, cu) order, n_s = |S|; more than
 *     max_source_cells: SM_E_CAPACITY.  G = the cells with a ground-like record, each with Zs = the minimum H.
 *   Rotation table.  n_fine = n_yaw * refine rows (n_yaw 1..1024, refine 1..16); row j = (c_j, s_j) = (llrint(cos(2 pi j / n_fine) *
 *     2^30), llrint(sin(2 pi j / n_fine) * 2^30)), computed on the host in double.  sm_locate_rotations returns the 2 * n_fine
 *     integers (c_0, s_0, c_1, ...).  Everything below uses the table's integers only.
 *   Rotated cell.  x = cu * C + C / 2, y = cv * C + C / 2; xr = (c * x - s * y + 2^29) >> 30, yr = (s * x + c * y + 2^29) >> 30 in
 *     int64 with arithmetic shifts (every product is below 2^61); ru = floor_div(xr, C), rv = floor_div(yr, C).
 *   score(j, du, dv) = the number of cells of S with (ru + du, rv + dv) inside the window and occ set there.
 *   Range.  R = (3 * max over S of max(|x|, |y|) / 2) / C + 2; du in [-R, nu - 1 + R], dv in [-R, nv - 1 + R].
 *   Coarse winner (k*, du*, dv*).  Over the rows j = k * refine, k in 0 .. n_yaw - 1, and every offset of the range: the largest score,
 *     of equal ones the smallest (k, dv, du).
 *   Refinement.  Over dj in -(refine - 1) .. refine - 1 with j = (k* * refine + dj) mod n_fine, and the nine offsets within one cell
 *     of (du*, dv*) (not cut to the range): the largest score, of equal ones the smallest (|dj|, dj, dv, du): (row, du, dv, score).
 *   Runner-up.  The largest coarse score over the candidates with circular |k - k*| > sep_yaw or max(|du - du*|, |dv - dv*|) >
 *     sep_cells; 0 without any.  sep_cells < 0: not searched, 0.
 *   Height.  The pairs are the cells of G whose rotated cell (row `row`) plus (du, dv) is a window cell with a Zt; d = Zt - Zs per
 *     pair, height_pairs = m = their number, dh = element (m - 1) / 2 of the sorted d; dh = 0 with m < min_ground.
 *   Status, the first that applies: SM_LOCATE_NO_TARGET (no occ cell), SM_LOCATE_NO_SOURCE (n_s = 0) -- for these two nothing is
 *     searched and every result field from `row` to `dh` is 0 --, SM_LOCATE_NONE (score * 256 < n_s * min_overlap_256),
 *     SM_LOCATE_AMBIGUOUS (runner_up * 256 > coarse_score * ambiguity_256), SM_LOCATE_OK.
 *   Pose.  For OK and AMBIGUOUS, in double, each entry rounded to float once: c = c_row * 2^-30, s = s_row * 2^-30, Cm = C * 2^-16,
 *     O = (double)origin, So = (double)source_origin; M[ua][ua] = c, M[ua][va] = -s, M[va][ua] = s, M[va][va] = c, M[a][a] = 1,
 *     M[ua][3] = (O[ua] + du * Cm) - (c * So[ua] - s * So[va]), M[va][3] = (O[va] + dv * Cm) - (s * So[ua] + c * So[va]), M[a][3] = (O[a] +
 *     sgn * dh * 2^-16) - So[a]: a point p of the source world goes to O + Rot(p - So) + (du Cm, dv Cm, sgn dh 2^-16).  Otherwise
 *     pose16_out is the identity; the call returns SM_OK for every status.
 *   Worked example (tests/locate_ref.py EXAMPLE): cell_mm 1000, up 3, 6 x 4 cells at the origin, min_records 1, dilate 0, n_yaw 4,
 *     refine 8, sep_yaw 0, sep_cells 1, min_ground 1.  Target occ at (1, 1), (2, 1), (4, 1), (5, 1); S = (0, 0), (1, 0).  k = 0 scores 2 at
 *     (du, dv) = (1, 1) and (4, 1), k = 2 scores 2 at (3, 2) and (6, 2), k = 1, 3 score 1: the coarse winner is (0, 1, 1), the smallest
 *     (k, dv, du).  dj = -1, 0, +1 all score 2 at (1, 1): dj = 0 stays, row 0.  The runner-up, (0, 1, 4), scores 2: 2 * 256 > 2 * 218,
 *     AMBIGUOUS.  Ground at H -16384, -32768 under (1, 1), (2, 1) and -81920, -65536 under S: d = 65536, 32768, dh = 32768.
 * The result is a function of the two multisets of (id, record) pairs alone: chunking, the split into files, plain or packed
 *   files and the model's share change no bit.  The device finds the coarse winner and the runner-up by a branch and bound over a
 *   max-pyramid of occ; SM_LOCATE_EXHAUSTIVE=1 (read per call) scores every coarse candidate instead -- the same result -- and is
 *   refused with SM_E_ARG above 2^36 lookups (n_yaw * range * n_s).  max_nodes only limits the nodes scored per round.
 * Side effects: none on files, model, tick, stored poses, keyframes or tracker state.  Synchronous.
 * Errors.  SM_E_ARG: NULLs; a parameter out of its range; a non-finite origin or source_origin; the header and set checks of
 *   sm_register_maps for both sets, a path that is in both; a call between sm_stage_conflict and sm_stage_cull; sm_locate_stats
 *   before any call.  SM_E_CAPACITY: more than max_source_cells cells in S.  SM_E_UNSUPPORTED: a sharded or rig context. */
enum { SM_LOCATE_OK = 0, SM_LOCATE_AMBIGUOUS = 1, SM_LOCATE_NONE = 2, SM_LOCATE_NO_TARGET = 3, SM_LOCATE_NO_SOURCE = 4 };
enum { SM_LOCATE_STRUCTURE = 0, SM_LOCATE_GROUND = 1, SM_LOCATE_OTHER = 2, SM_LOCATE_OUTSIDE = 3, SM_LOCATE_LOOSE = 4 };
typedef struct sm_locate_params {
    int32_t  cell_mm;            /* 50..4000                                                         default 500 */
    int32_t  up;                 /* 0..5: +x -x +y -y +z -z is up                                    default 3 */
    float    origin[3];          /* the target window's low corner, height zero on the up axis       default 0 0 0 */
    float    source_origin[3];   /* the point of the source world its cells are counted from         default 0 0 0 */
    int32_t  nu, nv;             /* the window's cells, 1..4096 each                                 default 256 256 */
    uint32_t structure_mask[8];  /* classes that may be structure                                    default all */
    int32_t  max_up;             /* 0..16384: |ni[a]| of a structure-like record at most             default 8192 (30 degrees) */
    uint32_t ground_mask[8];     /* classes that may be ground                                       default all */
    int32_t  min_up;             /* 0..16384, as sm_ground_params'                                   default 11585 */
    int32_t  normal_sign;        /* +1 / -1, as sm_ground_params'                                    default -1 */
    uint32_t min_records;        /* >= 1: structure-like records that make a cell occupied           default 2 */
    int32_t  dilate;             /* 0..2 cells                                                       default 1 */
    int32_t  n_yaw;              /* 1..1024 coarse rows                                              default 360 */
    int32_t  refine;             /* 1..16 fine rows per coarse row                                   default 8 */
    int32_t  sep_yaw;            /* >= 0: coarse rows the runner-up keeps away                       default 10 */
    int32_t  sep_cells;          /* cells the runner-up keeps away; < 0: no runner-up                default 8 */
    int32_t  min_ground;         /* >= 0: pairs the height needs                                     default 16 */
    int32_t  min_overlap_256;    /* 0..256                                                           default 128 */
    int32_t  ambiguity_256;      /* 0..65536                                                         default 218 */
    uint32_t max_source_cells;   /* 1..2^20                                                          default 2^18 */
    uint32_t max_nodes;          /* 4..2^24: nodes scored per round of the search                    default 2^20 */
} sm_locate_params;
typedef struct sm_locate_info {
    int32_t  status;             /* SM_LOCATE_* */
    int32_t  row, du, dv;        /* the refined winner: fine row, offsets in cells */
    uint32_t score;
    int32_t  coarse_k, coarse_du, coarse_dv;
    uint32_t coarse_score;
    uint32_t runner_up;
    uint32_t n_s;                /* cells of S */
    uint32_t target_cells;       /* occ cells */
    uint32_t height_pairs;
    int32_t  dh;                 /* 2^-16 m */
    uint64_t source_counts[5];   /* records by SM_LOCATE_STRUCTURE .. SM_LOCATE_LOOSE */
    uint64_t target_counts[5];
} sm_locate_info;
typedef struct sm_locate_stats_t {
    uint64_t source_records, target_records;
    uint64_t nodes;              /* inner nodes whose bound was computed (both searches) */
    uint64_t leaves;             /* coarse candidates scored (both searches) */
    uint32_t chunks, launches;
    uint32_t rounds;             /* rounds of the two searches */
    uint32_t levels;             /* pyramid levels above occ */
    uint32_t exhaustive;         /* 1: SM_LOCATE_EXHAUSTIVE=1 */
    uint32_t range;              /* R */
    float read_ms;               /* host: reading the files */
    float raster_ms;             /* device: both sets' rasters, the compaction, the rotated lists */
    float pyramid_ms;            /* device: occ, dilation, the pyramid */
    float search_ms;             /* host clock: both searches, refinement and height */
    float total_ms;
} sm_locate_stats_t;
int sm_default_locate_params(sm_locate_params *p);           /* pure, no context */
int sm_locate_rotations(const sm_locate_params *p, int32_t *table);   /* pure: 2 * n_yaw * refine integers */
int sm_locate_maps(sm_ctx *s, const sm_map_source *source, const sm_map_source *target, const sm_locate_params *p,
                   float *pose16_out, sm_locate_info *info);
int sm_locate_stats(sm_ctx *s, sm_locate_stats_t *out);      /* SM_E_ARG before the first call */

/* ---- per-pass entry points (GlobalModel / IndexMap methods), synchronous ---- */
/* Upload RGB / metric depth / semantic textures directly (bypasses p0). */
int sm_set_frame(sm_ctx *s, const uint8_t *rgb, const float *depth_metric,
                 const uint8_t *semantic);
int sm_set_tick(sm_ctx *s, int32_t tick);
/* GlobalModel::processConflict + updateConflict (src/GlobalModel.cpp:396-515): conflict test,
 * in-place confidence decrement marks; sets conflict_count. */
int sm_stage_conflict(sm_ctx *s, const float *pose16, float min_depth, float max_depth,
                      float fuse_thresh, int is_clean);
/* GlobalModel::backMapping + buildModelMap (src/GlobalModel.cpp:517-579,639-681): stable
 * compaction of surfels with conf > 0; sets count = offset. */
int sm_stage_cull(sm_ctx *s);
/* IndexMap::predictIndices (src/IndexMap.cpp:138-198) */
int sm_stage_splat(sm_ctx *s, const float *pose16, int32_t time, float depth_cutoff,
                   int32_t time_delta);
/* GlobalModel::dataAssociate + updateFuse + backMapping + concatenate + buildModelMap
 * (src/GlobalModel.cpp:246-394,581-637) */
int sm_stage_associate_fuse(sm_ctx *s, const float *pose16, int32_t time, float depth_min,
                            float depth_max);

/* Stopwatch::getTimings() equivalent (src/Utils/Stopwatch.h:85-88) -- needs enable_timing */
int sm_stage_timings(sm_ctx *s, sm_timings *out);
/* Copy the newest `n` (<= SM_FRAME_LOG_LEN) frame-log entries, oldest first; returns the
 * number written in *written.  Synchronises the stream. */
int sm_read_frame_log(sm_ctx *s, sm_frame_log *out, uint32_t n, uint32_t *written);

/* ---- device-memory helpers for callers that stage frames in HBM ---- */
void *sm_device_alloc(sm_ctx *s, size_t bytes);
int sm_device_free(sm_ctx *s, void *p);
int sm_device_upload(sm_ctx *s, void *dst_device, const void *src_host, size_t bytes);
/* Multi-GPU "all-gather into a single GlobalModel" (BASELINE configs[4]): export the model as
 * AoS (12 f32 / surfel) into a device staging buffer owned by the ctx (valid until the next
 * export/download on this ctx) so that RCCL can gather it without a host round trip ... */
int sm_export_model_device(sm_ctx *s, void **d_aos, uint32_t *n);
/* ... and append `n` AoS surfels that already live in this GPU's memory to the model
 * (GlobalModel::concatenate's glCopyBufferSubData, src/GlobalModel.cpp:624-629). */
int sm_append_model_aos_device(sm_ctx *s, const float *d_src12, uint32_t n);
int sm_device_download(sm_ctx *s, void *dst_host, const void *src_device, size_t bytes);

/* diagnostic: how many frames so far took the rare path of the two-launch frame (their association waited, inside its launch, for
 * the publisher and the cap repair: conflicts > W*H, or the "id 0" surfel died).  Synchronises. */
int sm_debug_slow_frames(sm_ctx *s, uint32_t *n);
/* diagnostic: squeezes between the two launches of a frame so far (DESIGN.md 4 "Tail squeeze") -- `tail`: those that started at a
 * dense tile and left dead slots below it, `full`: those that started at the first dead slot.  Synchronises. */
int sm_debug_squeezes(sm_ctx *s, uint32_t *tail, uint32_t *full);
/* Diagnostic: processes that hold compute queues on this context's GPU according to the KFD driver's tables (>= 1: this
 * one included), or -1 if /sys/class/kfd is not readable.  The in-place compaction switches to its ticket-ordered form
 * (no co-residency assumption) whenever the value is > 1 or a second context of this process shares the GPU; the value is
 * re-read at most once per second.  SM_COMPACT_TICKETS=1 / 0 overrides the detection. */
int sm_gpu_process_count(sm_ctx *s);

/* ---- ONE camera stream sharded over `world` GPUs (BASELINE configs[3]): no host or Python between the stages of a
 * frame.  Every rank addresses surfels by the slot number the single-GPU run uses and stores only the segments it owns (owner
 * of a frame's new surfels = fusing-frame index % world); the key map (min), the fused-pixel mask + 3 counters (sum) and -- when
 * the model has more slots than pixels and the conflict cap is on -- the conflict masks (sum) are all-reduced on the context's
 * own stream through the installed collective -- RCCL's ncclAllReduce, bound at run time by sm_shard_rccl_init, or any callback
 * with the same meaning (tests: several contexts on one GPU).  All ranks hold the same counters (sm_get_counts) after every
 * frame; results are bit-identical to the single-GPU path, the W*H conflict cap included. */
enum { SM_COLL_SUM = 0, SM_COLL_MIN = 1, SM_COLL_GATHER = 2 };
/* SUM / MIN: all-reduce `count` unsigned 64-bit words from `send` to `recv` (may be equal; device memory of this context) over
 * the ranks.  GATHER: all-gather -- every rank contributes `count` words at `send`, `recv` receives world * count words, rank q's
 * at recv + q * count (in place when send == recv + rank * count, as ncclAllGather).  Enqueued on `hip_stream`; returns 0 on
 * success */
typedef int (*sm_collective_fn)(void *user, const void *send, void *recv, size_t count, int op, void *hip_stream);
/* on a new context (no frame yet); allocates the second surfel set the sharded compaction stages through */
int sm_shard_stream_configure(sm_ctx *s, int rank, int world);
int sm_shard_set_collective(sm_ctx *s, sm_collective_fn fn, void *user);
/* RCCL bootstrap: rank 0 makes the 128-byte id, the host program hands it to every rank (MPI / torch.distributed /
 * a file), each rank calls sm_shard_rccl_init -- a collective call (ncclCommInitRank) */
int sm_shard_rccl_unique_id(void *out128);
int sm_shard_rccl_init(sm_ctx *s, const void *id128);
int sm_shard_rccl_finalize(sm_ctx *s);
/* ranks of the context's RCCL communicator as RCCL itself reports them (ncclCommCount), or a negative SM_E_* */
int sm_shard_rccl_nranks(sm_ctx *s);
/* SurfelMapping::processFrame (src/SurfelMapping.cpp:115-251) on every rank with the same arguments; the _device form
 * takes device pointers and only enqueues (sm_sync to wait).  A frame is a sequence of collectives every rank must enter: an
 * error return from one rank (a failed launch or a failed RCCL call -- nothing a frame's data can cause) leaves the others inside
 * a collective and the communicator undefined; treat it as fatal for the stream and destroy the contexts on all ranks.  (The
 * rig's exchanges, which do run fallible local steps between collectives, carry a status word instead: sm_rig_consolidate.)
 * Null images and the lifetime of the _device form's buffers: as at sm_process_frame / sm_process_frame_device. */
int sm_shard_frame_device(sm_ctx *s, const uint8_t *d_rgb, const uint16_t *d_depth_mm, const uint8_t *d_semantic, const float *pose16);
int sm_shard_frame(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16);
/* squeeze the dead slots out now (collective; frames do it every compact_period-th time by themselves) */
int sm_shard_compact(sm_ctx *s);
/* collective: compacts, then exposes this rank's part of the union as `*count` x 12 floats in device memory with zeros
 * in the other ranks' slots -- the integer (u32) sum over the ranks is the single GlobalModel in the reference's order */
int sm_shard_export_dense_device(sm_ctx *s, const float **d_out12, uint32_t *count);

/* ---- BASELINE configs[4]: a rig of `world` cameras, one context per rank (GPU), consolidated into a single GlobalModel.
 * Frames use sm_process_frame[_device] (no collective).  sm_rig_consolidate is collective: every rank passes its camera's
 * latest view; the union of the slices in rank order is cleaned against every view in rank order with
 * SurfelMapping::cleanPoints (src/SurfelMapping.cpp:496-532), each rank cleaning its own slice, and the cleaned slices are
 * appended in rank order to `global` (another context on the same GPU) on every rank.  The collective is the one installed
 * with sm_shard_rccl_init / sm_shard_set_collective after sm_rig_configure (world 1: none needed).
 * view_conflicts[world] (may be null): conflicts that took effect per view over all slices.  The reference's conflict cap -- at
 * most W*H conflicts per view, in the surfel order of the union (src/GlobalModel.cpp:54-57) -- is applied exactly: between a
 * view's conflict test and its cull the ranks exchange their conflict counts and every slice applies what the lower ranks
 * left of the W*H.  Views, counts and slices cross the ranks as all-gathers; every exchange carries a status word, so a rank
 * whose local step fails makes ALL ranks return an error together (nobody is left waiting inside a collective). */
int sm_rig_configure(sm_ctx *s, int rank, int world);
int sm_rig_consolidate(sm_ctx *s, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16, sm_ctx *global,
                       uint32_t *view_conflicts, uint32_t *total);
/* The single GlobalModel DURING a run, one step (collective; call it every K frames): every rank's surfels created since its
 * previous step are all-gathered -- per-GPU new-surfel lists, SURVEY.md 8e -- and appended to `global` in rank order
 * (GlobalModel::concatenate), then `global` is cleaned against every camera's latest view in rank order (SurfelMapping::cleanPoints)
 * -- the same on every rank, on `global`'s stream.  The camera's own model is not changed.  new_surfels / global_count (may be
 * null): surfels exchanged in this step, surfels in `global` after it. */
int sm_rig_consolidate_step(sm_ctx *s, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16, sm_ctx *global,
                            uint32_t *new_surfels, uint32_t *global_count);

#ifdef __cplusplus
}
#endif
#endif /* SM_C_API_H */
