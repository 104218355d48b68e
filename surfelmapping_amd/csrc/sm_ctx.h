// sm_ctx.h -- private to the core's sources, never installed: the context (struct sm_ctx), the owners of its HIP resources,
// the error channel, the constants, and the helpers that more than one source calls.  It includes no kernels: every kernel
// is defined and launched in exactly one source, and another source reaches it through a host helper declared below.
//
//   sm_api.hip       context lifecycle, the frame pipeline, the per-pass stage API, the sharded stream
//   sm_model_io.hip  model download / upload, map files, index map, raw cloud, depth, sm_render_image, device buffers
//   sm_view.hip      the model view (sm_render_model*)
//   sm_track.hip     tracking (sm_track_*)
//   sm_rccl.hip      the RCCL binding (sm_shard_rccl_*)
//   sm_rig.hip       rig consolidation (sm_rig_*)
//   sm_retire.hip    retirement (sm_retire*, sm_set_auto_retire)
//   sm_render_maps.hip  views of a map set (sm_render_*_maps): map files streamed through the renderers; the staging's allocation and intake
//   sm_recall.hip    paging in (sm_recall*, sm_set_auto_recall): records of map files near the camera back into the model
//   sm_warp.hip      closing loops (sm_warp_by_time, sm_loop_spread): the model and map files warped by surfel time
//   sm_search.hip    pose search before the tracker (sm_score_poses_window, sm_search_pose)
//   sm_lidar.hip     lidar sweeps (sm_lidar_*): beams against the live model and against streamed map files
//   sm_scene.hip     scenes (sm_render_image_scene, sm_lidar_sweep_scene): actor files resident for a call, drawn under a pose per view by both of the above
//   sm_place.hip     place recognition (sm_fern_*, sm_search_pose_at, sm_close_loop_at): fern codes, the keyframe database, the match
//   sm_stereo.hip    stereo depth (sm_stereo_*): census, matching costs, path costs, winner and depth of a rectified pair
//   sm_lidar_depth.hip  lidar depth (sm_lidar_depth*): a scan z-buffered into the camera and completed to a dense depth image
//   sm_fill.hip      hole filling (sm_fill_*, sm_render_image_ex's and sm_render_image_maps_ex's stage): depth of a view, push-pull completion
//   sm_blend.hip     blended views (sm_render_image_blend, sm_render_image_maps_blend): the visible layer's accumulation and normalisation, a stage of both render paths
//   sm_simplify.hip  simplification (sm_simplify, sm_simplify_maps): the model or a map set merged per voxel cell, two passes over the records
//   sm_register.hip  registration (sm_register_*): the rigid transform from one map set to another, voxel-cell ICP, one pass over each set
//   sm_compare.hip   change detection (sm_compare_*): every record of one map set labelled against the voxel tables of another, one pass over each set
//   sm_locate.hip    locating (sm_locate_*): where one map set lies in another without a guess, top-down occupancy correlated by branch and bound
//   sm_voxel.hip     what simplification, registration and change detection share (sm_voxel.h): the grid, the slot count and the tally's verdict; the lookup table; the ranked output
//   sm_pack.hip      packed map files (sm_pack_maps, sm_unpack_maps): the encoder, and the decoder the chunk stream runs on a packed file's chunks
// and, beside it, for everything that touches a map file: sm_mapfile.h (the format: checked open, writer, chunk plan; host only),
// sm_map_set.h (a listed set of files: the file index, the two openings, a rewrite's per-file record and temporary; host only) and
// sm_map_stream.h (the double-buffered chunk stream of sm_render_maps.hip, sm_lidar.hip, sm_recall.hip, sm_warp.hip, sm_simplify.hip, sm_register.hip and sm_compare.hip).  The staging
// they stream through (MapStaging) and the file index (FileIndex) are the context's, no feature's.  For the occupied slots and the
// compaction schedule: sm_slots.h (SlotSchedule; host only); for the arithmetic of rigid poses in double: sm_pose.h (host only,
// included by sm_track.hip and sm_warp.hip).  What alternates between consecutive frames is FrameSet, below.
#pragma once

#include "../../include/sm_c_api.h"
#include "sm_device.h"
#include "sm_map_set.h"
#include "sm_slots.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace sm { struct TrackState; struct TrackRgbState; struct RegState; struct RenderParams; struct ViewParams; struct ViewShade; struct RecallChunk; struct WarpChunk; struct MapsSoA; struct LidarGrid; struct LidarPose; }

// Hidden: libsurfelmapping_hip.so exports the C ABI and the kernels' host stubs, nothing of this namespace.  Its functions are
// defined qualified (sm_impl::name) so that the definitions keep the visibility.
namespace sm_impl __attribute__((visibility("hidden"))) {

using namespace sm;

inline thread_local std::string g_err;

inline void set_err(const char *what, hipError_t e, const char *file, int line)
{
    char buf[512];
    snprintf(buf, sizeof buf, "%s: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    g_err = buf;
}

#define HIPCK(expr)                                              \
    do {                                                         \
        hipError_t e_ = (expr);                                  \
        if (e_ != hipSuccess) {                                  \
            set_err(#expr, e_, __FILE__, __LINE__);              \
            return SM_E_HIP;                                     \
        }                                                        \
    } while (0)

// Owner of one HIP handle (device or pinned host memory, an event, a stream): move-only, released by its destructor on the
// current device (sm_destroy makes the context's device current).  It reads as the raw handle, so kernel arguments and argument
// structs take it unchanged.  put() releases what it holds and hands out the slot for a create call, filled only on success.
template <typename H, auto Release>
class Own {
public:
    Own() = default;
    Own(Own &&o) noexcept : h_(o.release()) {}
    Own &operator=(Own o) noexcept { std::swap(h_, o.h_); return *this; }
    ~Own() { if (h_) (void)Release(h_); }
    operator H() const { return h_; }
    H operator->() const { return h_; }
    H get() const { return h_; }
    H *put() { *this = Own(); return &h_; }
    H release() { H h = h_; h_ = nullptr; return h; }
private:
    H h_ = nullptr;
};
template <typename T> using Dev = Own<T *, hipFree>;
template <typename T> using Host = Own<T *, hipHostFree>;
using Event = Own<hipEvent_t, hipEventDestroy>;
using Stream = Own<hipStream_t, hipStreamDestroy>;

// the buffers behind one SurfelSet (Model is passed to kernels by value and stays a set of views)
struct SetBufs {
    Dev<float4> pos_conf, norm_rad;
    Dev<uint32_t> color;
    Dev<float> init_time, time;
    SurfelSet view() const { return {pos_conf, norm_rad, color, init_time, time}; }
};
constexpr int EV_RING = 256;
constexpr int N_EV = 9;           // start, prep, conflict, scan_cull, compact, associate, scan_new, append, + calibration
constexpr int MAX_GRID = 2048;   // 256 CUs x 8 workgroups
constexpr int COMPACT_GRID = 1024;  // k_compact: 256 CUs x 4 workgroups, must be fully co-resident (in-place hand-off)

// tracking (sm_track.hip, sm_k_track.h): scratch allocated by the first call, the last two processed poses
struct Tracker {
    Dev<uint16_t> d_depth;
    Dev<float4> d_v, d_n;
    Dev<uint64_t> d_key;
    Dev<int32_t> d_pred;
    Dev<double> d_part;
    Dev<TrackState> d_state;
    Host<TrackState> h_state;
    Dev<uint32_t> d_anchor;            // sm_track_frame_old: the newest time in the windowed prediction (order-preserving code, 0 = none)
    float hist[2][16];                 // [0] the last processed pose (T_prev), [1] the one before (T_prev2)
    int n_hist = 0;                    // poses processed so far (capped at 2)
    bool timed = false;                // SM_TRACK_TIMING=1 at the last call: events around every kernel
    int ev_iters = 0;                  // iterations the events of the last timed call cover
    std::vector<Event> ev;
    // the colour term (sm_track_frame_rgb): scratch allocated by its first call
    Dev<uint8_t> d_rgb;
    Dev<float> d_pyr;                  // the luminance pyramid, level after level
    Dev<float4> d_plane;               // the prediction as (surfel centre, luminance) per pixel
    Dev<double> d_part_rgb;
    Dev<TrackRgbState> d_rstate;
    Host<TrackRgbState> h_rstate;
    Dev<uint32_t> d_census;            // sm_old_in_view: the count (allocated by its first call)
    Event ev_census[2];                // SM_TRACK_TIMING=1: around k_loop_census
    bool census_timed = false;
    std::vector<int> ev_kind;          // of the last timed rgb call: what the interval after event 2 + k covers (kind | level << 4)
    // every processed frame's pose (begin_frame): the constant-velocity history of sm_track_frame
    void note_pose(const float *pose)
    {
        memcpy(hist[1], hist[0], 64);
        memcpy(hist[0], pose, 64);
        n_hist = std::min(n_hist + 1, 2);
    }
};

// model view (sm_view.hip): where the last render left its overflow-list length in the export scratch, and the diagnostic
// timing events (SM_RENDER_MODEL_TIMING=1)
struct ModelView {
    size_t ovf_off = 0;
    bool ovf_valid = false;
    bool timed = false;
    Event ev[4];
    // every user of the export scratch (ensure_export) may overwrite the overflow count
    void scratch_reused() { ovf_valid = false; }
};

// retirement (sm_retire.hip, sm_k_retire.h): scratch allocated by the first call, the periodic policy and its tally
struct Retire {
    Dev<uint64_t> d_mask;              // 1 bit per slot: retired by the last mark
    Dev<uint32_t> d_tile_ret, d_tile_base, d_total;   // retired per tile, their exclusive prefix, (total, slots marked)
    int32_t every = 0;                 // sm_set_auto_retire: 0 = off
    sm_retire_params params{};
    std::string prefix;
    Host<float> h_stage;               // pinned: one chunk of records on its way into a map file
    uint32_t files = 0;                // map files written so far
    uint64_t surfels = 0;              // ... and the surfels in them
    int32_t last_tick = 0;             // tick at the last retirement that wrote a file (the next file's startId)
    bool timed = false, stats_valid = false;   // SM_RETIRE_TIMING=1: events around every step of the last call
    Event ev[8];
};

// The staging every stream of map-file chunks goes through (streamed renderers, lidar, recall, warp), allocated whole by the first
// call that reads a file (maps_ensure_staging).  Chunk c of a pass goes through buffer c & 1 (MapStream, sm_map_stream.h): read into
// h_rec, copied on `copy` into d_rec; the renderers and the lidar unpack it into the one set of SoA planes (maps_intake).
struct MapStaging {
    static constexpr uint32_t CHUNK = 1u << 20;          // records per chunk (48 MiB), the chunk sm_retire writes files in
    Stream copy;                       // first: what follows is used on it
    Host<float4> h_rec[2];             // pinned
    Dev<float4> d_rec[2];
    Event ev_copy0[2], ev_copied[2];   // on `copy`: around the chunk's copy
    Event ev_k0[2], ev_k1[2];          // on the context's stream: around the chunk's kernels
    Dev<float4> d_pos_conf, d_norm_rad, d_box;
    Dev<uint32_t> d_color;
    Dev<float> d_time;
    // The packed pair, allocated whole by the first chunk of a packed file (maps_ensure_packed): the chunk's directory slice
    // through h_dir into d_dir, its payload through h_rec into d_pk, and k_unpack (sm_k_pack.h) decodes it into d_rec on the
    // context's stream before ev_k0, between ev_u0 and ev_u1 -- so no consumer of d_rec knows which format a file has.
    Host<uint8_t> h_dir[2];            // pinned, 32 bytes per block of the chunk
    Dev<uint8_t> d_dir[2], d_pk[2];    // (d_pk: a chunk of RAW blocks needs as much as d_rec)
    Event ev_u0[2], ev_u1[2];          // (ev_u1[1] is set last: the pair is whole or absent)
};

// views of a map set (sm_render_maps.hip, sm_k_render_maps.h): the per-view block and the last call's tally
struct RenderMaps {
    Dev<uint8_t> d_par;                // per-view parameters | shading | skipped counters | hit flags
    size_t par_bytes = 0;
    Event ev[2];                       // around the live model's kernels
    sm_maps_stats stats{};
    bool stats_valid = false;
};

// paging in (sm_recall.hip, sm_k_recall.h): scratch of the first call that reads a file, the last call's tally, the policy and its tally
struct Recall {
    Dev<uint64_t> d_mask;              // 4 words per block of 256 records: near
    Dev<uint32_t> d_blk_cnt, d_blk_base, d_run;   // near per block, their exclusive prefix, the call's running total
    Dev<float4> d_box;                 // recall_box_of's own block boxes (the retirement policy has no stream staging)
    Dev<RecallChunk> d_chunk;          // [2]: the scan's tally of the chunk in buffer c & 1
    Host<RecallChunk> h_chunk;         // pinned, [2]
    sm_recall_stats_t stats{};
    bool stats_valid = false;
    float radius = 0.0f;               // sm_set_auto_recall: <= 0 = off
    uint32_t rounds = 0;               // recalls the policy has made
    uint64_t surfels = 0;              // ... and the surfels they brought back
};

// the warp by surfel time (sm_warp.hip, sm_k_warp.h): scratch allocated by the first call, the last call's tally
struct Warp {
    Dev<float4> d_corr;                // the table, 3 float4 per row
    size_t corr_rows = 0;
    Dev<float4> d_box;                 // per block of 256 records: (min xyz | largest time), (max xyz | 0)
    Dev<uint32_t> d_sel;               // selected rows: [0], [1] of the chunk in buffer c & 1, [2] of the live model
    Dev<WarpChunk> d_chunk;            // [2]
    Host<WarpChunk> h_chunk;           // pinned, [2]
    Event ev[2];                       // around the live model's kernel
    sm_warp_stats_t stats{};
    bool stats_valid = false;
};

// pose search (sm_search.hip, sm_k_search.h): scratch allocated by the first call, sized for the frame and grown with the
// candidate list
struct Search {
    Dev<uint8_t> d_rgb;                // the frame's colour image, row-major
    Dev<float4> d_samp;                // the packed grid points, two float4 each: (v, Y_f), (n, 0)
    Dev<float4> d_plane;               // the prediction, two float4 per pixel: (p_m, Y_m), (n_m, valid)
    Dev<uint32_t> d_nsamp;             // how many grid points were packed
    Dev<float> d_cand;                 // 12 floats per candidate: columns 0..3 of its pose, rows 0..2
    Dev<uint32_t> d_scores;
    size_t cand_cap = 0;
    Event ev[2];                       // around the scoring kernels
};

// lidar sweeps (sm_lidar.hip, sm_k_lidar.h): the last sensor's tables on the device, the per-sweep poses, the device tally and
// the last call's.  Keys and output planes live in the export scratch.
struct Lidar {
    Dev<float> d_dir, d_el;            // the direction table (n_el * n_az * 3) and the elevations in radians
    std::vector<float> key;            // what the tables on the device were made of: n_az, n_el, az0, step, the elevations
    Dev<uint8_t> d_poses;              // LidarPose per sweep
    size_t pose_cap = 0;
    Dev<uint8_t> d_tally;              // LidarTally
    Event ev[2];                       // around the live model's kernels
    sm_lidar_stats_t stats{};
    bool stats_valid = false;
};

// place recognition (sm_place.hip, sm_k_place.h): the fern table, the staging of a frame to encode, the keyframe database (codes
// and times on the device, poses and times on the host) and the match's scratch.  on = false: none of it exists.
struct Place {
    bool on = false;
    sm_fern_params p{};
    Dev<uint4> d_table;                // per fern: x | y << 16, tr | tg << 16, tb | td << 16, 0
    Dev<uint8_t> d_rgb;                // sm_fern_encode's copies of the host images
    Dev<uint16_t> d_depth;
    Dev<uint32_t> d_code;              // the code of the last encode, and the query of a match
    Dev<uint32_t> d_codes;             // keyframe-major, n_ferns / 8 words each
    Dev<int32_t> d_times;
    size_t cap = 0;                    // keyframes the two hold
    std::vector<float> poses;          // 16 per keyframe
    std::vector<int32_t> times;
    Dev<unsigned long long> d_keys;    // [2]: the match's answers
    Dev<uint32_t> d_dis;               // dis_all, `cap` entries, allocated by the first match that asks
    size_t dis_cap = 0;
    uint32_t count() const { return (uint32_t)times.size(); }
    bool timed = false;                // SM_PLACE_TIMING=1 at sm_set_ferns: events around the two kernels (tools/place_probe.py)
    Event ev[4];                       // before / after k_fern_encode, before / after k_fern_match, of the last launches
    // the policy of sm_set_auto_place and its tally
    bool auto_on = false;
    sm_auto_place_params ap{};
    int64_t rest_until = 0;            // no attempt before this tick
    sm_auto_place_stats_t stats{};
};

// stereo depth (sm_stereo.hip, sm_k_stereo.h): everything sm_set_stereo allocates.  on = false: none of it exists.
struct Stereo {
    static constexpr int N_EV = 12;    // before the census, after it, after the costs, after each of up to 8 directions, after the selection
    bool on = false;
    sm_stereo_params p{};
    Dev<uint8_t> d_left, d_right;      // sm_stereo_depth's copies of the host images
    Dev<uint64_t> d_census[2];         // left, right
    Dev<uint8_t> d_cost;               // the matching costs, [y][x][d]
    Dev<uint16_t> d_vol;               // S, [y][x][d]
    Dev<uint16_t> d_depth, d_disp;     // the outputs of a call that names none of its own
    bool timed = false;                // SM_STEREO_TIMING=1 at sm_set_stereo: events around every kernel (tools/stereo_probe.py)
    Event ev[N_EV];
};

// hole filling (sm_fill.hip, sm_k_fill.h): the pyramid scratch beside d_export (which the render path is using), grown on demand;
// sm_fill_image's device copies of the host images; the last call's tally, folded from per-tile partial sums once its kernels are done
struct Fill {
    Dev<uint8_t> d_scratch;            // level-0 validity | records of levels 1.. | level-5 counts | the two kernels' per-tile tallies
    size_t bytes = 0;
    Dev<uint8_t> d_img;                // bgr | sem | depth_mm of sm_fill_image's batch
    size_t img_bytes = 0;
    Event ev[2];                       // around the stage
    sm_fill_stats_t stats{};
    bool stats_valid = false;
    bool pending = false;              // a stage is enqueued whose tallies and time are not in `stats` yet
    size_t off_pull = 0, off_push = 0; // ... and where its tallies lie in the scratch
    size_t n_pull = 0, n_push = 0;
};

// lidar depth (sm_lidar_depth.hip, sm_k_lidar_depth.h): everything sm_set_lidar_depth allocates, and the last call's tally, folded
// from the kernels' per-block parts once they are done.  on = false: none of it exists.
struct LidarDepth {
    static constexpr int MAX_LAUNCHES = 12;    // of the debug form, every step a launch; the default form makes four
    static constexpr int N_EV = MAX_LAUNCHES + 1;      // before the first launch and after each
    bool on = false;
    sm_lidar_depth_params p{};
    Dev<uint64_t> d_key;               // W * H, KEY_EMPTY between calls
    Dev<uint16_t> d_v, d_rowmax;       // the v plane after FILL_SMALL; FILL_LARGE's row pass
    Dev<uint16_t> d_tmp;               // the debug form's second v plane
    Dev<uint32_t> d_top;               // [W]
    Dev<uint32_t> d_part;              // the tallies: project's blocks | finish's tiles (uint4) | chain's tiles (uint2); the debug form:
                                       // project's blocks | eight words
    size_t part_project = 0, tiles = 0;
    Dev<uint16_t> d_depth, d_sparse;   // sm_lidar_depth's outputs on the device
    Dev<int32_t> d_index;
    Dev<float4> d_points;              // ... and its copy of the scan, grown on demand
    size_t points_cap = 0;
    bool timed = false;                // SM_LIDAR_DEPTH_TIMING=1 at sm_set_lidar_depth: an event after every launch (tools/lidar_depth_probe.py)
    bool unfused = false;              // SM_LIDAR_DEPTH_UNFUSED=1 at sm_set_lidar_depth: the debug form
    Event ev[N_EV];
    sm_lidar_depth_stats_t stats{};
    bool stats_valid = false;
    bool pending = false;              // a call is enqueued whose tallies and times are not in `stats` yet
    uint32_t blocks_project = 0;       // ... and how many blocks its projection had
    int n_slots = 0;                   // ... how many entries of launch_ms it has,
    bool ran[MAX_LAUNCHES] = {};       // ... and which of them it launched
};

// blended views (sm_blend.hip, sm_k_blend.h): the accumulators beside d_export, owned like the fill scratch and grown on demand;
// the last blended call's tally, folded from the device's once a batch's kernels are done
struct Blend {
    Dev<unsigned long long> d_scratch; // the tally (contributions, drawn, changed; 256 bytes) | SW, SB, SG, SR per pixel of a batch
    size_t bytes = 0;
    Event ev[2];                       // around what the stage runs outside a chunk stream
    sm_blend_stats_t stats{};
    bool stats_valid = false;
};

// The scratch of a pass that keeps some records of every chunk and writes them, in order, to one output (sm_voxel.h's
// RankedOutput: simplification's second pass, change detection's query), allocated by the first such call.  Calls on one context
// never overlap, so they share it.
struct RankScratch {
    static constexpr uint32_t BLOCKS = (1u << 20) / 256u;   // the blocks of 256 records of a chunk: one plane
    Dev<uint32_t> d_blk_cnt, d_blk_base;   // two planes: kept records per block of 256 records of a chunk, their rank in the output
    Dev<uint2> d_info;                 // [2]: (first rank, kept records) of the chunk in buffer c & 1
    Host<uint2> h_info;                // pinned, [2]
    Dev<float4> d_out[2];              // the kept records of a chunk (sm_simplify: [0] holds the whole output)
    size_t out_cap[2] = {0, 0};        // records
};

// What every map-set analysis call keeps on its context (sm_set_call.h defines the members): the device tally of `words` words,
// its pinned mirror and N events, made whole or not at all by the context's first such call.
template <int N>
struct CallScratch {
    static constexpr int N_EV = N;
    Dev<uint32_t> d_tally;             // (set last: it marks the scratch complete)
    Host<uint32_t> h_tally;            // pinned
    size_t words = 0;
    Event ev[N];
    int ensure(size_t tally_words);
    int clear(hipStream_t stream) const;             // the memset of the whole tally
    int read(sm_ctx *s, size_t n = 0) const;         // the tally's first n words (0: all) at h(), once the context's stream is idle
    const uint32_t *h() const { return h_tally.get(); }
};
// The labels of a labelled pass (sm_set_call.h's collect_labelled): per record of the chunk in buffer c & 1 its label, and the
// pinned buffers a chunk's labels leave through on their way to the caller.  Whole or absent, like the scratch.
template <typename T>
struct LabelPair {
    Dev<T> d[2];
    Host<T> h[2];                      // (h[1] is set last)
    int ensure();
};

// simplification (sm_simplify.hip, sm_k_simplify.h): the scratch of one chunk's second pass beside the context's RankScratch, the
// last call's tally.  The table lives for one call.
struct Simplify {
    Dev<uint32_t> d_code;              // per record of a chunk: not a representative | loose | its cell's slot
    CallScratch<2> scratch;            // error word | distinct cells | running rank | loose | merged | largest; around what runs outside a chunk stream
    sm_simplify_stats_t stats{};
    bool stats_valid = false;
};

// registration (sm_register.hip, sm_k_register.h): what outlives a call -- the tallies, the partial sums, the state and its pinned
// mirror, the events -- and the last call's tally.  Tables and samples live for one call.
struct Register {
    CallScratch<8> scratch;            // per level the simplification's tally words, then the regular samples; around the target's model and the finish, the source's model, the iterations, the tables' memsets
    Dev<double> d_part;
    Dev<RegState> d_state;
    Host<RegState> h_state;            // pinned
    sm_register_stats_t stats{};
    bool stats_valid = false;
};

// change detection (sm_compare.hip, sm_k_compare.h): the scratch of one chunk of the query beside the context's RankScratch, the
// buffers its labels leave through, the tallies and the last call's.  The tables live for one call.
struct Compare {
    LabelPair<uint8_t> label;
    Dev<uint8_t> d_keep;               // per record of a chunk: 1 = its label is in the write mask
    CallScratch<6> scratch;            // the fine table's tally words (SIMP_RUN: the running rank), the cover table's, the label counts; around the tables' memsets, the reference's model and the finish, a chunk of the query's model
    sm_compare_stats_t stats{};
    bool stats_valid = false;
};

// spatial tiling (sm_tile.hip, sm_k_tile.h): the tallies and events that outlive a call, the last call's tally.  The tile table,
// the batch buffers and the sort's scratch live for one call.
struct Tile {
    // [0]: error word | distinct tiles | running rank | loose; [1]: the loose records' running rank.  Events: around what runs outside
    // a chunk stream and around the sort; per piece buffer (two): around the gather, after the copy
    CallScratch<10> scratch;
    Dev<unsigned long long> d_bits;    // the OR and the AND of a batch's keys
    sm_tile_stats_t stats{};
    bool stats_valid = false;
};

// packing (sm_pack.hip, sm_k_pack.h): the tallies and events that outlive a call, the last call's tally.  The output buffers live
// for one call.
struct Pack {
    CallScratch<4> scratch;            // per buffer (two): the chunk's payload bytes | its RAW blocks; around the live model's chunks
    sm_pack_stats_t stats{};
    bool stats_valid = false;
};

// segmentation (sm_segment.hip, sm_k_segment.h): the scratch of one chunk's labelling beside the context's RankScratch, the buffers
// its labels leave through, the tallies and the last call's.  The table and the component rows live for one call.
struct Segment {
    Dev<uint32_t> d_code;              // per record of a chunk: its component's root slot | SMALL | SKIPPED | LOOSE
    LabelPair<uint32_t> label;
    CallScratch<8> scratch;            // the table's tally words (SIMP_RUN: the kept records' running rank), the openers', the counts; around the memsets, reading 1's model, link to reduce, a chunk of reading 2's model
    sm_segment_stats_t stats{};
    bool stats_valid = false;
};

// meshing (sm_mesh.hip, sm_k_mesh.h): the tally, its pinned mirror, the events and the last call's tally.  The tables, the owners'
// pairs and the mesh live for one call.
struct Mesh {
    // the cell table's tally words, the lattice table's, the running ranks, the counts, the totals.  Events: around the memsets, the
    // model's inserts, claim to cubes, the owners' sort, the emit; per piece buffer (two): after the copy
    CallScratch<12> scratch;
    sm_mesh_stats_t stats{};
    bool stats_valid = false;
};

// the ground map (sm_ground.hip, sm_k_ground.h): the tally, its pinned mirror, the events and the last call's stats.  The cells'
// accumulators and the planes live for one call.
struct Ground {
    // the counts by record kind and by cell state.  Events around: the memsets, reading 1's model, the fill, reading 2's model, finish
    // and state, the transform
    CallScratch<12> scratch;
    sm_ground_stats_t stats{};
    bool stats_valid = false;
};

// routes over the ground map (sm_route.hip, sm_k_route.h): the events, the pinned mirror of the rounds' counters and the last call's
// stats.  The planes, the flags and the paths live for one call.
struct Route {
    static constexpr int N_EV = 8;     // around: the planes' way up with prepare and seed, the rounds, next, the walk
    Event ev[N_EV];
    Host<uint32_t> h_counters;         // pinned (set last: it marks the block complete)
    sm_route_stats_t stats{};
    bool stats_valid = false;
};

// routes a car can follow (sm_car.hip, sm_k_car.h): as Route.  The moves' weights, the costs, the flags and the paths live for one call.
struct Car {
    static constexpr int N_EV = 8;     // around: the planes' way up with prepare and seed, the rounds, next, the walk
    Event ev[N_EV];
    Host<uint32_t> h_counters;         // pinned (set last: it marks the block complete)
    sm_route_car_stats_t stats{};
    bool stats_valid = false;
};

// locating one map set in another (sm_locate.hip, sm_k_locate.h): the tally, its pinned mirror, the events and the last call's
// stats, the pinned buffer of a round.  The rasters, the pyramid and the search's device buffers live for one call.
struct Locate {
    // the counts by record kind of both sets, the occupied cells.  Events around: the memsets, the target's model, the source's model
    // and the compaction, occ and the pyramid
    CallScratch<8> scratch;
    Host<uint8_t> h_round;             // pinned: a round's nodes on their way in, its bounds or best candidates on their way out
    sm_locate_stats_t stats{};
    bool stats_valid = false;
};

// ray casts (sm_rays.hip, sm_k_rays.h): the last call's stats.  The index, the rays and the planes live for one call.
struct Rays {
    sm_rays_stats_t stats{};
    bool stats_valid = false;
};

// point queries (sm_points.hip, sm_k_points.h): the last call's stats.  The index, the points and the planes live for one call.
struct Points {
    sm_points_stats_t stats{};
    bool stats_valid = false;
};

// scenes (sm_scene.hip, sm_k_scene.h): the actors of one call resident on the device -- the distinct files' records as they were
// read, the SoA planes and boxes k_maps_intake makes of them, the call's tables -- grown on demand and reloaded by every call (no
// cache across calls); the last call's tally
struct Scene {
    Dev<float4> d_rec;                 // the distinct files' records, three float4 each, file after file
    size_t rec_cap = 0;                // records
    Dev<float4> d_pos_conf, d_norm_rad, d_box;
    Dev<uint32_t> d_color;
    Dev<float> d_time;
    size_t row_cap = 0;                // rows of the planes (a multiple of 256; every file begins a block)
    Dev<uint8_t> d_tab;                // the device tally | SceneActor per actor | a pose row per (actor, view) | present per (actor, view)
    size_t tab_bytes = 0;
    Event ev[2];                       // around a batch's actor launches
    sm_scene_stats_t stats{};
    bool stats_valid = false;
};

// closing loops unasked (sm_loop.hip): the policy of sm_set_auto_loop and its tally
struct AutoLoop {
    bool on = false;
    bool search = false;               // sm_set_auto_loop_search: the attempt is sm_close_loop_search with `sp`
    sm_search_params sp{};
    sm_auto_loop_params p{};
    std::vector<std::string> paths;    // the caller's map files; the retirement policy's are added per attempt
    int64_t rest_until = 0;            // no census before this tick
    sm_auto_loop_stats_t stats{};
};

// The SM_* switches of the frame pipeline (sm_api.hip), read once by sm_create (read_switches): nothing on the per-frame path
// reads the environment.
struct Switches {
    bool defer_assoc = true;           // SM_DEFER_ASSOC=0: every frame launches its own association
    bool two_launch = true;            // SM_TWO_LAUNCH=0: the fixup step keeps its own launch (three launches per frame)
    bool tail_squeeze = true;          // SM_TAIL_SQUEEZE=0: a periodic compaction is the seven-launch compacting frame and squeezes every dead slot
    uint32_t tail_thresh = 0;          // SM_TAIL_THRESH (debug): dead slots that make a tile the tail squeeze's boundary (unset: TAIL_DEAD_THRESH)
    int pass_split = 0;                // SM_PASS_SPLIT=1|4: k_surfel_pass on whole / quarter tiles whatever the model's size (else: the grid policy picks)
    bool trace = false;                // SM_PASS_TRACE=<file prefix>: per-workgroup time stamps of the last k_surfel_pass and k_assoc_prep launches,
    std::string trace_prefix;          //   dumped by sm_destroy (tools/pass_trace.py)
    int compact_tickets = -1;          // SM_COMPACT_TICKETS=1: compactions always use the ticket-ordered kernel (several PROCESSES share a GPU);
                                       //   =0: never (contexts known not to run at the same time); unset: decided per compaction
    long capacity_wait_us = 2000;      // SM_CAPACITY_WAIT_US: how long an enqueue may let the device catch up before it compacts instead (SlotSchedule::decide_compact)
    bool check_alive = false;          // SM_CHECK_ALIVE (diagnostic): check the alive-bits / dead-count invariant after every stage; reported by sm_sync
    int pass_wg_per_cu = 0;            // SM_PASS_WG_PER_CU: workgroups of k_surfel_pass per CU taken as resident (0: what the occupancy query says)
    int compact_wg_per_cu = 0;         // SM_COMPACT_WG_PER_CU: the same for k_compact, within what the occupancy query allows (experiments)
};

// Work of the last frame that the host has not launched yet.  Each step is held back by the frame that produces it and taken
// exactly once -- by the next frame's preparation launch where it can ride on it (launch_prep), by finalize_if_pending before
// anything else reads its results.  The steps complete in this order: fixup, association, settle, statistics.
// take_*: the arguments (valid until the next hold) with the slot cleared, or null when nothing is held.
class HeldBack {
public:
    // two-launch frame: the fixup step (publisher, cap repair) of a frame whose association is held back too
    void hold_fixup(const FixArgs &x) { assert(!has_fix_ && !has_assoc_); fix_ = x; has_fix_ = true; }
    // the association of an asynchronous frame: held back until the next frame's images arrive, then it shares that frame's
    // preparation launch (k_assoc_prep)
    void hold_assoc(const AssocArgs &a) { assoc_ = a; has_assoc_ = true; }
    // A held-back fixup exists only with the held-back association of its frame and runs ahead of it: the two are taken together.
    // `fix`: that frame's fixup, or null -- it ran in a launch of its own.
    AssocArgs *take_assoc(FixArgs *&fix)
    {
        assert(has_assoc_ || !has_fix_);
        fix = std::exchange(has_fix_, false) ? &fix_ : nullptr;
        return std::exchange(has_assoc_, false) ? &assoc_ : nullptr;
    }
    // the last sharded frame's settle step: rides on the next k_prep, or runs stand-alone (k_shard_settle)
    void hold_settle(const ShardSettle &ss) { settle_ = ss; has_settle_ = true; }
    ShardSettle *take_settle() { return std::exchange(has_settle_, false) ? &settle_ : nullptr; }
    // the statistics of a direct-append frame (`nf`: the set its association counts into): completed by the next frame's fixup
    // publisher, or by k_frame_finalize
    void hold_stats(uint32_t *nf) { nf_ = nf; }
    uint32_t *take_stats() { return std::exchange(nf_, nullptr); }
private:
    bool has_fix_ = false, has_assoc_ = false, has_settle_ = false;
    FixArgs fix_{};
    AssocArgs assoc_{};
    ShardSettle settle_{};
    uint32_t *nf_ = nullptr;
};

// What alternates between consecutive frames (views; sm_ctx::frame_mem owns the memory).  A frame's association is held back and
// runs in the NEXT frame's preparation launch, which writes the other set; in a two-launch frame its fixup step rides on that
// launch too, so the per-frame scratch its publisher and repair crew read while the next frame's flag workgroups and association
// write theirs alternates as well.
struct FrameSet {
    float *depthT = nullptr;           // column-major frame images
    uint32_t *rgbsT = nullptr;
    uint2 *dcT = nullptr;              // (depth bits, rgbs) of the frame the conflict test sees
    uint8_t *tile_flags = nullptr;     // per-tile skip flags, evaluated by extra workgroups of the preparation launch
    uint4 *wave_cnt = nullptr;         // conflicts per quarter tile (one word per wave)
    uint2 *prep_part = nullptr;        // the flag workgroups' skip statistics
    uint32_t *nf_sub = nullptr;        // 2 x 64 sub-counters: new, fused (k_associate_direct)
    uint32_t *conf_sub = nullptr;      // 64 conflict sub-counters (zeroed by the frame's k_prep)
};

// Per-workgroup partial sums a frame's cull / pass leaves for the append that follows it (instead of same-address atomics)
struct PassPartials {
    Dev<uint2> d_compact;              // k_compact<true>: (visible, splat-skipped)
    Dev<uint4> d_lazy;                 // k_surfel_pass: (visible, splat-skipped, killed, conflict-skipped)
    Dev<uint2> d_fix;                  // k_pass_fixup: (visible added, resurrected), read when the cap bound; two sets of MAX_GRID
    int fix_set = 0;                   // ... which alternate: the previous frame's are read one frame later
    uint32_t n_compact = 0;            // workgroups whose partials the next append folds (0: the counters are complete)
    uint32_t n_fix = 0;                // worker workgroups of the last k_pass_fixup
    bool pass_live = false;            // the next append folds d_lazy and d_fix (not d_compact): only between a pass and the append after it
    void clear() { pass_live = false; }
    uint2 *fix_cur() const { return d_fix + (size_t)fix_set * MAX_GRID; }
    // what k_append_scan folds into the counters
    struct Fold { const uint2 *compact; uint32_t n_compact; const uint4 *lazy; const uint2 *fix; uint32_t n_fix; };
    Fold fold() const { return {d_compact, n_compact, pass_live ? d_lazy.get() : nullptr, pass_live ? fix_cur() : nullptr, n_fix}; }
};

// enable_timing: the per-frame time line (an event before the preparation launch, then one after each kernel) over a ring of
// frames, and which kernels the frame of each slot ran (sm_stage_timings)
struct Timeline {
    // compacted: the frame's cull was k_compact (not one that only marks the dead); one_pass: it ran the one-pass kernels
    // (k_surfel_pass + fixup); direct: ... and appended directly; merged: its preparation launch was k_assoc_prep (it carried the
    // previous frame's association, or the chain); deferred: its own association was held back (no kernel between its marks 4 and 5);
    // squeezed: a one-pass frame with a squeeze ahead of its pass -- scan + finalize end at mark 2, k_compact at mark 4, the pass at mark 5
    struct Flags { bool compacted, one_pass, direct, merged, deferred, squeezed; };
    std::unique_ptr<Event[][EV_RING]> ev;   // [N_EV][EV_RING]; whole or absent
    Flags flags[EV_RING] = {};
    uint64_t frames = 0, read = 0;     // frames recorded / read by sm_stage_timings so far
    int mark(hipStream_t st, int which, bool timed)
    {
        if (timed && ev) HIPCK(hipEventRecord(ev[which][frames % EV_RING], st));
        return SM_OK;
    }
    Flags &frame() { return flags[frames % EV_RING]; }      // this frame's (without the ring `frames` stays 0: the writes land in a slot nobody reads)
    void end_frame(bool timed) { if (timed && ev) frames++; }
};

}  // namespace sm_impl

using namespace sm_impl;

struct sm_ctx {
    // the streams come first: members die in reverse order, so everything used on them is released before they are
    Stream stream;
    Stream stream_in;                  // ONE copy stream.  (Two -- colour on one engine, depth + class on another -- were 80 instead of 89 us per frame on
                                       // one box of the pool and stalled for 10-16 ms every few dozen frames on others; tools/h2d_probe.hip: per frame, three
                                       // copies on two streams 68 us + stalls, on one stream 87, ONE copy of the whole frame 58 = the PCIe rate.)
    sm_config cfg{};
    int W = 0, H = 0, P = 0;
    uint32_t cap = 0;                 // MAX_VERTICES
    // Frame parity: begin_frame flips plane_set, and with it the FrameSet the frame uses.  A context that does not defer
    // (SM_DEFER_ASSOC=0, a sharded stream) has ONE set of buffers -- fset[1] views fset[0]'s (alias_frame_sets) -- and the conflict
    // sub-counters alternate all the same.  (Rounds 1-2 ran the depth filter chain of frame f+1 on a second stream instead; since
    // round 3 the chain is a stage of the preparation launch itself.)
    int plane_set = 0;                 // which set the current frame uses (FrameParams::par)
    FrameSet fset[2];
    const FrameSet &cur() const { return fset[plane_set]; }        // the current frame's
    const FrameSet &prev() const { return fset[plane_set ^ 1]; }   // the previous frame's: what its held-back steps still read
    void alias_frame_sets() { uint32_t *c = fset[1].conf_sub; fset[1] = fset[0]; fset[1].conf_sub = c; }
    // the key map alternates on its own schedule: only on the frames that splat (and only where the sets alternate)
    Dev<uint64_t> d_key[2];
    int key_set = 0;
    uint64_t *keyT() const { return d_key[key_set]; }
    std::vector<Dev<void>> frame_mem;  // the buffers behind fset
    Model M{};
    SetBufs m_bufs[2];                 // the buffers behind M.s[0] and M.s[1]
    Dev<DevState> d_state;
    Host<DevState> h_state;           // pinned mirror
    Dev<float> d_filteredT, d_lastT;   // column-major, like the FrameSet's planes
    // row-major staging of the caller's inputs
    Dev<uint8_t> d_rgb, d_sem;
    Dev<uint16_t> d_depth_raw;
    // sm_process_frame_async: a ring of device input sets filled on a copy stream, so that the H2D copy of frame f+1 runs while
    // frame f computes; images in buffers of sm_host_alloc are copied from in place, others through pinned staging
    static constexpr int IN_RING = 3;
    struct InSlot { Dev<uint8_t> rgb; uint8_t *sem = nullptr; uint16_t *depth = nullptr;   // one block: depth and class follow the colour image
                    Host<unsigned char> h_stage; Event ev_in, ev_free; bool used = false; };
    InSlot in[IN_RING];
    size_t in_off_depth = 0, in_off_sem = 0, in_bytes = 0;   // a frame's images as ONE block: colour | depth | class, 16-byte aligned (sm_host_alloc_frame)
    uint32_t in_next = 0;
    // The reference's ONE depth and ONE class texture (src/SurfelMapping.cpp:122-128): the last image given to ANY entry point
    // is current, a null image reads it.  Host forms that wait give into d_depth_raw / d_sem, the async form into an input set,
    // the device forms lend the caller's buffer.  Written by image_given(), read by current_depth() / current_sem() (sm_api.hip).
    const uint16_t *cur_depth = nullptr; const uint8_t *cur_sem = nullptr;             // null until one is given: the zeroed d_depth_raw / d_sem
    int in_depth_slot = -1, in_sem_slot = -1;                                          // the input sets that hold them, -1: none does
    // Pinned host buffers handed out by sm_host_alloc, with their sizes: the sources sm_process_frame_async copies from in
    // place.  Caller memory is never registered: hipHostRegister / hipHostUnregister of heap ranges left the runtime treating
    // later, unrelated host arrays at the same addresses as pinned -- a GPU memory fault in whatever copied to or from them next.
    std::vector<std::pair<Host<unsigned char>, size_t>> pinned;
    Dev<float> d_depth_f32;
    Dev<float> d_xs, d_ys;
    float h_wtab[169];                 // depth_smooth.frag's 13 x 13 weights (host-computed, handed to the chain stage as kernel arguments)
    // cull scratch
    Dev<uint64_t> d_cm, d_dm, d_zm;
    Dev<uint32_t> d_tile_cnt, d_tile_allow, d_tile_keep, d_tile_flag;
    Dev<uint32_t> d_group_tot, d_group_base;
    Dev<uint64_t> d_alive;             // 1 bit per slot: 0 = killed since the last physical compaction (free slots are 1)
    Dev<uint32_t> d_tile_dead;         // dead slots per tile
    size_t alive_words = 0, dead_tiles = 0;
    sm_slots::SlotSchedule slots;      // the occupied slots as the host knows them, which culls compact, what the compaction leaves (sm_slots.h)
    Host<unsigned long long> h_stat; unsigned long long *d_stat = nullptr;   // pinned, device-written: frames<<32 | occupied slots (read by `slots`)
    Dev<uint32_t> d_tb;                // per-tile bounds (8 words per tile)
    Dev<uint32_t> d_conf_part;         // per-workgroup partial counters of k_conflict (instead of same-address atomics)
    PassPartials part;
    // one pass over the surfels per frame (k_surfel_pass + k_pass_fixup) on the frames whose cull only marks the dead
    Dev<float> d_undo;                 // confidence before this frame's decrement, per slot (read only if the conflict cap binds)
    int fix_grid = 128;
    // direct append (k_associate_direct): candidate counts per association block / per group, group prefixes
    Dev<uint32_t> d_blk_cand, d_grp_cand;
    Dev<uint32_t> d_frame_sub;         // 2 x 64 sub-counters: visible, killed (k_surfel_pass); behind them the two FrameSets' nf_sub
    uint32_t n_grp = 0, cand_group = 16;
    Dev<unsigned long long> d_pass_trace;         // Switches::trace: per-workgroup time stamps of the last k_surfel_pass launch, dumped by sm_destroy
    int pass_trace_grid = 0;
    Dev<unsigned long long> d_ap_trace;           // the same for the last k_assoc_prep launch: (entry, exit) per workgroup
    int ap_trace_n[4] = {0, 0, 0, 0};             // its association / tile-flag / image workgroups (dispatch order); fixup workgroups ahead of them
    Dev<uint32_t> d_conf_sub;          // 2 x 64 conflict sub-counters: the two FrameSets' conf_sub
    uint32_t n_conf_part = 0;
    uint32_t tb_tiles = 0;
    int compact_grid = COMPACT_GRID;
    int pass_grid = MAX_GRID;          // workgroups of k_surfel_pass that are resident at once (a larger grid runs its tail as a second, thin wave)
    // association scratch
    Dev<uint64_t> d_validmask, d_fusedmask;
    Dev<uint2> d_blk_cnt;
    // slot-addressed sharding of one stream, in-stream form (sm_shard_stream_*)
    bool ss_on = false;
    bool rig_on = false;               // sm_rig_configure: rank / world / collective are used by sm_rig_consolidate only
    float rig_last_time = -1.0e30f;    // creation time stamp up to which this rank's surfels are in the incremental GlobalModel (sm_rig_consolidate_step)
    int ss_rank = 0, ss_world = 1;
    uint32_t ss_frames = 0;            // fusing frames so far = index of the next segment (its owner: index % world)
    sm_collective_fn ss_coll = nullptr;
    void *ss_user = nullptr;
    void *ss_comm = nullptr;           // ncclComm_t when the built-in RCCL binding is used
    Dev<uint64_t> d_galive, d_new_alive, d_gmask;
    Dev<uint32_t> d_chk;               // Switches::check_alive: result words of k_check_alive
    Dev<uint64_t> d_capx;              // the conflict-cap exchange of a sharded frame: total | quarter-tile counts | conflict masks (k_shard_cap_pack)
    Dev<uint32_t> d_ss_info;
    Switches sw;
    // deferred association (k_assoc_prep): the association of an asynchronous frame is held back until the next frame's images
    // arrive and then shares that frame's k_prep launch (three launches per frame instead of four).  Two-launch frame
    // (sw.two_launch): the frame's fixup step is held back with it and rides on the same launch; the candidate count moved into
    // the pass's launch
    bool defer_ok = false;             // this context may defer (sw.defer_assoc, not a sharded stream)
    HeldBack held;
    static constexpr uint32_t N_CREW = 32;
    int n_pix_blocks = 0;
    // export staging
    Dev<void> d_export;
    size_t export_bytes = 0;
    MapStaging staging;                // of every stream of map-file chunks
    sm_mapset::FileIndex index;        // of the map files the context has read or written (retirement, recall, warp)
    ModelView rm;
    Tracker trk;
    Retire ret;
    RenderMaps maps;
    Recall rec;
    Warp warp;
    AutoLoop aloop;
    Search srch;
    Lidar lid;
    Place place;
    Stereo stereo;
    LidarDepth ldepth;
    Fill fill;
    Blend blend;
    Simplify simp;
    // host frame state (src/SurfelMapping.h:100-103)
    int tick = 0;
    bool ref_set = false;
    bool raw_valid = false;            // a frame that computes the raw feedback cloud has run (every call but the reference frame)
    int raw_tick = 0;                  // its time stamp
    float curr_pose[16], last_pose[16];
    bool pending_cull = false;
    uint32_t count_before_cull = 0, offset_before_cull = 0;
    sm_counts counts{};
    std::vector<Dev<void>> user_allocs;
    Timeline tl;
    Dev<FrameLog> d_log;
    Register reg;                      // (nothing depends on where it lies; behind the frame path's members, which keep their places)
    Compare cmp;
    RankScratch ranked;
    Tile tile;
    Pack pack;
    Segment seg;
    Mesh mesh;
    Ground ground;
    Locate locate;
    Rays rays;
    Scene scene;
    Points points;
    Route route;
    Car car;
};

namespace sm_impl __attribute__((visibility("hidden"))) {

template <typename T>
int dalloc(Dev<T> &p, size_t n)
{
    HIPCK(hipMalloc(p.put(), std::max<size_t>(n, 1) * sizeof(T)));
    return SM_OK;
}

// A timed stretch of the context's stream between the events pair[0] and pair[1]: mark() records one of them, add_marked() waits
// for the second and adds the stretch to *ms_sum.
inline int mark(sm_ctx *s, const Event &e) { HIPCK(hipEventRecord(e, s->stream)); return SM_OK; }
inline int add_marked(const Event *pair, float *ms_sum)
{
    float ms = 0.0f;
    HIPCK(hipEventSynchronize(pair[1]));
    HIPCK(hipEventElapsedTime(&ms, pair[0], pair[1]));
    *ms_sum += ms;
    return SM_OK;
}

// ---- sm_api.hip ----
void invert4(const float *m, float *out);         // general 4x4 inverse, column-major, fp32
FrameParams make_params(const sm_ctx *s, const float *pose);
bool hip_runtime_conflict(const char *where);     // true (and g_err set) if more than one libamdhip64 is mapped into the process
int push_state(sm_ctx *s);
int pull_state(sm_ctx *s);
int finalize_if_pending(sm_ctx *s);
int ensure_compact(sm_ctx *s);
int rebuild_bounds(sm_ctx *s, uint32_t first_surfel, uint32_t count);
// The model has been written from outside the frame pipeline and is now the dense rows [0, count), of which [first_new, count)
// are new: count and offset, no dead slots, the compaction schedule restarted, the tile boxes from first_new's tile on rebuilt,
// the host's mirror and counts refreshed.  What an upload leaves; a retirement, a recall and the reset path leave the same.
int publish_dense(sm_ctx *s, uint32_t count, uint32_t first_new);
int ensure_export(sm_ctx *s, size_t bytes);
void fill_keys(sm_ctx *s, uint64_t *key, size_t n);                  // k_fill_keys on the context's stream
int clean_points_device(sm_ctx *s, const uint16_t *d_depth_mm, const uint8_t *d_semantic, const float *pose16, int exempt_first,
                        const std::function<long long(uint32_t)> *cap_hook = nullptr);
int ss_collective(sm_ctx *s, const void *send, void *recv, size_t count, int op);
// ---- sm_model_io.hip ----
void export_aos(sm_ctx *s, float *dst12, uint32_t first, uint32_t n);   // k_export_aos on the context's stream
void import_aos(sm_ctx *s, const float *d_src12, uint32_t first, uint32_t n);   // k_import_aos on the context's stream: n device records into slots first..
// the novel view's splat of the live model into `key` with ids id_base + slot (k_render_splat on the context's stream)
void render_splat_model(sm_ctx *s, const RenderParams &rp, uint64_t *key, uint32_t id_base);
// ---- sm_view.hip ----
// a model view's rules that need no context (SM_E_ARG with g_err set), and its kernel arguments
int check_model_view(const sm_model_view *v, const char *fn);
void model_view_params(const sm_model_view *v, ViewParams &vp, ViewShade &vs);
// the model view's splat (+ overflow) of the live model into `key` with ids id_base + slot, on the context's stream;
// d_ovf_n: 4 bytes, d_ovf: 4 bytes per live surfel.  `timing` (optional): three events recorded before the splat, between
// the two kernels and after the overflow (SM_RENDER_MODEL_TIMING).
int view_splat_model(sm_ctx *s, const ViewParams &vp, uint64_t *key, uint32_t *d_ovf_n, uint32_t *d_ovf, uint32_t id_base,
                     const Event *timing = nullptr);
// ---- sm_retire.hip ----
int auto_retire_after_frame(sm_ctx *s);           // the periodic policy: called once a frame is enqueued (one test unless it is due)
// ---- sm_render_maps.hip ----
int maps_ensure_staging(sm_ctx *s);               // the staging's copy stream, buffers and events: whole or absent
// k_maps_intake on the context's stream: n records at d_rec into the staging's SoA planes and its one box per 256 records
void maps_intake(sm_ctx *s, const float4 *d_rec, uint32_t n);
// ... into planes and boxes of the caller's (the scenes' resident actors)
void maps_intake_to(sm_ctx *s, const float4 *d_rec, uint32_t n, const MapsSoA &out, float4 *d_box);
// ---- sm_pack.hip ----
int maps_ensure_packed(sm_ctx *s);                // the staging's packed pair: whole or absent
// k_unpack on the context's stream: the nblk blocks (n records) whose directory entries lie at d_dir and whose payload, beginning
// at the first block's offset, at d_payload, decoded into n 48-byte records at d_rec
void maps_unpack(sm_ctx *s, const uint8_t *d_dir, const uint8_t *d_payload, uint32_t n, int32_t pos_step_log2, float4 *d_rec);
// ---- sm_scene.hip ----
// The actors of a scene call as the host knows them once its arguments and every actor's header are checked (scene_check), and,
// after scene_load, what the static sources' loops need to draw them.  The render path and the lidar's pass get it as a pointer,
// null without actors: they then enqueue what they always did.
struct ScenePlan {
    struct File { std::string path; uint32_t count, rec0, row0; };   // rec0: first record in d_rec; row0: first row of the planes
    const sm_scene *scene = nullptr;
    uint32_t n_views = 0;
    std::vector<File> files;           // the distinct ones, in order of first mention
    std::vector<uint32_t> file_of;     // per actor
    uint64_t ids = 0;                  // records summed over the actors, present or not
    uint64_t resident = 0, rows = 0;   // records of the distinct files; rows of the planes they take
    uint32_t id_base = 0;              // A, the static total (scene_load)
    uint32_t n_wg = 0;                 // workgroups of a splat: the actors' blocks
    int cull = 1;
};
// host only: SM_E_ARG / SM_E_CAPACITY with g_err set, else the plan
int scene_check(const sm_scene *scene, uint32_t n_views, const char *fn, ScenePlan &plan);
// the id limit against the static total; then, unless the call draws nothing, the files read, uploaded and unpacked and the
// call's tables on the device.  The call's tally begins here.
int scene_load(sm_ctx *s, ScenePlan &plan, uint64_t static_total, bool draw, const char *fn);
// One batch's actor launches on the context's stream, after every static source: the splat of views [v0, v0 + b) into the batch's
// key planes, then the resolve of the actors' keys into the batch's output planes.  d_rps / d_poses: the batch's first.
int scene_draw_image(sm_ctx *s, const ScenePlan &plan, const RenderParams *d_rps, uint32_t v0, uint32_t b, uint64_t *d_key, size_t npix,
                     uint8_t *d_bgr, uint8_t *d_sem);
int scene_draw_lidar(sm_ctx *s, const ScenePlan &plan, const LidarGrid &g, const LidarPose *d_poses, uint32_t v0, uint32_t b, uint64_t *d_key,
                     size_t nbeams, float *d_range, int32_t *d_id, uint8_t *d_rgb, uint8_t *d_sem);
int scene_fold(sm_ctx *s);             // once the batch's stream is waited for: its actor time into the tally
int scene_end(sm_ctx *s, const ScenePlan &plan);   // the device tally into the call's
// ---- sm_lidar.hip ----
// sm_lidar_sweep (src null), sm_lidar_sweep_maps and, with a plan, sm_lidar_sweep_scene; fn: the one the call came through
int lidar_sweep(sm_ctx *s, const sm_map_source *src, const sm_lidar_sensor *sn, const float *poses16, uint32_t n_sweeps, float *range, int32_t *id,
                uint8_t *rgb, uint8_t *sem, const char *fn, ScenePlan *scene = nullptr);
// ---- sm_recall.hip ----
// the periodic policy: called by a frame that has just retired (one test unless it is on).  wrote_file: this round's retirement
// wrote the policy's newest file, at this pose -- every row of it is far, so the recall does not read it
int auto_recall_after_retire(sm_ctx *s, bool wrote_file);
// For the file index, when the retirement policy writes a file (its setter has allocated the scratch): the box of the finite
// centres and the largest non-NaN time of n AoS records in device memory folded into lo / hi / *max_time (k_recall_mark +
// k_recall_scan on the context's stream; waits)
int recall_box_of(sm_ctx *s, const float *d_rec12, uint32_t n, float lo[3], float hi[3], float *max_time);
int recall_ensure_scratch(sm_ctx *s);             // what recall_box_of needs (sm_set_auto_retire allocates it with its own)
// what the two policies require of each other when both are on (SM_E_ARG with g_err set otherwise)
int check_recall_policy(float radius, const sm_retire_params &rp, const char *who);

// ---- sm_track.hip ----
// the time window of a prediction: surfels with lo < m[7] <= hi; INT32_MIN / INT32_MAX leave that end open
struct TrackWindow { int32_t lo, hi; };
// One tracked frame, whichever public form it came through (fn names it in the error texts): rgb null = sm_track_frame's depth
// schedule, otherwise sm_track_frame_rgb's; win null = the whole model.  It never consults the policy of sm_set_auto_loop.
// pred16 (null: T_prev, the pose of the last processed frame) is the camera the prediction is drawn at (sm_search_pose_at).
int track_windowed(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params,
                   const sm_track_rgb_params *rgb_params, const TrackWindow *win, float *pose16_out, sm_track_info *info,
                   sm_track_rgb_info *rgb_info, float *anchor_time, const char *fn, const float *pred16 = nullptr);
// What sm_search.hip takes from a tracked frame's preparation.  The prediction's camera and image, the grid of `stride` and the
// association gates, as the trackers' kernels get them:
struct SearchFrame {
    float tinv_prev[16];               // world -> prediction camera
    float fx, fy, cx, cy;
    int W, H;
    int stride, ni, nj, n;             // the grid: ni columns x nj rows, n = ni * nj
    float dist, cos_angle;
};
// the buffers the preparation leaves on the context's stream: vertex and normal per grid point (row-major over the grid), slot per
// pixel (-1: none), and the surfels in view of the prediction (a device word)
struct SearchBufs { const float4 *v, *n; const int32_t *pred; const uint32_t *in_view; };
// sm_track_frame_window's checks and preparation for the grid of `stride` (tp's own pixel_stride is not used), enqueued:
// *no_model when there is no processed frame or no live surfel (nothing is enqueued then).  fresh = false: the prediction of the
// last call stands (same frame, same window, same pred16, nothing ran in between) and only the grid's vertex stage runs again.
// pred16 as track_windowed's.
int search_prepare(sm_ctx *s, const uint16_t *depth_mm, const sm_track_params &tp, int32_t stride, int32_t min_time, int32_t max_time,
                   bool fresh, SearchFrame *f, SearchBufs *b, bool *no_model, const char *fn, const float *pred16 = nullptr);
// ---- sm_search.hip ----
// sm_search_pose's rules for its parameters (SM_E_ARG with g_err set)
int check_search_params(const sm_search_params &p, const char *who);
// sm_search_pose (pred16 null: the prediction at T_prev) and sm_search_pose_at; fn: the one the call came through
int search_pose(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pred16, const float *centre16, const sm_track_params *tp,
                const sm_track_rgb_params *rp, const sm_search_params *sp, int32_t min_time, int32_t max_time, float *pose16_out,
                sm_search_info *info, const char *fn);
// ---- sm_place.hip ----
void place_reset(sm_ctx *s);                      // sm_reset: the database is empty again (the table stays)
// sm_warp_by_time's pose rule (sm_warp.hip, warp_pose) for every stored keyframe pose
void place_warp_poses(sm_ctx *s, const std::function<void(float *, int32_t)> &warp_pose);
// sm_track_frame (rgb null) / sm_track_frame_rgb while sm_set_auto_place is on, after the track (and the auto-loop policy's work):
// the frame's code, the match, one attempt at the matched place, the keyframe.  loop_closed: that policy closed a loop on this call
int auto_place_after_track(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const sm_track_params *params,
                           const sm_track_rgb_params *rgb_params, float *pose16_out, int track_status, bool loop_closed);
// ---- sm_fill.hip ----
// sm_fill_params' ranges (SM_E_ARG with g_err set); p null: nothing to check
int check_fill_params(const sm_fill_params *p, const char *who);
// device bytes the stage needs beside its planes for n images of w x h (the pyramid scratch): what a batch of views costs above its keys
size_t fill_scratch_bytes(const sm_fill_params &p, int w, int h, size_t n);
// k_fill_key_depth on the context's stream: depth_mm of `total` keys of novel views
void fill_key_depth(sm_ctx *s, const uint64_t *key, size_t total, uint16_t *d_depth);
// The render paths' use of the stage.  fill_begin: a call that may fill starts (the tally is the new call's).  fill_enqueue: the
// completion of n device images in place on the context's stream (d_depth null: no depth).  fill_fold: waits for the stage and adds
// its tallies and time to the call's; a call enqueues its next pass only after it.
void fill_begin(sm_ctx *s);
int fill_enqueue(sm_ctx *s, const sm_fill_params &p, int w, int h, uint32_t n, uint8_t *d_bgr, uint8_t *d_sem, uint16_t *d_depth);
int fill_fold(sm_ctx *s);
// ---- sm_blend.hip ----
// sm_blend_params' ranges (SM_E_ARG with g_err set); p null: nothing to check
int check_blend_params(const sm_blend_params *p, const char *who);
// The render paths' use of the stage, all on the context's stream.  blend_begin: a blended call starts (the tally is the new
// call's).  blend_clear: accumulators for `pixels` pixels (all views of a batch), zeroed with the device's tally.  blend_mark: what
// follows up to blend_normalise is timed by the stage itself (a chunk stream times its own kernels: blend_add_ms).
// blend_accum_model: the live model's fragments into the accumulators of the view whose keys are d_key (`acc_pixel`: where that
// view begins in the batch).  blend_accum_chunk: the chunk in the context's staging (after maps_intake) into `views` views.
// blend_normalise: the sums become the colours of `views` views of npix pixels in d_bgr, over the nearest colours it holds.
// blend_fold: waits for the stream and adds the batch's tally and time to the call's.
void blend_begin(sm_ctx *s);
int blend_clear(sm_ctx *s, size_t pixels);
int blend_mark(sm_ctx *s);
void blend_accum_model(sm_ctx *s, const sm_blend_params &p, const RenderParams &rp, const uint64_t *d_key, size_t acc_pixel);
void blend_accum_chunk(sm_ctx *s, const sm_blend_params &p, uint32_t n, const RenderParams *d_rps, const uint64_t *d_key, size_t npix,
                       uint32_t views, int cull);
int blend_normalise(sm_ctx *s, const uint64_t *d_key, size_t npix, uint32_t views, uint8_t *d_bgr, const uint8_t *d_sem);
void blend_add_ms(sm_ctx *s, float ms);
int blend_fold(sm_ctx *s);
// ---- the novel view behind sm_render_image, _ex and _blend (sm_model_io.hip) and its map-set form (sm_render_maps.hip) ----
int render_image(sm_ctx *s, const float *view16, int w, int h, float fx, float fy, float cx, float cy, const sm_blend_params *blend,
                 const sm_fill_params *fill, uint8_t *bgr_out, uint8_t *sem_out, uint16_t *depth_mm_out, const char *who);
int render_image_maps(sm_ctx *s, const sm_map_source *src, const float *views16, uint32_t n_views, int w, int h, float fx, float fy,
                      float cx, float cy, const sm_blend_params *blend, const sm_fill_params *fill, uint8_t *bgr_out, uint8_t *sem_out,
                      uint16_t *depth_mm_out, const char *fn, ScenePlan *scene = nullptr);
// ---- sm_loop.hip ----
// sm_track_frame (rgb null) / sm_track_frame_rgb while sm_set_auto_loop is on: the young-window track, the census, one attempt
int auto_loop_track(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *guess16, const sm_track_params *params,
                    const sm_track_rgb_params *rgb_params, float *pose16_out, sm_track_info *info, sm_track_rgb_info *rgb_info);
// ---- sm_warp.hip ----
// sm_close_loop's rules for its parameters (SM_E_ARG with g_err set)
int check_loop_params(const sm_loop_params &p, const char *who);
// sm_close_loop (rgb null: the depth-only measurement) and sm_close_loop_rgb; search: sm_close_loop_search, whose step 1 is
// sm_search_pose with sp (null: its defaults); place16 non-null: sm_close_loop_at, whose step 1 is sm_search_pose_at there.
// who: the one of the four the call came through.
int close_loop(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const float *pose16, const sm_map_source *src,
               const sm_track_params *tp, const sm_track_rgb_params *rp, const sm_loop_params *lp, bool search, const sm_search_params *sp,
               float *pose16_out, sm_loop_info *info, const char *who, const float *place16 = nullptr);

// ---- what several sources ask of their arguments (SM_E_ARG with g_err set) ----
// what works on the whole map (retirement, recall, warp, loop closure and its policy, pose search) refuses a context that holds a
// part of it
inline int check_whole_map(const sm_ctx *s, const char *who)
{
    if (s->ss_on || s->rig_on) { g_err = std::string(who) + ": a sharded or rig context holds only its own surfels"; return SM_E_UNSUPPORTED; }
    return SM_OK;
}

// ... and what reads or changes the whole model refuses the half-done cull of the per-pass stage API
inline int check_not_mid_cull(const sm_ctx *s, const char *who)
{
    if (s->pending_cull) { g_err = std::string(who) + " between sm_stage_conflict and sm_stage_cull"; return SM_E_ARG; }
    return SM_OK;
}

inline int check_pose(const float *pose16, const char *who)          // null: the entry point's default
{
    if (pose16)
        for (int i = 0; i < 16; ++i)
            if (!std::isfinite(pose16[i])) { g_err = std::string(who) + ": non-finite pose"; return SM_E_ARG; }
    return SM_OK;
}

inline int check_map_source(const sm_map_source *src, const char *who)
{
    if (src->n_paths && !src->paths) { g_err = std::string(who) + ": null paths"; return SM_E_ARG; }
    for (uint32_t i = 0; i < src->n_paths; ++i)
        if (!src->paths[i]) { g_err = std::string(who) + ": null path"; return SM_E_ARG; }
    return SM_OK;
}

// n records out of the model into host memory, `chunk` at a time through the export scratch (which holds a chunk: ensure_export):
// produce(d_dst, first, m) launches what fills the scratch with records [first, first + m), they are copied to
// dst + first * dst_stride floats (0: a staging buffer that each(first, m) empties), the stream is waited for, each() runs.
template <typename Produce, typename Each>
int drain_export(sm_ctx *s, uint32_t n, uint32_t chunk, float *dst, size_t dst_stride, Produce produce, Each each)
{
    for (uint32_t first = 0; first < n; first += chunk) {
        const uint32_t m = std::min(chunk, n - first);
        produce((float *)s->d_export.get(), first, m);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(dst + (size_t)first * dst_stride, s->d_export, (size_t)m * 48, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        if (int rc = each(first, m)) return rc;
    }
    return SM_OK;
}
inline int no_hook(uint32_t, uint32_t) { return SM_OK; }

}  // namespace sm_impl
