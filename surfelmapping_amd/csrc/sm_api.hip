// sm_api.hip -- C-ABI (include/sm_c_api.h) of the gfx950 surfel-fusion core: context lifecycle, buffers, frame sequencing
// (SurfelMapping::processFrame, /root/reference/src/SurfelMapping.cpp:115-251), the per-pass stage API, the sharded stream,
// and launches of the kernels in sm_kernels.h.  The other features live in their own sources (sm_ctx.h lists them).  No CPU
// fallback: without a HIP device sm_create() fails with SM_E_NO_DEVICE.
#include "sm_ctx.h"
#include "sm_kernels.h"

#include <hip/hip_runtime.h>

#include <dirent.h>
#include <link.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace sm;

namespace {

// column-major 4x4 product, c_ij = ((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j) + a_i3 b_3j
void mul4(const float *a, const float *b, float *out)
{
    float r[16];
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i)
            r[j * 4 + i] = ((a[i] * b[j * 4] + a[4 + i] * b[j * 4 + 1]) + a[8 + i] * b[j * 4 + 2]) + a[12 + i] * b[j * 4 + 3];
    memcpy(out, r, sizeof r);
}

// exp of DESIGN.md "Arithmetic": k = rint(x*log2e); r = (x - k*ln2hi) - k*ln2lo; degree-6 Horner; ldexp
float exp_spec(float x)
{
    const float LOG2E = 1.44269502162933349609375f;
    const float LN2HI = 0.693145751953125f, LN2LO = 1.428606765330187045037746429443359375e-06f;
    const float k = rintf(x * LOG2E);
    const float r = (x - k * LN2HI) - k * LN2LO;
    float p = 1.0f / 720.0f;
    p = 1.0f / 120.0f + r * p;
    p = 1.0f / 24.0f + r * p;
    p = 1.0f / 6.0f + r * p;
    p = 0.5f + r * p;
    p = 1.0f + r * p;
    p = 1.0f + r * p;
    return ldexpf(p, (int)k);
}

}  // namespace

// Two HIP runtimes in one process.  PyTorch's ROCm wheels bundle their own libamdhip64.so (soname libamdhip64.so.7) and
// request it by the name "libamdhip64.so"; this library requests "libamdhip64.so.7".  The dynamic loader matches a
// request against the names / sonames of what is loaded already: torch first -> its copy satisfies our request (one
// runtime, fine); this library first -> ROCm's copy is loaded, torch's later request for "libamdhip64.so" does not match its
// soname, so torch/lib/libamdhip64.so is loaded TOO, and torch / its RCCL then run on another runtime than the one that
// owns this library's device memory (seen as a process exit inside RCCL: gpurun_out/pytest_gpu2.log, round 1).
// surfelmapping_amd.capi.load() avoids it by pre-loading torch's copy when torch is installed; any other host gets a
// refusal with the two paths instead of undefined behaviour.
namespace {
int collect_hip_runtime(struct dl_phdr_info *info, size_t, void *data)
{
    auto *v = static_cast<std::vector<std::string> *>(data);
    if (info->dlpi_name && std::strstr(info->dlpi_name, "libamdhip64")) v->push_back(info->dlpi_name);
    return 0;
}
}  // namespace

bool sm_impl::hip_runtime_conflict(const char *where)
{
    std::vector<std::string> libs;
    dl_iterate_phdr(collect_hip_runtime, &libs);
    std::sort(libs.begin(), libs.end());
    libs.erase(std::unique(libs.begin(), libs.end()), libs.end());
    if (libs.size() <= 1) return false;
    g_err = std::string(where) + ": two HIP runtimes are loaded in this process (" + libs[0] + ", " + libs[1] +
            "); device memory of one is not valid in the other.  Load the other user's runtime first (Python: import torch, or "
            "surfelmapping_amd.capi, before anything that loads ROCm's libamdhip64; C++: link RCCL and this library against the same ROCm)";
    return true;
}

// Contexts of one process that share a GPU: the in-place compaction kernel waits on tile hand-off flags and, in its
// default form, needs its whole grid resident -- two of them running at the same time can starve each other
// (SM_E_STALL).  As soon as a second context exists on a device, compactions there use the ticket-ordered form of the
// kernel, which makes no residency assumption (SM_COMPACT_TICKETS=1 forces it, e.g. when several PROCESSES share a GPU;
// =0 keeps the round-robin form for a process whose contexts never run at the same time).
namespace {
constexpr int MAX_DEV = 64;
std::mutex g_compact_mu;
int g_ctx_on_dev[MAX_DEV] = {};

// Other PROCESSES on the same GPU are invisible to the counter above.  The KFD driver lists every process with its
// queues under /sys/class/kfd/kfd/proc/<pid>/queues/<n>/gpuid (host pids: inside a container our own pid does not match,
// so processes are only counted).  Device -> gpuid goes through the PCI address (topology/nodes/<n>/properties location_id).
// Returns the number of processes that hold queues on this device's GPU (>= 1 once this process has a context there),
// or -1 if the tables cannot be read.
int kfd_processes_on_gpu(int dev)
{
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof bus, dev) != hipSuccess) return -1;
    unsigned dom = 0, b = 0, d = 0, f = 0;
    if (sscanf(bus, "%x:%x:%x.%x", &dom, &b, &d, &f) != 4) return -1;
    const unsigned long want_loc = ((unsigned long)b << 8) | ((unsigned long)d << 3) | f;
    unsigned long gpuid = 0;
    bool found = false;
    for (int n = 0; n < 64 && !found; ++n) {
        char path[128];
        snprintf(path, sizeof path, "/sys/class/kfd/kfd/topology/nodes/%d/properties", n);
        FILE *fp = fopen(path, "r");
        if (!fp) { if (n > 16) break; continue; }
        char key[64]; unsigned long val, loc = ~0ul, domain = 0;
        while (fscanf(fp, "%63s %lu", key, &val) == 2) {
            if (!strcmp(key, "location_id")) loc = val;
            else if (!strcmp(key, "domain")) domain = val;
        }
        fclose(fp);
        if (loc == want_loc && domain == dom) {
            snprintf(path, sizeof path, "/sys/class/kfd/kfd/topology/nodes/%d/gpu_id", n);
            FILE *fg = fopen(path, "r");
            if (fg) { found = fscanf(fg, "%lu", &gpuid) == 1 && gpuid != 0; fclose(fg); }
        }
    }
    if (!found) return -1;
    DIR *pd = opendir("/sys/class/kfd/kfd/proc");
    if (!pd) return -1;
    int procs = 0;
    while (struct dirent *pe = readdir(pd)) {
        if (pe->d_name[0] < '0' || pe->d_name[0] > '9') continue;
        char qdir[256];
        snprintf(qdir, sizeof qdir, "/sys/class/kfd/kfd/proc/%s/queues", pe->d_name);
        DIR *qd = opendir(qdir);
        if (!qd) continue;
        bool here = false;
        while (struct dirent *qe = readdir(qd)) {
            if (qe->d_name[0] < '0' || qe->d_name[0] > '9') continue;
            char gp[400];
            snprintf(gp, sizeof gp, "%s/%s/gpuid", qdir, qe->d_name);
            FILE *fg = fopen(gp, "r");
            unsigned long g = 0;
            if (fg) { if (fscanf(fg, "%lu", &g) == 1 && g == gpuid) here = true; fclose(fg); }
            if (here) break;
        }
        closedir(qd);
        if (here) ++procs;
    }
    closedir(pd);
    return procs;
}

// cached per device, refreshed at most once per second (a few sysfs reads: ~0.2 ms)
bool gpu_shared_with_other_process(int dev)
{
    static std::mutex mu;
    static std::chrono::steady_clock::time_point last[MAX_DEV];
    static int cached[MAX_DEV];
    static bool valid[MAX_DEV] = {};
    if (dev < 0 || dev >= MAX_DEV) return false;
    std::lock_guard<std::mutex> lk(mu);
    const auto now = std::chrono::steady_clock::now();
    if (!valid[dev] || std::chrono::duration_cast<std::chrono::milliseconds>(now - last[dev]).count() > 1000) {
        cached[dev] = kfd_processes_on_gpu(dev);
        last[dev] = now; valid[dev] = true;
    }
    return cached[dev] > 1;
}

bool compaction_needs_tickets(const sm_ctx *s)
{
    const int dev = s->cfg.device;
    if (s->sw.compact_tickets >= 0) return s->sw.compact_tickets != 0;
    if (dev < 0 || dev >= MAX_DEV) return true;
    {
        std::lock_guard<std::mutex> lk(g_compact_mu);
        if (g_ctx_on_dev[dev] > 1) return true;
    }
    return gpu_shared_with_other_process(dev);
}

// every SM_* switch of this source, once per context (sm_create); Switches explains them
Switches read_switches()
{
    Switches sw;
    auto off = [](const char *name) { const char *e = std::getenv(name); return e && e[0] == '0'; };
    auto num = [](const char *name, long unset) { const char *e = std::getenv(name); return e ? std::atol(e) : unset; };
    sw.defer_assoc = !off("SM_DEFER_ASSOC");
    sw.two_launch = !off("SM_TWO_LAUNCH");
    sw.tail_squeeze = !off("SM_TAIL_SQUEEZE");
    sw.tail_thresh = (uint32_t)std::max(1l, num("SM_TAIL_THRESH", (long)TAIL_DEAD_THRESH));
    sw.pass_split = (int)num("SM_PASS_SPLIT", 0);
    if (const char *e = std::getenv("SM_PASS_TRACE")) { sw.trace = true; sw.trace_prefix = e; }
    if (std::getenv("SM_COMPACT_TICKETS")) sw.compact_tickets = off("SM_COMPACT_TICKETS") ? 0 : 1;
    sw.capacity_wait_us = num("SM_CAPACITY_WAIT_US", 2000);
    sw.check_alive = std::getenv("SM_CHECK_ALIVE") != nullptr;
    if (std::getenv("SM_PASS_WG_PER_CU")) sw.pass_wg_per_cu = (int)std::max(1l, num("SM_PASS_WG_PER_CU", 1));
    if (std::getenv("SM_COMPACT_WG_PER_CU")) sw.compact_wg_per_cu = (int)std::max(1l, num("SM_COMPACT_WG_PER_CU", 1));
    return sw;
}

// Workgroups of k_surfel_pass and of k_compact that are resident at once on `device`; left as they are where the device cannot be asked.
void resident_grids(const Switches &sw, int device, int *pass_grid, int *compact_grid)
{
    int cus = 0, per_cu = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) return;
    // k_surfel_pass: with more workgroups than the chip holds at once the surplus starts when the first ones are done --
    // on a model where every tile has work (20 M scattered surfels: ~10 tiles per workgroup) that is a second pass at an
    // eighth of the occupancy.  Grid = what is resident; tiles go round-robin.  (sw.pass_wg_per_cu overrides.)
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_surfel_pass<1>, 256, 0) == hipSuccess && per_cu > 0) {
        // the occupancy API over-reports by one block per CU here (measured; MI355X_MICROARCH.md)
        const int want = sw.pass_wg_per_cu ? sw.pass_wg_per_cu : std::max(1, per_cu - 1);
        *pass_grid = std::max(256, std::min(cus * want, MAX_GRID));
    }
    // the in-place compaction needs every workgroup of k_compact resident at once
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_compact<true>, 256, 0) == hipSuccess && per_cu > 0) {
        // the occupancy API can over-report by one block per CU (MI355X_MICROARCH.md): stay at <= 4 and below it
        // <= 4 per CU: in that range the limit is VGPR/LDS-bound and the API is exact; above it keep a margin
        // (sw.compact_wg_per_cu overrides the margin for experiments)
        const int want = sw.compact_wg_per_cu ? std::min(per_cu, sw.compact_wg_per_cu) : std::min(per_cu, 4);
        *compact_grid = std::max(1, cus * want);
    }
}

int alloc_set(SetBufs &b, size_t cap)
{
    return dalloc(b.pos_conf, cap) || dalloc(b.norm_rad, cap) || dalloc(b.color, cap) || dalloc(b.init_time, cap) ||
           dalloc(b.time, cap) ? SM_E_HIP : SM_OK;
}

int grid_surfels(const sm_ctx *s)
{
    return (int)std::min<uint64_t>(std::max<uint64_t>(s->slots.tiles(), 1), MAX_GRID);
}

// SM_CHECK_ALIVE=1 (diagnostic): check the alive-bits / dead-count invariant after a stage; reported by sm_sync
void check_alive(sm_ctx *s, uint32_t stage)
{
    if (!s->d_chk) return;
    hipLaunchKernelGGL(k_check_alive, dim3(64), dim3(256), 0, s->stream, s->d_state, s->d_alive, s->d_tile_dead, s->d_chk, stage);
}

int take_error(sm_ctx *s)
{
    if (s->h_state->error != 0) {
        const int e = s->h_state->error;
        s->h_state->error = 0;
        HIPCK(hipMemcpyAsync(&s->d_state->error, &s->h_state->error, sizeof(int32_t), hipMemcpyHostToDevice, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        g_err = e == SM_E_CAPACITY ? "model capacity (MAX_VERTICES) exceeded; frame's new surfels dropped"
              : e == SM_E_UNSUPPORTED ? "unsupported operation flagged on the device"
              : "device-side error";
        return e;
    }
    return SM_OK;
}

// ---- launches ----

// workgroups of the direct association (k_associate_direct / k_assoc_prep): one per two association blocks (every thread
// takes two consecutive pixels)
static inline uint32_t assoc_wgs(const sm_ctx *s)
{
    return (uint32_t)(s->n_pix_blocks + 1) / 2u;
}

// the one launch site of each held-back step (HeldBack: who holds them back, who takes them)
int launch_fixup(sm_ctx *s, const FrameParams &fp, const FixArgs &x)
{
    hipLaunchKernelGGL(k_pass_fixup, dim3(x.n_crew + 1), dim3(256), 0, s->stream, s->M, s->d_state, fp, x);
    HIPCK(hipGetLastError());
    return SM_OK;
}

int launch_assoc(sm_ctx *s, const AssocArgs &a, uint32_t stage)
{
    hipLaunchKernelGGL((k_associate_direct<false>), dim3(assoc_wgs(s)), dim3(PIX_BLOCK), 0, s->stream, a, ShardArgs{});
    HIPCK(hipGetLastError());
    check_alive(s, stage + 16u * (uint32_t)(s->tick & 0xFFFF));
    return SM_OK;
}

int launch_settle(sm_ctx *s, const ShardSettle &ss)
{
    hipLaunchKernelGGL(k_shard_settle, dim3(ss.n), dim3(PIX_BLOCK), 0, s->stream, ss);
    HIPCK(hipGetLastError());
    return SM_OK;
}

// The held-back work in the order it must complete.  `all` = false stops after the association: what a frame that cannot carry
// the previous frame's association needs (its statistics are still completed by this frame's fixup publisher).
int complete_held(sm_ctx *s, bool all)
{
    FixArgs *fx;
    if (const AssocArgs *a = s->held.take_assoc(fx)) {
        // two-launch frame: that frame's fixup step has not run either -- in a launch of its own, first (the association's
        // slow_conf_sub is null as fill_assoc_args left it: nothing to wait for)
        if (fx && launch_fixup(s, a->fp, *fx)) return SM_E_HIP;
        if (launch_assoc(s, *a, 3u)) return SM_E_HIP;
    }
    if (!all) return SM_OK;
    // a sharded frame whose settle step has not run yet: stand-alone, before anything reads its results
    if (const ShardSettle *ss = s->held.take_settle()) if (launch_settle(s, *ss)) return SM_E_HIP;
    if (uint32_t *nf = s->held.take_stats()) {
        hipLaunchKernelGGL(k_frame_finalize, dim3(1), dim3(256), 0, s->stream, s->d_state, nf, s->part.fix_cur(), s->part.n_fix, s->d_log);
        HIPCK(hipGetLastError());
    }
    return SM_OK;
}

// The preparation launch: the image planes, and besides them
//   tile_flags: the frame's tile skip flags for the one-pass surfel kernel (a frame whose cull only marks the dead)
//   carry:      the held-back association (and fixup) of the previous frame, if there is one
//   chain:      the frame runs the depth pre-processing chain p0a..p0e (preprocess = 1): the launch is k_assoc_prep<true>, whose
//               image workgroups are chain tiles (prep_chain_block) -- with or without an association to carry
// Returns the number of flag workgroups the launch ran (0: none asked for), < 0 on error.
int launch_prep(sm_ctx *s, const uint8_t *rgb, const uint16_t *raw, const uint8_t *sem, const FrameParams &fp, bool clear_keys,
                bool tile_flags = false, bool carry = false, const ChainArgs *chain = nullptr)
{
    const int tiles = ((s->W + 31) / 32) * ((s->H + 31) / 32);
    // the frame's tile skip flags for the one-pass surfel kernel: a few extra workgroups (128 tiles each per round)
    TilePrep tp{};
    const uint64_t ntl = s->slots.tiles();
    const FrameSet &f = s->cur();
    if (clear_keys && tile_flags) {
        tp.nfb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((ntl + 1023) / 1024, 1), 64);     // one tile per thread (k_prep: 1 024 threads)
        tp.st = s->d_state; tp.tb = s->d_tb; tp.tile_flags = f.tile_flags; tp.wave_cnt = f.wave_cnt; tp.prep_part = f.prep_part;
    }
    FixArgs *fxp = nullptr;
    AssocArgs *carried = carry ? s->held.take_assoc(fxp) : nullptr;
    s->tl.frame().merged = carried || chain;
    uint32_t *conf_sub = clear_keys ? f.conf_sub : nullptr;      // a frame's preparation (clear_keys) also zeroes that frame's conflict sub-counters
    if (carried || chain) {
        // the held-back association of the previous frame (if any) + this frame's tile flags + its image / chain tiles in one launch
        // (a sharded stream's settle step rides on k_prep only: stand-alone here)
        if (const ShardSettle *ss = chain ? s->held.take_settle() : nullptr) if (launch_settle(s, *ss)) return SM_E_HIP;
        static const AssocArgs none{};          // nothing carried: the launch has no association workgroups
        const AssocArgs &a = carried ? *carried : none;
        if (tp.nfb) {
            tp.nfb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((ntl + 255) / 256, 1), 128);     // one tile per thread
            if (carried) { tp.grp_cand = a.grp_cand; tp.n_grp = a.n_grp; tp.prev_time = a.fp.time; }
        }
        // two-launch frame: the held-back association's frame has not had its fixup step yet -- its publisher and repair crew
        // open this launch, the association and the flag workgroups check for themselves whether they have to wait for them
        const FixArgs fx = fxp ? *fxp : FixArgs{};
        const uint32_t n_fix = fxp ? 1u + fx.n_crew : 0u;
        if (fxp) {
            carried->slow_conf_sub = fx.conf_sub; carried->slow_need = n_fix;
            if (tp.nfb) { tp.slow_conf_sub = fx.conf_sub; tp.slow_cap = a.fp.conflict_cap; tp.slow_need = n_fix; tp.slow_par = a.fp.par; }
        }
        PrepArgs pa;
        pa.rgb = rgb; pa.depth_raw = raw; pa.sem = sem; pa.depth_f32 = nullptr; pa.depthT = f.depthT; pa.rgbsT = f.rgbsT;
        pa.keyT = clear_keys ? s->keyT() : nullptr; pa.dcT = f.dcT;
        pa.conf_sub = conf_sub;
        const uint32_t n_assoc = carried ? assoc_wgs(s) : 0u;
        const ChainArgs ca = chain ? *chain : ChainArgs{};
        const uint32_t n_img = chain ? (uint32_t)(((s->W + CH_TX - 1) / CH_TX) * ((s->H + CH_TY - 1) / CH_TY)) : (uint32_t)tiles;
        if (s->d_ap_trace) { s->ap_trace_n[0] = (int)n_assoc; s->ap_trace_n[1] = (int)tp.nfb; s->ap_trace_n[2] = (int)n_img; s->ap_trace_n[3] = (int)n_fix; }    // (chain: dispatched image | association | flags; the fixup workgroups before them)
        const dim3 grid(n_fix + tp.nfb + n_assoc + n_img);
        const auto assoc_prep = chain ? k_assoc_prep<true> : k_assoc_prep<false>;
        hipLaunchKernelGGL(assoc_prep, grid, dim3(PIX_BLOCK), 0, s->stream, a, pa, fp, tp, n_assoc, n_img, ca, fx, n_fix, s->d_ap_trace);
        HIPCK(hipGetLastError());
        return (int)tp.nfb;
    }
    // the previous frame of a sharded stream is finished by extra workgroups of this launch
    const ShardSettle *held = s->held.take_settle();
    const ShardSettle ss = held ? *held : ShardSettle{};
    hipLaunchKernelGGL(k_prep, dim3(tiles + tp.nfb + (ss.n + 3u) / 4u), dim3(1024), 0, s->stream, rgb, raw, sem, (const float *)nullptr, f.depthT, f.rgbsT,
                       clear_keys ? s->keyT() : nullptr, fp, f.dcT, conf_sub, tp, ss);
    HIPCK(hipGetLastError());
    return (int)tp.nfb;
}

// p2: the conflict test alone (masks, per-tile counts, per-workgroup partial sums); nothing of the model changes
int launch_conflict_test(sm_ctx *s, const FrameParams &fp, bool timed = false)
{
    if (finalize_if_pending(s)) return SM_E_HIP;
    s->n_conf_part = (uint32_t)grid_surfels(s);
    hipLaunchKernelGGL(k_conflict, dim3(s->n_conf_part), dim3(256), 0, s->stream, s->M, s->d_state, fp, s->cur().dcT,
                       s->d_cm, s->d_dm, s->d_zm, s->d_tile_cnt, s->d_tb, s->cur().tile_flags, s->d_conf_part, s->d_alive,
                       s->cur().conf_sub);
    HIPCK(hipGetLastError());
    if (s->tl.mark(s->stream, 2, timed)) return SM_E_HIP;
    return SM_OK;
}

// the scan / finalize step of a cull that does not fold it into the cull kernel: applies the conflict cap of `fp`
int launch_conflict_finalize(sm_ctx *s, const FrameParams &fp, bool timed = false)
{
    if (fp.compact_now) {
        // this cull compacts: the survivor prefixes are needed, scan them with one workgroup per 1024 tiles.
        // A cull that only marks the dead gets its totals from k_conflict's partial sums in the finalize kernel.
        const int ngroups = std::max<int>(1, (int)((s->slots.tiles() + GROUP - 1) / GROUP));
        hipLaunchKernelGGL(k_scan_cull, dim3(ngroups), dim3(1024), 0, s->stream, s->d_state, s->d_tile_cnt, s->d_tile_allow,
                           s->d_tile_keep, s->d_group_tot, s->d_tile_dead, 0u, 0u);
        HIPCK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_cull_finalize, dim3(1), dim3(1024), 0, s->stream, s->d_state, fp, s->d_cm, s->d_dm, s->d_zm,
                       s->d_tile_cnt, s->d_tile_allow, s->d_tile_keep, s->d_group_tot, s->d_group_base, s->d_conf_part, s->n_conf_part,
                       s->d_alive, s->d_tile_dead, s->d_stat);
    HIPCK(hipGetLastError());
    if (s->tl.mark(s->stream, 3, timed)) return SM_E_HIP;
    return SM_OK;
}

int launch_conflict(sm_ctx *s, const FrameParams &fp, bool timed = false)
{
    int rc = launch_conflict_test(s, fp, timed);
    if (rc) return rc;
    return launch_conflict_finalize(s, fp, timed);
}

struct PassGrid { int split, grid, fix_workers; };

// Grid policy of k_surfel_pass and its fixup step, from an ESTIMATE of the occupied slots (SlotSchedule::estimate_slots), not from
// the host's bound, which after a hundred unsynchronised frames is the capacity.
// `two`: two-launch frame, `direct`: the frame appends directly.
PassGrid pass_grid_policy(sm_ctx *s, bool two, bool direct)
{
    // Grid: up to 2 048 workgroups while the model is small (most tiles are skipped by their flags; a wide grid spreads the few
    // hundred tiles with work), but no more than are RESIDENT once every workgroup has many tiles with work (>= 4 per
    // workgroup: beyond ~8 M slots) -- the surplus would start when the first ones finish and run a second, thin wave
    // (20 M scattered surfels: 160 us with 2 048 workgroups, 140 with 1 536 = 6 per CU, 152 with 5, 172 with 7)
    const uint64_t tiles_b = s->slots.tiles_of(s->slots.estimate_slots());
    // (8 192 / 16 384 / never on 100 and 200 KITTI frames: 38.7 / 38.4 / 38.5 us per frame -- the two forms are level there, and a
    //  scattered model pays 1.5x for quarter tiles at 20 M surfels: the lower threshold stays)
    const bool persistent = tiles_b > (uint64_t)(4 * MAX_GRID);
    // Quarter-tile units (k_surfel_pass<4>: four workgroups per tile sequence) while tiles are few and some of them dense; whole
    // tiles once every workgroup owns many (the scattered 20 M-surfel model: ~50 listed slots per tile, batches of 8 tiles)
    PassGrid g;
    g.split = s->sw.pass_split == 1 || s->sw.pass_split == 4 ? s->sw.pass_split : persistent ? 1 : 4;
    g.grid = persistent ? std::min(grid_surfels(s), s->pass_grid) : grid_surfels(s);
    if (g.split == 4) {
        // (all of them resident: 2 048 workgroups were 17.5 us where 1 536 are 14.1 -- the last quarter started when the first left)
        const int max_seq = 3 * MAX_GRID / 16;       // 384 sequences = 1 536 workgroups, six per CU
        g.grid = 4 * (int)std::min<uint64_t>(std::max<uint64_t>(s->slots.tiles(), 1), (uint64_t)max_seq);
    }
    // fixup workers: the cap repair strides over the tiles; with direct append they first count the frame's candidate pixels, one group each
    g.fix_workers = two ? (int)sm_ctx::N_CREW
                  : direct ? std::max(std::min(g.grid, s->fix_grid), (int)std::min<uint32_t>(s->n_grp, MAX_GRID)) : std::min(g.grid, s->fix_grid);
    return g;
}

// conflict test + cull (marks only) + splat in ONE pass over the surfels, then the publisher / cap fixup kernel.
// direct: the frame appends directly (k_associate_direct follows): the pass also counts the candidate pixels, the fixup
// publishes their group prefixes and the new count.  n_prep: the flag workgroups the frame's preparation launch ran.
// squeezed: a squeeze ran ahead of the pass and has taken the marks 2..4 (Timeline::Flags): the pass ends at the association's mark 5.
int launch_surfel_pass(sm_ctx *s, const FrameParams &fp, bool timed, bool direct, uint32_t n_prep, bool squeezed = false)
{
    if (n_prep == 0) { g_err = "internal: one-pass frame without tile flags from the preparation launch"; return SM_E_ARG; }
    // two-launch frame: the association will be held back, and the fixup step with it (launch_prep carries both); the candidate
    // pixels are counted by extra workgroups of the pass's own launch
    const bool two = s->sw.two_launch && s->defer_ok && timed && direct;
    const PassGrid g = pass_grid_policy(s, two, direct);
    const int grid = g.grid;
    PassPartials &pp = s->part;
    const uint32_t n_fix_prev = pp.n_fix;
    const uint2 *fix_prev = pp.fix_cur();
    pp.fix_set ^= 1;
    s->n_conf_part = (uint32_t)grid;
    pp.n_compact = (uint32_t)grid;
    pp.pass_live = true;
    pp.n_fix = (uint32_t)g.fix_workers;
    const FrameSet &f = s->cur();
    uint32_t *sub = f.conf_sub;
    const uint32_t tile_bound = (uint32_t)std::max<uint64_t>(s->slots.tiles(), 1);
    if (s->d_pass_trace) s->pass_trace_grid = grid;
    CandArgs ca{};
    ca.n_pass = (uint32_t)grid;
    if (two) {
        ca.n_grp = s->n_grp; ca.cg = s->cand_group; ca.n_pix_blocks = s->n_pix_blocks;
        ca.depthT = f.depthT; ca.xs = s->d_xs; ca.ys = s->d_ys; ca.blk_cand = s->d_blk_cand; ca.grp_cand = s->d_grp_cand;
    }
    const auto pass = g.split == 4 ? k_surfel_pass<4> : k_surfel_pass<1>;
    hipLaunchKernelGGL(pass, dim3(grid + (two ? (int)s->n_grp : 0)), dim3(256), 0, s->stream, s->M, s->d_state, fp, f.dcT, s->d_cm, s->d_dm /* km */,
                       f.wave_cnt, s->d_tb, f.tile_flags, pp.d_lazy, s->d_alive, s->d_tile_dead, sub, s->keyT(), s->d_undo, tile_bound,
                       s->d_frame_sub, ca, s->d_pass_trace);
    HIPCK(hipGetLastError());
    if (!squeezed && (s->tl.mark(s->stream, 2, timed) || s->tl.mark(s->stream, 3, timed))) return SM_E_HIP;
    FixArgs x{};
    DirectArgs &da = x.da;
    da.on = direct ? (two ? 2 : 1) : 0;
    da.blk_cand = s->d_blk_cand; da.grp_cand = s->d_grp_cand; da.n_grp = s->n_grp; da.cg = s->cand_group; da.n_pix_blocks = s->n_pix_blocks;
    da.depthT = f.depthT; da.xs = s->d_xs; da.ys = s->d_ys;
    da.frame_sub = s->d_frame_sub;
    // the previous frame's new / fused counters (its association may run next to this publisher)
    da.nf_prev = s->prev().nf_sub;
    // (the previous frame's fixup partials: only if it appended directly and nothing has completed its statistics since;
    //  the fixup's publisher completes the previous frame's statistics first)
    da.fix_prev = fix_prev; da.n_fix_prev = s->held.take_stats() ? n_fix_prev : 0u;
    da.log = s->d_log;
    x.cm = s->d_cm; x.km = s->d_dm; x.wave_cnt = f.wave_cnt; x.tile_flags = f.tile_flags; x.part = pp.d_lazy; x.n_part = (uint32_t)grid;
    x.fix_part = pp.fix_cur(); x.alive = s->d_alive; x.tile_dead = s->d_tile_dead; x.conf_sub = sub; x.keyT = s->keyT(); x.undo = s->d_undo;
    x.host_stat = s->d_stat; x.prep_part = f.prep_part; x.n_prep = n_prep; x.tb = s->d_tb; x.n_crew = (uint32_t)g.fix_workers;
    if (two) s->held.hold_fixup(x);
    else if (launch_fixup(s, fp, x)) return SM_E_HIP;
    if (!squeezed && s->tl.mark(s->stream, 4, timed)) return SM_E_HIP;
    check_alive(s, 1u + 16u * (uint32_t)(s->tick & 0xFFFF));
    return SM_OK;
}

void fill_assoc_args(const sm_ctx *s, const FrameParams &fp, AssocArgs &a)
{
    a.M = s->M; a.st = s->d_state; a.fp = fp;
    const FrameSet &f = s->cur();
    a.depthT = f.depthT; a.rgbsT = f.rgbsT; a.keyT = s->keyT(); a.xs = s->d_xs; a.ys = s->d_ys;
    a.blk_cand = s->d_blk_cand; a.grp_cand = s->d_grp_cand; a.nf = f.nf_sub; a.tb = s->d_tb;
    a.alive = s->d_alive; a.tile_dead = s->d_tile_dead; a.n_grp = s->n_grp; a.cg = s->cand_group; a.host_stat = s->d_stat;
    a.slow_conf_sub = nullptr; a.slow_need = 0u;
}

// association + in-place fuse + direct append (the frame's last kernel; its statistics are completed later)
int launch_associate_direct(sm_ctx *s, const FrameParams &fp, bool timed)
{
    AssocArgs a;
    fill_assoc_args(s, fp, a);
    s->tl.frame().deferred = s->defer_ok;
    // asynchronous plain stream: hold the association back; the next frame's preparation launch carries it (k_assoc_prep),
    // anything else that needs its results launches it first (finalize_if_pending)
    if (s->defer_ok && timed) s->held.hold_assoc(a);
    else if (launch_assoc(s, a, 2u)) return SM_E_HIP;
    s->part.clear();
    s->held.hold_stats(s->cur().nf_sub);
    s->slots.append_enqueued();
    if (s->tl.mark(s->stream, 5, timed) || s->tl.mark(s->stream, 6, timed) || s->tl.mark(s->stream, 7, timed)) return SM_E_HIP;
    return SM_OK;
}

int launch_compact(sm_ctx *s, const FrameParams &fp, bool splat, bool timed)
{
    s->part.clear();
    if (!fp.compact_now) {
        // deferred compaction: the cull only marks the dead -- lean kernel, no co-residency requirement
        if (splat) { g_err = "internal: a frame's cull that only marks the dead is k_surfel_pass"; return SM_E_ARG; }
        const int grid = grid_surfels(s);
        s->part.n_compact = 0u;
        hipLaunchKernelGGL(k_cull_lazy, dim3(grid), dim3(256), 0, s->stream, s->M, s->d_state, fp, s->d_cm, s->d_dm, s->d_zm,
                           s->d_tile_cnt, s->d_tile_allow, s->d_alive, s->d_tile_dead);
        HIPCK(hipGetLastError());
        if (s->tl.mark(s->stream, 4, timed)) return SM_E_HIP;
        return SM_OK;
    }
    const int grid = std::min(grid_surfels(s), s->compact_grid);
    const uint32_t epoch = s->slots.next_cull_epoch();
    // (a maintenance compaction -- ensure_compact -- kills nothing and draws nothing: what the next append folds stays as it is)
    if (!fp.maintenance) s->part.n_compact = splat ? (uint32_t)grid : 0u;
    FrameParams fpc = fp;
    fpc.compact_tickets = compaction_needs_tickets(s) ? 1 : 0;
    const auto compact = splat ? k_compact<true> : k_compact<false>;
    hipLaunchKernelGGL(compact, dim3(grid), dim3(256), 0, s->stream, s->M, s->d_state, fpc, s->d_cm,
                       s->d_dm, s->d_zm, s->d_tile_cnt, s->d_tile_allow, s->d_tile_keep, s->keyT(), s->d_tile_flag, epoch,
                       s->d_group_base, s->d_tb, s->cur().tile_flags, s->part.d_compact, s->d_alive, s->d_tile_dead);
    HIPCK(hipGetLastError());
    if (s->tl.mark(s->stream, 4, timed)) return SM_E_HIP;
    return SM_OK;
}

// after a cull that is not followed by the append kernel (which does this itself): restore the alive mask
int launch_post_fill(sm_ctx *s)
{
    hipLaunchKernelGGL(k_post_fill, dim3(1024), dim3(256), 0, s->stream, s->d_state, s->d_alive, s->d_tile_dead);
    HIPCK(hipGetLastError());
    check_alive(s, 4u + 16u * (uint32_t)(s->tick & 0xFFFF));
    return SM_OK;
}

int ss_compact(sm_ctx *s);

int launch_associate_only(sm_ctx *s, const FrameParams &fp)
{
    hipLaunchKernelGGL(k_associate, dim3(s->n_pix_blocks), dim3(PIX_BLOCK), 0, s->stream, s->M, s->d_state, fp,
                       s->cur().depthT, s->cur().rgbsT, s->keyT(), s->d_xs, s->d_ys, s->d_validmask, s->d_fusedmask, s->d_blk_cnt, s->d_tb);
    HIPCK(hipGetLastError());
    return SM_OK;
}

// association + in-place fuse, then the dense ordered append (frames that compact; the frame after reset(); the per-pass API,
// whose sm_sync pulls the exact bound right after)
int launch_associate(sm_ctx *s, const FrameParams &fp, bool timed)
{
    int rc = launch_associate_only(s, fp);
    if (rc) return rc;
    if (s->tl.mark(s->stream, 5, timed) || s->tl.mark(s->stream, 6, timed)) return SM_E_HIP;
    // the append derives its own prefix from the per-block counts (no scan kernel)
    const PassPartials::Fold f = s->part.fold();
    hipLaunchKernelGGL(k_append_scan, dim3(s->n_pix_blocks), dim3(PIX_BLOCK), 0, s->stream, s->M, s->d_state, fp, s->cur().depthT,
                       s->cur().rgbsT, s->d_xs, s->d_ys, s->d_validmask, s->d_fusedmask, s->d_blk_cnt, s->d_log, s->d_tb, f.compact,
                       f.n_compact, s->d_alive, s->d_tile_dead, s->d_stat, f.lazy, f.fix, f.n_fix);
    s->part.clear();
    s->slots.append_enqueued();
    HIPCK(hipGetLastError());
    if (s->tl.mark(s->stream, 7, timed)) return SM_E_HIP;
    check_alive(s, 5u + 16u * (uint32_t)(s->tick & 0xFFFF));
    return SM_OK;
}

// The kill-nothing compaction (enqueue only): k_scan_cull -> k_cull_finalize -> k_compact<false> over the dead counts and alive words
// alone -- no conflict masks exist and none are read.  Nothing of the last frame may be held back or pending (the caller completes it).
//   in_frame: between the two launches of a frame -- k_compact itself restores the alive words and resets the skip flags of the
//             tiles it rewrites; the key map has just been cleared, no id is outstanding.  Otherwise the caller launches k_post_fill,
//             and the key map's slot numbers are translated here.
//   tail:     the squeeze may start at the first dense tile and leave the few dead slots below it (TAIL_DEAD_THRESH); otherwise
//             it starts at the first dead slot and leaves none.
int launch_squeeze(sm_ctx *s, bool in_frame, bool tail, bool timed)
{
    FrameParams fp = make_params(s, s->curr_pose);
    fp.maintenance = in_frame ? 2 : 1;
    fp.compact_now = 1;
    fp.conflict_cap = 0xFFFFFFFFu;
    fp.no_masks = 1;
    fp.tail_thresh = tail ? s->sw.tail_thresh : 0u;
    const uint64_t tiles = s->slots.tiles() + 1;
    const int ngroups = std::max<int>(1, (int)((tiles + GROUP - 1) / GROUP));
    hipLaunchKernelGGL(k_scan_cull, dim3(ngroups), dim3(1024), 0, s->stream, s->d_state, s->d_tile_cnt, s->d_tile_allow,
                       s->d_tile_keep, s->d_group_tot, s->d_tile_dead, 1u, fp.tail_thresh);
    hipLaunchKernelGGL(k_cull_finalize, dim3(1), dim3(1024), 0, s->stream, s->d_state, fp, s->d_cm, s->d_dm, s->d_zm,
                       s->d_tile_cnt, s->d_tile_allow, s->d_tile_keep, s->d_group_tot, s->d_group_base, s->d_conf_part, 0u,
                       s->d_alive, s->d_tile_dead, s->d_stat);
    if (!in_frame && s->slots.keys_are_slots())     // ids of the index map: slot -> position among the live surfels, as the API hands them out
        hipLaunchKernelGGL(k_remap_keys, dim3((s->P + 255) / 256), dim3(256), 0, s->stream, s->d_state, s->keyT(), s->P, s->d_alive,
                           s->d_tile_keep, s->d_group_base);
    HIPCK(hipGetLastError());
    if (s->tl.mark(s->stream, 2, timed) || s->tl.mark(s->stream, 3, timed)) return SM_E_HIP;
    return launch_compact(s, fp, false, timed);
}

// empty the model on the device (reset path; synchronises)
int discard_model(sm_ctx *s)
{
    int rc = pull_state(s);
    if (rc) return rc;
    if (s->h_state->count == 0 && !s->slots.maybe_garbage() && s->h_state->conflict_count == 0 && s->h_state->visible_count == 0) return SM_OK;
    if (s->slots.maybe_garbage()) {
        HIPCK(hipMemsetAsync(s->d_alive, 0xFF, s->alive_words * 8, s->stream));
        HIPCK(hipMemsetAsync(s->d_tile_dead, 0, s->dead_tiles * 4, s->stream));
        s->slots.model_discarded();
    }
    s->h_state->conflict_count = 0; s->h_state->visible_count = 0;      // no conflict pass, no index map in the initialising frame
    return publish_dense(s, 0, 0);
}

// tail of processFrame (src/SurfelMapping.cpp:244-248)
void end_frame(sm_ctx *s, bool timed = true)
{
    if (s->cfg.preprocess) std::swap(s->d_lastT, s->d_filteredT);   // :244 LAST <- DEPTH_FILTERED without a copy
    memcpy(s->last_pose, s->curr_pose, 64);               // :245 (LAST aliases the metric depth when preprocess == 0)
    s->tl.end_frame(timed);
    s->tick++;
}

// First half of SurfelMapping::processFrame once the textures are on the device
// (src/SurfelMapping.cpp:130-169): pre-processing and the reference-frame early-out.
// `tile_flags`, `carry`: as launch_prep takes them; *n_prep: the flag workgroups it ran.
// Returns 1 when the fusing passes must follow, 0 when the call ends here, <0 on error.
int begin_frame(sm_ctx *s, const uint8_t *d_rgb, const uint16_t *d_raw, const uint8_t *d_sem, const float *pose, bool tile_flags, bool carry,
                FrameParams *fp_out, uint32_t *n_prep)
{
    if (s->pending_cull) { g_err = "sm_stage_conflict without sm_stage_cull"; return SM_E_ARG; }
    memcpy(s->curr_pose, pose, 64);
    s->trk.note_pose(pose);                               // the tracker's constant-velocity history (sm_track_frame)
    FrameParams fp = make_params(s, pose);
    const bool fusing = s->ref_set && s->tick != 0;
    int rc;
    if ((rc = s->tl.mark(s->stream, 8, fusing))) return rc;    // back-to-back pair 8 -> 0: the cost of an event record itself
    if ((rc = s->tl.mark(s->stream, 0, fusing))) return rc;
    // The reference frame and the frame after reset() do not draw the index map: its textures keep what the last
    // predictIndices left (src/SurfelMapping.cpp:142-169), so the key map is neither cleared nor exchanged then.
    const bool will_splat = fusing;
    // frame parity: the frame takes the other FrameSet, so that the pre-processing of frame f+1 never touches what frame f still
    // reads; the key map follows on the frames that draw it
    s->plane_set ^= 1;
    fp.par = s->plane_set;
    if (s->defer_ok && will_splat) s->key_set ^= 1;
    // metriciseDepth + filterDepth + removeMovings (src/SurfelMapping.cpp:136-139,156,254-365): with preprocess = 1 the whole
    // chain is one stage of the preparation launch (prep_chain_block); the reference frame stops before removeMovings
    ChainArgs ca{};
    if (s->cfg.preprocess) {
        ca.lastT = s->d_lastT; ca.filteredT = s->d_filteredT; memcpy(ca.w, s->h_wtab, sizeof ca.w);
        ca.border = (int)std::ceil(s->cfg.stereo_border - 0.5f);
        ca.do_movings = s->ref_set ? 1 : 0;
        if (s->ref_set) {                                 // src/SurfelMapping.cpp:345-349
            float linv[16];
            invert4(s->last_pose, linv);
            mul4(linv, s->curr_pose, ca.t_c2l.m);
        }
    }
    if ((rc = launch_prep(s, d_rgb, d_raw, d_sem, fp, will_splat, tile_flags, carry, s->cfg.preprocess ? &ca : nullptr)) < 0) return rc;
    *n_prep = (uint32_t)rc;
    // preprocess == 0: DEPTH_FILTERED and LAST are the metric depth itself (nothing reads them on the
    // hot path); they alias the frame's depthT in sm_download_depth instead of being copied every frame.
    if (!s->ref_set) {                                    // src/SurfelMapping.cpp:142-154
        if (s->cfg.preprocess) std::swap(s->d_lastT, s->d_filteredT);   // LAST <- DEPTH_FILTERED without a copy
        memcpy(s->last_pose, s->curr_pose, 64);
        s->ref_set = true;
        s->tick++;
        return 0;
    }
    if ((rc = s->tl.mark(s->stream, 1, fusing))) return rc;
    s->raw_valid = true;                                  // computeFeedbackBuffers (src/SurfelMapping.cpp:164,172): on demand here
    s->raw_tick = s->tick;
    if (s->tick == 0) {
        // after reset(): computeFeedbackBuffers + GlobalModel::initialize + buildModelMap
        // (src/SurfelMapping.cpp:161-169): the raw cloud of this frame becomes the model
        fp.init_mode = 1;
        fp.log_frame = 0;
        // GlobalModel::initialize writes the raw cloud from the first slot of modelVbo on and sets count to the number written
        // (src/GlobalModel.cpp:211-228): a map that was
        // uploaded after reset() is discarded, not extended
        if ((rc = discard_model(s))) return rc;
        s->part.clear();
        s->part.n_compact = 0;                            // no cull / splat ran: nothing to fold into visible_count
        if ((rc = launch_associate(s, fp, false))) return rc;
        end_frame(s, false);
        return 0;
    }
    fp.splat_follows = 1;
    fp.log_frame = 1;
    *fp_out = fp;
    return 1;
}

// the plain frame forms on a sharded context: refused (before a form that does not wait takes the caller's images as current)
int refuse_sharded(const sm_ctx *s)
{
    if (s->ss_on) { g_err = "context is configured for sharding: use the sm_shard_* entry points"; return SM_E_ARG; }
    return SM_OK;
}

// SurfelMapping::processFrame body (src/SurfelMapping.cpp:130-251); enqueue only.
int enqueue_frame(sm_ctx *s, const uint8_t *d_rgb, const uint16_t *d_raw, const uint8_t *d_sem, const float *pose)
{
    if (int rc = refuse_sharded(s)) return rc;
    FrameParams fp;
    // the cull's kind is decided first: a frame whose cull only marks the dead lets k_prep evaluate the tile skip flags for
    // the one-pass surfel kernel
    const bool fusing = s->ref_set && s->tick != 0 && !s->pending_cull;
    using Due = sm_slots::SlotSchedule::Due;
    const Due due = fusing ? s->slots.decide_due() : Due::forced;
    const bool compact_now = due != Due::none;
    // Tail squeeze: a compaction only the period asked for, on an asynchronous plain stream, keeps the frame's regular form --
    // the slots that are dead ALREADY are squeezed out between the preparation launch and the pass; this frame's own victims
    // wait for the next one like every other frame's.  (A forced compaction must leave no dead slot and append densely: the
    // compacting frame.)
    const bool squeeze = fusing && due == Due::period && s->sw.tail_squeeze && s->defer_ok;
    // a held-back association rides on this frame's k_prep launch if this is again a fusing frame; anything else (the frame
    // after reset, ...) needs its results first
    // (a compacting frame too: its k_prep launch has no tile flags to make; the doubled words of DevState a merged publisher
    //  leaves set are cleared by k_cull_finalize there, by the next pass's launch otherwise)
    const bool carry = fusing && s->defer_ok;
    int rc = SM_OK;
    uint32_t n_prep = 0;
    if (!carry && (rc = complete_held(s, false))) return rc;
    rc = begin_frame(s, d_rgb, d_raw, d_sem, pose, fusing && (!compact_now || squeeze), carry, &fp, &n_prep);
    if (rc <= 0) return rc;
    fp.compact_now = compact_now && !squeeze ? 1u : 0u;
    if (squeeze) {
        // the preparation launch carried the previous frame's fixup and association; its statistics (the dead-slot total the
        // squeeze starts from) are completed now, not by this frame's publisher
        if ((rc = complete_held(s, true))) return rc;
        if ((rc = launch_squeeze(s, true, true, true))) return rc;
        s->slots.squeezed_in_frame();
    } else
        s->slots.cull_noted(fp.compact_now != 0u);
    s->slots.keys_drawn(fp.compact_now == 0u);      // this frame's splat writes slot numbers iff nothing moves
    // a cull that only marks the dead is ONE pass over the surfels (k_surfel_pass + k_pass_fixup: conflict test, decrement, cull,
    // splat), and the association appends the new surfels directly (no append kernel)
    const bool one_pass = !fp.compact_now;
    Timeline::Flags &fl = s->tl.frame();
    fl.compacted = !one_pass || squeeze; fl.one_pass = fl.direct = one_pass; fl.squeezed = squeeze;
    if (one_pass) {
        if ((rc = launch_surfel_pass(s, fp, true, true, n_prep, squeeze))) return rc;        // :178-197
        if ((rc = launch_associate_direct(s, fp, true))) return rc;         // :212-239
        end_frame(s);
        return SM_OK;
    }
    if ((rc = launch_conflict(s, fp, true))) return rc;           // :178-187
    if ((rc = launch_compact(s, fp, true, true))) return rc;      // :189-197 (cull + mirror + index map)
    if ((rc = launch_associate(s, fp, true))) return rc;   // :212-239
    end_frame(s);
    return SM_OK;
}

// ---- the current depth and class image (sm_ctx::cur_depth / cur_sem): one owner for every entry point ----
// "this image was given, here": a non-null image becomes current; `slot` is the async input set that holds it, -1 for
// d_depth_raw / d_sem and for a buffer of the caller's (borrowed: see sm_process_frame_device in the header)
void image_given(sm_ctx *s, const uint16_t *d_depth, const uint8_t *d_sem, int slot)
{
    if (d_depth) { s->cur_depth = d_depth; s->in_depth_slot = slot; }
    if (d_sem) { s->cur_sem = d_sem; s->in_sem_slot = slot; }
}

// "which image is current": what a null image reads (the zeroed staging planes until one has been given)
const uint16_t *current_depth(const sm_ctx *s) { return s->cur_depth ? s->cur_depth : s->d_depth_raw.get(); }
const uint8_t *current_sem(const sm_ctx *s) { return s->cur_sem ? s->cur_sem : s->d_sem.get(); }

// A frame that was enqueued without waiting read the current images: an input set that holds one of them (other than the
// frame's own, `own`) is busy until that frame has prepared too -- sm_process_frame_async waits for ev_free before it refills a set
int hold_current_sets(sm_ctx *s, int own)
{
    for (int o : {s->in_depth_slot, s->in_sem_slot})
        if (o >= 0 && o != own) { HIPCK(hipEventRecord(s->in[o].ev_free, s->stream)); s->in[o].used = true; }
    return SM_OK;
}

// host images of a form that waits: into the staging planes, on the context's stream (so a frame enqueued earlier that reads
// them as the current images has its preparation launch ahead of the copy), and current from here on
int upload_inputs(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth, const uint8_t *sem)
{
    const size_t P = (size_t)s->P;
    hipStream_t st = s->stream;
    if (rgb) HIPCK(hipMemcpyAsync(s->d_rgb, rgb, P * 3, hipMemcpyHostToDevice, st));
    if (depth) HIPCK(hipMemcpyAsync(s->d_depth_raw, depth, P * 2, hipMemcpyHostToDevice, st));
    if (sem) HIPCK(hipMemcpyAsync(s->d_sem, sem, P, hipMemcpyHostToDevice, st));
    image_given(s, depth ? s->d_depth_raw.get() : nullptr, sem ? s->d_sem.get() : nullptr, -1);
    return SM_OK;
}

// one FrameSet's buffers (s->frame_mem owns them): the planes and the skip flags zeroed
int alloc_frame_set(sm_ctx *s, FrameSet &f)
{
    auto get = [s](auto *&p, size_t n, bool zero) -> int {
        Dev<void> m;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof *p;
        HIPCK(hipMalloc(m.put(), bytes));
        if (zero) HIPCK(hipMemset(m, 0, bytes));
        p = static_cast<std::remove_reference_t<decltype(p)>>(m.get());
        s->frame_mem.push_back(std::move(m));
        return SM_OK;
    };
    const size_t P = (size_t)s->P;
    return get(f.depthT, P, true) || get(f.rgbsT, P, true) || get(f.dcT, P, true) || get(f.tile_flags, s->tb_tiles, true) ||
           get(f.wave_cnt, s->dead_tiles, false) || get(f.prep_part, 256, false) ? SM_E_HIP : SM_OK;
}

// sm_create's buffers in order, up to the first failure (g_err is set only where dalloc failed)
int alloc_ctx(sm_ctx *s)
{
    const size_t P = (size_t)s->P, cap = s->cap, nwords = s->alive_words, ntiles = s->dead_tiles, tb = s->tb_tiles;
    if (hipStreamCreateWithFlags(s->stream.put(), hipStreamNonBlocking) != hipSuccess ||
        alloc_set(s->m_bufs[0], cap) ||      // one SoA set: the compaction is in place
        dalloc(s->d_state, 1) || dalloc(s->d_log, FRAME_LOG_LEN) || hipHostMalloc(s->h_state.put(), sizeof(DevState), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(s->h_stat.put(), 8, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer((void **)&s->d_stat, s->h_stat, 0) != hipSuccess ||
        dalloc(s->d_filteredT, P) || dalloc(s->d_lastT, P) ||
        // what alternates between frames: twice where a frame's association is held back, else both frames see the one set
        alloc_frame_set(s, s->fset[0]) || dalloc(s->d_key[0], P) ||
        (s->defer_ok && (alloc_frame_set(s, s->fset[1]) || dalloc(s->d_key[1], P))) ||
        dalloc(s->d_rgb, P * 3) || dalloc(s->d_sem, P) || dalloc(s->d_depth_raw, P) || dalloc(s->d_depth_f32, P) ||
        dalloc(s->d_xs, (size_t)s->W * 2) || dalloc(s->d_ys, (size_t)s->H * 2) ||
        dalloc(s->d_cm, nwords) || dalloc(s->d_dm, nwords) || dalloc(s->d_zm, nwords) ||
        dalloc(s->d_alive, nwords) || hipMemset(s->d_alive, 0xFF, nwords * 8) != hipSuccess ||
        dalloc(s->d_tile_dead, ntiles) || hipMemset(s->d_tile_dead, 0, ntiles * 4) != hipSuccess ||
        dalloc(s->d_tile_cnt, ntiles * 3) || dalloc(s->d_tile_allow, ntiles) || dalloc(s->d_tile_keep, ntiles) || dalloc(s->d_tile_flag, ntiles) ||
        hipMemset(s->d_tile_flag, 0, ntiles * 4) != hipSuccess ||
        dalloc(s->d_group_tot, (ntiles / GROUP + 2) * 4) || dalloc(s->d_group_base, ntiles / GROUP + 2) ||
        dalloc(s->d_conf_part, (size_t)MAX_GRID * 4) || dalloc(s->part.d_compact, (size_t)MAX_GRID) || dalloc(s->part.d_lazy, (size_t)MAX_GRID) ||
        dalloc(s->part.d_fix, (size_t)MAX_GRID * 2 + 2) || dalloc(s->d_undo, cap + TILE) ||
        dalloc(s->d_conf_sub, (size_t)2 * SUB_SET) || hipMemset(s->d_conf_sub, 0, (size_t)2 * SUB_SET * 4) != hipSuccess ||
        dalloc(s->d_tb, tb * 8) ||
        dalloc(s->d_validmask, (P + 63) / 64 + 4) || dalloc(s->d_fusedmask, (P + 63) / 64 + 4) || dalloc(s->d_blk_cnt, (size_t)s->n_pix_blocks) ||
        dalloc(s->d_blk_cand, (size_t)s->n_grp * CAND_GROUP_MAX) || dalloc(s->d_grp_cand, (size_t)s->n_grp) ||
        dalloc(s->d_frame_sub, (size_t)6 * SUB_SET) || hipMemset(s->d_frame_sub, 0, (size_t)6 * SUB_SET * 4) != hipSuccess)
        return SM_E_HIP;
    s->M.s[0] = s->m_bufs[0].view();
    *s->h_stat = 0ull;
    for (int i = 0; i < 2; ++i) { s->fset[i].nf_sub = s->d_frame_sub + (2 + 2 * i) * SUB_SET; s->fset[i].conf_sub = s->d_conf_sub + i * SUB_SET; }
    if (!s->defer_ok) s->alias_frame_sets();
    return SM_OK;
}

}  // namespace

// ---- helpers the other sources call (declared in sm_ctx.h) ----

// general 4x4 inverse, column-major, cofactor expansion, inv = adj * (1/det), fp32
// (the role of Eigen::Matrix4f::inverse() at src/GlobalModel.cpp:419, src/IndexMap.cpp:157)
void sm_impl::invert4(const float *m, float *out)
{
    float a[16];
    a[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] +
           m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    a[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] -
           m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    a[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] +
           m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    a[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] -
            m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    a[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] -
           m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    a[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] +
           m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    a[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] -
           m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    a[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] +
            m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    a[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] +
           m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    a[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] -
           m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    a[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] +
            m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    a[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] -
            m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    a[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] -
           m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    a[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] +
           m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    a[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] -
            m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    a[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] +
            m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const float det = m[0] * a[0] + m[1] * a[4] + m[2] * a[8] + m[3] * a[12];
    const float rdet = 1.0f / det;
    for (int i = 0; i < 16; ++i) out[i] = a[i] * rdet;
}

FrameParams sm_impl::make_params(const sm_ctx *s, const float *pose)
{
    FrameParams fp;
    memset(&fp, 0, sizeof fp);
    memcpy(fp.pose, pose, 64);
    invert4(pose, fp.t_inv);
    const sm_config &c = s->cfg;
    fp.fx = c.fx; fp.fy = c.fy; fp.cx = c.cx; fp.cy = c.cy;
    fp.inv_fx = (float)(1.0 / (double)c.fx);
    fp.inv_fy = (float)(1.0 / (double)c.fy);
    fp.cols = (float)c.width; fp.rows = (float)c.height;
    fp.W = c.width; fp.H = c.height; fp.P = s->P;
    fp.min_depth = c.near_clip; fp.max_depth = c.far_clip;
    fp.conflict_thresh = c.fuse_thresh;
    fp.fuse_thresh = c.fuse_thresh;
    fp.stereo_border = c.stereo_border;
    fp.is_clean = 0;
    fp.time = s->tick;
    fp.time_delta = c.time_delta;
    fp.depth_cutoff = c.far_clip;
    fp.conflict_cap = c.conflict_cap ? (uint32_t)s->P : 0xFFFFFFFFu;
    fp.max_vertices = s->cap;
    fp.init_mode = 0;
    fp.inv_fx_fb = 1.0f / c.fx;
    fp.inv_fy_fb = 1.0f / c.fy;
    fp.use_bounds = c.disable_tile_bounds ? 0 : 1;
    fp.compact_now = 1;                     // the per-pass entry points compact at every cull
    fp.maintenance = 0;
    fp.par = s->plane_set;
    return fp;
}

int sm_impl::push_state(sm_ctx *s)
{
    HIPCK(hipMemcpyAsync(s->d_state, s->h_state, sizeof(DevState), hipMemcpyHostToDevice, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    s->slots.state_pushed(s->h_state->stat_frames, s->h_state->count);      // the pinned statistic follows what the host wrote
    return SM_OK;
}

// a direct-append frame leaves its new / fused totals, the dead-slot total and its log entry to be completed by the next
// frame's fixup publisher, and a deferring context its association (and fixup) to the next frame's preparation launch:
// everything else that reads their results asks for the completion first
int sm_impl::finalize_if_pending(sm_ctx *s)
{
    return complete_held(s, true);
}

int sm_impl::pull_state(sm_ctx *s)
{
    int rcf = finalize_if_pending(s);
    if (rcf) return rcf;
    HIPCK(hipMemcpyAsync(s->h_state, s->d_state, sizeof(DevState), hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    const DevState &d = *s->h_state;
    s->counts.count = s->pending_cull ? s->count_before_cull : d.count - d.garbage;   // dead slots are not surfels
    s->counts.offset = d.offset - (d.garbage - d.holes_last);   // (empty slots of fused candidates lie above `offset`)
    s->counts.data_count = d.data_count;
    s->counts.conflict_count = d.conflict_count;
    s->counts.unstable_count = d.unstable_count;
    s->counts.fused_count = d.fused_count;
    s->counts.visible_count = d.visible_count;
    s->counts.tick = s->tick;
    s->slots.state_pulled(d.count, d.cull_n, s->pending_cull);
    return SM_OK;
}

// Physical compaction outside a frame: every entry point that exposes slots as surfel ids (downloads, the per-pass
// API, rendering, sharding, uploads) first squeezes out the slots that deferred culls left dead.  Nothing is killed:
// empty conflict masks, then the regular scan + in-place compaction, with the key map's ids translated on the way.
int sm_impl::ensure_compact(sm_ctx *s)
{
    if (finalize_if_pending(s)) return SM_E_HIP;
    if (s->ss_on) {
        // slot-addressed sharding: a rank's arrays always hold the (dead) slots of the other ranks' surfels; the compaction is
        // a collective step, so every rank must be making this same call
        int rc = ss_compact(s);
        if (rc) return rc;
        HIPCK(hipStreamSynchronize(s->stream));
        return SM_OK;
    }
    if (!s->slots.maybe_garbage()) return SM_OK;
    if (s->pending_cull) { g_err = "internal: deferred compaction with a pending per-pass cull"; return SM_E_ARG; }
    int rc = launch_squeeze(s, false, false, false);     // always full and dense: ids are positions among the live surfels
    if (rc) return rc;
    if ((rc = launch_post_fill(s))) return rc;
    s->slots.compacted_outside_frame();
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

// rebuild the bounds of every tile that holds a surfel with index >= first_surfel (after the model was written
// from outside the frame pipeline); the state on the device must already carry the new count
int sm_impl::rebuild_bounds(sm_ctx *s, uint32_t first_surfel, uint32_t count)
{
    const uint32_t t0 = first_surfel / TILE;
    if (t0 < s->tb_tiles) {
        const uint32_t n = s->tb_tiles - t0;
        hipLaunchKernelGGL(k_tile_bounds_reset, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->d_tb, t0, n);
        HIPCK(hipGetLastError());
    }
    const uint32_t k0 = t0 * TILE;
    if (count > k0) {
        hipLaunchKernelGGL(k_tile_bounds_build, dim3((count - k0 + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, s->d_tb, k0);
        HIPCK(hipGetLastError());
    }
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

int sm_impl::publish_dense(sm_ctx *s, uint32_t count, uint32_t first_new)
{
    DevState &d = *s->h_state;
    d.count = count;                             // src/GlobalModel.cpp:995
    d.offset = count;
    d.garbage = 0; d.garbage_prev = 0; d.first_live = 0; d.do_compact = 0;
    s->slots.published_dense();
    int rc = push_state(s);
    if (rc) return rc;
    if ((rc = rebuild_bounds(s, first_new, count))) return rc;
    return pull_state(s);
}

int sm_impl::ensure_export(sm_ctx *s, size_t bytes)
{
    s->rm.scratch_reused();
    if (bytes <= s->export_bytes) return SM_OK;
    s->export_bytes = 0;
    HIPCK(hipMalloc(s->d_export.put(), bytes));
    s->export_bytes = bytes;
    return SM_OK;
}

void sm_impl::fill_keys(sm_ctx *s, uint64_t *key, size_t n)
{
    hipLaunchKernelGGL(k_fill_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, key, (int)n);
}

// SurfelMapping::cleanPoints with the view already in device memory (sm_clean_points_ex uploads it; sm_rig_consolidate
// takes it from the gathered views of the rig).  `cap_hook`, if given, runs between the conflict test (which changes nothing)
// and the cull: it receives this model's conflict count and returns the number of them that may take effect, in surfel order
// (src/GlobalModel.cpp:54-57: conflictVbo holds W*H records) -- a rig slice learns its share of the union's W*H there -- or a
// negative error code, which abandons the cull with the model untouched.
int sm_impl::clean_points_device(sm_ctx *s, const uint16_t *d_depth_mm, const uint8_t *d_semantic, const float *pose16, int exempt_first,
                                 const std::function<long long(uint32_t)> *cap_hook)
{
    if (s->pending_cull) { g_err = "sm_stage_conflict without sm_stage_cull"; return SM_E_ARG; }
    // cleanPoints culls without redrawing the index map (src/SurfelMapping.cpp:496-532): the map keeps ids of the model
    // as it was, so they are settled (slot -> position) before this cull changes the positions
    int rc = ensure_compact(s);
    if (rc) return rc;
    memcpy(s->curr_pose, pose16, 64);
    FrameParams fp = make_params(s, pose16);
    if ((rc = launch_prep(s, s->d_rgb, d_depth_mm, d_semantic, fp, false)) < 0) return rc;   // metriciseDepth only
    fp.max_depth = s->cfg.far_clip - 15.0f;     // src/SurfelMapping.cpp:515
    fp.conflict_thresh = 0.1f;                  // :516
    fp.is_clean = 1;                            // :517
    fp.no_exempt = exempt_first ? 0 : 1;
    fp.compact_now = s->slots.decide_compact() ? 1u : 0u;
    if ((rc = launch_conflict_test(s, fp))) return rc;
    if (cap_hook) {
        std::vector<uint32_t> part((size_t)s->n_conf_part * 4);
        HIPCK(hipMemcpyAsync(part.data(), s->d_conf_part, part.size() * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        uint64_t local = 0;
        for (uint32_t b = 0; b < s->n_conf_part; ++b) local += part[(size_t)b * 4 + 1];
        const long long allow = (*cap_hook)((uint32_t)local);
        if (allow < 0) return (int)allow;
        fp.conflict_cap = (uint32_t)std::min<long long>(allow, 0xFFFFFFFFll);
    }
    s->slots.cull_noted(fp.compact_now != 0u);
    if ((rc = launch_conflict_finalize(s, fp))) return rc;
    if ((rc = launch_compact(s, fp, false, false))) return rc;
    if ((rc = launch_post_fill(s))) return rc;
    return sm_sync(s);
}

// =============================================================================================
extern "C" {

int sm_api_version(void) { return SM_API_VERSION; }

const char *sm_last_error(void) { return g_err.c_str(); }

int sm_default_config(sm_config *c, int width, int height, float fx, float fy, float cx, float cy)
{
    if (!c) return SM_E_ARG;
    memset(c, 0, sizeof *c);
    c->width = width; c->height = height;
    c->fx = fx; c->fy = fy; c->cx = cx; c->cy = cy;
    c->near_clip = 1.0f;
    c->far_clip = 30.0f;
    c->fuse_thresh = 0.0f;
    c->max_sqrt_vertices = 5000;
    c->time_delta = 200;
    c->stereo_border = 80.0f;
    c->preprocess = 1;
    c->conflict_cap = 1;
    c->device = 0;
    c->enable_timing = 0;
    c->compact_period = 24;
    return SM_OK;
}

sm_ctx *sm_create(const sm_config *c)
{
    if (!c || c->width <= 0 || c->height <= 0 || c->max_sqrt_vertices <= 0 || c->compact_period < 0 ||
        (uint64_t)c->width * c->height > (1u << 30) || (uint64_t)c->max_sqrt_vertices * c->max_sqrt_vertices > 0x7FFFFFFFull) {
        g_err = "sm_create: bad config";
        return nullptr;
    }
    if (hip_runtime_conflict("sm_create")) return nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || c->device >= ndev) {
        g_err = "sm_create: no HIP device visible (this library has no CPU fallback)";
        return nullptr;
    }
    if (hipSetDevice(c->device) != hipSuccess) { g_err = "hipSetDevice failed"; return nullptr; }
    std::unique_ptr<sm_ctx> s(new sm_ctx());
    s->cfg = *c;
    s->W = c->width; s->H = c->height; s->P = c->width * c->height;
    s->in_off_depth = ((size_t)s->P * 3 + 15) & ~(size_t)15;
    s->in_off_sem = s->in_off_depth + (((size_t)s->P * 2 + 15) & ~(size_t)15);
    s->in_bytes = s->in_off_sem + (size_t)s->P;
    s->cap = (uint32_t)c->max_sqrt_vertices * (uint32_t)c->max_sqrt_vertices;
    for (int i = 0; i < 16; ++i) s->curr_pose[i] = s->last_pose[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    const size_t P = (size_t)s->P, cap = s->cap;
    const size_t nwords = (cap + 63) / 64 + TILE_WORDS, ntiles = (cap + TILE - 1) / TILE + 1;
    s->n_pix_blocks = (s->P + PIX_BLOCK - 1) / PIX_BLOCK;
    s->alive_words = nwords; s->dead_tiles = ntiles;
    s->tb_tiles = (uint32_t)(ntiles + P / 2 / TILE + 8);
    s->sw = read_switches();
    s->defer_ok = s->sw.defer_assoc;       // deferred association (three launches per frame; with or without the depth filter chain)
    // candidate groups: small groups make the counting workgroups short (k_pass_fixup 3.5 -> 2.5 us at 1242x375 with 4
    // instead of 16 blocks per group) but every association wave sums all groups before its own: keep ~250-500 groups
    s->cand_group = s->n_pix_blocks <= 2048 ? 4u : s->n_pix_blocks <= 4096 ? 8u : 16u;
    s->n_grp = (uint32_t)((s->n_pix_blocks + s->cand_group - 1) / s->cand_group);
    if (alloc_ctx(s.get())) { if (g_err.empty()) g_err = "sm_create: allocation failed"; return nullptr; }

    // pixel-centre coordinates exactly as data.vert sees them:
    // texcoord = float((i+0.5)/(double)(float)W) (src/GlobalModel.cpp:71-72), x = texcoord*cols (data.vert:62-63)
    std::vector<float> xs(s->W * 2), ys(s->H * 2);   // [0,W): data.vert coordinates; [W,2W): FeedbackBuffer's (src/FeedbackBuffer.cpp:47-53)
    const float cols = (float)s->W, rows = (float)s->H;
    const float px = 1.0f / cols, py = 1.0f / rows;
    bool clamp_ok = true;
    auto tex = [](float t, int n) { float f = std::floor(t * (float)n); if (!(f >= 0.0f)) return 0; if (f > (float)(n - 1)) return n - 1; return (int)f; };
    uint32_t odd = 0;
    for (int i = 0; i < s->W; ++i) {
        const float tc = (float)((i + 0.5) / (double)cols);
        xs[i] = tc * cols;
        xs[s->W + i] = (float)((double)((float)i / cols) + 1.0 / (double)(2.0f * cols)) * cols;
        clamp_ok = clamp_ok && (int)xs[s->W + i] == i;
        clamp_ok = clamp_ok && tex(tc, s->W) == i && tex(tc - px, s->W) == std::max(i - 1, 0) &&
                   tex(tc + px, s->W) == std::min(i + 1, s->W - 1) && (int)xs[i] == i;
    }
    for (int j = 0; j < s->H; ++j) {
        const float tc = (float)((j + 0.5) / (double)rows);
        ys[j] = tc * rows;
        ys[s->H + j] = (float)((double)((float)j / rows) + 1.0 / (double)(2.0f * rows)) * rows;
        clamp_ok = clamp_ok && (int)ys[s->H + j] == j;
        clamp_ok = clamp_ok && tex(tc, s->H) == j && tex(tc - py, s->H) == std::max(j - 1, 0) &&
                   tex(tc + py, s->H) == std::min(j + 1, s->H - 1) && (int)ys[j] == j;
    }
    if (!clamp_ok) {   // the kernels index neighbours as i+-1 / j+-1; refuse sizes where fp32 texcoords disagree
        g_err = "sm_create: texel addressing for this image size is not the simple clamp form";
        return nullptr;
    }
    for (int i = 0; i < s->W; ++i) odd += (uint32_t)((s->H + ((i & 1) ? 1 : 0)) / 2);
    s->slots = sm_slots::SlotSchedule(TILE, s->cap, odd, c->compact_period, s->sw.capacity_wait_us, s->h_stat.get());      // a frame's candidate pixels: the most it can append
    // depth_smooth.frag weights: the host passes 0.5/30^2 as "sigPix" (src/SurfelMapping.cpp:292-309)
    float *wtab = s->h_wtab;
    {
        const float sigma_intensity = 30.0f;
        const float sigPix = 0.5f / (sigma_intensity * sigma_intensity);
        for (int iy = -6; iy <= 6; ++iy)
            for (int ix = -6; ix <= 6; ++ix)
                wtab[(iy + 6) * 13 + (ix + 6)] = exp_spec(-((float)(ix * ix + iy * iy) * sigPix));
    }
    memset(s->h_state, 0, sizeof(DevState));
    bool ok = hipMemcpy(s->d_xs, xs.data(), xs.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(s->d_ys, ys.data(), ys.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(s->d_state, s->h_state, sizeof(DevState), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(s->d_filteredT, 0, P * 4) == hipSuccess && hipMemset(s->d_lastT, 0, P * 4) == hipSuccess &&
         hipMemset(s->d_rgb, 0, P * 3) == hipSuccess && hipMemset(s->d_sem, 0, P) == hipSuccess &&
         hipMemset(s->d_depth_raw, 0, P * 2) == hipSuccess && hipMemset(s->d_depth_f32, 0, P * 4) == hipSuccess &&
         hipDeviceSynchronize() == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_tile_bounds_reset, dim3((s->tb_tiles + 255) / 256), dim3(256), 0, s->stream, s->d_tb, 0u, s->tb_tiles);
        fill_keys(s.get(), s->keyT(), s->P);
        ok = hipStreamSynchronize(s->stream) == hipSuccess;
    }
    if (!ok) { g_err = "sm_create: device initialisation failed"; return nullptr; }
    if (s->sw.check_alive && (hipMalloc(s->d_chk.put(), 32) != hipSuccess || hipMemset(s->d_chk, 0, 32) != hipSuccess)) s->d_chk = {};
    if (s->sw.trace) { (void)hipMalloc(s->d_pass_trace.put(), (size_t)MAX_GRID * 64); (void)hipMalloc(s->d_ap_trace.put(), (size_t)65536 * 16); }
    resident_grids(s->sw, c->device, &s->pass_grid, &s->compact_grid);
    if (c->enable_timing) {                                       // all or nothing: without the whole ring the context runs untimed
        std::unique_ptr<Event[][EV_RING]> ev(new Event[N_EV][EV_RING]);
        bool made = true;
        for (int k = 0; k < N_EV && made; ++k)
            for (int i = 0; i < EV_RING && made; ++i) made = hipEventCreate(ev[k][i].put()) == hipSuccess;
        if (made) s->tl.ev = std::move(ev);
    }
    if (c->device >= 0 && c->device < MAX_DEV) { std::lock_guard<std::mutex> lk(g_compact_mu); g_ctx_on_dev[c->device]++; }
    return s.release();
}

void sm_destroy(sm_ctx *s)
{
    if (!s) return;
    if (s->cfg.device >= 0 && s->cfg.device < MAX_DEV) { std::lock_guard<std::mutex> lk(g_compact_mu); g_ctx_on_dev[s->cfg.device]--; }
    (void)hipSetDevice(s->cfg.device);         // every owner releases on the context's device
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->ss_comm) (void)sm_shard_rccl_finalize(s);         // a communicator the caller did not finalize
    if (s->stream_in) (void)hipStreamSynchronize(s->stream_in);
    if (s->d_pass_trace) {
        // SM_PASS_TRACE=<prefix>: the last k_surfel_pass launch's per-workgroup record (wall_clock64 at entry / first tile /
        // after it / exit, that tile, its compacted entries, XCC | HW_ID, tiles) -> <prefix>.<n>.bin (tools/pass_trace.py)
        static std::atomic<int> n_dump{0};
        std::vector<unsigned long long> h((size_t)std::max(s->pass_trace_grid, 0) * 8);
        if (!h.empty() && hipMemcpy(h.data(), s->d_pass_trace, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            char path[512];
            snprintf(path, sizeof path, "%s.%d.bin", s->sw.trace_prefix.c_str(), n_dump++);
            if (FILE *f = fopen(path, "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
        }
    }
    if (s->d_ap_trace) {
        const int n = s->ap_trace_n[0] + s->ap_trace_n[1] + s->ap_trace_n[2] + s->ap_trace_n[3];
        std::vector<unsigned long long> h((size_t)std::max(std::min(n, 65536), 0) * 2 + 3);
        if (n > 0 && hipMemcpy(h.data() + 3, s->d_ap_trace, (h.size() - 3) * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            h[0] = (unsigned long long)s->ap_trace_n[0] | ((unsigned long long)s->ap_trace_n[3] << 32); h[1] = (unsigned long long)s->ap_trace_n[1]; h[2] = (unsigned long long)s->ap_trace_n[2];
            char path[512];
            snprintf(path, sizeof path, "%s.assoc_prep.bin", s->sw.trace_prefix.c_str());
            if (FILE *f = fopen(path, "wb")) { fwrite(h.data(), 8, h.size(), f); fclose(f); }
        }
    }
    delete s;
}

int sm_sync(sm_ctx *s)
{
    if (!s) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = pull_state(s);
    if (rc) return rc;
    if (s->d_chk) {
        uint32_t h[8] = {0};
        HIPCK(hipMemcpy(h, s->d_chk, sizeof h, hipMemcpyDeviceToHost));
        if (h[0]) {
            fprintf(stderr, "SM_CHECK_ALIVE: %u tiles violate occupied - dead == live bits; first seen: stage %u (frame tick %u), tile %u, live bits %u, occupied - dead %u, slots %u\n",
                    h[0], h[1] & 15u, h[1] >> 4, h[2], h[3], h[4], h[5]);
            HIPCK(hipMemset(s->d_chk, 0, sizeof h));
        }
    }
    return take_error(s);
}

int sm_process_frame_device(sm_ctx *s, const uint8_t *d_rgb, const uint16_t *d_depth_mm, const uint8_t *d_semantic,
                            const float *pose16)
{
    if (!s || !d_rgb || !pose16) { g_err = "sm_process_frame_device: null argument"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (int rc = refuse_sharded(s)) return rc;
    // a null depth / semantic keeps the previous texture (src/SurfelMapping.cpp:124-128); one given is current from here on,
    // in the caller's buffer
    image_given(s, d_depth_mm, d_semantic, -1);
    int rc = enqueue_frame(s, d_rgb, current_depth(s), current_sem(s), pose16);
    const int rh = hold_current_sets(s, -1);
    if (!rc) rc = rh;
    return rc ? rc : auto_retire_after_frame(s);
}

int sm_process_frame(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16)
{
    if (!s || !rgb || !pose16) { g_err = "sm_process_frame: null argument (rgb and pose are required)"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = upload_inputs(s, rgb, depth_mm, semantic);
    if (rc) return rc;
    rc = enqueue_frame(s, s->d_rgb, current_depth(s), current_sem(s), pose16);     // (an input set it reads is free again: the call waits)
    if (rc) return rc;
    rc = sm_sync(s);                     // (a sticky SM_E_CAPACITY of this frame is still reported when the policy retires after it)
    const int rr = auto_retire_after_frame(s);
    return rc ? rc : rr;
}

void *sm_host_alloc(sm_ctx *s, size_t bytes)
{
    if (!s || !bytes) return nullptr;
    if (hipSetDevice(s->cfg.device) != hipSuccess) return nullptr;
    Host<unsigned char> p;
    if (hipHostMalloc(p.put(), bytes, hipHostMallocDefault) != hipSuccess) { g_err = "sm_host_alloc: hipHostMalloc failed"; return nullptr; }
    s->pinned.emplace_back(std::move(p), bytes);
    return s->pinned.back().first;
}

int sm_host_alloc_frame(sm_ctx *s, uint8_t **rgb, uint16_t **depth_mm, uint8_t **semantic)
{
    if (!s || !rgb || !depth_mm || !semantic) { g_err = "sm_host_alloc_frame: null argument"; return SM_E_ARG; }
    unsigned char *blk = static_cast<unsigned char *>(sm_host_alloc(s, s->in_bytes));
    if (!blk) return SM_E_HIP;
    *rgb = blk; *depth_mm = reinterpret_cast<uint16_t *>(blk + s->in_off_depth); *semantic = blk + s->in_off_sem;
    return SM_OK;
}

int sm_host_free(sm_ctx *s, void *p)
{
    if (!s || !p) return SM_E_ARG;
    auto it = std::find_if(s->pinned.begin(), s->pinned.end(), [p](const auto &b) { return b.first == p; });
    if (it == s->pinned.end()) { g_err = "sm_host_free: not a buffer of sm_host_alloc"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (s->stream_in) HIPCK(hipStreamSynchronize(s->stream_in));
    (void)it->first.release();
    s->pinned.erase(it);
    HIPCK(hipHostFree(p));
    return SM_OK;
}

int sm_process_frame_async(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16)
{
    if (!s || !rgb || !pose16) { g_err = "sm_process_frame_async: null argument (rgb and pose are required)"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (int rc = refuse_sharded(s)) return rc;
    const size_t P = (size_t)s->P;
    if (!s->stream_in) {                  // the copy stream and the ring, built whole before the context takes them
        Stream st;
        sm_ctx::InSlot ring[sm_ctx::IN_RING];
        HIPCK(hipStreamCreateWithFlags(st.put(), hipStreamNonBlocking));
        for (auto &sl : ring) {
            HIPCK(hipMalloc(sl.rgb.put(), s->in_bytes));
            sl.depth = reinterpret_cast<uint16_t *>(sl.rgb + s->in_off_depth); sl.sem = sl.rgb + s->in_off_sem;
            HIPCK(hipEventCreateWithFlags(sl.ev_in.put(), hipEventDisableTiming));
            HIPCK(hipEventCreateWithFlags(sl.ev_free.put(), hipEventDisableTiming));
        }
        std::move(std::begin(ring), std::end(ring), s->in);
        s->stream_in = std::move(st);
    }
    const int slot = (int)(s->in_next++ % sm_ctx::IN_RING);
    sm_ctx::InSlot &sl = s->in[slot];
    // the set is free again when the frame that used it last has run its preparation launch (the only reader of the images).
    // The HOST waits for that (three frames back: normally long past) rather than only the copy stream: it bounds the copies and
    // frames in flight.  With the host free to run ahead, hipMemcpyAsync stalled for 7-12 ms every few dozen frames (2 k instead
    // of 16 k frames/s) -- measured with registered and with hipHostMalloc'ed sources alike.
    if (sl.used) HIPCK(hipEventSynchronize(sl.ev_free));
    auto is_pinned = [&](const void *ptr, size_t n) {
        const unsigned char *q = static_cast<const unsigned char *>(ptr);
        for (auto &pr : s->pinned) if (q >= pr.first && q + n <= pr.first + pr.second) return true;
        return false;
    };
    const unsigned char *rgb_b = rgb, *dep_b = reinterpret_cast<const unsigned char *>(depth_mm);
    int rc = SM_OK;
    if (depth_mm && semantic && dep_b == rgb_b + s->in_off_depth && semantic == rgb_b + s->in_off_sem && is_pinned(rgb, s->in_bytes)) {
        // a frame block of sm_host_alloc_frame: ONE copy
        HIPCK(hipMemcpyAsync(sl.rgb, rgb, s->in_bytes, hipMemcpyHostToDevice, s->stream_in));
    } else if (!is_pinned(rgb, P * 3) || (depth_mm && !is_pinned(depth_mm, P * 2)) || (semantic && !is_pinned(semantic, P))) {
        // pageable caller memory: through this set's pinned staging in the frame-block layout (host memcpys; the previous copy out
        // of it -- three frames ago -- must have completed), then ONE copy of what was given
        if (!sl.h_stage) HIPCK(hipHostMalloc(sl.h_stage.put(), s->in_bytes, hipHostMallocDefault));
        if (sl.used) HIPCK(hipEventSynchronize(sl.ev_in));
        memcpy(sl.h_stage, rgb, P * 3);
        if (depth_mm) memcpy(sl.h_stage + s->in_off_depth, depth_mm, P * 2);
        if (semantic) memcpy(sl.h_stage + s->in_off_sem, semantic, P);
        if (depth_mm && semantic) HIPCK(hipMemcpyAsync(sl.rgb, sl.h_stage, s->in_bytes, hipMemcpyHostToDevice, s->stream_in));
        else {
            HIPCK(hipMemcpyAsync(sl.rgb, sl.h_stage, P * 3, hipMemcpyHostToDevice, s->stream_in));
            if (depth_mm) HIPCK(hipMemcpyAsync(sl.depth, sl.h_stage + s->in_off_depth, P * 2, hipMemcpyHostToDevice, s->stream_in));
            if (semantic) HIPCK(hipMemcpyAsync(sl.sem, sl.h_stage + s->in_off_sem, P, hipMemcpyHostToDevice, s->stream_in));
        }
    } else {
        // separate pinned buffers (sm_host_alloc): copied from in place, one after the other
        HIPCK(hipMemcpyAsync(sl.rgb, rgb, P * 3, hipMemcpyHostToDevice, s->stream_in));
        if (depth_mm) HIPCK(hipMemcpyAsync(sl.depth, depth_mm, P * 2, hipMemcpyHostToDevice, s->stream_in));
        if (semantic) HIPCK(hipMemcpyAsync(sl.sem, semantic, P, hipMemcpyHostToDevice, s->stream_in));
    }
    // a null depth / semantic keeps the previous texture (src/SurfelMapping.cpp:124-128)
    image_given(s, depth_mm ? sl.depth : nullptr, semantic ? sl.sem : nullptr, slot);
    HIPCK(hipEventRecord(sl.ev_in, s->stream_in));
    HIPCK(hipStreamWaitEvent(s->stream, sl.ev_in, 0));
    rc = enqueue_frame(s, sl.rgb, current_depth(s), current_sem(s), pose16);
    HIPCK(hipEventRecord(sl.ev_free, s->stream));
    sl.used = true;
    // a frame without its own depth / semantic image read another set's
    const int rh = hold_current_sets(s, slot);
    if (!rc) rc = rh;
    return rc ? rc : auto_retire_after_frame(s);
}

int sm_inputs_consumed(sm_ctx *s)
{
    if (!s) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    if (s->stream_in) HIPCK(hipStreamSynchronize(s->stream_in));
    return SM_OK;
}

int sm_clean_points(sm_ctx *s, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16)
{
    return sm_clean_points_ex(s, depth_mm, semantic, pose16, 1);
}

int sm_clean_points_ex(sm_ctx *s, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16, int exempt_first)
{
    if (!s || !depth_mm || !semantic || !pose16) { g_err = "sm_clean_points: null argument"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (s->pending_cull) { g_err = "sm_stage_conflict without sm_stage_cull"; return SM_E_ARG; }
    int rc = finalize_if_pending(s);             // (a held-back association still reads the staging buffers' frame planes)
    if (rc) return rc;
    if ((rc = upload_inputs(s, nullptr, depth_mm, semantic))) return rc;
    return clean_points_device(s, current_depth(s), current_sem(s), pose16, exempt_first);
}

int sm_clean_points_cb(sm_ctx *s, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16, int exempt_first,
                       sm_cap_fn fn, void *user)
{
    if (!s || !depth_mm || !semantic || !pose16) { g_err = "sm_clean_points: null argument"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (s->pending_cull) { g_err = "sm_stage_conflict without sm_stage_cull"; return SM_E_ARG; }
    int rc = finalize_if_pending(s);
    if (rc) return rc;
    if ((rc = upload_inputs(s, nullptr, depth_mm, semantic))) return rc;
    if (!fn) return clean_points_device(s, current_depth(s), current_sem(s), pose16, exempt_first);
    const std::function<long long(uint32_t)> hook = [&](uint32_t local) { return fn(user, local); };
    return clean_points_device(s, current_depth(s), current_sem(s), pose16, exempt_first, &hook);
}

int sm_reset(sm_ctx *s)
{
    if (!s) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    // the index map survives reset() (the reference only resets the model buffer, src/SurfelMapping.cpp:436-441): bring
    // its ids to the form the API hands out (positions among the live surfels) while the slots can still be translated
    int rc = s->pending_cull ? SM_OK : ensure_compact(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;
    const uint32_t cur = s->h_state->cur;
    memset(s->h_state, 0, sizeof(DevState));
    s->h_state->cur = cur;
    s->tick = 0;                                 // refFrameIsSet stays (src/SurfelMapping.cpp:436-441)
    s->pending_cull = false;
    place_reset(s);                              // the keyframes index a map that is gone
    if ((rc = push_state(s))) return rc;
    if ((rc = rebuild_bounds(s, 0, 0))) return rc;
    return pull_state(s);
}

int sm_get_counts(sm_ctx *s, sm_counts *out)
{
    if (!s || !out) return SM_E_ARG;
    *out = s->counts;
    out->tick = s->tick;
    return SM_OK;
}

// ---- per-pass entry points ----

int sm_set_frame(sm_ctx *s, const uint8_t *rgb, const float *depth_metric, const uint8_t *semantic)
{
    if (!s) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = finalize_if_pending(s);             // (a held-back association still reads the planes this call rewrites)
    if (rc) return rc;
    if ((rc = upload_inputs(s, rgb, nullptr, semantic))) return rc;
    if (depth_metric) HIPCK(hipMemcpyAsync(s->d_depth_f32, depth_metric, (size_t)s->P * 4, hipMemcpyHostToDevice, s->stream));
    FrameParams fp = make_params(s, s->curr_pose);
    // re-pack every plane from the staged inputs; depth only when given (else keep depthT)
    const int tiles = ((s->W + 31) / 32) * ((s->H + 31) / 32);
    TilePrep tp;
    memset(&tp, 0, sizeof tp);
    ShardSettle ss;
    memset(&ss, 0, sizeof ss);
    hipLaunchKernelGGL(k_prep, dim3(tiles), dim3(1024), 0, s->stream, s->d_rgb, (const uint16_t *)nullptr, current_sem(s),
                       depth_metric ? s->d_depth_f32 : nullptr, depth_metric ? s->cur().depthT : nullptr, s->cur().rgbsT,
                       (uint64_t *)nullptr, fp, s->cur().dcT, (uint32_t *)nullptr, tp, ss);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

int sm_set_tick(sm_ctx *s, int32_t tick)
{
    if (!s) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = finalize_if_pending(s);
    if (rc) return rc;
    s->tick = tick;
    s->ref_set = true;
    return SM_OK;
}

int sm_stage_conflict(sm_ctx *s, const float *pose16, float min_depth, float max_depth, float fuse_thresh, int is_clean)
{
    if (!s || !pose16) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = s->pending_cull ? SM_OK : ensure_compact(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;
    if (s->pending_cull) {
        // processConflict may be called again before backMapping (it only rewrites conflictVbo,
        // src/GlobalModel.cpp:449-454): re-arm the not yet applied cull.
        s->h_state->count = s->h_state->cull_n;
        s->h_state->cur = s->h_state->cull_src;
        s->h_state->offset = s->offset_before_cull;
        s->pending_cull = false;
        if ((rc = push_state(s))) return rc;
        if ((rc = pull_state(s))) return rc;
    }
    memcpy(s->curr_pose, pose16, 64);
    FrameParams fp = make_params(s, pose16);
    fp.min_depth = min_depth; fp.max_depth = max_depth; fp.conflict_thresh = fuse_thresh; fp.is_clean = is_clean;
    s->count_before_cull = s->h_state->count;
    s->offset_before_cull = s->h_state->offset;
    if ((rc = launch_conflict(s, fp))) return rc;
    s->pending_cull = true;
    return sm_sync(s);
}

int sm_stage_cull(sm_ctx *s)
{
    if (!s) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    if (!s->pending_cull) { g_err = "sm_stage_cull without sm_stage_conflict"; return SM_E_ARG; }
    FrameParams fp = make_params(s, s->curr_pose);
    int rc = launch_compact(s, fp, false, false);
    if (rc) return rc;
    s->pending_cull = false;
    return sm_sync(s);
}

int sm_stage_splat(sm_ctx *s, const float *pose16, int32_t time, float depth_cutoff, int32_t time_delta)
{
    if (!s || !pose16) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    if (s->pending_cull) { g_err = "sm_stage_splat between sm_stage_conflict and sm_stage_cull"; return SM_E_ARG; }
    int rc = ensure_compact(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;
    memcpy(s->curr_pose, pose16, 64);
    FrameParams fp = make_params(s, pose16);
    fp.time = time; fp.depth_cutoff = depth_cutoff; fp.time_delta = time_delta;
    HIPCK(hipMemsetAsync(&s->d_state->visible_count, 0, 4, s->stream));
    s->part.clear();
    s->part.n_compact = 0;                       // k_splat counts with an atomic; no k_compact partials to fold in
    fill_keys(s, s->keyT(), s->P);
    HIPCK(hipGetLastError());
    const int grid = (int)std::min<uint64_t>(std::max<uint64_t>(((uint64_t)s->h_state->count + 255) / 256, 1), MAX_GRID);
    hipLaunchKernelGGL(k_splat, dim3(grid), dim3(256), 0, s->stream, s->M, s->d_state, fp, s->keyT());
    HIPCK(hipGetLastError());
    return sm_sync(s);
}

int sm_stage_associate_fuse(sm_ctx *s, const float *pose16, int32_t time, float depth_min, float depth_max)
{
    if (!s || !pose16) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    if (s->pending_cull) { g_err = "sm_stage_associate_fuse between sm_stage_conflict and sm_stage_cull"; return SM_E_ARG; }
    memcpy(s->curr_pose, pose16, 64);
    FrameParams fp = make_params(s, pose16);
    fp.time = time; fp.min_depth = depth_min; fp.max_depth = depth_max;
    int rc = ensure_compact(s);
    if (rc) return rc;
    if ((rc = launch_associate(s, fp, false))) return rc;
    return sm_sync(s);
}

int sm_stage_timings(sm_ctx *s, sm_timings *out)
{
    if (!s || !out) return SM_E_ARG;
    memset(out, 0, sizeof *out);
    if (!s->tl.ev) { g_err = "sm_stage_timings: create the context with enable_timing=1"; return SM_E_UNSUPPORTED; }
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipStreamSynchronize(s->stream));
    Timeline &tl = s->tl;
    uint64_t first = tl.read;
    if (tl.frames - first > EV_RING) first = tl.frames - EV_RING;
    double seg[7] = {0}, run = 0, ovh = 0, cull[2] = {0, 0};
    double own[6] = {0};          // pass, fixup (one-pass frames) | conflict (others) | associate (direct) | associate, append (others)
    double prep2[2] = {0, 0};     // k_prep alone | k_assoc_prep
    double scan_own = 0;          // k_scan_cull + k_cull_finalize on the frames that ran k_conflict
    uint32_t nfr = 0, ncls[2] = {0, 0}, n_op = 0, n_dir = 0, n_merged = 0, n_alone = 0, n_sq = 0;
    for (uint64_t f = first; f < tl.frames; ++f) {
        const int slot = (int)(f % EV_RING);
        const Timeline::Flags &fl = tl.flags[slot];
        float ms = 0;
        bool ok = true;
        double loc[7];
        for (int k = 0; k < 7 && ok; ++k) {
            ok = hipEventElapsedTime(&ms, tl.ev[k][slot], tl.ev[k + 1][slot]) == hipSuccess;
            loc[k] = ms;
        }
        float o = 0;
        if (!ok || hipEventElapsedTime(&ms, tl.ev[0][slot], tl.ev[7][slot]) != hipSuccess ||
            hipEventElapsedTime(&o, tl.ev[8][slot], tl.ev[0][slot]) != hipSuccess)
            continue;
        for (int k = 0; k < 7; ++k) seg[k] += loc[k];
        cull[fl.compacted ? 1 : 0] += loc[3];
        ncls[fl.compacted ? 1 : 0]++;
        // (a squeezed frame: marks 1..2 k_frame_finalize + scan + finalize -- all three go to the scan figure --, 3..4 k_compact, 4..5
        //  the pass; its fixup and association are held back: it has no fixup segment and stays out of that average)
        if (fl.squeezed) { own[0] += loc[4]; scan_own += loc[1]; n_op++; n_sq++; }
        else if (fl.one_pass) { own[0] += loc[1]; own[1] += loc[3]; n_op++; } else { own[2] += loc[1]; scan_own += loc[2]; }
        if (fl.direct) { n_dir++; if (!fl.deferred) { own[3] += loc[4]; n_alone++; } } else { own[4] += loc[4]; own[5] += loc[6]; }
        prep2[fl.merged ? 1 : 0] += loc[0];
        if (fl.merged) n_merged++;
        run += ms;
        ovh += o;
        nfr++;
    }
    tl.read = tl.frames;
    out->frames = nfr;
    if (nfr) {
        const double inv = 1.0 / nfr;
        // every segment contains one event record; subtract its measured cost (the back-to-back pair) so that the
        // per-kernel figures are launch durations, comparable with rocprofv3's
        const double oh = ovh * inv;
        out->event_overhead = (float)oh;
        for (double &x : seg) x = std::max(0.0, x - oh * nfr);
        out->k_prep = (float)(seg[0] * inv); out->k_conflict = (float)(seg[1] * inv); out->k_scan_cull = (float)(seg[2] * inv);
        out->k_compact = (float)(seg[3] * inv); out->k_associate = (float)(seg[4] * inv); out->k_scan_new = (float)(seg[5] * inv);
        out->k_append = (float)(seg[6] * inv);
        out->k_cull_lazy = ncls[0] ? (float)std::max(0.0, cull[0] / ncls[0] - oh) : 0.0f;
        out->k_compact_own = ncls[1] ? (float)std::max(0.0, cull[1] / ncls[1] - oh) : 0.0f;
        out->frames_compact = ncls[1];
        auto avg = [&](double sum, uint32_t n) { return n ? (float)std::max(0.0, sum / n - oh) : 0.0f; };
        out->k_surfel_pass = avg(own[0], n_op); out->k_pass_fixup = avg(own[1], n_op - n_sq); out->k_conflict_own = avg(own[2], nfr - n_op);
        out->k_scan_own = avg(scan_own, nfr - n_op + n_sq);
        out->k_associate_direct = avg(own[3], n_alone); out->k_associate_own = avg(own[4], nfr - n_dir); out->k_append_own = avg(own[5], nfr - n_dir);
        out->frames_one_pass = n_op; out->frames_direct = n_dir;
        out->k_assoc_prep = avg(prep2[1], n_merged); out->k_prep_own = avg(prep2[0], nfr - n_merged);
        out->frames_merged = n_merged; out->frames_assoc_alone = n_alone;
        out->preprocess = out->k_prep;
        out->conflict = out->k_conflict + out->k_scan_cull + out->k_compact;
        out->index_map = 0.0f;
        out->data_association = out->k_associate;
        out->concatenate = out->k_scan_new + out->k_append;
        out->run = (float)(run * inv);
    }
    return SM_OK;
}

int sm_read_frame_log(sm_ctx *s, sm_frame_log *out, uint32_t n, uint32_t *written)
{
    if (!s || !out || !written) return SM_E_ARG;
    static_assert(sizeof(sm_frame_log) == sizeof(FrameLog), "frame log layout");
    static_assert(SM_FRAME_LOG_LEN == FRAME_LOG_LEN, "frame log length");
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = pull_state(s);
    if (rc) return rc;
    const uint32_t total = s->h_state->frames_logged;
    uint32_t m = std::min(std::min(n, total), (uint32_t)FRAME_LOG_LEN);
    std::vector<FrameLog> ring(FRAME_LOG_LEN);
    HIPCK(hipMemcpy(ring.data(), s->d_log, sizeof(FrameLog) * FRAME_LOG_LEN, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < m; ++k) {
        const uint32_t idx = (total - m + k) % FRAME_LOG_LEN;
        memcpy(&out[k], &ring[idx], sizeof(FrameLog));
    }
    *written = m;
    return SM_OK;
}

int sm_debug_slow_frames(sm_ctx *s, uint32_t *n)
{
    if (!s || !n) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = pull_state(s);
    if (rc) return rc;
    *n = s->h_state->slow_frames;
    return SM_OK;
}

int sm_debug_squeezes(sm_ctx *s, uint32_t *tail, uint32_t *full)
{
    if (!s || !tail || !full) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = pull_state(s);
    if (rc) return rc;
    *tail = s->h_state->sq_tail; *full = s->h_state->sq_full;
    return SM_OK;
}

int sm_gpu_process_count(sm_ctx *s)
{
    if (!s) return SM_E_ARG;
    return kfd_processes_on_gpu(s->cfg.device);
}

}  // extern "C"

// ---- ONE stream sharded over `world` GPUs, in-stream form: slot-addressed, no host in the frame ----------------------
//
// Every rank addresses surfels by the slot number the single-GPU run uses (k_associate_direct: slot = offset + candidate
// pixels before the pixel -- computable on every rank, the frame is replicated) and stores only the segments it owns
// (segment = one frame's new surfels, owner = frame index % world); everywhere else its alive bits are 0, its tile
// bounds empty, so the one-pass surfel kernel runs unchanged and skips what it does not own.  DevState is replicated:
// all ranks publish the same counts.  A frame is  k_prep | k_surfel_pass | k_pass_fixup | all-reduce(min) key map |
// k_associate_direct<shard> | all-reduce(sum) fused mask + 3 counters | k_shard_settle, all on the context's stream.

int sm_impl::ss_collective(sm_ctx *s, const void *send, void *recv, size_t count, int op)
{
    if (!s->ss_coll) {
        if (s->ss_world == 1) {          // one rank and no communicator: reduction and gather are the identity
            if (send != recv) HIPCK(hipMemcpyAsync(recv, send, count * 8, hipMemcpyDeviceToDevice, s->stream));
            return SM_OK;
        }
        g_err = "sharded stream: no collective installed (sm_shard_rccl_init or sm_shard_set_collective)";
        return SM_E_ARG;
    }
    const int rc = s->ss_coll(s->ss_user, send, recv, count, op, s->stream);
    if (rc && g_err.empty()) g_err = "sharded stream: the collective callback failed";
    return rc;
}

namespace {

// Physical compaction between two frames of a sharded stream (k_shard_* in sm_kernels.h); enqueue only.
int ss_compact(sm_ctx *s)
{
    if (finalize_if_pending(s)) return SM_E_HIP;
    const uint64_t nw = ((uint64_t)s->slots.bound() + 63) / 64;
    const uint64_t tiles = s->slots.tiles();
    const int g1 = (int)std::min<uint64_t>(std::max<uint64_t>((nw + 255) / 256, 1), 1024);
    const int gt = (int)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), MAX_GRID);
    hipLaunchKernelGGL(k_shard_alive_copy, dim3(g1), dim3(256), 0, s->stream, s->d_state, s->d_alive, s->d_galive, s->d_new_alive, (uint32_t)nw);
    HIPCK(hipGetLastError());
    int rc = ss_collective(s, s->d_galive, s->d_galive, (size_t)nw, SM_COLL_SUM);
    if (rc) return rc;
    hipLaunchKernelGGL(k_shard_tile_popc, dim3(std::max(1, std::min(gt / 16 + 1, 256))), dim3(256), 0, s->stream, s->d_state, s->d_galive, s->d_tile_keep);
    hipLaunchKernelGGL(k_shard_scan, dim3(1), dim3(1024), 0, s->stream, s->d_state, s->d_tile_keep, s->d_tile_allow, s->d_ss_info, s->d_stat);
    hipLaunchKernelGGL(k_shard_stage, dim3(gt), dim3(256), 0, s->stream, s->M, s->d_state, s->d_alive, s->d_galive, s->d_tile_allow, s->d_ss_info,
                       s->d_new_alive);
    hipLaunchKernelGGL(k_shard_unstage, dim3(gt), dim3(256), 0, s->stream, s->M, s->d_state, s->d_ss_info, s->d_new_alive, s->d_alive,
                       s->d_tile_dead, s->d_tb);
    HIPCK(hipGetLastError());
    s->slots.compacted_sharded();
    s->part.clear();
    return SM_OK;
}

}  // namespace

extern "C" {

int sm_shard_stream_configure(sm_ctx *s, int rank, int world)
{
    if (!s || world < 1 || rank < 0 || rank >= world) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    if (s->ss_on) { g_err = "sm_shard_stream_configure: already configured"; return SM_E_ARG; }
    int rc = pull_state(s);
    if (rc) return rc;
    if (s->h_state->count != 0 || s->slots.maybe_garbage() || s->tick != 0 || s->ref_set) {
        g_err = "sm_shard_stream_configure: the context must be new (no frame, no model)";
        return SM_E_ARG;
    }
    SetBufs set1;                              // staging set of the sharded compaction
    Dev<uint64_t> galive, new_alive, gmask, capx;
    Dev<uint32_t> info;
    if ((rc = alloc_set(set1, s->cap)) || (rc = dalloc(galive, s->alive_words)) || (rc = dalloc(new_alive, s->alive_words)) ||
        (rc = dalloc(gmask, (size_t)(s->P + 63) / 64 + 4)) || (rc = dalloc(info, 4)) ||
        (rc = dalloc(capx, (size_t)1 + (size_t)(2 + TILE_WORDS) * s->dead_tiles)))
        return rc;
    HIPCK(hipMemset(info, 0, 16));
    s->M.s[1] = set1.view();
    s->m_bufs[1] = std::move(set1);
    s->d_galive = std::move(galive); s->d_new_alive = std::move(new_alive); s->d_gmask = std::move(gmask);
    s->d_ss_info = std::move(info); s->d_capx = std::move(capx);
    s->ss_on = true; s->ss_rank = rank; s->ss_world = world; s->ss_frames = 0;
    s->aloop.on = false;                                  // (sm_set_auto_loop: a rank holds only its own surfels)
    s->defer_ok = false;                       // the association of a sharded frame sits between two collectives:
    s->alias_frame_sets();                     // one set of buffers from here on (no frame has run: the first)
    return SM_OK;
}

int sm_shard_set_collective(sm_ctx *s, sm_collective_fn fn, void *user)
{
    if (!s || !(s->ss_on || s->rig_on)) { g_err = "sm_shard_set_collective: call sm_shard_stream_configure or sm_rig_configure first"; return SM_E_ARG; }
    s->ss_coll = fn; s->ss_user = user;
    return SM_OK;
}

int sm_shard_compact(sm_ctx *s)
{
    if (!s || !s->ss_on) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    return ss_compact(s);
}

// SurfelMapping::processFrame for one rank of a sharded stream; images already on the device; enqueue only
int sm_shard_frame_device(sm_ctx *s, const uint8_t *d_rgb, const uint16_t *d_depth_mm, const uint8_t *d_semantic, const float *pose16)
{
    if (!s || !d_rgb || !pose16) { g_err = "sm_shard_frame_device: null argument"; return SM_E_ARG; }
    if (!s->ss_on) { g_err = "sm_shard_frame_device: call sm_shard_stream_configure first"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (s->pending_cull) { g_err = "sm_stage_conflict without sm_stage_cull"; return SM_E_ARG; }
    if (s->ref_set && s->tick == 0) { g_err = "reset() is not supported in sharded mode"; return SM_E_UNSUPPORTED; }
    const bool fusing = s->ref_set && s->tick != 0;
    int rc;
    if (fusing) {
        // The compaction schedule must be the same on every rank: the period counter, and a capacity bound that only uses
        // what all ranks know (after a synchronisation the host's bound is the device's count, identical everywhere).
        bool compact = s->slots.period_due();
        if (!compact && s->slots.bound_may_overflow()) {
            if ((rc = pull_state(s))) return rc;
            compact = s->slots.bound_may_overflow();
        }
        if (compact && s->slots.culls_since_compact() > 0) {
            if ((rc = ss_compact(s))) return rc;
            if (s->slots.bound_may_overflow() && (rc = pull_state(s))) return rc;
        }
    }
    FrameParams fp;
    uint32_t n_prep = 0;
    image_given(s, d_depth_mm, d_semantic, -1);          // the caller's buffers, as in sm_process_frame_device
    rc = begin_frame(s, d_rgb, current_depth(s), current_sem(s), pose16, fusing, false, &fp, &n_prep);
    if (rc >= 0 && hold_current_sets(s, -1)) return SM_E_HIP;
    if (rc <= 0) return rc;
    fp.compact_now = 0u;
    fp.conflict_cap = 0xFFFFFFFFu;            // applied over all ranks below (k_shard_cap_pack / k_shard_cap_repair), not per shard
    fp.shard_slots = 1;
    s->slots.cull_noted(false);
    s->slots.keys_drawn(true);
    Timeline::Flags &fl = s->tl.frame();
    fl.compacted = false; fl.one_pass = fl.direct = true; fl.squeezed = false;
    if ((rc = launch_surfel_pass(s, fp, true, true, n_prep))) return rc;
    // The W*H conflict cap acts in surfel order over ALL ranks: exchange the conflict masks and take this rank's surplus back
    // before anything reads the key map (k_shard_cap_pack / k_shard_cap_repair).  Conflicts <= surfels, so a model with no
    // more slots than pixels cannot reach the cap; the bound is the host's, the same on every rank.
    if (s->cfg.conflict_cap && (uint64_t)s->slots.bound() > (uint64_t)s->P) {
        const uint32_t tbnd = (uint32_t)std::min<uint64_t>(s->slots.tiles(), s->dead_tiles);
        const int gp = (int)std::min<uint32_t>(std::max<uint32_t>((tbnd * (uint32_t)TILE_WORDS + 255u) / 256u, 1u), 1024u);
        hipLaunchKernelGGL(k_shard_cap_pack, dim3(gp), dim3(256), 0, s->stream, s->d_state, s->cur().wave_cnt, s->d_cm,
                           s->cur().conf_sub, s->d_capx, tbnd);
        HIPCK(hipGetLastError());
        if ((rc = ss_collective(s, s->d_capx, s->d_capx, (size_t)1 + (size_t)(2 + TILE_WORDS) * tbnd, SM_COLL_SUM))) return rc;
        hipLaunchKernelGGL(k_shard_cap_repair, dim3(std::min<uint32_t>(std::max<uint32_t>(tbnd, 1u), (uint32_t)MAX_GRID)), dim3(256), 0, s->stream, s->M,
                           s->d_state, fp, s->d_capx, tbnd, (uint32_t)s->P, s->cur().wave_cnt, s->d_dm /* km */, s->cur().tile_flags, s->d_alive,
                           s->d_tile_dead, s->keyT(), s->d_undo, s->d_tb);
        HIPCK(hipGetLastError());
    }
    if ((rc = ss_collective(s, s->keyT(), s->keyT(), (size_t)s->P, SM_COLL_MIN))) return rc;
    ShardArgs sh;
    sh.validmask = s->d_validmask; sh.ownmask = s->d_fusedmask; sh.gmask = s->d_gmask; sh.nwords = (uint32_t)((s->P + 63) / 64);
    sh.owner = (int)(s->ss_frames % (uint32_t)s->ss_world) == s->ss_rank ? 1 : 0;
    AssocArgs aa;
    fill_assoc_args(s, fp, aa);
    hipLaunchKernelGGL((k_associate_direct<true>), dim3(assoc_wgs(s)), dim3(PIX_BLOCK), 0, s->stream, aa, sh);
    HIPCK(hipGetLastError());
    if ((rc = s->tl.mark(s->stream, 5, true))) return rc;
    if ((rc = ss_collective(s, s->d_gmask, s->d_gmask, (size_t)sh.nwords + 4, SM_COLL_SUM))) return rc;   // in place, like the key map
    // the frame's last step (counts from the reduced mask, the owner's foreign-fused slots, the totals over the ranks) is
    // only needed by the next frame's surfel pass: it rides on that frame's k_prep (finalize_if_pending runs it earlier if asked)
    ShardSettle ss;
    ss.n = (uint32_t)s->n_pix_blocks; ss.st = s->d_state; ss.validmask = s->d_validmask; ss.ownmask = s->d_fusedmask; ss.gmask = s->d_gmask;
    ss.nwords = sh.nwords; ss.blk_cand = s->d_blk_cand; ss.grp_cand = s->d_grp_cand; ss.nf = s->cur().nf_sub; ss.alive = s->d_alive;
    ss.tile_dead = s->d_tile_dead; ss.owner = sh.owner; ss.cap_pixels = s->cfg.conflict_cap ? (uint32_t)s->P : 0xFFFFFFFFu; ss.max_vertices = s->cap; ss.cg = s->cand_group;
    s->held.hold_settle(ss);
    if ((rc = s->tl.mark(s->stream, 6, true)) || (rc = s->tl.mark(s->stream, 7, true))) return rc;
    s->part.clear();
    s->held.hold_stats(s->cur().nf_sub);
    s->slots.append_enqueued();
    s->ss_frames++;
    end_frame(s);
    return SM_OK;
}

int sm_shard_frame(sm_ctx *s, const uint8_t *rgb, const uint16_t *depth_mm, const uint8_t *semantic, const float *pose16)
{
    if (!s || !rgb || !pose16) { g_err = "sm_shard_frame: null argument"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    int rc = upload_inputs(s, rgb, depth_mm, semantic);
    if (rc) return rc;
    if ((rc = sm_shard_frame_device(s, s->d_rgb, nullptr, nullptr, pose16))) return rc;      // (given or not, the current images)
    return sm_sync(s);
}

// This rank's part of the (compacted) union as a dense AoS plane of `*count` surfels with zeros where other ranks own the
// slot: the integer sum of the planes over the ranks is the single GlobalModel.  Collective (it compacts first).
int sm_shard_export_dense_device(sm_ctx *s, const float **d_out12, uint32_t *count)
{
    if (!s || !d_out12 || !count || !s->ss_on) return SM_E_ARG;
    HIPCK(hipSetDevice(s->cfg.device));
    if (hip_runtime_conflict("sm_shard_export_dense_device")) return SM_E_HIP;
    int rc = ensure_compact(s);
    if (rc) return rc;
    if ((rc = pull_state(s))) return rc;
    const uint32_t n = s->h_state->count;
    if ((rc = ensure_export(s, (size_t)std::max<uint32_t>(n, 1) * 48))) return rc;
    if (n) hipLaunchKernelGGL(k_shard_export_aos, dim3((n + 255) / 256), dim3(256), 0, s->stream, s->M, s->d_state, s->d_alive, (float *)s->d_export.get(), n);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(s->stream));
    *d_out12 = (const float *)s->d_export.get();
    *count = n;
    return SM_OK;
}

}  // extern "C"
