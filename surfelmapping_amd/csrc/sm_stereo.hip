// sm_stereo.hip -- stereo depth (DESIGN.md "4m. Stereo depth"): the buffers of a context that estimates depth (sm_set_stereo), the
// depth image of a rectified pair from host or device images (sm_stereo_depth*), and the intermediates of the last call
// (sm_stereo_download).  Kernels: sm_k_stereo.h.
#include "sm_ctx.h"
#include "sm_k_stereo.h"

#include <cstdlib>

using namespace sm;

namespace {

const int DIRS[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};

// what every entry point with a context asks first; stereo: the context must have it
int stereo_check(sm_ctx *s, bool stereo, const char *who)
{
    if (!s) { g_err = std::string(who) + ": null context"; return SM_E_ARG; }
    if (int rc = check_whole_map(s, who)) return rc;
    if (int rc = check_not_mid_cull(s, who)) return rc;
    if (stereo && !s->stereo.on) { g_err = std::string(who) + ": the context has no stereo (sm_set_stereo)"; return SM_E_ARG; }
    return SM_OK;
}

const char *check_params(const sm_stereo_params &p)
{
    if (p.max_disp != 64 && p.max_disp != 128 && p.max_disp != 192 && p.max_disp != 256) return "max_disp is not 64, 128, 192 or 256";
    if (p.paths != 4 && p.paths != 8) return "paths is not 4 or 8";
    if (p.p1 < 1 || p.p2 < p.p1 || p.p2 > 1023) return "p1 and p2 must satisfy 1 <= p1 <= p2 <= 1023";
    if (p.uniqueness < 0 || p.uniqueness > 100) return "uniqueness is a percentage in 0..100";
    if (p.lr_max_diff < 0 || p.lr_max_diff > p.max_disp) return "lr_max_diff is outside 0..max_disp";
    if (!std::isfinite(p.baseline) || !(p.baseline > 0.0f)) return "baseline is not finite and positive";
    return nullptr;
}

template <int N>
void launch_paths_and_select(sm_ctx *s, uint16_t *d_depth, uint16_t *d_disp)
{
    Stereo &st = s->stereo;
    for (int r = 0; r < st.p.paths; ++r) {
        StereoPathArgs a;
        a.cost = st.d_cost; a.vol = st.d_vol;
        a.W = s->W; a.H = s->H; a.D = st.p.max_disp;
        a.dx = DIRS[r][0]; a.dy = DIRS[r][1];
        a.p1 = st.p.p1; a.p2 = st.p.p2;
        a.first = r == 0;
        a.n_paths = a.dy == 0 ? s->H : a.dx == 0 ? s->W : s->W + s->H - 1;
        hipLaunchKernelGGL(k_stereo_path<N>, dim3((unsigned)a.n_paths), dim3(64), 0, s->stream, a);
        if (st.timed) (void)hipEventRecord(st.ev[3 + r], s->stream);
    }
    StereoSelectArgs a;
    a.vol = st.d_vol; a.depth = d_depth; a.disp = d_disp;
    a.W = s->W; a.D = st.p.max_disp;
    a.uniqueness = st.p.uniqueness; a.lr_max_diff = st.p.lr_max_diff;
    a.K = ((double)s->cfg.fx * (double)st.p.baseline) * 16000.0;
    hipLaunchKernelGGL(k_stereo_select<N>, dim3((unsigned)s->H), dim3(ST_SELECT_THREADS), (size_t)s->W, s->stream, a);
    if (st.timed) (void)hipEventRecord(st.ev[3 + st.p.paths], s->stream);
}

// the whole chain for images on the device, enqueued on the context's stream
int stereo_device(sm_ctx *s, const uint8_t *d_left, const uint8_t *d_right, uint16_t *d_depth, uint16_t *d_disp)
{
    Stereo &st = s->stereo;
    const int W = s->W, H = s->H, D = st.p.max_disp;
    if (st.timed) HIPCK(hipEventRecord(st.ev[0], s->stream));
    StereoCensusArgs ca;
    ca.rgb[0] = d_left; ca.rgb[1] = d_right;
    ca.census[0] = st.d_census[0]; ca.census[1] = st.d_census[1];
    ca.W = W; ca.H = H;
    hipLaunchKernelGGL(k_stereo_census, dim3((W + ST_TX - 1) / ST_TX, (H + ST_TY - 1) / ST_TY, 2), dim3(256), 0, s->stream, ca);
    HIPCK(hipGetLastError());
    if (st.timed) HIPCK(hipEventRecord(st.ev[1], s->stream));
    StereoCostArgs co;
    co.cl = st.d_census[0]; co.cr = st.d_census[1]; co.cost = st.d_cost;
    co.W = W; co.D = D;
    co.n = (size_t)s->P * (size_t)(D / 4);
    hipLaunchKernelGGL(k_stereo_cost, dim3((unsigned)((co.n + 255) / 256)), dim3(256), 0, s->stream, co);
    HIPCK(hipGetLastError());
    if (st.timed) HIPCK(hipEventRecord(st.ev[2], s->stream));
    switch (D / 64) {
    case 1: launch_paths_and_select<1>(s, d_depth, d_disp); break;
    case 2: launch_paths_and_select<2>(s, d_depth, d_disp); break;
    case 3: launch_paths_and_select<3>(s, d_depth, d_disp); break;
    default: launch_paths_and_select<4>(s, d_depth, d_disp); break;
    }
    HIPCK(hipGetLastError());
    return SM_OK;
}

}  // namespace

extern "C" {

int sm_default_stereo_params(const sm_config *c, sm_stereo_params *p)
{
    if (!c || !p) { g_err = "sm_default_stereo_params: null argument"; return SM_E_ARG; }
    p->max_disp = 128;
    p->paths = 8;
    p->p1 = 7;
    p->p2 = 86;
    p->uniqueness = 5;
    p->lr_max_diff = 1;
    p->baseline = 0.54f;
    return SM_OK;
}

int sm_set_stereo(sm_ctx *s, const sm_stereo_params *p)
{
    const char *who = "sm_set_stereo";
    int rc;
    if ((rc = stereo_check(s, false, who))) return rc;
    if (p)
        if (const char *why = check_params(*p)) { g_err = std::string(who) + ": " + why; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (s->stereo.on) HIPCK(hipStreamSynchronize(s->stream));       // an enqueued call still uses the buffers
    s->stereo = Stereo();                                // (the old buffers go first: two volumes need not fit at once)
    if (!p) return SM_OK;
    Stereo st;
    st.p = *p;
    const size_t P = (size_t)s->P, V = P * (size_t)p->max_disp;
    if ((rc = dalloc(st.d_left, P * 3)) || (rc = dalloc(st.d_right, P * 3)) || (rc = dalloc(st.d_census[0], P)) ||
        (rc = dalloc(st.d_census[1], P)) || (rc = dalloc(st.d_cost, V)) || (rc = dalloc(st.d_vol, V)) || (rc = dalloc(st.d_depth, P)) ||
        (rc = dalloc(st.d_disp, P))) {
        (void)hipGetLastError();                         // (the failed allocation's error is reported, not left behind)
        return rc;
    }
    // what sm_stereo_download returns before the first call
    HIPCK(hipMemsetAsync(st.d_census[0], 0, P * 8, s->stream));
    HIPCK(hipMemsetAsync(st.d_census[1], 0, P * 8, s->stream));
    HIPCK(hipMemsetAsync(st.d_vol, 0, V * 2, s->stream));
    const char *te = std::getenv("SM_STEREO_TIMING");
    st.timed = te && te[0] == '1';
    if (st.timed)
        for (Event &e : st.ev) {
            HIPCK(hipEventCreate(e.put()));
            HIPCK(hipEventRecord(e, s->stream));          // (so that a query before the first launch finds recorded events)
        }
    HIPCK(hipStreamSynchronize(s->stream));
    st.on = true;
    s->stereo = std::move(st);
    return SM_OK;
}

// Diagnostic, deliberately not part of include/sm_c_api.h (tools/stereo_probe.py): device times of the last call's kernels of a
// context whose sm_set_stereo ran with SM_STEREO_TIMING=1 -- ms[0] the census, ms[1] the costs, ms[2..9] the directions in order
// (-1 for those `paths` leaves out), ms[10] the selection; -1 each otherwise.  Waits for the stream.
int sm_debug_stereo_ms(sm_ctx *s, float *ms11)
{
    if (!s || !ms11) return SM_E_ARG;
    for (int i = 0; i < 11; ++i) ms11[i] = -1.0f;
    const Stereo &st = s->stereo;
    if (!st.on || !st.timed) return SM_OK;
    HIPCK(hipSetDevice(s->cfg.device));
    HIPCK(hipStreamSynchronize(s->stream));
    HIPCK(hipEventElapsedTime(&ms11[0], st.ev[0], st.ev[1]));
    HIPCK(hipEventElapsedTime(&ms11[1], st.ev[1], st.ev[2]));
    for (int r = 0; r < st.p.paths; ++r) HIPCK(hipEventElapsedTime(&ms11[2 + r], st.ev[2 + r], st.ev[3 + r]));
    HIPCK(hipEventElapsedTime(&ms11[10], st.ev[2 + st.p.paths], st.ev[3 + st.p.paths]));
    return SM_OK;
}

int sm_stereo_depth_device(sm_ctx *s, const uint8_t *d_left, const uint8_t *d_right, uint16_t *d_depth_mm_out, uint16_t *d_disp16_out)
{
    const char *who = "sm_stereo_depth_device";
    int rc;
    if ((rc = stereo_check(s, true, who))) return rc;
    if (!d_left || !d_right) { g_err = std::string(who) + ": null image"; return SM_E_ARG; }
    if (((uintptr_t)d_depth_mm_out | (uintptr_t)d_disp16_out) & 1u) { g_err = std::string(who) + ": misaligned output"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    return stereo_device(s, d_left, d_right, d_depth_mm_out, d_disp16_out);
}

int sm_stereo_depth(sm_ctx *s, const uint8_t *rgb_left, const uint8_t *rgb_right, uint16_t *depth_mm_out, uint16_t *disp16_out)
{
    const char *who = "sm_stereo_depth";
    int rc;
    if ((rc = stereo_check(s, true, who))) return rc;
    if (!rgb_left || !rgb_right) { g_err = std::string(who) + ": null image"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    Stereo &st = s->stereo;
    const size_t P = (size_t)s->P;
    HIPCK(hipMemcpyAsync(st.d_left, rgb_left, P * 3, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(st.d_right, rgb_right, P * 3, hipMemcpyHostToDevice, s->stream));
    if ((rc = stereo_device(s, st.d_left, st.d_right, depth_mm_out ? st.d_depth.get() : nullptr, disp16_out ? st.d_disp.get() : nullptr)))
        return rc;
    if (depth_mm_out) HIPCK(hipMemcpyAsync(depth_mm_out, st.d_depth, P * 2, hipMemcpyDeviceToHost, s->stream));
    if (disp16_out) HIPCK(hipMemcpyAsync(disp16_out, st.d_disp, P * 2, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

int sm_stereo_download(sm_ctx *s, uint64_t *census_left, uint64_t *census_right, uint16_t *volume)
{
    const char *who = "sm_stereo_download";
    if (int rc = stereo_check(s, true, who)) return rc;
    HIPCK(hipSetDevice(s->cfg.device));
    Stereo &st = s->stereo;
    const size_t P = (size_t)s->P;
    if (census_left) HIPCK(hipMemcpyAsync(census_left, st.d_census[0], P * 8, hipMemcpyDeviceToHost, s->stream));
    if (census_right) HIPCK(hipMemcpyAsync(census_right, st.d_census[1], P * 8, hipMemcpyDeviceToHost, s->stream));
    if (volume) HIPCK(hipMemcpyAsync(volume, st.d_vol, P * (size_t)st.p.max_disp * 2, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));
    return SM_OK;
}

}  // extern "C"
