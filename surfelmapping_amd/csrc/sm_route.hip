// sm_route.hip -- routes over the ground map (sm_route_ground; DESIGN.md "4ac. Routes"): the caller's state and clear2 planes up,
// one launch for the multipliers and the edge bits, the goals seeded, then rounds of the tiled relaxation -- a launch a round, the
// flags of the tiles double-buffered, the count of the flags a round raised read from pinned memory every rounds_per_check rounds --
// until no flag is up; `next` and the info from the costs, the paths along `next`, and what the caller asked for back.  Kernels:
// sm_k_route.h.  It reads nothing of the model and of no file.  Everything on the device is allocated per call and freed when it
// ends; the context keeps the events, the pinned counters and the last call's stats.
#include "sm_ctx.h"
#include "sm_map_stream.h"
#include "sm_set_call.h"
#include "sm_k_route.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

enum { EV_PREP0 = 0, EV_PREP1, EV_RELAX0, EV_RELAX1, EV_NEXT0, EV_NEXT1, EV_WALK0, EV_WALK1, N_EV };
static_assert(N_EV == Route::N_EV, "the context holds the events of a call");
static_assert(ROUTE_NONE == SM_ROUTE_NONE, "the header's");
static_assert(ROUTE_FREE == SM_GROUND_FREE && ROUTE_UNKNOWN == SM_GROUND_UNKNOWN, "the states are the ground map's");

constexpr int64_t MAX_CELLS = 1 << 22, MAX_FIELD_CELLS = 1 << 26, MAX_PATH_WORDS = 1 << 26;

int check_params(const sm_route_params *p, const char *who)
{
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (p->nu < 1 || p->nu > 4096) return bad("nu outside 1..4096");
    if (p->nv < 1 || p->nv > 4096) return bad("nv outside 1..4096");
    if ((int64_t)p->nu * p->nv > MAX_CELLS) return bad("nu * nv above 2^22");
    if (p->body_cells < 0 || p->body_cells > 255) return bad("body_cells outside 0..255");
    if (p->soft_cells < 0 || p->soft_cells > 255) return bad("soft_cells outside 0..255");
    if (p->near_weight < 0 || p->near_weight > 14) return bad("near_weight outside 0..14");
    if (p->unknown_passable != 0 && p->unknown_passable != 1) return bad("unknown_passable is 0 or 1");
    if (p->max_steps < 0 || p->max_steps > MAX_CELLS) return bad("max_steps outside 0..2^22");
    if (p->rounds_per_check < 1 || p->rounds_per_check > ROUTE_MAX_BATCH) return bad("rounds_per_check outside 1..64");
    if (p->max_rounds < 1) return bad("max_rounds below 1");
    return SM_OK;
}

// SM_ROUTE_TILE and SM_ROUTE_SWEEPS, read per call
int read_switches(RouteArgs &a, const char *who)
{
    a.T = 32;
    if (const char *e = std::getenv("SM_ROUTE_TILE")) {
        const int t = std::atoi(e);
        if (t != 16 && t != 32 && t != 64) { g_err = std::string(who) + ": SM_ROUTE_TILE is 16, 32 or 64"; return SM_E_ARG; }
        a.T = t;
    }
    a.sweeps = a.T * a.T / 2;           // a path inside a tile is rarely longer; a tile the cap stops raises its own flag
    if (const char *e = std::getenv("SM_ROUTE_SWEEPS")) {
        const int n = std::atoi(e);
        if (n < 1 || n > 65536) { g_err = std::string(who) + ": SM_ROUTE_SWEEPS outside 1..65536"; return SM_E_ARG; }
        a.sweeps = n;
    }
    return SM_OK;
}

int ensure(Route &r)
{
    if (r.h_counters) return SM_OK;
    for (Event &e : r.ev) HIPCK(hipEventCreate(e.put()));
    HIPCK(hipHostMalloc((void **)r.h_counters.put(), ROUTE_COUNTER_WORDS * 4, hipHostMallocDefault));   // (set last: it marks the block complete)
    return SM_OK;
}

void launch_relax(const RouteArgs &a, uint32_t G, hipStream_t st, const uint8_t *m, const uint8_t *edge, uint32_t *cost, uint32_t *now, uint32_t *next,
                  uint32_t *counters, int word)
{
    const dim3 grid((unsigned)((size_t)G * a.tu * a.tv));
    if (a.T == 16) hipLaunchKernelGGL(k_route_relax<16>, grid, dim3(256), 0, st, a, G, m, edge, cost, now, next, counters, word);
    else if (a.T == 32) hipLaunchKernelGGL(k_route_relax<32>, grid, dim3(256), 0, st, a, G, m, edge, cost, now, next, counters, word);
    else hipLaunchKernelGGL(k_route_relax<64>, grid, dim3(256), 0, st, a, G, m, edge, cost, now, next, counters, word);
}

}  // namespace

extern "C" {

int sm_default_route_params(sm_route_params *p)
{
    if (!p) { g_err = "sm_default_route_params: null argument"; return SM_E_ARG; }
    *p = sm_route_params{};
    p->nu = p->nv = 256;
    p->body_cells = 0;
    p->soft_cells = 0;
    p->near_weight = 0;
    p->unknown_passable = 0;
    p->max_steps = 4096;
    p->rounds_per_check = 4;
    p->max_rounds = 65536;
    return SM_OK;
}

int sm_route_ground(sm_ctx *s, const sm_route_params *p, const uint8_t *state, const uint32_t *clear2, uint32_t n_fields, const uint32_t *goal_first,
                    const int32_t *goals, uint32_t n_starts, const int32_t *starts, uint32_t *cost, uint8_t *next, uint32_t *path, uint32_t *path_len,
                    uint32_t *path_cost, sm_route_info *info)
{
    const char *who = "sm_route_ground";
    const double t_begin = now_ms();
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (!s || !p || !state || !clear2 || !goal_first || !info) return bad("null argument");
    int rc;
    if ((rc = check_params(p, who))) return rc;
    const uint32_t G = n_fields;
    const size_t N = (size_t)p->nu * p->nv;
    if (G < 1) return bad("no field");
    if ((uint64_t)G * N > (uint64_t)MAX_FIELD_CELLS) return bad("fields * nu * nv above 2^26");
    if (goal_first[0] != 0) return bad("goal_first[0] is not 0");
    for (uint32_t f = 0; f < G; ++f)
        if (goal_first[f + 1] < goal_first[f]) return bad("goal_first falls");
    const uint32_t n_goals = goal_first[G];
    if (n_goals > (uint32_t)MAX_FIELD_CELLS) return bad("more than 2^26 goals");
    if (n_goals && !goals) return bad("null goals");
    for (uint32_t i = 0; i < n_goals; ++i)
        if (goals[2 * (size_t)i] < 0 || goals[2 * (size_t)i] >= p->nu || goals[2 * (size_t)i + 1] < 0 || goals[2 * (size_t)i + 1] >= p->nv)
            return bad("a goal outside the window");
    if (n_starts && !starts) return bad("null starts");
    const size_t row = (size_t)p->max_steps + 1;
    if ((uint64_t)n_starts * row > (uint64_t)MAX_PATH_WORDS) return bad("starts * (max_steps + 1) above 2^26");
    for (uint32_t i = 0; i < n_starts; ++i) {
        const int32_t *t = starts + 3 * (size_t)i;
        if (t[0] < 0 || (uint32_t)t[0] >= G) return bad("a start's field outside 0..fields - 1");
        if (t[1] < 0 || t[1] >= p->nu || t[2] < 0 || t[2] >= p->nv) return bad("a start outside the window");
    }
    RouteArgs a{};
    if ((rc = read_switches(a, who))) return rc;
    a.nu = p->nu; a.nv = p->nv;
    a.body2 = p->body_cells * p->body_cells;
    a.S2 = p->soft_cells * p->soft_cells;
    a.near_weight = p->near_weight;
    a.unknown_passable = p->unknown_passable;
    a.tu = (a.nu + a.T - 1) / a.T; a.tv = (a.nv + a.T - 1) / a.T;
    const size_t tiles = (size_t)a.tu * a.tv, slots = (size_t)G * tiles;

    HIPCK(hipSetDevice(s->cfg.device));
    Route &rt = s->route;
    if ((rc = ensure(rt))) return rc;
    const Event *ev = rt.ev;
    sm_route_stats_t st{};
    st.tile = (uint32_t)a.T;
    st.sweep_cap = (uint32_t)a.sweeps;

    // ---- the call's device memory, one block: every part starts on a multiple of 16 bytes
    const bool want_next = next || n_starts;
    size_t bytes = 0;
    const auto part = [&](size_t n) { const size_t at = bytes; bytes += (n + 15) & ~(size_t)15; return at; };
    const size_t o_cost = part((size_t)G * N * 4), o_clear2 = part(N * 4), o_flags = part(2 * slots * 4), o_info = part((size_t)G * ROUTE_INFO_WORDS * 4),
                 o_counters = part(ROUTE_COUNTER_WORDS * 4), o_first = part(((size_t)G + 1) * 4), o_goals = part((size_t)n_goals * 8),
                 o_starts = part((size_t)n_starts * 12), o_path = part(path ? (size_t)n_starts * row * 4 : 0), o_len = part((size_t)n_starts * 4),
                 o_pcost = part((size_t)n_starts * 4), o_state = part(N), o_m = part(N), o_edge = part(N), o_next = part(want_next ? (size_t)G * N : 0);
    Dev<uint8_t> mem;                  // freed when the call ends
    if ((rc = dalloc(mem, bytes))) { (void)hipGetLastError(); return rc; }
    uint8_t *b = mem.get();
    uint32_t *d_cost = (uint32_t *)(b + o_cost), *d_clear2 = (uint32_t *)(b + o_clear2), *d_flags = (uint32_t *)(b + o_flags), *d_info = (uint32_t *)(b + o_info),
             *d_counters = (uint32_t *)(b + o_counters), *d_first = (uint32_t *)(b + o_first), *d_path = path ? (uint32_t *)(b + o_path) : nullptr,
             *d_len = (uint32_t *)(b + o_len), *d_pcost = (uint32_t *)(b + o_pcost);
    int *d_goals = (int *)(b + o_goals), *d_starts = (int *)(b + o_starts);
    uint8_t *d_state = b + o_state, *d_m = b + o_m, *d_edge = b + o_edge, *d_next = want_next ? b + o_next : nullptr;
    uint32_t launches = 0;

    // ---- planes up, the multipliers and the edges, the goals
    if ((rc = mark(s, ev[EV_PREP0]))) return rc;
    HIPCK(hipMemcpyAsync(d_state, state, N, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(d_clear2, clear2, N * 4, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(d_first, goal_first, ((size_t)G + 1) * 4, hipMemcpyHostToDevice, s->stream));
    if (n_goals) HIPCK(hipMemcpyAsync(d_goals, goals, (size_t)n_goals * 8, hipMemcpyHostToDevice, s->stream));
    if (n_starts) HIPCK(hipMemcpyAsync(d_starts, starts, (size_t)n_starts * 12, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemsetAsync(d_cost, 0xFF, (size_t)G * N * 4, s->stream));
    HIPCK(hipMemsetAsync(d_flags, 0, o_first - o_flags, s->stream));                 // the flags, the info, the counters
    hipLaunchKernelGGL(k_route_prepare, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, a, (const uint8_t *)d_state, (const uint32_t *)d_clear2, d_m, d_edge);
    launches++;
    if (n_goals) {
        hipLaunchKernelGGL(k_route_seed, dim3((n_goals + 255) / 256), dim3(256), 0, s->stream, a, G, (const uint32_t *)d_first, (const int *)d_goals,
                           (const uint8_t *)d_m, d_cost, d_flags, d_info, d_counters);
        launches++;
    }
    if ((rc = mark(s, ev[EV_PREP1])) || (rc = mark(s, ev[EV_RELAX0]))) return rc;

    // ---- rounds: round r reads the flags of plane r & 1 and raises those of the other; its count is word ROUND0 + (r mod batch)
    uint32_t *h = rt.h_counters.get();
    uint32_t rounds = 0, up = 1;       // rounds enqueued; the flags the last round read back raised (before the first: unknown)
    bool first_batch = true;
    while (up) {
        if (rounds >= (uint32_t)p->max_rounds) {
            HIPCK(hipStreamSynchronize(s->stream));
            g_err = std::string(who) + ": flags still up after max_rounds rounds";
            return SM_E_STALL;
        }
        const int batch = (int)std::min<uint32_t>((uint32_t)p->rounds_per_check, (uint32_t)p->max_rounds - rounds);
        if (!first_batch) HIPCK(hipMemsetAsync(d_counters, 0, ROUTE_COUNTER_WORDS * 4, s->stream));
        for (int i = 0; i < batch; ++i, ++rounds) {
            uint32_t *now = d_flags + (size_t)(rounds & 1u) * slots, *nxt = d_flags + (size_t)((rounds + 1) & 1u) * slots;
            launch_relax(a, G, s->stream, d_m, d_edge, d_cost, now, nxt, d_counters, ROUTE_C_ROUND0 + i);
        }
        launches += (uint32_t)batch;
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(h, d_counters, ROUTE_COUNTER_WORDS * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        uint32_t in = first_batch ? h[ROUTE_C_SEEDED] : up;
        for (int i = 0; i < batch; ++i) {
            if (in) st.rounds++;                          // a round that found a flag up
            in = h[ROUTE_C_ROUND0 + i];
        }
        st.tile_visits += h[ROUTE_C_VISITS];
        up = in;
        first_batch = false;
    }
    if ((rc = mark(s, ev[EV_RELAX1])) || (rc = mark(s, ev[EV_NEXT0]))) return rc;

    // ---- next and the info; the paths
    {
        const unsigned gy = (unsigned)std::min<uint32_t>(G, 1024u);
        hipLaunchKernelGGL(k_route_next, dim3((unsigned)((N + 255) / 256), gy), dim3(256), 0, s->stream, a, G, (const uint8_t *)d_m, (const uint8_t *)d_edge,
                           (const uint32_t *)d_cost, d_next, d_info);
        launches++;
    }
    if ((rc = mark(s, ev[EV_NEXT1])) || (rc = mark(s, ev[EV_WALK0]))) return rc;
    if (n_starts) {
        if (d_path) HIPCK(hipMemsetAsync(d_path, 0xFF, (size_t)n_starts * row * 4, s->stream));
        hipLaunchKernelGGL(k_route_walk, dim3((n_starts + 255) / 256), dim3(256), 0, s->stream, a, n_starts, (const int *)d_starts, (const uint32_t *)d_cost,
                           (const uint8_t *)d_next, (uint32_t)p->max_steps, d_path, d_len, d_pcost);
        launches++;
    }
    if ((rc = mark(s, ev[EV_WALK1]))) return rc;
    HIPCK(hipGetLastError());
    if ((rc = add_marked(&ev[EV_PREP0], &st.prepare_ms)) || (rc = add_marked(&ev[EV_RELAX0], &st.relax_ms)) || (rc = add_marked(&ev[EV_NEXT0], &st.next_ms)) ||
        (rc = add_marked(&ev[EV_WALK0], &st.walk_ms)))
        return rc;

    // ---- what the caller asked for, one copy each (nothing has been written so far)
    const double t_copy = now_ms();
    std::vector<uint32_t> h_info((size_t)G * ROUTE_INFO_WORDS);
    HIPCK(hipMemcpyAsync(h_info.data(), d_info, h_info.size() * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));                // (before anything of the caller's is touched)
    const auto back = [&](void *dst, const void *d_src, size_t n) -> int {
        if (dst && n) HIPCK(hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, s->stream));
        return SM_OK;
    };
    if ((rc = back(cost, d_cost, (size_t)G * N * 4)) || (rc = back(next, d_next, (size_t)G * N)) || (rc = back(path, d_path, (size_t)n_starts * row * 4)) ||
        (rc = back(path_len, d_len, (size_t)n_starts * 4)) || (rc = back(path_cost, d_pcost, (size_t)n_starts * 4)))
        return rc;
    HIPCK(hipStreamSynchronize(s->stream));
    for (uint32_t f = 0; f < G; ++f) {
        const uint32_t *w = &h_info[(size_t)f * ROUTE_INFO_WORDS];
        info[f] = sm_route_info{w[ROUTE_I_USED], w[ROUTE_I_DROPPED], w[ROUTE_I_REACHED], w[ROUTE_I_REACHED] ? w[ROUTE_I_MAX] : 0u};
    }
    st.copy_ms = (float)(now_ms() - t_copy);
    st.launches = launches;
    st.total_ms = (float)(now_ms() - t_begin);
    rt.stats = st;                                        // (a call that fails leaves the last one's)
    rt.stats_valid = true;
    return SM_OK;
}

SM_STATS_GETTER(sm_route_stats, sm_route_stats_t, route, "sm_route_ground")

}  // extern "C"
