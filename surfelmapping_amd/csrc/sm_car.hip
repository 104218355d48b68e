// sm_car.hip -- routes a car can follow (sm_route_car; DESIGN.md "4ad. Routes for a car"): sm_route.hip's call in shape -- the
// caller's state and clear2 planes up, one launch for the multipliers and the edge bits, one for the weights of every state's four
// moves, the goals seeded, then rounds of the tiled relaxation over (cell, heading), a launch a round, the flags of the tiles
// double-buffered, the count of the flags a round raised read from pinned memory every rounds_per_check rounds, until no flag is up;
// `next` and the info from the costs, the path words along `next`, and what the caller asked for back.  Kernels: sm_k_car.h.  It
// reads nothing of the model and of no file.  Everything on the device is allocated per call and freed when it ends; the context
// keeps the events, the pinned counters and the last call's stats.
#include "sm_ctx.h"
#include "sm_map_stream.h"
#include "sm_set_call.h"
#include "sm_k_car.h"

using namespace sm;
using sm_mapfile::now_ms;

namespace {

enum { EV_PREP0 = 0, EV_PREP1, EV_RELAX0, EV_RELAX1, EV_NEXT0, EV_NEXT1, EV_WALK0, EV_WALK1, N_EV };
static_assert(N_EV == Car::N_EV, "the context holds the events of a call");
static_assert(ROUTE_NONE == SM_ROUTE_NONE, "the header's");
static_assert(ROUTE_FREE == SM_GROUND_FREE && ROUTE_UNKNOWN == SM_GROUND_UNKNOWN, "the states are the ground map's");

constexpr int64_t MAX_CELLS = 1 << 22, MAX_FIELD_CELLS = 1 << 23, MAX_PATH_WORDS = 1 << 26;

int check_params(const sm_route_car_params *p, const char *who)
{
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    if (p->nu < 1 || p->nu > 4096) return bad("nu outside 1..4096");
    if (p->nv < 1 || p->nv > 4096) return bad("nv outside 1..4096");
    if ((int64_t)p->nu * p->nv > MAX_CELLS) return bad("nu * nv above 2^22");
    if (p->body_cells < 0 || p->body_cells > 255) return bad("body_cells outside 0..255");
    if (p->soft_cells < 0 || p->soft_cells > 255) return bad("soft_cells outside 0..255");
    if (p->near_weight < 0 || p->near_weight > 14) return bad("near_weight outside 0..14");
    if (p->unknown_passable != 0 && p->unknown_passable != 1) return bad("unknown_passable is 0 or 1");
    if (p->turn_cells < 1 || p->turn_cells > 16) return bad("turn_cells outside 1..16");
    if (p->turn_cost < 0 || p->turn_cost > 4095) return bad("turn_cost outside 0..4095");
    if (p->reverse_weight < 0 || p->reverse_weight > 15) return bad("reverse_weight outside 0..15");
    if (p->max_steps < 0 || p->max_steps > MAX_CELLS) return bad("max_steps outside 0..2^22");
    if (p->rounds_per_check < 1 || p->rounds_per_check > CAR_MAX_BATCH) return bad("rounds_per_check outside 1..64");
    if (p->max_rounds < 1) return bad("max_rounds below 1");
    return SM_OK;
}

// SM_CAR_TILE and SM_CAR_SWEEPS, read per call
int read_switches(RouteArgs &a, int turn_cells, const char *who)
{
    a.T = 32;
    if (const char *e = std::getenv("SM_CAR_TILE")) {
        const int t = std::atoi(e);
        if (t != 16 && t != 32) { g_err = std::string(who) + ": SM_CAR_TILE is 16 or 32"; return SM_E_ARG; }
        a.T = t;
    }
    if (a.T < 2 * turn_cells) { g_err = std::string(who) + ": SM_CAR_TILE=16 with turn_cells above 8 (a tile is at least 2 turn_cells wide)"; return SM_E_ARG; }
    a.sweeps = a.T * a.T;               // a sequence of moves inside a tile is rarely longer; a tile the cap stops raises its own flag
    if (const char *e = std::getenv("SM_CAR_SWEEPS")) {
        const int n = std::atoi(e);
        if (n < 1 || n > 65536) { g_err = std::string(who) + ": SM_CAR_SWEEPS outside 1..65536"; return SM_E_ARG; }
        a.sweeps = n;
    }
    return SM_OK;
}

int ensure(Car &r)
{
    if (r.h_counters) return SM_OK;
    for (Event &e : r.ev) HIPCK(hipEventCreate(e.put()));
    HIPCK(hipHostMalloc((void **)r.h_counters.put(), CAR_COUNTER_WORDS * 4, hipHostMallocDefault));   // (set last: it marks the block complete)
    return SM_OK;
}

void launch_relax(const CarArgs &a, uint32_t G, hipStream_t st, const uint2 *wts, uint32_t *cost, uint32_t *now, uint32_t *next, uint32_t *counters, int word)
{
    const dim3 grid((unsigned)((size_t)G * a.r.tu * a.r.tv));
    if (a.r.T == 16) hipLaunchKernelGGL((k_car_relax<16, 256>), grid, dim3(256), 0, st, a, G, wts, cost, now, next, counters, word);
    else hipLaunchKernelGGL((k_car_relax<32, 256>), grid, dim3(256), 0, st, a, G, wts, cost, now, next, counters, word);
}

}  // namespace

extern "C" {

int sm_default_route_car_params(sm_route_car_params *p)
{
    if (!p) { g_err = "sm_default_route_car_params: null argument"; return SM_E_ARG; }
    *p = sm_route_car_params{};
    p->nu = p->nv = 256;
    p->body_cells = 0;
    p->soft_cells = 0;
    p->near_weight = 0;
    p->unknown_passable = 0;
    p->turn_cells = 2;
    p->turn_cost = 0;
    p->reverse_weight = 0;
    p->max_steps = 4096;
    p->rounds_per_check = 4;
    p->max_rounds = 65536;
    return SM_OK;
}

int sm_route_car(sm_ctx *s, const sm_route_car_params *p, const uint8_t *state, const uint32_t *clear2, uint32_t n_fields, const uint32_t *goal_first,
                 const int32_t *goals, uint32_t n_starts, const int32_t *starts, uint32_t *cost, uint8_t *next, uint32_t *path, uint32_t *path_len,
                 uint32_t *path_cost, sm_route_car_info *info)
{
    const char *who = "sm_route_car";
    const double t_begin = now_ms();
    auto bad = [&](const char *what) { g_err = std::string(who) + ": " + what; return SM_E_ARG; };
    // (the context is looked at last: every rule about the arguments holds, and can be tried, without a device)
    if (!p || !state || !clear2 || !goal_first || !info) return bad("null argument");
    int rc;
    if ((rc = check_params(p, who))) return rc;
    const uint32_t G = n_fields;
    const size_t N = (size_t)p->nu * p->nv;
    if (G < 1) return bad("no field");
    if ((uint64_t)G * N > (uint64_t)MAX_FIELD_CELLS) return bad("fields * nu * nv above 2^23");
    if (goal_first[0] != 0) return bad("goal_first[0] is not 0");
    for (uint32_t f = 0; f < G; ++f)
        if (goal_first[f + 1] < goal_first[f]) return bad("goal_first falls");
    const uint32_t n_goals = goal_first[G];
    if (n_goals > (uint32_t)(8 * MAX_FIELD_CELLS)) return bad("more than 2^26 goals");
    if (n_goals && !goals) return bad("null goals");
    for (uint32_t i = 0; i < n_goals; ++i) {
        const int32_t *g = goals + 3 * (size_t)i;
        if (g[0] < 0 || g[0] >= p->nu || g[1] < 0 || g[1] >= p->nv) return bad("a goal outside the window");
        if (g[2] < -1 || g[2] > 7) return bad("a goal's heading outside -1..7");
    }
    if (n_starts && !starts) return bad("null starts");
    const size_t row = (size_t)p->max_steps + 1;
    if ((uint64_t)n_starts * row > (uint64_t)MAX_PATH_WORDS) return bad("starts * (max_steps + 1) above 2^26");
    for (uint32_t i = 0; i < n_starts; ++i) {
        const int32_t *t = starts + 4 * (size_t)i;
        if (t[0] < 0 || (uint32_t)t[0] >= G) return bad("a start's field outside 0..fields - 1");
        if (t[1] < 0 || t[1] >= p->nu || t[2] < 0 || t[2] >= p->nv) return bad("a start outside the window");
        if (t[3] < 0 || t[3] > 7) return bad("a start's heading outside 0..7");
    }
    CarArgs ca{};
    RouteArgs &a = ca.r;
    if ((rc = read_switches(a, p->turn_cells, who))) return rc;
    ca.n = p->turn_cells;
    ca.turn_cost = p->turn_cost;
    ca.reverse_weight = p->reverse_weight;
    a.nu = p->nu; a.nv = p->nv;
    a.body2 = p->body_cells * p->body_cells;
    a.S2 = p->soft_cells * p->soft_cells;
    a.near_weight = p->near_weight;
    a.unknown_passable = p->unknown_passable;
    a.tu = (a.nu + a.T - 1) / a.T; a.tv = (a.nv + a.T - 1) / a.T;
    const size_t tiles = (size_t)a.tu * a.tv, slots = (size_t)G * tiles;
    if (!s) return bad("null context");

    HIPCK(hipSetDevice(s->cfg.device));
    Car &rt = s->car;
    if ((rc = ensure(rt))) return rc;
    const Event *ev = rt.ev;
    sm_route_car_stats_t st{};
    st.tile = (uint32_t)a.T;
    st.sweep_cap = (uint32_t)a.sweeps;

    // ---- the call's device memory, one block: every part starts on a multiple of 16 bytes
    const bool want_next = next || n_starts;
    size_t bytes = 0;
    const auto part = [&](size_t n) { const size_t at = bytes; bytes += (n + 15) & ~(size_t)15; return at; };
    const size_t o_cost = part((size_t)G * 8 * N * 4), o_clear2 = part(N * 4), o_flags = part(2 * slots * 4), o_info = part((size_t)G * CAR_INFO_WORDS * 4),
                 o_counters = part(CAR_COUNTER_WORDS * 4), o_first = part(((size_t)G + 1) * 4), o_goals = part((size_t)n_goals * 12),
                 o_starts = part((size_t)n_starts * 16), o_path = part(path ? (size_t)n_starts * row * 4 : 0), o_len = part((size_t)n_starts * 4),
                 o_pcost = part((size_t)n_starts * 4), o_state = part(N), o_m = part(N), o_edge = part(N), o_wts = part(8 * N * 8), o_next = part(want_next ? (size_t)G * 8 * N : 0);
    Dev<uint8_t> mem;                  // freed when the call ends
    if ((rc = dalloc(mem, bytes))) { (void)hipGetLastError(); return rc; }
    uint8_t *b = mem.get();
    uint32_t *d_cost = (uint32_t *)(b + o_cost), *d_clear2 = (uint32_t *)(b + o_clear2), *d_flags = (uint32_t *)(b + o_flags), *d_info = (uint32_t *)(b + o_info),
             *d_counters = (uint32_t *)(b + o_counters), *d_first = (uint32_t *)(b + o_first), *d_path = path ? (uint32_t *)(b + o_path) : nullptr,
             *d_len = (uint32_t *)(b + o_len), *d_pcost = (uint32_t *)(b + o_pcost);
    int *d_goals = (int *)(b + o_goals), *d_starts = (int *)(b + o_starts);
    uint2 *d_wts = (uint2 *)(b + o_wts);
    uint8_t *d_state = b + o_state, *d_m = b + o_m, *d_edge = b + o_edge, *d_next = want_next ? b + o_next : nullptr;
    uint32_t launches = 0;

    // ---- planes up, the multipliers and the edges, the moves' weights, the goals
    if ((rc = mark(s, ev[EV_PREP0]))) return rc;
    HIPCK(hipMemcpyAsync(d_state, state, N, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(d_clear2, clear2, N * 4, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemcpyAsync(d_first, goal_first, ((size_t)G + 1) * 4, hipMemcpyHostToDevice, s->stream));
    if (n_goals) HIPCK(hipMemcpyAsync(d_goals, goals, (size_t)n_goals * 12, hipMemcpyHostToDevice, s->stream));
    if (n_starts) HIPCK(hipMemcpyAsync(d_starts, starts, (size_t)n_starts * 16, hipMemcpyHostToDevice, s->stream));
    HIPCK(hipMemsetAsync(d_cost, 0xFF, (size_t)G * 8 * N * 4, s->stream));
    HIPCK(hipMemsetAsync(d_flags, 0, o_first - o_flags, s->stream));                 // the flags, the info, the counters
    hipLaunchKernelGGL(k_car_cells, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s->stream, a, (const uint8_t *)d_state, (const uint32_t *)d_clear2, d_m, d_edge);
    hipLaunchKernelGGL(k_car_prepare, dim3((unsigned)((8 * N + 255) / 256)), dim3(256), 0, s->stream, ca, (const uint8_t *)d_m, (const uint8_t *)d_edge, d_wts);
    launches += 2;
    if (n_goals) {
        hipLaunchKernelGGL(k_car_seed, dim3((n_goals + 255) / 256), dim3(256), 0, s->stream, ca, G, (const uint32_t *)d_first, (const int *)d_goals,
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
        if (!first_batch) HIPCK(hipMemsetAsync(d_counters, 0, CAR_COUNTER_WORDS * 4, s->stream));
        for (int i = 0; i < batch; ++i, ++rounds) {
            uint32_t *now = d_flags + (size_t)(rounds & 1u) * slots, *nxt = d_flags + (size_t)((rounds + 1) & 1u) * slots;
            launch_relax(ca, G, s->stream, d_wts, d_cost, now, nxt, d_counters, CAR_C_ROUND0 + i);
        }
        launches += (uint32_t)batch;
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(h, d_counters, CAR_COUNTER_WORDS * 4, hipMemcpyDeviceToHost, s->stream));
        HIPCK(hipStreamSynchronize(s->stream));
        uint32_t in = first_batch ? h[CAR_C_SEEDED] : up;
        for (int i = 0; i < batch; ++i) {
            if (in) st.rounds++;                          // a round that found a flag up
            in = h[CAR_C_ROUND0 + i];
        }
        st.tile_visits += h[CAR_C_VISITS];
        up = in;
        first_batch = false;
    }
    if ((rc = mark(s, ev[EV_RELAX1])) || (rc = mark(s, ev[EV_NEXT0]))) return rc;

    // ---- next and the info; the paths
    {
        const unsigned gy = (unsigned)std::min<uint32_t>(G, 1024u);
        hipLaunchKernelGGL(k_car_next, dim3((unsigned)((N + 255) / 256), gy), dim3(256), 0, s->stream, ca, G, (const uint2 *)d_wts, (const uint32_t *)d_cost,
                           d_next, d_info);
        launches++;
    }
    if ((rc = mark(s, ev[EV_NEXT1])) || (rc = mark(s, ev[EV_WALK0]))) return rc;
    if (n_starts) {
        if (d_path) HIPCK(hipMemsetAsync(d_path, 0xFF, (size_t)n_starts * row * 4, s->stream));
        hipLaunchKernelGGL(k_car_walk, dim3((n_starts + 255) / 256), dim3(256), 0, s->stream, ca, n_starts, (const int *)d_starts, (const uint32_t *)d_cost,
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
    std::vector<uint32_t> h_info((size_t)G * CAR_INFO_WORDS);
    HIPCK(hipMemcpyAsync(h_info.data(), d_info, h_info.size() * 4, hipMemcpyDeviceToHost, s->stream));
    HIPCK(hipStreamSynchronize(s->stream));                // (before anything of the caller's is touched)
    const auto back = [&](void *dst, const void *d_src, size_t n) -> int {
        if (dst && n) HIPCK(hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, s->stream));
        return SM_OK;
    };
    if ((rc = back(cost, d_cost, (size_t)G * 8 * N * 4)) || (rc = back(next, d_next, (size_t)G * 8 * N)) || (rc = back(path, d_path, (size_t)n_starts * row * 4)) ||
        (rc = back(path_len, d_len, (size_t)n_starts * 4)) || (rc = back(path_cost, d_pcost, (size_t)n_starts * 4)))
        return rc;
    HIPCK(hipStreamSynchronize(s->stream));
    for (uint32_t f = 0; f < G; ++f) {
        const uint32_t *w = &h_info[(size_t)f * CAR_INFO_WORDS];
        info[f] = sm_route_car_info{w[CAR_I_USED], w[CAR_I_DROPPED], w[CAR_I_STATES], w[CAR_I_CELLS], w[CAR_I_STATES] ? w[CAR_I_MAX] : 0u};
    }
    st.copy_ms = (float)(now_ms() - t_copy);
    st.launches = launches;
    st.total_ms = (float)(now_ms() - t_begin);
    rt.stats = st;                                        // (a call that fails leaves the last one's)
    rt.stats_valid = true;
    return SM_OK;
}

SM_STATS_GETTER(sm_route_car_stats, sm_route_car_stats_t, car, "sm_route_car")

}  // extern "C"
