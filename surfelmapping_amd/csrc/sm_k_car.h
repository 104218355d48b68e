// sm_k_car.h -- routes a car can follow (DESIGN.md "4ad. Routes for a car"; the specification is sm_c_api.h's "routes a car can
// follow").  Included by sm_car.hip only.  The cell rules are sm_d_route.h's, shared with sm_k_route.h.  Cell (u, v) is at
// v * nu + u, state (u, v, h) at (h * nv + v) * nu + u; field f's planes start at f * 8 * nu * nv.
//   k_car_cells        one lane per cell: the byte m and the byte of edge bits, as k_route_prepare writes them
//   k_car_prepare      one lane per state: the weights of its four moves F, L, R, B, 16 bits each in one 8-byte word, CAR_NO_MOVE
//                      where the move does not exist.  Shared by every field
//   k_car_seed         one lane per goal: a goal in a passable cell gives its state (all 8 with heading -1) cost 0 and raises its
//                      tile's flag of round 0; the goals by field to the info words
//   k_car_relax<T, NT> one workgroup of NT lanes per (field, tile of T x T cells x 8 headings) whose flag of this round is up: the
//                      tile's 8 T T costs in LDS, each lane owns 8 T T / NT states (a row piece of one heading, so the heading of
//                      an owned state is known at compile time).  A move's target lies up to 2 n cells away: what an owned state
//                      reaches OUTSIDE the tile is read once, at the start of the visit, and folded into one register value
//                      min(w + cost[target]); those moves are then struck from the lane's copy of the weights, and the sweeps run
//                      over the targets inside the tile only, until a sweep changes nothing or the cap (then the tile raises its own
//                      flag of the next round).  The changed states go back to the plane, and each of the 8 neighbouring tiles gets
//                      its flag of the next round raised when a changed cell lies within 2 n cells of the border or corner facing it
//                      (T >= 2 n: no move reaches past a neighbouring tile)
//   k_car_next         one lane per cell and field, the 8 headings in turn: `next` from `cost`; the info words
//   k_car_walk         one lane per start: the path words along `next`, the unit cells of the turns included
// As in sm_k_route.h no workgroup waits for another, and none relies on seeing another's stores within a launch: a target outside
// the tile is read as it is found, and whatever it holds is the weight of a real sequence of moves or ROUTE_NONE; the states another
// tile may write in the same launch are read, and every state is written, with relaxed agent-scope atomics; the flags are raised
// with atomics and read in the NEXT launch only.  Every loop has a fixed bound.  Every index is checked against the window or the
// tile before it is used.  Nothing is ever added to ROUTE_NONE, and no candidate of 2^31 or more is kept.
#pragma once

#include "sm_d_route.h"

namespace sm {

constexpr uint32_t CAR_NO_MOVE = 0xFFFFu;                // in the place of a weight (a weight is at most 20 415)
constexpr uint32_t CAR_LIMIT = 0x80000000u;              // a cost is below it
enum { CAR_F = 0, CAR_L, CAR_R, CAR_B, CAR_MOVES };
// the info words of a field: goals used, goals dropped, reachable states, reachable cells, largest cost
enum { CAR_I_USED = 0, CAR_I_DROPPED, CAR_I_STATES, CAR_I_CELLS, CAR_I_MAX, CAR_INFO_WORDS };
// the counter block: tile visits, then per round of a batch the flags it raised for the next
enum { CAR_C_VISITS = 0, CAR_C_SEEDED = 1, CAR_C_ROUND0 = 2, CAR_MAX_BATCH = 64, CAR_COUNTER_WORDS = CAR_C_ROUND0 + CAR_MAX_BATCH };

struct CarArgs {
    RouteArgs r;                       // the window, the cell rules, the tiling, the sweep cap
    int n;                             // turn_cells
    int turn_cost, reverse_weight;
};

// the target of move mv out of a state with heading h: the cell offset and the heading there
__device__ __forceinline__ void car_target(int n, int h, int mv, int &dx, int &dy, int &ht)
{
    if (mv == CAR_F) { dx = route_du(h); dy = route_dv(h); ht = h; }
    else if (mv == CAR_B) { dx = -route_du(h); dy = -route_dv(h); ht = h; }
    else {
        ht = (h + (mv == CAR_L ? 1 : 7)) & 7;
        dx = n * (route_du(h) + route_du(ht));
        dy = n * (route_dv(h) + route_dv(ht));
    }
}
__device__ __forceinline__ uint32_t car_weight(uint2 w, int mv) { return ((mv & 2) ? w.y : w.x) >> ((mv & 1) * 16) & 0xFFFFu; }
__device__ __forceinline__ void car_strike(uint2 &w, int mv)
{
    const uint32_t bits = CAR_NO_MOVE << ((mv & 1) * 16);
    if (mv & 2) w.y |= bits; else w.x |= bits;
}

__global__ void __launch_bounds__(256) k_car_cells(RouteArgs a, const uint8_t *__restrict__ state, const uint32_t *__restrict__ clear2,
                                                   uint8_t *__restrict__ m, uint8_t *__restrict__ edge)
{
    const size_t N = (size_t)a.nu * a.nv;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    const int u = (int)(c % a.nu), v = (int)(c / a.nu);
    const uint32_t mp = route_m(a, state, clear2, u, v);
    m[c] = (uint8_t)mp;
    edge[c] = (uint8_t)route_edge_bits(a, state, clear2, u, v, mp);
}

__global__ void __launch_bounds__(256) k_car_prepare(CarArgs a, const uint8_t *__restrict__ m, const uint8_t *__restrict__ edge, uint2 *__restrict__ wts)
{
    const int nu = a.r.nu, nv = a.r.nv;
    const size_t N = (size_t)nu * nv;
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= 8 * N) return;
    const int h = (int)(s / N);
    const size_t c = s % N;
    const int u = (int)(c % nu), v = (int)(c / nu);
    uint32_t w[CAR_MOVES] = {CAR_NO_MOVE, CAR_NO_MOVE, CAR_NO_MOVE, CAR_NO_MOVE};
    const uint32_t mp = m[c], e = edge[c];
    if (mp) {
        // (an edge that exists ends inside the window)
        if (e >> h & 1u) w[CAR_F] = route_len(h) * (mp + m[(size_t)(v + route_dv(h)) * nu + (u + route_du(h))]);
        const int hb = (h + 4) & 7;
        if (a.reverse_weight > 0 && (e >> hb & 1u))
            w[CAR_B] = (uint32_t)a.reverse_weight * route_len(hb) * (mp + m[(size_t)(v + route_dv(hb)) * nu + (u + route_du(hb))]);
        for (int mv = CAR_L; mv <= CAR_R; ++mv) {
            const int h2 = (h + (mv == CAR_L ? 1 : 7)) & 7;
            int cu = u, cv = v;
            uint32_t sum = (uint32_t)a.turn_cost, mc = mp;
            bool ok = true;
            for (int i = 0; i < 2 * a.n && i < 32; ++i) {
                const int k = i < a.n ? h : h2;
                if (cu < 0 || cv < 0 || cu >= nu || cv >= nv || !(edge[(size_t)cv * nu + cu] >> k & 1u)) { ok = false; break; }
                cu += route_du(k); cv += route_dv(k);
                if (cu < 0 || cv < 0 || cu >= nu || cv >= nv) { ok = false; break; }     // (no edge leaves the window)
                const uint32_t mq = m[(size_t)cv * nu + cu];
                sum += route_len(k) * (mc + mq);
                mc = mq;
            }
            if (ok) w[mv] = sum;
        }
    }
    wts[s] = make_uint2(w[CAR_F] | w[CAR_L] << 16, w[CAR_R] | w[CAR_B] << 16);
}

__global__ void __launch_bounds__(256) k_car_seed(CarArgs a, uint32_t G, const uint32_t *__restrict__ goal_first, const int *__restrict__ goals,
                                                  const uint8_t *__restrict__ m, uint32_t *cost, uint32_t *flags, uint32_t *info, uint32_t *counters)
{
    const uint32_t total = goal_first[G];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    uint32_t lo = 0, hi = G;           // the field f with goal_first[f] <= i < goal_first[f + 1]
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (goal_first[mid] <= i) lo = mid; else hi = mid;
    }
    const uint32_t f = lo;
    const int u = goals[3 * (size_t)i], v = goals[3 * (size_t)i + 1], h = goals[3 * (size_t)i + 2];
    if (u < 0 || v < 0 || u >= a.r.nu || v >= a.r.nv || h < -1 || h > 7) return;   // (the host has refused these)
    const size_t N = (size_t)a.r.nu * a.r.nv, c = (size_t)v * a.r.nu + u;
    if (!m[c]) { atomicAdd(&info[f * CAR_INFO_WORDS + CAR_I_DROPPED], 1u); return; }
    atomicAdd(&info[f * CAR_INFO_WORDS + CAR_I_USED], 1u);
    for (int k = 0; k < 8; ++k)
        if (h < 0 || h == k) __hip_atomic_store(&cost[((size_t)f * 8 + k) * N + c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const size_t tile = (size_t)(v / a.r.T) * a.r.tu + (u / a.r.T);
    if (atomicExch(&flags[(size_t)f * a.r.tu * a.r.tv + tile], 1u) == 0u) atomicAdd(&counters[CAR_C_SEEDED], 1u);
}

template <int T, int NT>
__global__ void __launch_bounds__(NT) k_car_relax(CarArgs a, uint32_t G, const uint2 *__restrict__ wts, uint32_t *cost, uint32_t *flags_now,
                                                   uint32_t *flags_next, uint32_t *counters, int round_word)
{
    constexpr int TT = T * T, PER = 8 * TT / NT;
    static_assert(TT % NT == 0, "a lane's states of one j share a heading");
    __shared__ uint32_t s_cost[8 * TT];
    __shared__ uint32_t s_border;

    const int nu = a.r.nu, nv = a.r.nv, n = a.n;
    const size_t tiles = (size_t)a.r.tu * a.r.tv;
    const size_t slot = blockIdx.x;                       // f * tiles + tile
    if (slot >= (size_t)G * tiles) return;
    if (flags_now[slot] == 0u) return;                    // (raised in an earlier launch, or never)
    const uint32_t f = (uint32_t)(slot / tiles);
    const int tile = (int)(slot % tiles), tx = tile % a.r.tu, ty = tile / a.r.tu;
    const int u0 = tx * T, v0 = ty * T;
    const size_t N = (size_t)nu * nv;
    uint32_t *fc = cost + (size_t)f * 8 * N;
    const int lane = threadIdx.x;
    if (lane == 0) {
        s_border = 0u;
        atomicAdd(&counters[CAR_C_VISITS], 1u);
    }

    // ---- this lane's states: local index i = lane + NT j = (h T + y) T + x.  Their costs to LDS, their weights to registers; the
    // moves that leave the tile folded into ext and struck
    uint2 w[PER];
    uint32_t ext[PER], first[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = lane + NT * j, x = i % T, y = (i / T) % T;
        const int h = (NT * j) / TT;                     // (compile time: TT is a multiple of NT)
        const int u = u0 + x, v = v0 + y;
        uint32_t c = ROUTE_NONE, best = ROUTE_NONE;
        uint2 wt = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
        if (u < nu && v < nv) {
            const size_t g = ((size_t)h * nv + v) * nu + u;
            c = __hip_atomic_load(&fc[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            wt = wts[g];
#pragma unroll
            for (int mv = 0; mv < CAR_MOVES; ++mv) {
                const uint32_t wm = car_weight(wt, mv);
                if (wm == CAR_NO_MOVE) continue;
                int dx, dy, ht;
                car_target(n, h, mv, dx, dy, ht);
                const int qx = x + dx, qy = y + dy;
                if (qx >= 0 && qy >= 0 && qx < T && qy < T) continue;          // inside the tile: the sweeps' business
                car_strike(wt, mv);
                const int qu = u0 + qx, qv = v0 + qy;
                if (qu < 0 || qv < 0 || qu >= nu || qv >= nv) continue;        // (a move that exists ends inside the window)
                const uint32_t cq = __hip_atomic_load(&fc[((size_t)ht * nv + qv) * nu + qu], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cq >= CAR_LIMIT) continue;
                const uint32_t cand = cq + wm;
                if (cand < CAR_LIMIT && cand < best) best = cand;
            }
        }
        s_cost[i] = c;
        first[j] = c;
        ext[j] = best;
        w[j] = wt;
    }
    __syncthreads();
    if (lane == 0) flags_now[slot] = 0u;                  // consumed (every lane has read it): nobody else touches this round's plane

    // ---- relax in LDS.  A lane writes its own states only; what it reads of the others' may be a sweep old, which delays and never
    // harms: every value is the weight of a sequence of moves
    int sweeps = 0, changed;
    do {
        changed = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if ((w[j].x & w[j].y) == 0xFFFFFFFFu && ext[j] == ROUTE_NONE) continue;
            const int i = lane + NT * j;
            const int h = (NT * j) / TT;
            const uint32_t old = s_cost[i];
            uint32_t best = ext[j] < old ? ext[j] : old;
#pragma unroll
            for (int mv = 0; mv < CAR_MOVES; ++mv) {
                const uint32_t wm = car_weight(w[j], mv);
                if (wm == CAR_NO_MOVE) continue;
                int dx, dy, ht;
                car_target(n, h, mv, dx, dy, ht);
                const int q = i + (ht - h) * TT + dy * T + dx;                  // inside the tile: the others were struck
                if (q < 0 || q >= 8 * TT) continue;
                const uint32_t cq = s_cost[q];
                if (cq >= CAR_LIMIT) continue;
                const uint32_t cand = cq + wm;
                if (cand < CAR_LIMIT && cand < best) best = cand;
            }
            if (best < old) { s_cost[i] = best; changed = 1; }
        }
        ++sweeps;
        changed = __syncthreads_or(changed);
    } while (changed && sweeps < a.r.sweeps);

    // ---- the changed states back, and which neighbours they concern: bit k = the tile in direction k, within 2 n cells of whose
    // facing border or corner a changed cell lies
    const int R = 2 * n;
    uint32_t border = 0u;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = lane + NT * j, x = i % T, y = (i / T) % T;
        const int h = (NT * j) / TT;
        const uint32_t c = s_cost[i];
        if (c >= first[j]) continue;
        const int u = u0 + x, v = v0 + y;
        if (u >= nu || v >= nv) continue;                  // (a state outside the window has no move and never changes)
        __hip_atomic_store(&fc[((size_t)h * nv + v) * nu + u], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int E = x >= T - R, W = x < R, S = y >= T - R, Nn = y < R;
        border |= (uint32_t)(E | (E & S) << 1 | S << 2 | (W & S) << 3 | W << 4 | (W & Nn) << 5 | Nn << 6 | (E & Nn) << 7);
    }
    if (border) atomicOr(&s_border, border);
    __syncthreads();
    if (lane < 8) {
        const int nx = tx + route_du(lane), ny = ty + route_dv(lane);
        if ((s_border >> lane & 1u) && nx >= 0 && ny >= 0 && nx < a.r.tu && ny < a.r.tv)
            if (atomicExch(&flags_next[(size_t)f * tiles + (size_t)ny * a.r.tu + nx], 1u) == 0u) atomicAdd(&counters[round_word], 1u);
    } else if (lane == 8 && changed) {                    // the cap ended the visit: the tile is not at rest yet
        if (atomicExch(&flags_next[slot], 1u) == 0u) atomicAdd(&counters[round_word], 1u);
    }
}

// `next` of the states of every field; block y strides over the fields.  next_out null: the info only.
__global__ void __launch_bounds__(256) k_car_next(CarArgs a, uint32_t G, const uint2 *__restrict__ wts, const uint32_t *__restrict__ cost,
                                                  uint8_t *__restrict__ next_out, uint32_t *info)
{
    __shared__ uint32_t s_states, s_cells, s_max;
    const int nu = a.r.nu, nv = a.r.nv;
    const size_t N = (size_t)nu * nv;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = c < N;
    const int u = in ? (int)(c % nu) : 0, v = in ? (int)(c / nu) : 0;
    for (uint32_t f = blockIdx.y; f < G; f += gridDim.y) {
        if (threadIdx.x == 0) { s_states = 0u; s_cells = 0u; s_max = 0u; }
        __syncthreads();
        if (in) {
            const uint32_t *fc = cost + (size_t)f * 8 * N;
            uint32_t states = 0u, most = 0u;
            for (int h = 0; h < 8; ++h) {
                const uint32_t cp = fc[(size_t)h * N + c];
                uint32_t nx = ROUTE_NEXT_NONE;
                if (cp < CAR_LIMIT) {
                    ++states;
                    most = cp > most ? cp : most;
                    if (cp == 0u) nx = ROUTE_NEXT_GOAL;
                    else {
                        const uint2 wt = wts[(size_t)h * N + c];
#pragma unroll
                        for (int mv = CAR_MOVES - 1; mv >= 0; --mv) {
                            const uint32_t wm = car_weight(wt, mv);
                            if (wm == CAR_NO_MOVE) continue;
                            int dx, dy, ht;
                            car_target(a.n, h, mv, dx, dy, ht);
                            const int qu = u + dx, qv = v + dy;
                            if (qu < 0 || qv < 0 || qu >= nu || qv >= nv) continue;   // (a move that exists ends inside the window)
                            const uint32_t cq = fc[((size_t)ht * nv + qv) * nu + qu];
                            if (cq >= CAR_LIMIT) continue;
                            if (cq + wm == cp) nx = (uint32_t)mv;
                        }
                    }
                }
                if (next_out) next_out[((size_t)f * 8 + h) * N + c] = (uint8_t)nx;
            }
            if (states) {
                atomicAdd(&s_states, states);
                atomicAdd(&s_cells, 1u);
                atomicMax(&s_max, most);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_states) {
            atomicAdd(&info[f * CAR_INFO_WORDS + CAR_I_STATES], s_states);
            atomicAdd(&info[f * CAR_INFO_WORDS + CAR_I_CELLS], s_cells);
            atomicMax(&info[f * CAR_INFO_WORDS + CAR_I_MAX], s_max);
        }
        __syncthreads();
    }
}

// path: [n_starts][max_steps + 1], filled with 0xFFFFFFFF before the launch (null: lengths and costs only)
__global__ void __launch_bounds__(256) k_car_walk(CarArgs a, uint32_t n_starts, const int *__restrict__ starts, const uint32_t *__restrict__ cost,
                                                  const uint8_t *__restrict__ next, uint32_t max_steps, uint32_t *__restrict__ path,
                                                  uint32_t *__restrict__ path_len, uint32_t *__restrict__ path_cost)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_starts) return;
    const int nu = a.r.nu, nv = a.r.nv;
    const size_t N = (size_t)nu * nv;
    const uint32_t f = (uint32_t)starts[4 * (size_t)i];
    int u = starts[4 * (size_t)i + 1], v = starts[4 * (size_t)i + 2], h = starts[4 * (size_t)i + 3] & 7;
    const uint32_t *fc = cost + (size_t)f * 8 * N;
    const uint8_t *fn = next + (size_t)f * 8 * N;
    const uint32_t c0 = fc[((size_t)h * nv + v) * nu + u];
    uint32_t len = 0;
    if (c0 != ROUTE_NONE) {
        uint32_t *row = path ? path + (size_t)i * ((size_t)max_steps + 1) : nullptr;
        if (row) row[0] = (uint32_t)((size_t)v * nu + u) | (uint32_t)h << 22;
        len = 1;
        bool inside = true;
        // at most max_steps + 1 words: every turn of the loop writes at least one, or ends it
        while (len <= max_steps && inside) {
            const int mv = fn[((size_t)h * nv + v) * nu + u];
            if (mv >= CAR_MOVES) break;
            const int cells = (mv == CAR_L || mv == CAR_R) ? 2 * a.n : 1;
            const int h2 = mv == CAR_L ? (h + 1) & 7 : mv == CAR_R ? (h + 7) & 7 : h;
            for (int s = 0; s < cells && s < 32 && len <= max_steps; ++s) {
                const int hs = (cells == 1 || s < a.n) ? h : h2;               // the heading this cell is passed with
                const int k = mv == CAR_B ? (h + 4) & 7 : hs;
                u += route_du(k); v += route_dv(k);
                if (u < 0 || v < 0 || u >= nu || v >= nv) { inside = false; break; }   // (a move that exists stays inside the window)
                if (row) row[len] = (uint32_t)((size_t)v * nu + u) | (uint32_t)hs << 22 | (uint32_t)(mv == CAR_B) << 25;
                ++len;
            }
            h = h2;
        }
    }
    path_len[i] = len;
    path_cost[i] = c0;
}

}  // namespace sm
