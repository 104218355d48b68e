// sm_k_route.h -- routes over the ground map (DESIGN.md "4ac. Routes"; the specification is sm_c_api.h's "routes").  Included by
// sm_route.hip only.  Planes are row-major over the window: cell (u, v) at v * nu + u; field f's planes start at f * nu * nv.
//   k_route_prepare    one lane per cell: the byte m (the multiplier, 0 = impassable) and the byte of edge bits (bit k: the edge in
//                      direction k exists, the window's border and the corner rule applied).  Shared by every field
//   k_route_seed       one lane per goal: a passable goal gets cost 0 and raises its tile's flag of round 0; the goals by field to
//                      the info words
//   k_route_relax<T>   one workgroup of 256 lanes per (field, tile of T x T cells) whose flag of this round is up: the tile's costs
//                      and a one-cell halo, the m bytes of both in LDS; each lane owns T * T / 256 cells and lowers them from their
//                      8 neighbours, sweep after sweep, until a sweep changes nothing or the sweep cap (then the tile raises its own
//                      flag of the next round); the changed cells go back to the plane, and each of the 8 neighbouring tiles whose
//                      facing border row, column or corner changed gets its flag of the next round raised
//   k_route_next       one lane per cell and field: `next` from `cost`; the reachable cells and the largest cost to the info words
//   k_route_walk       one lane per start: the path along `next`
// No workgroup waits for another, and none relies on seeing another's stores within a launch: a halo cell is read as it is found,
// and whatever it holds is the cost of a real path or ROUTE_NONE (costs only fall, every store is a whole 32-bit word).  The cells
// another tile may write in the same launch are read, and every cell is written, with relaxed agent-scope atomics, so the compiler
// assumes nothing about them; the flags are raised with atomics and read in the NEXT launch only.  Every loop has a fixed bound.
// Every index is checked against the window before it is used.  Nothing is ever added to ROUTE_NONE.
#pragma once

#include "sm_d_route.h"

namespace sm {

// the info words of a field: goals used, goals dropped, reachable cells, largest cost
enum { ROUTE_I_USED = 0, ROUTE_I_DROPPED, ROUTE_I_REACHED, ROUTE_I_MAX, ROUTE_INFO_WORDS };
// the counter block: tile visits, then per round of a batch the flags it raised for the next
enum { ROUTE_C_VISITS = 0, ROUTE_C_SEEDED = 1, ROUTE_C_ROUND0 = 2, ROUTE_MAX_BATCH = 64, ROUTE_COUNTER_WORDS = ROUTE_C_ROUND0 + ROUTE_MAX_BATCH };

__global__ void __launch_bounds__(256) k_route_prepare(RouteArgs a, const uint8_t *__restrict__ state, const uint32_t *__restrict__ clear2,
                                                       uint8_t *__restrict__ m, uint8_t *__restrict__ edge)
{
    const size_t N = (size_t)a.nu * a.nv;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    const int u = (int)(c % a.nu), v = (int)(c / a.nu);
    const uint32_t mp = route_m(a, state, clear2, u, v);
    const uint32_t e = route_edge_bits(a, state, clear2, u, v, mp);
    m[c] = (uint8_t)mp;
    edge[c] = (uint8_t)e;
}

__global__ void __launch_bounds__(256) k_route_seed(RouteArgs a, uint32_t G, const uint32_t *__restrict__ goal_first, const int *__restrict__ goals,
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
    const int u = goals[2 * (size_t)i], v = goals[2 * (size_t)i + 1];
    if (u < 0 || v < 0 || u >= a.nu || v >= a.nv) return;              // (the host has refused these)
    const size_t N = (size_t)a.nu * a.nv, c = (size_t)v * a.nu + u;
    if (!m[c]) { atomicAdd(&info[f * ROUTE_INFO_WORDS + ROUTE_I_DROPPED], 1u); return; }
    atomicAdd(&info[f * ROUTE_INFO_WORDS + ROUTE_I_USED], 1u);
    __hip_atomic_store(&cost[f * N + c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const size_t tile = (size_t)(v / a.T) * a.tu + (u / a.T);
    if (atomicExch(&flags[(size_t)f * a.tu * a.tv + tile], 1u) == 0u) atomicAdd(&counters[ROUTE_C_SEEDED], 1u);
}

// the LDS row stride of a tile of T cells and its halo: rows of consecutive lanes' cells stay on distinct banks, and for T = 16,
// where a 32-lane group covers two rows, the second row starts 16 banks after the first
template <int T> struct RouteTile {
    static constexpr int STRIDE = T == 16 ? 48 : T + 2;
    static constexpr int ROWS = T + 2;
    static constexpr int PER_LANE = T * T / 256;
};

template <int T>
__global__ void __launch_bounds__(256) k_route_relax(RouteArgs a, uint32_t G, const uint8_t *__restrict__ m, const uint8_t *__restrict__ edge,
                                                     uint32_t *cost, uint32_t *flags_now, uint32_t *flags_next, uint32_t *counters, int round_word)
{
    using RT = RouteTile<T>;
    constexpr int STRIDE = RT::STRIDE, ROWS = RT::ROWS, PER = RT::PER_LANE;
    __shared__ uint32_t s_cost[ROWS * STRIDE];
    __shared__ uint8_t s_m[ROWS * STRIDE];
    __shared__ uint32_t s_border;

    const size_t tiles = (size_t)a.tu * a.tv;
    const size_t slot = blockIdx.x;                       // f * tiles + tile
    if (slot >= (size_t)G * tiles) return;
    if (flags_now[slot] == 0u) return;                    // (raised in an earlier launch, or never)
    const uint32_t f = (uint32_t)(slot / tiles);
    const int tile = (int)(slot % tiles), tx = tile % a.tu, ty = tile / a.tu;
    const int u0 = tx * T, v0 = ty * T;
    const size_t N = (size_t)a.nu * a.nv;
    uint32_t *fc = cost + (size_t)f * N;
    const int lane = threadIdx.x;
    if (lane == 0) {
        s_border = 0u;
        atomicAdd(&counters[ROUTE_C_VISITS], 1u);
    }

    // ---- the tile and its halo: cells outside the window are NONE and impassable
    for (int i = lane; i < ROWS * ROWS; i += 256) {
        const int x = i % ROWS, y = i / ROWS;             // local, the halo included: the cell (u0 + x - 1, v0 + y - 1)
        const int u = u0 + x - 1, v = v0 + y - 1;
        uint32_t c = ROUTE_NONE, mm = 0u;
        if (u >= 0 && v >= 0 && u < a.nu && v < a.nv) {
            const size_t g = (size_t)v * a.nu + u;
            c = __hip_atomic_load(&fc[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mm = m[g];
        }
        s_cost[y * STRIDE + x] = c;
        s_m[y * STRIDE + x] = (uint8_t)mm;
    }
    // ---- this lane's cells: local linear index lane + 256 j, so that the lanes of a wave hold neighbouring cells of a row
    uint32_t em[PER], first[PER];                         // edge bits | m << 8; the cost the visit found
    __syncthreads();
    if (lane == 0) flags_now[slot] = 0u;                  // consumed (every lane has read it): nobody else touches this round's plane
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = lane + 256 * j, x = i % T, y = i / T;
        const int u = u0 + x, v = v0 + y;
        uint32_t e = 0u;
        if (u < a.nu && v < a.nv) e = edge[(size_t)v * a.nu + u];
        const int at = (y + 1) * STRIDE + (x + 1);
        em[j] = e | ((uint32_t)s_m[at] << 8);
        first[j] = s_cost[at];
    }

    // ---- relax in LDS.  A lane writes its own cells only; what it reads of the others' may be a sweep old, which delays and never
    // harms: every value is the cost of a path
    int sweeps = 0, changed;
    do {
        changed = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const uint32_t e = em[j] & 0xFFu;
            if (!e) continue;
            const int i = lane + 256 * j, x = i % T, y = i / T;
            const int at = (y + 1) * STRIDE + (x + 1);
            const uint32_t mp = em[j] >> 8;
            const uint32_t old = s_cost[at];
            uint32_t best = old;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!(e >> k & 1u)) continue;
                const int q = at + route_dv(k) * STRIDE + route_du(k);
                const uint32_t cq = s_cost[q];
                if (cq == ROUTE_NONE) continue;
                const uint32_t cand = cq + route_len(k) * (mp + s_m[q]);
                best = cand < best ? cand : best;
            }
            if (best < old) { s_cost[at] = best; changed = 1; }
        }
        ++sweeps;
        changed = __syncthreads_or(changed);
    } while (changed && sweeps < a.sweeps);

    // ---- the changed cells back, and which borders they lie on: bit k = the border facing the neighbouring tile in direction k
    uint32_t border = 0u;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = lane + 256 * j, x = i % T, y = i / T;
        const uint32_t c = s_cost[(y + 1) * STRIDE + (x + 1)];
        if (c >= first[j]) continue;
        const int u = u0 + x, v = v0 + y;                 // (inside the window: a cell outside has no edge and never changes)
        __hip_atomic_store(&fc[(size_t)v * a.nu + u], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int E = x == T - 1, W = x == 0, S = y == T - 1, Nn = y == 0;
        border |= (uint32_t)(E | (E & S) << 1 | S << 2 | (W & S) << 3 | W << 4 | (W & Nn) << 5 | Nn << 6 | (E & Nn) << 7);
    }
    if (border) atomicOr(&s_border, border);
    __syncthreads();
    if (lane < 8) {
        const int nx = tx + route_du(lane), ny = ty + route_dv(lane);
        if ((s_border >> lane & 1u) && nx >= 0 && ny >= 0 && nx < a.tu && ny < a.tv)
            if (atomicExch(&flags_next[(size_t)f * tiles + (size_t)ny * a.tu + nx], 1u) == 0u) atomicAdd(&counters[round_word], 1u);
    } else if (lane == 8 && changed) {                    // the cap ended the visit: the tile is not at rest yet
        if (atomicExch(&flags_next[slot], 1u) == 0u) atomicAdd(&counters[round_word], 1u);
    }
}

// `next` of the cells of every field; block y strides over the fields, so a block's lanes share one.  next_out null: the info only.
__global__ void __launch_bounds__(256) k_route_next(RouteArgs a, uint32_t G, const uint8_t *__restrict__ m, const uint8_t *__restrict__ edge,
                                                    const uint32_t *__restrict__ cost, uint8_t *__restrict__ next_out, uint32_t *info)
{
    __shared__ uint32_t s_reached, s_max;
    const size_t N = (size_t)a.nu * a.nv;
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = c < N;
    const int u = in ? (int)(c % a.nu) : 0, v = in ? (int)(c / a.nu) : 0;
    const uint32_t mp = in ? m[c] : 0u, e = in ? edge[c] : 0u;
    for (uint32_t f = blockIdx.y; f < G; f += gridDim.y) {
        if (threadIdx.x == 0) { s_reached = 0u; s_max = 0u; }
        __syncthreads();
        if (in) {
            const uint32_t *fc = cost + (size_t)f * N;
            const uint32_t cp = fc[c];
            uint32_t nx = ROUTE_NEXT_NONE;
            if (mp && cp != ROUTE_NONE) {
                atomicAdd(&s_reached, 1u);
                atomicMax(&s_max, cp);
                if (cp == 0u) nx = ROUTE_NEXT_GOAL;
                else {
#pragma unroll
                    for (int k = 7; k >= 0; --k) {
                        if (!(e >> k & 1u)) continue;
                        const size_t q = (size_t)(v + route_dv(k)) * a.nu + (u + route_du(k));
                        const uint32_t cq = fc[q];
                        if (cq == ROUTE_NONE) continue;
                        if (cq + route_len(k) * (mp + m[q]) == cp) nx = (uint32_t)k;
                    }
                }
            }
            if (next_out) next_out[(size_t)f * N + c] = (uint8_t)nx;
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_reached) {
            atomicAdd(&info[f * ROUTE_INFO_WORDS + ROUTE_I_REACHED], s_reached);
            atomicMax(&info[f * ROUTE_INFO_WORDS + ROUTE_I_MAX], s_max);
        }
    }
}

// path: [n_starts][max_steps + 1], filled with 0xFFFFFFFF before the launch (null: lengths and costs only)
__global__ void __launch_bounds__(256) k_route_walk(RouteArgs a, uint32_t n_starts, const int *__restrict__ starts, const uint32_t *__restrict__ cost,
                                                    const uint8_t *__restrict__ next, uint32_t max_steps, uint32_t *__restrict__ path,
                                                    uint32_t *__restrict__ path_len, uint32_t *__restrict__ path_cost)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_starts) return;
    const size_t N = (size_t)a.nu * a.nv;
    const uint32_t f = (uint32_t)starts[3 * (size_t)i];
    int u = starts[3 * (size_t)i + 1], v = starts[3 * (size_t)i + 2];
    const uint32_t *fc = cost + (size_t)f * N;
    const uint8_t *fn = next + (size_t)f * N;
    const uint32_t c0 = fc[(size_t)v * a.nu + u];
    uint32_t len = 0;
    if (c0 != ROUTE_NONE) {
        uint32_t *row = path ? path + (size_t)i * ((size_t)max_steps + 1) : nullptr;
        for (;;) {                     // at most max_steps + 1 cells, each inside the window (an edge never leaves it)
            const size_t c = (size_t)v * a.nu + u;
            if (row) row[len] = (uint32_t)c;
            ++len;
            const int k = fn[c];
            if (k >= 8 || len > max_steps) break;
            u += route_du(k); v += route_dv(k);
            if (u < 0 || v < 0 || u >= a.nu || v >= a.nv) break;
        }
    }
    path_len[i] = len;
    path_cost[i] = c0;
}

}  // namespace sm
