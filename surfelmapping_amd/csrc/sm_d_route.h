// sm_d_route.h -- the cell rules of the routes over the ground map (sm_c_api.h's "routes": passable, multiplier, directions, edges),
// once, for the kernels of sm_k_route.h and of sm_k_car.h: device functions and constants only, no kernel.
#pragma once

#include "sm_device.h"

namespace sm {

constexpr uint32_t ROUTE_NONE = 0xFFFFFFFFu;             // SM_ROUTE_NONE
constexpr int ROUTE_NEXT_GOAL = 8, ROUTE_NEXT_NONE = 255;
constexpr int ROUTE_FREE = 1, ROUTE_UNKNOWN = 0;         // the ground map's states that may be passable

struct RouteArgs {
    int nu, nv;
    int body2;                         // body_cells^2
    int S2, near_weight;               // soft_cells^2 (0: every multiplier is 1)
    int unknown_passable;
    int T, tu, tv;                     // the tile edge; tiles along u and v
    int sweeps;                        // the cap on the sweeps of one visit
};

__device__ __forceinline__ int route_du(int k) { return (k == 0 || k == 1 || k == 7) ? 1 : (k >= 3 && k <= 5) ? -1 : 0; }
__device__ __forceinline__ int route_dv(int k) { return (k >= 1 && k <= 3) ? 1 : (k >= 5) ? -1 : 0; }
__device__ __forceinline__ uint32_t route_len(int k) { return (k & 1) ? 17u : 12u; }

// the multiplier of a cell inside the window, 0 if it is impassable
__device__ __forceinline__ uint32_t route_m(const RouteArgs &a, const uint8_t *state, const uint32_t *clear2, int u, int v)
{
    if (u < 0 || v < 0 || u >= a.nu || v >= a.nv) return 0u;
    const size_t c = (size_t)v * a.nu + u;
    const int st = state[c];
    if (!(st == ROUTE_FREE || (st == ROUTE_UNKNOWN && a.unknown_passable))) return 0u;
    const uint32_t c2 = clear2[c];
    if (c2 < (uint32_t)a.body2) return 0u;
    if (a.S2 == 0) return 1u;
    const uint32_t lim = c2 < (uint32_t)a.S2 ? c2 : (uint32_t)a.S2;
    return 1u + ((uint32_t)a.near_weight * ((uint32_t)a.S2 - lim)) / (uint32_t)a.S2;
}

// the edge bits of the cell (u, v) whose multiplier is mp: bit k = the edge in direction k exists, the window's border and the
// corner rule applied
__device__ __forceinline__ uint32_t route_edge_bits(const RouteArgs &a, const uint8_t *state, const uint32_t *clear2, int u, int v, uint32_t mp)
{
    uint32_t e = 0;
    if (mp) {
        uint32_t pass = 0;             // bit k: the neighbour in direction k is in the window and passable
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (route_m(a, state, clear2, u + route_du(k), v + route_dv(k))) pass |= 1u << k;
        e = pass & 0x55u;
#pragma unroll
        for (int k = 1; k < 8; k += 2)                   // a diagonal needs both cells beside it: k - 1 and k + 1 are those
            if ((pass >> k & 1u) && (pass >> (k - 1) & 1u) && (pass >> ((k + 1) & 7) & 1u)) e |= 1u << k;
    }
    return e;
}

}  // namespace sm
