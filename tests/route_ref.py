"""Routes over the ground map, restated (sm_route_ground; include/sm_c_api.h, "routes"; DESIGN.md "4ac. Routes").  This file is the
contract the HIP path is compared with, bit for bit.  Everything is in integers.

Window.     nu x nv cells, planes row-major: cell (u, v) at [v, u], its number v * nu + u.
Passable.   (state == FREE, or state == UNKNOWN and unknown_passable) and clear2 >= body_cells^2.
Multiplier. S2 = soft_cells^2; m = 1 if soft_cells == 0 else 1 + (near_weight * (S2 - min(clear2, S2))) // S2.  0 here: impassable.
Directions. k = 0..7: (du, dv) = DIRS[k]; L_k = 12 for even k, 17 for odd k.
Edges.      p -> q = p + DIRS[k] exists when p and q are in the window and passable and, for odd k, (pu + du, pv) and (pu, pv + dv) are
            passable too.  Its cost is L_k * (m[p] + m[q]).
cost.       The shortest-path distance to the nearest passable goal of the field, NONE where there is none.
next.       8 at cost 0; 255 impassable or unreachable; else the smallest k whose edge exists with cost[q] + w == cost[p].
Paths.      From a start along next to a cell with next == 8; path_len = min(cells, max_steps + 1), path_cost = cost[start]; a start
            without a cost: length 0, cost NONE.

Worked by hand: EXAMPLES below (the header's)."""
import heapq

import numpy as np

NONE = 0xFFFFFFFF
NEXT_GOAL, NEXT_NONE = 8, 255
UNKNOWN, FREE, OBSTACLE, STEP = range(4)
DIRS = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
LEN = (12, 17, 12, 17, 12, 17, 12, 17)
DEFAULTS = dict(body_cells=0, soft_cells=0, near_weight=0, unknown_passable=0, max_steps=4096, rounds_per_check=4, max_rounds=65536)
MAX_EDGE = 17 * 30                       # L_k * (m[p] + m[q]) at most
MAX_CELLS = 1 << 22


def multiplier(state, clear2, body_cells=0, soft_cells=0, near_weight=0, unknown_passable=0, **_):
    """uint8[nv, nu]: m of a passable cell, 0 of an impassable one"""
    state = np.asarray(state)
    clear2 = np.asarray(clear2).astype(np.int64)
    ok = (state == FREE) | ((state == UNKNOWN) & bool(unknown_passable))
    ok &= clear2 >= body_cells * body_cells
    if soft_cells == 0:
        m = np.ones(state.shape, np.int64)
    else:
        s2 = soft_cells * soft_cells
        m = 1 + (near_weight * (s2 - np.minimum(clear2, s2))) // s2
    return np.where(ok, m, 0).astype(np.uint8)


def edges(m):
    """uint8[nv, nu]: bit k = the edge in direction k exists"""
    nv, nu = m.shape
    big = np.zeros((nv + 2, nu + 2), bool)
    big[1:-1, 1:-1] = m > 0
    at = lambda du, dv: big[1 + dv:1 + dv + nv, 1 + du:1 + du + nu]
    e = np.zeros((nv, nu), np.uint8)
    for k, (du, dv) in enumerate(DIRS):
        ok = at(0, 0) & at(du, dv)
        if k & 1:
            ok = ok & at(du, 0) & at(0, dv)
        e |= (ok.astype(np.uint8) << k).astype(np.uint8)
    return e


def dijkstra(m, e, goals):
    """(cost uint32[nv, nu], goals used, goals dropped) of one field: a binary heap over the cells"""
    nv, nu = m.shape
    cost = [NONE] * (nu * nv)
    mm = m.reshape(-1).tolist()
    ee = e.reshape(-1).tolist()
    heap = []
    used = dropped = 0
    for u, v in goals:
        assert 0 <= u < nu and 0 <= v < nv
        c = v * nu + u
        if not mm[c]:
            dropped += 1
            continue
        used += 1
        if cost[c]:
            cost[c] = 0
            heap.append((0, c))
    heapq.heapify(heap)
    step = [dv * nu + du for du, dv in DIRS]
    while heap:
        d, c = heapq.heappop(heap)
        if d != cost[c]:
            continue
        ec, mc = ee[c], mm[c]
        for k in range(8):
            if ec >> k & 1:
                q = c + step[k]
                nd = d + LEN[k] * (mc + mm[q])
                if nd < cost[q]:
                    cost[q] = nd
                    heapq.heappush(heap, (nd, q))
    return np.array(cost, np.uint32).reshape(nv, nu), used, dropped


def sweep_until_stable(m, e, goals):
    """the same cost by plain relaxation: every cell from its 8 neighbours, again and again, until nothing changes"""
    nv, nu = m.shape
    big = np.full((nv + 2, nu + 2), NONE, np.int64)
    bm = np.zeros((nv + 2, nu + 2), np.int64)
    bm[1:-1, 1:-1] = m
    for u, v in goals:
        if m[v, u]:
            big[v + 1, u + 1] = 0
    mi = m.astype(np.int64)
    while True:
        cur = big[1:-1, 1:-1]
        best = cur.copy()
        for k, (du, dv) in enumerate(DIRS):
            q = big[1 + dv:1 + dv + nv, 1 + du:1 + du + nu]
            qm = bm[1 + dv:1 + dv + nv, 1 + du:1 + du + nu]
            ok = ((e >> k) & 1).astype(bool) & (q != NONE)
            best = np.where(ok, np.minimum(best, q + LEN[k] * (mi + qm)), best)
        if (best == cur).all():
            return cur.astype(np.uint32)
        big[1:-1, 1:-1] = best


def next_of(cost, m, e):
    """uint8[nv, nu]: next as a function of cost"""
    nv, nu = cost.shape
    c = cost.astype(np.int64)
    big = np.full((nv + 2, nu + 2), NONE, np.int64)
    big[1:-1, 1:-1] = c
    bm = np.zeros((nv + 2, nu + 2), np.int64)
    bm[1:-1, 1:-1] = m
    mi = m.astype(np.int64)
    nxt = np.full((nv, nu), NEXT_NONE, np.uint8)
    for k in range(7, -1, -1):
        du, dv = DIRS[k]
        q = big[1 + dv:1 + dv + nv, 1 + du:1 + du + nu]
        qm = bm[1 + dv:1 + dv + nv, 1 + du:1 + du + nu]
        ok = ((e >> k) & 1).astype(bool) & (q != NONE) & (q + LEN[k] * (mi + qm) == c)
        nxt[ok] = k
    nxt[c == 0] = NEXT_GOAL
    nxt[(m == 0) | (c == NONE)] = NEXT_NONE
    return nxt


def walk(cost, nxt, u, v, max_steps):
    """(cells, path_len, path_cost) of one start; cells has max_steps + 1 entries, padded with NONE"""
    nv, nu = cost.shape
    cells = [NONE] * (max_steps + 1)
    c0 = int(cost[v, u])
    if c0 == NONE:
        return cells, 0, NONE
    n = 0
    while True:
        cells[n] = v * nu + u
        n += 1
        k = int(nxt[v, u])
        if k >= 8 or n > max_steps:
            break
        u, v = u + DIRS[k][0], v + DIRS[k][1]
    return cells, n, c0


def route(state, clear2, goals, starts=(), **params):
    """dict(cost uint32[G, nv, nu], next uint8[G, nv, nu], path uint32[n, max_steps + 1], path_len, path_cost uint32[n], info: per field
    dict(goals_used, goals_dropped, reachable, max_cost), m, edge) of the goal sets `goals` (a list of lists of (u, v)) and the starts
    (field, u, v)"""
    p = dict(DEFAULTS, **params)
    state = np.asarray(state, np.uint8)
    clear2 = np.asarray(clear2, np.uint32)
    nv, nu = state.shape
    assert 1 <= nu <= 4096 and 1 <= nv <= 4096 and nu * nv <= MAX_CELLS
    m = multiplier(state, clear2, **p)
    e = edges(m)
    cost, nxt, info = [], [], []
    for g in goals:
        c, used, dropped = dijkstra(m, e, g)
        reached = c[c != NONE]
        cost.append(c)
        nxt.append(next_of(c, m, e))
        info.append(dict(goals_used=used, goals_dropped=dropped, reachable=int(reached.size), max_cost=int(reached.max()) if reached.size else 0))
    out = dict(cost=np.stack(cost), next=np.stack(nxt), info=info, m=m, edge=e)
    ms = p["max_steps"]
    path = np.full((len(starts), ms + 1), NONE, np.uint32)
    plen = np.zeros(len(starts), np.uint32)
    pcost = np.zeros(len(starts), np.uint32)
    for i, (f, u, v) in enumerate(starts):
        cells, n, c0 = walk(out["cost"][f], out["next"][f], u, v, ms)
        path[i], plen[i], pcost[i] = cells, n, c0
    out.update(path=path, path_len=plen, path_cost=pcost)
    return out


def edge_cost(m, a, b, nu):
    """the cost of the edge between the neighbouring cells numbered a and b"""
    (ua, va), (ub, vb) = (a % nu, a // nu), (b % nu, b // nu)
    assert max(abs(ua - ub), abs(va - vb)) == 1
    return (17 if ua != ub and va != vb else 12) * (int(m[va, ua]) + int(m[vb, ub]))


# ---- the header's examples: (state, clear2, goals, params, expected cost by rows, expected m or None)
def examples():
    s1 = np.full((3, 3), FREE, np.uint8)
    s1[1, 1] = OBSTACLE
    c1 = np.full((3, 3), 9, np.uint32)
    c1[1, 1] = 0
    e1 = np.array([[0, 24, 48], [24, NONE, 72], [48, 72, 96]], np.uint32)
    s2 = np.full((1, 4), FREE, np.uint8)
    c2 = np.array([[4, 1, 2, 4]], np.uint32)
    e2 = np.array([[312, 216, 72, 0]], np.uint32)
    return [dict(state=s1, clear2=c1, goals=[[(0, 0)]], params=dict(body_cells=0, soft_cells=0), cost=e1, m=None),
            dict(state=s2, clear2=c2, goals=[[(3, 0)]], params=dict(soft_cells=2, near_weight=8), cost=e2, m=np.array([[1, 7, 5, 1]], np.uint8))]


# ---- scenes: (state uint8[nv, nu], clear2 uint32[nv, nu])
def clearance(state, reach_cells=8):
    """clear2 of a state plane as the ground map defines it: min(reach^2, squared distance to the nearest blocking cell)"""
    nv, nu = state.shape
    block = np.argwhere(state != FREE)
    vv, uu = np.mgrid[0:nv, 0:nu]
    best = np.full((nv, nu), reach_cells * reach_cells, np.int64)
    for bv, bu in block:
        np.minimum(best, (vv - bv) ** 2 + (uu - bu) ** 2, out=best)
    return best.astype(np.uint32)


def random_field(nu, nv, seed, density=0.30, reach_cells=8):
    rng = np.random.default_rng(seed)
    state = np.where(rng.random((nv, nu)) < density, OBSTACLE, FREE).astype(np.uint8)
    return state, clearance(state, reach_cells)


def serpentine(nu, nv, every=4, reach_cells=1):
    """walls in every `every`-th column, open at alternating ends: one long corridor from the left edge to the right"""
    state = np.full((nv, nu), FREE, np.uint8)
    for i, u in enumerate(range(every - 1, nu - 1, every)):
        state[:, u] = OBSTACLE
        state[nv - 1 if i % 2 == 0 else 0, u] = FREE
    return state, clearance(state, reach_cells) if nu * nv <= 1 << 14 else np.where(state == FREE, 1, 0).astype(np.uint32)


def pockets(nu=24, nv=20):
    """an open field with a walled pocket at (4..8, 4..8): what is inside cannot leave, what is outside cannot enter"""
    state = np.full((nv, nu), FREE, np.uint8)
    state[3:10, 3] = state[3:10, 9] = OBSTACLE
    state[3, 3:10] = state[9, 3:10] = OBSTACLE
    return state, clearance(state, 4)


def detour(nu=21, nv=9):
    """a straight lane along v = 4 hugging a wall (row 5), open space above: cheap cells lie away from the wall"""
    state = np.full((nv, nu), FREE, np.uint8)
    state[5, 2:nu - 2] = OBSTACLE
    return state, clearance(state, 4)
