"""Routes a car can follow, restated (sm_route_car; include/sm_c_api.h, "routes a car can follow"; DESIGN.md "4ad. Routes for a
car").  This file is the contract the HIP path is compared with, bit for bit.  Everything is in integers.

Cells.      The window, passable, the multiplier m, the directions k = 0..7 with L_k and the unit edge p -> p + DIRS[k] with its
            existence rule and its cost e_k(p) = L_k * (m[p] + m[q]) are route_ref's (imported, not reworded).
States.     (u, v, h), heading h = direction k = h; plane index (h * nv + v) * nu + u.
Moves out of (p, h), by code:
  0 F       to (p + d_h, h) when the unit edge exists; weight e_h(p)
  1 L, 2 R  s = +1 / -1, h' = (h + s) & 7: n = turn_cells unit edges along d_h, then n along d_h'; exists when all 2 n exist; weight
            their sum + turn_cost; to (p + n d_h + n d_h', h')
  3 B       with reverse_weight > 0: to (p - d_h, h) when the unit edge in direction (h + 4) & 7 exists; weight reverse_weight * that edge
Goals.      (u, v, h) per field; h = -1 seeds all 8 headings; a goal in an impassable cell is dropped and counted.
cost.       The least total weight of a move sequence from the state to a goal state, 0 at goals, NONE where there is none; a
            candidate cost[target] + w >= 2^31 is never stored (the Dijkstra below, over the reversed graph, never pushes one: it
            stops at popped costs >= 2^31).
next.       8 at cost 0; 255 at NONE; else the smallest move code whose move exists with cost[target] + w == cost[state].
Paths.      Words cell | heading << 22 | reverse << 25: the start, then every unit cell passed along next until next == 8; an L or R
            gives 2 n cells, the first n with heading h, the rest with h'; B one cell with reverse 1.  path_len = min(words,
            max_steps + 1), path_cost = cost[start]; a start without a cost: length 0, cost NONE.

Worked by hand or on the prototype: EXAMPLES below (the header's)."""
import heapq

import numpy as np

import route_ref as rr
from route_ref import DIRS, FREE, LEN, NONE, OBSTACLE  # noqa: F401

F, L, R, B = range(4)
MOVES = ("F", "L", "R", "B")
NEXT_GOAL, NEXT_NONE = 8, 255
LIMIT = 1 << 31
MAX_WEIGHT = 32 * rr.MAX_EDGE + 4095
DEFAULTS = dict(body_cells=0, soft_cells=0, near_weight=0, unknown_passable=0, turn_cells=2, turn_cost=0, reverse_weight=0, max_steps=4096,
                rounds_per_check=4, max_rounds=65536)


def word(cell, h, reverse=0):
    return cell | h << 22 | reverse << 25


def move_table(m, e, turn_cells=2, turn_cost=0, reverse_weight=0, **_):
    """(exists bool[4, 8, nv, nu], weight int64[4, 8, nv, nu], offset: offset[mv][h] = (du, dv, h') of the move's target), by numpy:
    the polylines of all states at once"""
    nv, nu = m.shape
    n = turn_cells
    P = 2 * n + 1
    mi = m.astype(np.int64)
    bm = np.zeros((nv + 2 * P, nu + 2 * P), np.int64)
    bm[P:P + nv, P:P + nu] = mi
    be = np.zeros((8, nv + 2 * P, nu + 2 * P), bool)            # the unit edge k out of a cell exists
    bc = np.zeros((8, nv + 2 * P, nu + 2 * P), np.int64)        # ... and its cost
    for k, (du, dv) in enumerate(DIRS):
        be[k, P:P + nv, P:P + nu] = (e >> k) & 1
        bc[k, P:P + nv, P:P + nu] = LEN[k] * (mi + bm[P + dv:P + dv + nv, P + du:P + du + nu])
    at = lambda a, ox, oy: a[P + oy:P + oy + nv, P + ox:P + ox + nu]
    exists = np.zeros((4, 8, nv, nu), bool)
    weight = np.zeros((4, 8, nv, nu), np.int64)
    offset = [[None] * 8 for _ in range(4)]
    for h in range(8):
        du, dv = DIRS[h]
        exists[F, h], weight[F, h], offset[F][h] = at(be[h], 0, 0), at(bc[h], 0, 0), (du, dv, h)
        hb = (h + 4) & 7
        offset[B][h] = (-du, -dv, h)
        if reverse_weight > 0:
            exists[B, h], weight[B, h] = at(be[hb], 0, 0), reverse_weight * at(bc[hb], 0, 0)
        for mv, s in ((L, 1), (R, -1)):
            h2 = (h + s) & 7
            ok = np.ones((nv, nu), bool)
            total = np.full((nv, nu), turn_cost, np.int64)
            ox = oy = 0
            for i in range(2 * n):
                k = h if i < n else h2
                ok = ok & at(be[k], ox, oy)
                total = total + at(bc[k], ox, oy)
                ox, oy = ox + DIRS[k][0], oy + DIRS[k][1]
            exists[mv, h], weight[mv, h], offset[mv][h] = ok, total, (ox, oy, h2)
    weight[~exists] = 0
    assert weight.max(initial=0) <= MAX_WEIGHT
    return exists, weight, offset


def arcs(table, nu, nv):
    """per move code (source state indices, target state indices, weights), all int64, sources ascending"""
    exists, weight, offset = table
    N = nu * nv
    out = []
    for mv in range(4):
        src, tgt, w = [], [], []
        for h in range(8):
            du, dv, h2 = offset[mv][h]
            c = np.flatnonzero(exists[mv, h].reshape(-1))
            src.append(h * N + c)
            tgt.append(h2 * N + c + dv * nu + du)
            w.append(weight[mv, h].reshape(-1)[c])
        out.append((np.concatenate(src), np.concatenate(tgt), np.concatenate(w)))
    return out


def seeds(m, goals):
    """(the goal states in passable cells, goals used, goals dropped)"""
    nv, nu = m.shape
    N = nu * nv
    states, used, dropped = [], 0, 0
    for u, v, h in goals:
        assert 0 <= u < nu and 0 <= v < nv and -1 <= h <= 7
        if not m[v, u]:
            dropped += 1
            continue
        used += 1
        states += [k * N + v * nu + u for k in range(8) if h < 0 or h == k]
    return states, used, dropped


def dijkstra(m, table, goals):
    """(cost uint32[8, nv, nu], goals used, goals dropped) of one field: a binary heap over the states of the reversed graph"""
    nv, nu = m.shape
    S = 8 * nu * nv
    src, tgt, w = (np.concatenate(x) for x in zip(*arcs(table, nu, nv)))
    order = np.argsort(tgt, kind="stable")
    into_first = np.searchsorted(tgt[order], np.arange(S + 1)).tolist()   # the arcs into state t: order[into_first[t] : into_first[t + 1]]
    into_src, into_w = src[order].tolist(), w[order].tolist()
    cost = [NONE] * S
    goal_states, used, dropped = seeds(m, goals)
    heap = []
    for s in goal_states:
        if cost[s]:
            cost[s] = 0
            heap.append((0, s))
    heapq.heapify(heap)
    while heap:
        d, t = heapq.heappop(heap)
        if d != cost[t]:
            continue
        for i in range(into_first[t], into_first[t + 1]):
            nd = d + into_w[i]
            if nd < LIMIT and nd < cost[into_src[i]]:
                cost[into_src[i]] = nd
                heapq.heappush(heap, (nd, into_src[i]))
    return np.array(cost, np.uint32).reshape(8, nv, nu), used, dropped


def sweep_until_stable(m, table, goals):
    """the same cost by plain relaxation: every state along its moves, again and again, until nothing changes"""
    nv, nu = m.shape
    cost = np.full(8 * nu * nv, NONE, np.int64)
    cost[np.array(seeds(m, goals)[0], np.int64)] = 0
    moves = arcs(table, nu, nv)
    while True:
        new = cost.copy()
        for src, tgt, w in moves:
            cand = cost[tgt] + w
            ok = (cost[tgt] < LIMIT) & (cand < LIMIT)
            new[src[ok]] = np.minimum(new[src[ok]], cand[ok])
        if (new == cost).all():
            return cost.astype(np.uint32).reshape(8, nv, nu)
        cost = new


def next_of(cost, table):
    """uint8[8, nv, nu]: next as a function of cost"""
    _, nv, nu = cost.shape
    c = cost.astype(np.int64).reshape(-1)
    nxt = np.full(c.shape, NEXT_NONE, np.uint8)
    for mv, (src, tgt, w) in reversed(list(enumerate(arcs(table, nu, nv)))):
        ok = (c[tgt] < LIMIT) & (c[tgt] + w == c[src])
        nxt[src[ok]] = mv
    nxt[c == 0] = NEXT_GOAL
    nxt[c == NONE] = NEXT_NONE
    return nxt.reshape(8, nv, nu)


def move_cells(u, v, h, mv, n):
    """the unit cells move mv out of (u, v, h) passes: [(u, v, heading, reverse)], the last one the state it leads to"""
    if mv == F:
        return [(u + DIRS[h][0], v + DIRS[h][1], h, 0)]
    if mv == B:
        return [(u - DIRS[h][0], v - DIRS[h][1], h, 1)]
    h2 = (h + (1 if mv == L else -1)) & 7
    out = []
    for i in range(2 * n):
        k = h if i < n else h2
        u, v = u + DIRS[k][0], v + DIRS[k][1]
        out.append((u, v, k, 0))
    return out


def walk(cost, nxt, u, v, h, max_steps, n):
    """(words, path_len, path_cost) of one start; words has max_steps + 1 entries, padded with NONE"""
    _, nv, nu = cost.shape
    c0 = int(cost[h, v, u])
    if c0 == NONE:
        return [NONE] * (max_steps + 1), 0, NONE
    words = [word(v * nu + u, h)]
    while len(words) <= max_steps:
        mv = int(nxt[h, v, u])
        if mv >= 4:
            break
        for u, v, h, rev in move_cells(u, v, h, mv, n):
            assert 0 <= u < nu and 0 <= v < nv
            words.append(word(v * nu + u, h, rev))
    words = words[:max_steps + 1]
    return words + [NONE] * (max_steps + 1 - len(words)), len(words), c0


def add_paths(out, starts, max_steps, turn_cells):
    """path, path_len and path_cost of the starts (field, u, v, h) into the result `out`"""
    path = np.full((len(starts), max_steps + 1), NONE, np.uint32)
    plen = np.zeros(len(starts), np.uint32)
    pcost = np.zeros(len(starts), np.uint32)
    for i, (f, u, v, h) in enumerate(starts):
        assert 0 <= h <= 7
        path[i], plen[i], pcost[i] = walk(out["cost"][f], out["next"][f], u, v, h, max_steps, turn_cells)
    out.update(path=path, path_len=plen, path_cost=pcost)
    return out


def route_car(state, clear2, goals, starts=(), **params):
    """dict(cost uint32[G, 8, nv, nu], next uint8[G, 8, nv, nu], path uint32[n, max_steps + 1], path_len, path_cost uint32[n], info: per
    field dict(goals_used, goals_dropped, reachable_states, reachable_cells, max_cost), m, edge, table) of the goal sets `goals` (a
    list of lists of (u, v, h)) and the starts (field, u, v, h)"""
    p = dict(DEFAULTS, **params)
    state = np.asarray(state, np.uint8)
    clear2 = np.asarray(clear2, np.uint32)
    nv, nu = state.shape
    assert 1 <= nu <= 4096 and 1 <= nv <= 4096 and nu * nv <= rr.MAX_CELLS and len(goals) * nu * nv <= 1 << 23
    assert 1 <= p["turn_cells"] <= 16 and 0 <= p["turn_cost"] <= 4095 and 0 <= p["reverse_weight"] <= 15
    m = rr.multiplier(state, clear2, **p)
    e = rr.edges(m)
    table = move_table(m, e, **p)
    cost, nxt, info = [], [], []
    for g in goals:
        c, used, dropped = dijkstra(m, table, g)
        has = c != NONE
        cost.append(c)
        nxt.append(next_of(c, table))
        info.append(dict(goals_used=used, goals_dropped=dropped, reachable_states=int(has.sum()), reachable_cells=int(has.any(axis=0).sum()),
                         max_cost=int(c[has].max()) if has.any() else 0))
    out = dict(cost=np.stack(cost), next=np.stack(nxt), info=info, m=m, edge=e, table=table)
    add_paths(out, starts, p["max_steps"], p["turn_cells"])
    return out


# ---- the header's examples: (state, clear2, params, goals, [((u, v), the costs at h = 0..7 or {h: cost})])
def examples():
    N_ = NONE
    free = lambda nu, nv: (np.full((nv, nu), FREE, np.uint8), np.full((nv, nu), 9, np.uint32))
    s1, c1 = free(5, 3)
    s2, c2 = free(7, 7)
    s3, c3 = np.full((1, 4), FREE, np.uint8), np.array([[4, 1, 2, 4]], np.uint32)
    soft = dict(soft_cells=2, near_weight=8)
    return [
        dict(name="1", state=s1, clear2=c1, params=dict(turn_cells=1), goals=[(4, 1, -1)], at={(0, 1): [96, 116, N_, N_, N_, N_, N_, 116]}),
        dict(name="1, reverse", state=s1, clear2=c1, params=dict(turn_cells=1, reverse_weight=2), goals=[(4, 1, -1)],
             at={(0, 1): [96, 116, 290, 464, 192, 464, 290, 116]}),
        dict(name="1, one heading", state=s1, clear2=c1, params=dict(turn_cells=1, turn_cost=5), goals=[(4, 1, 0)],
             at={(0, 1): [96, N_, N_, N_, N_, N_, N_, N_]}),
        dict(name="2", state=s2, clear2=c2, params=dict(turn_cells=1), goals=[(0, 6, 4)], at={(3, 0): {0: 304}, (2, 0): {0: 280}, (4, 0): {0: N_}}),
        dict(name="2, turn cost", state=s2, clear2=c2, params=dict(turn_cells=1, turn_cost=9), goals=[(0, 6, 4)], at={(3, 0): {0: 340}}),
        dict(name="3", state=s3, clear2=c3, params=dict(turn_cells=1, reverse_weight=3, **soft), goals=[(3, 0, -1)],
             at={(u, 0): {0: a, 4: b} for u, (a, b) in enumerate(zip((312, 216, 72, 0), (936, 648, 216, 0)))}),
    ]


def check_example(ex, cost):
    """cost uint32[8, nv, nu] of example ex against what the header says"""
    for (u, v), want in ex["at"].items():
        for h, c in (enumerate(want) if isinstance(want, list) else want.items()):
            assert int(cost[h, v, u]) == c, (ex["name"], (u, v, h), int(cost[h, v, u]), c)


# ---- scenes: (state uint8[nv, nu], clear2 uint32[nv, nu])
def random_field(nu, nv, seed, density=0.03, reach_cells=8):
    """scattered single-cell obstacles (a car needs room: route_ref's density leaves (cell, heading) space in crumbs)"""
    return rr.random_field(nu, nv, seed, density=density, reach_cells=reach_cells)


def boxes(nu=130, nv=100):
    """an open window with a few boxes in it"""
    state = np.full((nv, nu), FREE, np.uint8)
    for u0, v0, w, h in ((20, 10, 6, 30), (60, 40, 25, 5), (95, 60, 8, 8), (10, 75, 30, 4), (5, 55, 10, 3)):
        state[v0:v0 + h, u0:u0 + w] = OBSTACLE
    return state, np.where(state == FREE, 9, 0).astype(np.uint32)
