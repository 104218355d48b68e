"""Routes over the ground map (sm_route_ground, sm_route_stats; capi.route_ground; DESIGN.md "4ac. Routes").
CPU: the restatement (route_ref.py) against the header's two examples worked by hand, its Dijkstra against a plain relaxation, the
overflow bound, `next` as a function of `cost`; the library's symbols, defaults, header and the argument rules that need no device.
GPU: cost, next, the paths and info of the HIP path against the restatement, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from surfelmapping_amd.capi import SmRouteParams  # noqa: F401  (the binding's symbol: without it nothing here can run)

import route_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sm_default_route_params", "sm_route_ground", "sm_route_stats")
SOFT = dict(soft_cells=3, near_weight=14)
# the random fields: (nu, nv, seed, body_cells) -- a seed and a goal set (random_case) with which, in the restatement alone, at least
# half of the passable cells are reachable and at least one is not (asserted in the test): 758 of 765 at 33 x 33 with body_cells 0
RANDOM_FIELDS = ((33, 33, 3, 0), (33, 33, 3, 2), (65, 40, 3, 0), (65, 40, 3, 2))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_header_examples():
    one, two = rr.examples()
    got = rr.route(one["state"], one["clear2"], one["goals"], starts=[(0, 2, 2), (0, 1, 1)], **one["params"])
    assert got["cost"][0].tolist() == [[0, 24, 48], [24, rr.NONE, 72], [48, 72, 96]]
    assert got["next"][0].tolist() == [[8, 4, 4], [6, 255, 6], [6, 4, 4]]
    assert got["next"][0, 2, 2] == 4                                           # 4 and 6 both reach 96: the smaller wins
    assert got["path"][0, :5].tolist() == [8, 7, 6, 3, 0] and got["path_len"].tolist() == [5, 0] and got["path_cost"].tolist() == [96, rr.NONE]
    assert got["info"] == [dict(goals_used=1, goals_dropped=0, reachable=8, max_cost=96)]
    got = rr.route(two["state"], two["clear2"], two["goals"], **two["params"])
    assert got["m"].tolist() == [[1, 7, 5, 1]] and got["cost"][0].tolist() == [[312, 216, 72, 0]]
    assert got["next"][0].tolist() == [[0, 0, 0, 8]]
    for ex in (one, two):
        assert (rr.route(ex["state"], ex["clear2"], ex["goals"], **ex["params"])["cost"][0] == ex["cost"]).all()


def test_bound_leaves_no_overflow():
    assert rr.MAX_EDGE == 510 == 17 * (15 + 15) and rr.MAX_EDGE * rr.MAX_CELLS < 1 << 31
    m = rr.multiplier(np.full((1, 2), rr.FREE), np.zeros((1, 2)), soft_cells=255, near_weight=14)
    assert m.tolist() == [[15, 15]]


@pytest.mark.parametrize("seed", (1, 2, 3))
@pytest.mark.parametrize("body", (0, 1))
def test_dijkstra_equals_relaxation(seed, body):
    state, clear2 = rr.random_field(23, 17, seed, density=0.25)
    p = dict(body_cells=body, **SOFT)
    m = rr.multiplier(state, clear2, **p)
    e = rr.edges(m)
    free = np.argwhere(m > 0)
    goals = [(int(free[0][1]), int(free[0][0])), (int(free[-1][1]), int(free[-1][0])), (0, 0)]
    cost, used, dropped = rr.dijkstra(m, e, goals)
    assert used + dropped == 3 and used >= 2
    assert (cost == rr.sweep_until_stable(m, e, goals)).all()
    # edges are symmetric, and a diagonal edge implies both straight ones beside it
    nv, nu = m.shape
    for k, (du, dv) in enumerate(rr.DIRS):
        bit = (e >> k) & 1
        back = np.zeros_like(bit)
        v0, v1, u0, u1 = max(0, -dv), nv - max(0, dv), max(0, -du), nu - max(0, du)
        back[v0:v1, u0:u1] = ((e >> ((k + 4) % 8)) & 1)[v0 + dv:v1 + dv, u0 + du:u1 + du]
        assert (bit == back).all(), k


@pytest.mark.parametrize("nu,nv,seed,body", RANDOM_FIELDS)
def test_next_is_a_function_of_cost(nu, nv, seed, body):
    want, _ = random_case(nu, nv, seed, body)
    cost, nxt, m = want["cost"][0], want["next"][0], want["m"]
    assert (nxt == rr.next_of(cost, m, want["edge"])).all()
    # ... and says what it should: along next the cost falls by the edge's cost
    for v, u in np.argwhere(nxt < 8):
        du, dv = rr.DIRS[nxt[v, u]]
        assert int(cost[v + dv, u + du]) + rr.edge_cost(m, v * nu + u, (v + dv) * nu + u + du, nu) == int(cost[v, u])
    assert ((nxt == 8) == (cost == 0)).all() and ((nxt == 255) == (cost == rr.NONE)).all()


def test_library_exports_defaults_and_binding():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None and name in capi.SYMBOLS
    p = capi.route_params()
    got = {k: getattr(p, k) for k, _ in capi.SmRouteParams._fields_}
    assert got == dict(rr.DEFAULTS, nu=256, nv=256)
    q = capi.route_params(nu=7, body_cells=3, rounds_per_check=8)
    assert (q.nu, q.nv, q.body_cells, q.rounds_per_check) == (7, 256, 3, 8)
    with pytest.raises(KeyError):
        capi.route_params(body=1)
    assert callable(capi.route_ground) and callable(capi.route_stats)
    assert not hasattr(capi.SurfelMap, "route_ground") and not hasattr(capi.SurfelMap, "route_stats")
    assert capi.ROUTE_NONE == rr.NONE and capi.ROUTE_DIRS == rr.DIRS and capi.SM_E_STALL == -6
    header = open(os.path.join(ROOT, "include", "sm_c_api.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
    for line in ("typedef struct sm_route_params {", "typedef struct sm_route_info {", "typedef struct sm_route_stats_t {",
                 "#define SM_ROUTE_NONE 0xFFFFFFFFu", "SM_E_STALL = -6"):
        assert line in header, line


def test_argument_rules_that_need_no_device():
    from surfelmapping_amd import capi
    L = capi.load()
    p, st, info = capi.route_params(nu=2, nv=2), capi.SmRouteStats(), capi.SmRouteInfo()
    state, clear2 = np.ones(4, np.uint8), np.ones(4, np.uint32)
    first, goals = np.array([0, 1], np.uint32), np.zeros(2, np.int32)
    cost = np.full(4, 0xA5A5A5A5, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sm_default_route_params(None) == capi.SM_E_ARG
    assert L.sm_route_ground(None, C.byref(p), ptr(state), ptr(clear2), 1, ptr(first), ptr(goals), 0, None, ptr(cost), None, None, None, None,
                             C.byref(info)) == capi.SM_E_ARG
    assert L.sm_route_stats(None, C.byref(st)) == capi.SM_E_ARG
    assert (cost == 0xA5A5A5A5).all()
    with pytest.raises(KeyError):
        capi.route_ground(None, dict(state=state.reshape(2, 2), clear2=clear2.reshape(2, 2)), [[(0, 0)]], planes=("cost", "prev"))
    with pytest.raises(ValueError):
        capi.route_ground(None, dict(state=state.reshape(2, 2), clear2=clear2), [[(0, 0)]])


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
_CASES = {}


def _ctx():
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(64, 48, 40.0, 40.0, 31.5, 23.5, preprocess=0, stereo_border=0.0, max_sqrt_vertices=64))


@pytest.fixture(scope="module")
def m():
    ctx = _ctx()
    yield ctx
    ctx.close()


def random_case(nu, nv, seed, body):
    """(the restatement of a random field with one goal set and a few starts, the call's arguments); computed once.  The goal set: one
    goal in each of the largest connected pieces of the passable cells, piece after piece, until half of the passable cells are
    reachable (one piece is enough with body_cells 0; a body of 2 cells leaves a field of 30 % obstacles in crumbs); at least one
    piece stays without a goal"""
    key = (nu, nv, seed, body)
    if key not in _CASES:
        state, clear2 = rr.random_field(nu, nv, seed)
        p = dict(body_cells=body, **SOFT)
        mm = rr.multiplier(state, clear2, **p)
        ee = rr.edges(mm)
        free = np.argwhere(mm > 0)
        left, pieces = set(map(tuple, free.tolist())), []
        while left:
            v, u = min(left)
            piece = set(map(tuple, np.argwhere(rr.dijkstra(mm, ee, [(u, v)])[0] != rr.NONE).tolist()))
            pieces.append((-len(piece), (u, v)))
            left -= piece
        goals, reached = [[]], 0
        for size, uv in sorted(pieces):
            if 2 * reached >= len(free):
                break
            goals[0].append(uv)
            reached -= size
        assert len(goals[0]) < len(pieces)
        starts = [(0, int(u), int(v)) for v, u in free[:: max(1, len(free) // 5)]] + [(0, 0, 0)]
        args = dict(ground=dict(state=state, clear2=clear2), goals=goals, starts=starts, max_steps=nu * nv, **p)
        _CASES[key] = (rr.route(state, clear2, goals, starts=starts, max_steps=nu * nv, **p), args)
    return _CASES[key]


def check(got, want, what, keys=("cost", "next", "path", "path_len", "path_cost")):
    """what the call returned against the restatement, bit for bit"""
    for k in keys:
        if k.startswith("path") and k not in want:
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    assert got["info"] == want["info"], (what, got["info"], want["info"])


def run(m, state, clear2, goals, what, starts=None, want=None, **kw):
    """route_ground against the restatement; -> (what the call returned, the restatement)"""
    from surfelmapping_amd import capi
    got = capi.route_ground(m, dict(state=state, clear2=clear2), goals, starts=starts, **kw)
    if want is None:
        want = rr.route(state, clear2, goals, starts=starts or (), **kw)
    check(got, want, what, keys=("cost", "next") + (("path", "path_len", "path_cost") if starts else ()))
    return got, want


def with_env(fn, **env):
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


def check_path(want, i, nu):
    """path i of a result: steps follow next, cells are neighbours, the edges sum to the start's cost"""
    f = 0
    n = int(want["path_len"][i])
    cells = [int(c) for c in want["path"][i, :n]]
    assert (want["path"][i, n:] == rr.NONE).all()
    total = 0
    for a, b in zip(cells, cells[1:]):
        du, dv = rr.DIRS[want["next"][f, a // nu, a % nu]]
        assert b == a + dv * nu + du
        total += rr.edge_cost(want["m"], a, b, nu)
    assert want["next"][f, cells[-1] // nu, cells[-1] % nu] == 8 and total == int(want["path_cost"][i]) == int(want["cost"][f, cells[0] // nu, cells[0] % nu])


@pytest.mark.gpu
def test_gpu_header_examples(m):
    from surfelmapping_amd import capi
    one, two = rr.examples()
    got, _ = run(m, one["state"], one["clear2"], one["goals"], "example 1", starts=[(0, 2, 2), (0, 1, 1)], max_steps=8, **one["params"])
    assert got["cost"][0].tolist() == [[0, 24, 48], [24, rr.NONE, 72], [48, 72, 96]] and got["next"][0, 2, 2] == 4
    assert got["path"][0, :5].tolist() == [8, 7, 6, 3, 0] and got["path_len"].tolist() == [5, 0]
    st = capi.route_stats(m)
    assert st["rounds"] == 1 and st["tile_visits"] == 1 and st["tile"] == 32 and st["launches"] == 2 + 4 + 2 and st["total_ms"] > 0
    got, _ = run(m, two["state"], two["clear2"], two["goals"], "example 2", **two["params"])
    assert got["cost"][0].tolist() == [[312, 216, 72, 0]]


@pytest.mark.gpu
@pytest.mark.parametrize("nu,nv", ((1, 1), (1, 300), (300, 1), (4096, 1)))
def test_gpu_degenerate_windows(m, nu, nv):
    state = np.full((nv, nu), rr.FREE, np.uint8)
    n = nu * nv
    if n > 1:
        state.reshape(-1)[(2 * n) // 3] = rr.OBSTACLE                       # the far third is cut off
    clear2 = rr.clearance(state, 3) if n <= 300 else np.minimum(np.abs(np.arange(n) - (2 * n) // 3) ** 2, 9).astype(np.uint32).reshape(nv, nu)
    starts = [(0, 0, 0), (0, nu - 1, nv - 1)]
    got, want = run(m, state, clear2, [[(0, 0)]], (nu, nv), starts=starts, max_steps=n, **SOFT)
    assert want["info"][0]["reachable"] == max(1, (2 * n) // 3)
    assert got["path_len"].tolist() == [1, 1 if n == 1 else 0]


@pytest.mark.gpu
@pytest.mark.parametrize("nu,nv,seed,body", RANDOM_FIELDS)
def test_gpu_random_fields(m, nu, nv, seed, body):
    from surfelmapping_amd import capi
    want, args = random_case(nu, nv, seed, body)
    passable, reached = int((want["m"] > 0).sum()), want["info"][0]["reachable"]
    assert 2 * reached >= passable and reached < passable, (passable, reached)   # neither all NONE nor all reached
    got = capi.route_ground(m, **args)
    check(got, want, (nu, nv, seed, body))
    assert int(want["path_len"].max()) > (5 if body == 0 else 0)
    for i in range(len(args["starts"])):
        if want["path_len"][i]:
            check_path(want, i, nu)


@pytest.fixture(scope="module")
def snake():
    state, clear2 = rr.serpentine(48, 48)
    goals, starts = [[(0, 0)]], [(0, 46, 1), (0, 47, 47), (0, 3, 5)]
    return state, clear2, goals, starts, rr.route(state, clear2, goals, starts=starts, max_steps=4096)


@pytest.mark.gpu
def test_gpu_serpentine_reactivates_tiles(m, snake):
    from surfelmapping_amd import capi
    state, clear2, goals, starts, want = snake
    assert want["info"][0]["reachable"] == int((state == rr.FREE).sum()) and want["path_len"][0] > 400
    stats = {}
    for name, env, kw in (("tile 16", dict(SM_ROUTE_TILE=16), {}), ("tile 32", dict(SM_ROUTE_TILE=32), {}), ("tile 64", dict(SM_ROUTE_TILE=64), {}),
                          ("default", {}, {}), ("one sweep", dict(SM_ROUTE_TILE=16, SM_ROUTE_SWEEPS=1), {}),
                          ("check every round", dict(SM_ROUTE_TILE=16), dict(rounds_per_check=1)),
                          ("check every 8", dict(SM_ROUTE_TILE=16), dict(rounds_per_check=8))):
        with_env(lambda: run(m, state, clear2, goals, name, starts=starts, want=want, max_steps=4096, **kw), **env)
        stats[name] = capi.route_stats(m)
        print(name, stats[name])
    s16 = stats["tile 16"]
    assert s16["tile"] == 16 and s16["rounds"] > 9 and s16["tile_visits"] > 9      # more rounds than the 9 tiles: tiles were taken up again
    assert stats["tile 64"]["rounds"] == 1 and stats["tile 64"]["tile_visits"] == 1
    assert stats["one sweep"]["sweep_cap"] == 1 and stats["one sweep"]["rounds"] > s16["rounds"]
    # (how many rounds and visits a schedule takes may differ from run to run -- a tile reads its halo as it finds it --, the bits not)
    for name in ("check every round", "check every 8"):
        assert stats[name]["rounds"] > 9 and stats[name]["launches"] >= stats[name]["rounds"] + 3, name


@pytest.mark.gpu
def test_gpu_detour(m):
    state, clear2 = rr.detour()
    nv, nu = state.shape
    goals, starts = [[(nu - 1, 4)]], [(0, 0, 4)]
    near, wn = run(m, state, clear2, goals, "weighted", starts=starts, max_steps=100, soft_cells=3, near_weight=14)
    flat, wf = run(m, state, clear2, goals, "unweighted", starts=starts, max_steps=100, near_weight=0, soft_cells=3)
    a, b = (set(g["path"][0, :g["path_len"][0]].tolist()) for g in (near, flat))
    assert a != b and near["path_len"][0] >= flat["path_len"][0] and wn["m"].max() == 13 and wf["m"].max() == 1
    # the weighted path keeps away from the wall where the plain one runs along it
    row = lambda cells: [c // nu for c in cells]
    assert min(row(a)) < min(row(b)) == 4


@pytest.mark.gpu
def test_gpu_goals(m):
    from surfelmapping_amd import capi
    state, clear2 = rr.pockets()
    outside, inside, wall = (20, 15), (6, 6), (3, 5)
    got, want = run(m, state, clear2, [[wall]], "an impassable goal", starts=[(0, 1, 1)])
    assert got["info"] == [dict(goals_used=0, goals_dropped=1, reachable=0, max_cost=0)] and (got["cost"] == rr.NONE).all() and got["path_len"][0] == 0
    got, _ = run(m, state, clear2, [[inside]], "a goal in the pocket")
    assert got["info"][0]["reachable"] == 25 and (got["cost"][0, 4:9, 4:9] != rr.NONE).all()
    sets = [[outside], [inside, wall], [outside, inside, (0, 0), (23, 19), outside]]
    three, want = run(m, state, clear2, sets, "three fields", starts=[(2, 6, 5), (0, 6, 5), (1, 6, 5), (2, 12, 12)], **SOFT)
    assert [i["goals_used"] for i in three["info"]] == [1, 1, 5] and three["info"][1]["goals_dropped"] == 1
    assert three["path_len"].tolist()[1] == 0 and three["path_len"][2] == 2 and three["info"][2]["reachable"] == int((state == rr.FREE).sum())
    for f, g in enumerate(sets):
        alone = capi.route_ground(m, dict(state=state, clear2=clear2), [g], **SOFT)
        assert (alone["cost"][0] == three["cost"][f]).all() and (alone["next"][0] == three["next"][f]).all() and alone["info"][0] == three["info"][f]


@pytest.mark.gpu
def test_gpu_paths_and_null_outputs(m):
    from surfelmapping_amd import capi
    want, args = random_case(65, 40, 3, 0)
    goal = args["goals"][0][0]
    far = int(np.argmax(want["path_len"]))
    nv_, nu_ = np.argwhere(want["cost"][0] == rr.NONE)[0]
    starts = [args["starts"][far], (0,) + goal, (0, int(nu_), int(nv_))]
    assert want["path_len"][far] > 6
    short = rr.route(args["ground"]["state"], args["ground"]["clear2"], args["goals"], starts=starts, max_steps=4, body_cells=0, **SOFT)
    assert short["path_len"].tolist() == [5, 1, 0] and short["path_cost"][0] == want["path_cost"][far]
    kw = dict(args, starts=starts, max_steps=4)
    got = capi.route_ground(m, **kw)
    check(got, short, "truncated")
    only = capi.route_ground(m, planes=(), **kw)
    assert only["cost"] is None and only["next"] is None
    check(only, short, "paths only", keys=("path", "path_len", "path_cost"))
    planes = capi.route_ground(m, **dict(kw, starts=None))
    assert "path" not in planes
    check(planes, short, "planes only", keys=("cost", "next"))
    one = capi.route_ground(m, planes=("next",), **dict(kw, starts=None))
    assert one["cost"] is None and (one["next"] == short["next"]).all()


@pytest.mark.gpu
def test_gpu_end_to_end_and_order(tmp_path):
    """ground_maps of a small synthetic set, then route_ground on its planes; between two identical ground_maps calls and after a
    frame the route has a fresh context's bits, and the second ground map the first's"""
    from surfelmapping_amd import capi, synth
    import ground_ref as gr
    import recall_ref as cr
    import test_ground as tg
    rows = tg.random_rows(600, 5)
    path = str(tmp_path / "set.bin")
    cr.write_map(path, rows)
    gkw = dict(cell_mm=100, nu=64, nv=34, reach_cells=6)
    want_g = gr.ground_set([rows], **gkw)
    free = np.argwhere(want_g["state"] == gr.FREE)
    assert len(free) > 100
    goals = [[(int(free[0][1]), int(free[0][0]))], [(int(free[-1][1]), int(free[-1][0]))]]
    starts = [(0, int(free[-1][1]), int(free[-1][0])), (1, int(free[len(free) // 2][1]), int(free[len(free) // 2][0]))]
    rkw = dict(body_cells=1, unknown_passable=1, max_steps=500, **SOFT)
    want = rr.route(want_g["state"], want_g["clear2"], goals, starts=starts, **rkw)
    assert want["info"][0]["reachable"] > 50

    fresh = _ctx()
    g1 = fresh.ground_maps([path], **gkw)
    tg.check(g1, want_g, "ground")
    r1 = capi.route_ground(fresh, g1, goals, starts=starts, **rkw)
    check(r1, want, "fresh")
    g2 = fresh.ground_maps([path], **gkw)
    tg.check(g2, want_g, "ground again")
    fresh.close()

    cam = dict(width=64, height=48, fx=40.0, fy=40.0, cx=31.5, cy=23.5)
    busy = _ctx()
    for frame in synth.make_sequence(cam, synth.kitti_trajectory(2), seed=3):
        busy.process_frame(*frame)
    r2 = capi.route_ground(busy, g1, goals, starts=starts, **rkw)
    check(r2, want, "after frames")
    busy.close()


@pytest.mark.gpu
def test_gpu_refusals(m, snake):
    from surfelmapping_amd import capi
    fresh = _ctx()
    with pytest.raises(capi.SurfelMapError) as e:
        capi.route_stats(fresh)
    assert e.value.rc == capi.SM_E_ARG
    fresh.close()
    state, clear2 = np.full((4, 5), rr.FREE, np.uint8), np.full((4, 5), 9, np.uint32)
    g = dict(state=state, clear2=clear2)

    def refused(what, rc=capi.SM_E_ARG, ground=g, goals=[[(0, 0)]], **kw):
        with pytest.raises(capi.SurfelMapError) as e:
            capi.route_ground(m, ground, goals, **kw)
        assert e.value.rc == rc and what in str(e.value), (what, str(e.value))

    for key, values in (("body_cells", (-1, 256)), ("soft_cells", (-1, 256)), ("near_weight", (-1, 15)), ("unknown_passable", (-1, 2)),
                        ("max_steps", (-1, (1 << 22) + 1)), ("rounds_per_check", (0, 65)), ("max_rounds", (0, -5))):
        for v in values:
            refused(key, **{key: v})
    # the limits, refused before anything is allocated or read: the planes here are one word
    with pytest.raises(capi.SurfelMapError) as e:
        p = capi.route_params(nu=2048, nv=2049)
        info = capi.SmRouteInfo()
        first = np.array([0, 0], np.uint32)
        one = np.ones(1, np.uint32)
        ptr = one.ctypes.data_as(C.c_void_p)
        m._chk(m._L.sm_route_ground(m._h, C.byref(p), ptr, ptr, 1, first.ctypes.data_as(C.c_void_p), None, 0, None, None, None, None, None, None,
                                    C.byref(info)), "sm_route_ground")
    assert e.value.rc == capi.SM_E_ARG and "2^22" in str(e.value)
    for nu, nv, G, n_starts, steps, what in ((4097, 1, 1, 0, 0, "nu outside"), (1, 4097, 1, 0, 0, "nv outside"), (2048, 2048, 17, 0, 0, "2^26"),
                                             (4, 4, 0, 0, 0, "no field"), (4, 4, 1, 17, (1 << 22), "starts * (max_steps + 1)")):
        with pytest.raises(capi.SurfelMapError) as e:
            p = capi.route_params(nu=nu, nv=nv, max_steps=steps)
            info = (capi.SmRouteInfo * 32)()
            first = np.zeros(33, np.uint32)
            m._chk(m._L.sm_route_ground(m._h, C.byref(p), ptr, ptr, G, first.ctypes.data_as(C.c_void_p), None, n_starts, ptr, None, None, None, None, None,
                                        info), "sm_route_ground")
        assert e.value.rc == capi.SM_E_ARG and what in str(e.value), (what, str(e.value))
    for goal in ((5, 0), (0, 4), (-1, 0), (0, -1)):
        refused("a goal outside the window", goals=[[goal]])
    for start in ((0, 5, 0), (0, 0, 4), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
        refused("start", starts=[start])
    with_env(lambda: refused("SM_ROUTE_TILE"), SM_ROUTE_TILE=24)
    with_env(lambda: refused("SM_ROUTE_SWEEPS"), SM_ROUTE_SWEEPS=0)
    # a call that does not converge within max_rounds: SM_E_STALL, nothing written, the last call's stats left
    s_state, s_clear2, goals, starts, want = snake
    good, _ = run(m, s_state, s_clear2, goals, "before the stall", want=want, starts=starts, max_steps=4096)
    before = capi.route_stats(m)
    p = capi.route_params(nu=48, nv=48, max_rounds=1)
    cost = np.full((48, 48), 0xA5A5A5A5, np.uint32)
    nxt = np.full((48, 48), 0xA5, np.uint8)
    info = capi.SmRouteInfo(7, 7, 7, 7)
    first, flat = np.array([0, 1], np.uint32), np.zeros(2, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = with_env(lambda: m._L.sm_route_ground(m._h, C.byref(p), ptr(s_state), ptr(s_clear2), 1, ptr(first), ptr(flat), 0, None, ptr(cost), ptr(nxt),
                                               None, None, None, C.byref(info)), SM_ROUTE_TILE=16)
    assert rc == capi.SM_E_STALL and "max_rounds" in m._L.sm_last_error().decode()
    assert (cost == 0xA5A5A5A5).all() and (nxt == 0xA5).all() and info.goals_used == 7 and capi.route_stats(m) == before
    run(m, s_state, s_clear2, goals, "after the stall", want=want, starts=starts, max_steps=4096)
