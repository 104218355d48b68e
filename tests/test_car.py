"""Routes a car can follow (sm_route_car, sm_route_car_stats; capi.route_car; DESIGN.md "4ad. Routes for a car").
CPU: the restatement (car_ref.py) against the header's three examples, its Dijkstra against a plain relaxation, `next` as a function
of `cost`, the path words re-derived from `next`, the lower bound by sm_route_ground's field; the library's symbols, defaults, header
and every argument rule (the call looks at its context last, so none of them needs a device).
GPU: cost, next, the paths and info of the HIP path against the restatement, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from surfelmapping_amd.capi import SmRouteCarParams  # noqa: F401  (the binding's symbol: without it nothing here can run)

import car_ref as cr
import route_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sm_default_route_car_params", "sm_route_car", "sm_route_car_stats")
SOFT = dict(soft_cells=3, near_weight=14)                                  # test_route's multipliers
# the random fields: 70 x 40 crosses the borders of 32-cell tiles along both axes with a partial last tile; (turn_cells, turn_cost,
# reverse_weight) x body_cells.  2 % of the cells are obstacles (a car needs room: at route's density the states fall apart), seed 1
NU, NV, SEED, DENSITY = 70, 40, 1, 0.02
CAR_PARAMS = ((1, 0, 0), (2, 7, 0), (3, 0, 3), (4, 3, 2))
RANDOM_CASES = tuple((n, tc, rw, body) for n, tc, rw in CAR_PARAMS for body in (0, 2))
MAX_STEPS = 24                                                             # of the random cases: some paths fit, some are cut


def car_kw(n, tc, rw, body=0, **more):
    return dict(turn_cells=n, turn_cost=tc, reverse_weight=rw, body_cells=body, **more)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_header_examples():
    for ex in cr.examples():
        got = cr.route_car(ex["state"], ex["clear2"], [ex["goals"]], **ex["params"])
        cr.check_example(ex, got["cost"][0])
    one, two, three = cr.examples()[0], cr.examples()[3], cr.examples()[5]
    # example 1: the two R moves behind the 116, as path words
    got = cr.route_car(one["state"], one["clear2"], [one["goals"]], starts=[(0, 0, 1, 1), (0, 0, 1, 3)], max_steps=8, **one["params"])
    cells = lambda *uvh: [cr.word(v * 5 + u, h) for u, v, h in uvh]
    assert got["path"][0, :5].tolist() == cells((0, 1, 1), (1, 2, 1), (2, 2, 0), (3, 2, 0), (4, 1, 7))
    assert got["path_len"].tolist() == [5, 0] and got["path_cost"].tolist() == [116, cr.NONE]
    assert got["next"][0, 1, 1, 0] == cr.R and got["next"][0, 0, 1, 0] == cr.F and got["next"][0, :, 1, 4].tolist() == [8] * 8
    assert got["info"] == [dict(goals_used=1, goals_dropped=0, reachable_states=int((got["cost"] != cr.NONE).sum()), reachable_cells=15, max_cost=int(
        got["cost"][got["cost"] != cr.NONE].max()))]
    # example 2: the half turn is 6 n cells wide -- four L turns from (3, 0) end at (3, 6) heading 4
    got = cr.route_car(two["state"], two["clear2"], [two["goals"]], starts=[(0, 3, 0, 0)], max_steps=20, **two["params"])
    cell, head, rev = (got["path"][0, :12] & 0x3FFFFF, got["path"][0, :12] >> 22 & 7, got["path"][0, :12] >> 25)
    assert got["path_len"][0] == 12 and cell.tolist() == [3, 4, 12, 20, 27, 34, 40, 46, 45, 44, 43, 42] and not rev.any()
    assert head.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4] and (cell % 7).max() - 3 == 3 and (cell // 7).max() == 6   # 3 n to the side, 6 n across
    # example 3: reversing at heading 4 costs three times driving at heading 0, and says so in the words
    got = cr.route_car(three["state"], three["clear2"], [three["goals"]], starts=[(0, 0, 0, 4)], max_steps=8, **three["params"])
    assert got["m"].tolist() == [[1, 7, 5, 1]]
    assert got["path"][0, :4].tolist() == [cr.word(0, 4), cr.word(1, 4, 1), cr.word(2, 4, 1), cr.word(3, 4, 1)] and got["path_cost"][0] == 936


def test_weights_fit_and_costs_do_not_wrap():
    assert cr.MAX_WEIGHT == 32 * 510 + 4095 == 20415 < 1 << 15 and cr.LIMIT + (1 << 15) < 1 << 32
    # the dearest turn there is: 16 cells, diagonal, every multiplier 15, turn_cost 4095
    state = np.full((40, 40), rr.FREE, np.uint8)
    m = rr.multiplier(state, np.zeros((40, 40)), soft_cells=255, near_weight=14)
    exists, weight, _ = cr.move_table(m, rr.edges(m), turn_cells=16, turn_cost=4095, reverse_weight=15)
    assert m.max() == 15 and exists[cr.L].any() and weight.max() == 16 * 12 * 30 + 16 * 17 * 30 + 4095 <= cr.MAX_WEIGHT


@pytest.mark.parametrize("seed", (1, 2, 3))
@pytest.mark.parametrize("n,tc,rw", ((1, 0, 0), (2, 9, 3)))
def test_dijkstra_equals_relaxation(seed, n, tc, rw):
    state, clear2 = cr.random_field(23, 17, seed, density=0.05)
    m = rr.multiplier(state, clear2, **SOFT)
    table = cr.move_table(m, rr.edges(m), **car_kw(n, tc, rw))
    free = np.argwhere(m > 0)
    goals = [(int(free[0][1]), int(free[0][0]), -1), (int(free[-1][1]), int(free[-1][0]), 3), (int(np.argwhere(m == 0)[0][1]), int(np.argwhere(m == 0)[0][0]), 0)]
    cost, used, dropped = cr.dijkstra(m, table, goals)
    assert (used, dropped) == (2, 1) and (cost != cr.NONE).sum() > 200
    assert (cost == cr.sweep_until_stable(m, table, goals)).all()


def test_the_range_rule_cuts_at_2_to_the_31():
    """a corridor too short to reach 2^31: the rule by a lowered limit -- both statements of the cost keep what is below and drop the rest"""
    state, clear2 = np.full((1, 40), rr.FREE, np.uint8), np.full((1, 40), 9, np.uint32)
    m = rr.multiplier(state, clear2)
    table = cr.move_table(m, rr.edges(m), turn_cells=1)
    full = cr.dijkstra(m, table, [(39, 0, 0)])[0]
    old = cr.LIMIT
    try:
        cr.LIMIT = 500
        cut, swept = cr.dijkstra(m, table, [(39, 0, 0)])[0], cr.sweep_until_stable(m, table, [(39, 0, 0)])
    finally:
        cr.LIMIT = old
    assert (cut == swept).all() and (cut == np.where(full < 500, full, cr.NONE)).all() and (cut[0] != cr.NONE).sum() == 21


def random_case(n, tc, rw, body, _cache={}):
    """(the restatement of the random field with two goal sets -- one of any heading, one of a fixed heading -- and 16 starts, the
    call's arguments); computed once and never changed"""
    key = (n, tc, rw, body)
    if key not in _cache:
        state, clear2 = cr.random_field(NU, NV, SEED, density=DENSITY)
        p = car_kw(n, tc, rw, body, **SOFT)
        m = rr.multiplier(state, clear2, **p)
        free = np.argwhere(m > 0)
        near = lambda u, v: tuple(int(x) for x in free[np.argmin((free[:, 1] - u) ** 2 + (free[:, 0] - v) ** 2)][::-1])
        goals = [[near(60, 30) + (-1,), near(5, 5) + (-1,)], [near(12, 9) + (2,), (int(np.argwhere(m == 0)[0][1]), int(np.argwhere(m == 0)[0][0]), 5)]]
        want = cr.route_car(state, clear2, goals, max_steps=MAX_STEPS, **p)
        starts = []
        for f in (0, 1):
            has = np.argwhere((want["cost"][f] != cr.NONE) & (want["cost"][f] > 0))
            none = np.argwhere((want["cost"][f] == cr.NONE) & (m > 0)[None])
            far = np.argsort(want["cost"][f][tuple(has.T)])
            picks = [has[far[-1]], has[far[len(far) // 2]], has[far[len(far) // 4]], has[far[5]], has[far[len(far) // 8]], none[0], none[len(none) // 2]]
            starts += [(f, int(u), int(v), int(h)) for h, v, u in picks]
        starts += [(0,) + goals[0][0][:2] + (3,), (1, goals[1][1][0], goals[1][1][1], 0)]          # a goal state; an impassable cell
        cr.add_paths(want, starts, MAX_STEPS, n)
        args = dict(ground=dict(state=state, clear2=clear2), goals=goals, starts=starts, max_steps=MAX_STEPS, **p)
        _cache[key] = (want, args)
    return _cache[key]


@pytest.mark.parametrize("n,tc,rw,body", RANDOM_CASES)
def test_random_cases_hold_their_condition(n, tc, rw, body):
    """in the restatement alone: per field at least half of the passable states have a cost and at least one has none; the starts
    include unreachable, whole and truncated paths"""
    want, args = random_case(n, tc, rw, body)
    passable = 8 * int((want["m"] > 0).sum())
    for i in want["info"]:
        assert 2 * i["reachable_states"] >= passable and i["reachable_states"] < passable, (i, passable)
    assert want["info"][0]["goals_used"] == 2 and want["info"][1]["goals_dropped"] == 1
    lens = want["path_len"].tolist()
    assert len(lens) == 16 and lens.count(0) >= 5 and lens.count(MAX_STEPS + 1) >= 2 and sum(1 < x <= MAX_STEPS for x in lens) >= 2 and 1 in lens, lens


@pytest.mark.parametrize("n,tc,rw,body", RANDOM_CASES[2:6])
def test_next_is_a_function_of_cost(n, tc, rw, body):
    want, _ = random_case(n, tc, rw, body)
    exists, weight, offset = want["table"]
    for f in (0, 1):
        cost, nxt = want["cost"][f], want["next"][f]
        assert (nxt == cr.next_of(cost, want["table"])).all()
        assert ((nxt == 8) == (cost == 0)).all() and ((nxt == 255) == (cost == cr.NONE)).all() and set(np.unique(nxt)) <= {0, 1, 2, 3, 8, 255}
        # along next the cost falls by exactly the move's weight, and no smaller move code does as well
        for h, v, u in np.argwhere(nxt < 4):
            mv = int(nxt[h, v, u])
            du, dv, h2 = offset[mv][h]
            assert exists[mv, h, v, u] and int(cost[h2, v + dv, u + du]) + int(weight[mv, h, v, u]) == int(cost[h, v, u])
            for less in range(mv):
                du, dv, h2 = offset[less][h]
                assert not exists[less, h, v, u] or cost[h2, v + dv, u + du] == cr.NONE or int(cost[h2, v + dv, u + du]) + int(weight[less, h, v, u]) > int(cost[h, v, u])


def rederive(want, start, max_steps, n, nu):
    """the path words of a start from `next` alone, move by move, with the weights summed from the unit edges"""
    f, u, v, h = start
    words, total = [cr.word(v * nu + u, h)], 0
    m = want["m"]
    for _ in range(10000):
        mv = int(want["next"][f, h, v, u])
        if mv >= 4:
            break
        exists, weight, _ = want["table"]
        assert exists[mv, h, v, u]
        total += int(weight[mv, h, v, u])
        for u2, v2, h2, rev in cr.move_cells(u, v, h, mv, n):
            assert max(abs(u2 - u), abs(v2 - v)) == 1 and m[v2, u2] > 0     # unit steps over passable cells
            words.append(cr.word(v2 * nu + u2, h2, rev))
            u, v, h = u2, v2, h2
    return words, total, mv


@pytest.mark.parametrize("n,tc,rw,body", RANDOM_CASES[2:6])
def test_path_words_follow_next(n, tc, rw, body):
    want, args = random_case(n, tc, rw, body)
    for i, start in enumerate(args["starts"]):
        ln = int(want["path_len"][i])
        assert (want["path"][i, ln:] == cr.NONE).all()
        if want["cost"][start[0], start[3], start[2], start[1]] == cr.NONE:
            assert ln == 0 and want["path_cost"][i] == cr.NONE
            continue
        words, total, last = rederive(want, start, MAX_STEPS, n, NU)
        assert last == 8 and total == int(want["path_cost"][i]) == int(want["cost"][start[0], start[3], start[2], start[1]])
        assert ln == min(len(words), MAX_STEPS + 1) and want["path"][i, :ln].tolist() == words[:ln]


@pytest.mark.parametrize("n,tc,rw", ((1, 0, 0), (1, 0, 1), (2, 11, 15), (3, 4095, 4)))
@pytest.mark.parametrize("seed,body", ((1, 0), (2, 1)))
def test_lower_bound_by_the_route_field(n, tc, rw, seed, body):
    """every car path is an 8-connected path with the same unit costs (times reverse_weight >= 1, plus turn_cost >= 0): the least
    cost over the headings is at least sm_route_ground's, and NONE where that is NONE"""
    state, clear2 = cr.random_field(33, 29, seed, density=0.05)
    p = dict(body_cells=body, **SOFT)
    m = rr.multiplier(state, clear2, **p)
    free = np.argwhere(m > 0)
    cells = [(int(free[3][1]), int(free[3][0])), (int(free[-7][1]), int(free[-7][0]))]
    route = rr.route(state, clear2, [cells], **p)["cost"][0]
    car = cr.route_car(state, clear2, [[c + (-1,) for c in cells]], turn_cells=n, turn_cost=tc, reverse_weight=rw, **p)["cost"][0]
    best = car.min(axis=0)
    assert (best >= route).all() and (best[route == rr.NONE] == cr.NONE).all() and (best != cr.NONE).sum() > 100
    assert (best[tuple(zip(*[(v, u) for u, v in cells]))] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the library, without a device
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_defaults_and_binding():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None and name in capi.SYMBOLS
    p = capi.route_car_params()
    got = {k: getattr(p, k) for k, _ in capi.SmRouteCarParams._fields_}
    assert got == dict(cr.DEFAULTS, nu=256, nv=256)
    q = capi.route_car_params(nu=7, turn_cells=5, reverse_weight=2)
    assert (q.nu, q.nv, q.turn_cells, q.reverse_weight) == (7, 256, 5, 2)
    with pytest.raises(KeyError):
        capi.route_car_params(turn=1)
    assert callable(capi.route_car) and callable(capi.route_car_stats) and not hasattr(capi.SurfelMap, "route_car")
    assert capi.CAR_MOVES == cr.MOVES == ("F", "L", "R", "B")
    row = np.array([cr.word(5, 0), cr.word(6, 1), cr.word((1 << 22) - 1, 7, 1), cr.NONE, cr.NONE], np.uint32)
    cell, head, rev = capi.car_path_cells(row)
    assert cell.tolist() == [5, 6, (1 << 22) - 1] and head.tolist() == [0, 1, 7] and rev.tolist() == [0, 0, 1]
    header = open(os.path.join(ROOT, "include", "sm_c_api.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
    for line in ("typedef struct sm_route_car_params {", "typedef struct sm_route_car_info {", "typedef struct sm_route_car_stats_t {",
                 "#define SM_CAR_MOVE_F 0", "#define SM_CAR_MOVE_L 1", "#define SM_CAR_MOVE_R 2", "#define SM_CAR_MOVE_B 3",
                 '(DESIGN.md "4ad. Routes for a car")', "96 116 NONE NONE NONE NONE NONE 116", "96 116 290 464 192 464 290 116",
                 "the cost is 304", "it is 340", "it is 280", "312 216 72 0", "936 648 216 0", "32 * 510 + 4095 = 20 415",
                 "the turning radius is about 3 * turn_cells cells"):
        assert line in header, line


class Call:
    """one raw sm_route_car call on a 5 x 4 window with every output poisoned: .rc, .error and whether anything was written"""

    def __init__(self, ctx=None, G=1, first=(0, 1), goals=((0, 0, -1),), starts=(), null=(), nu=5, nv=4, planes=True, env=None, **over):
        from surfelmapping_amd import capi
        L = capi.load()
        p = capi.route_car_params(nu=nu, nv=nv, **over)
        n_cells = 20 if planes else 1
        state, clear2 = np.full(n_cells, rr.FREE, np.uint8), np.full(n_cells, 9, np.uint32)
        first, goals = np.array(first, np.uint32), np.array(goals, np.int32).reshape(-1, 3)
        st = np.array(starts, np.int32).reshape(-1, 4)
        steps = max(0, min(int(p.max_steps), 64))
        self.out = dict(cost=np.full(8 * n_cells, 0xA5A5A5A5, np.uint32), next=np.full(8 * n_cells, 0xA5, np.uint8),
                        path=np.full(max(1, len(st)) * (steps + 1), 0xA5A5A5A5, np.uint32), path_len=np.full(max(1, len(st)), 0xA5A5A5A5, np.uint32),
                        path_cost=np.full(max(1, len(st)), 0xA5A5A5A5, np.uint32))
        self.info = (capi.SmRouteCarInfo * 32)(*[capi.SmRouteCarInfo(7, 7, 7, 7, 7) for _ in range(32)])
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        args = dict(p=C.byref(p), state=ptr(state), clear2=ptr(clear2), first=ptr(first), goals=ptr(goals) if len(goals) else None,
                    starts=ptr(st) if len(st) else None, info=self.info)
        for k in null:
            args[k] = None
        for k, v in (env or {}).items():
            os.environ[k] = str(v)
        try:
            self.rc = L.sm_route_car(ctx, args["p"], args["state"], args["clear2"], G, args["first"], args["goals"], len(st),
                                     args["starts"], *[ptr(self.out[k]) for k in ("cost", "next", "path", "path_len", "path_cost")], args["info"])
        finally:
            for k in (env or {}):
                os.environ.pop(k, None)
        self.error = L.sm_last_error().decode()
        self.untouched = (all((self.out[k] == (0xA5 if k == "next" else 0xA5A5A5A5)).all() for k in self.out)
                          and all(self.info[i].goals_used == 7 and self.info[i].max_cost == 7 for i in range(32)))


def refusals(ctx):
    """every argument rule of sm_route_car: (what the error names, the call) -- the same list without a device and with one"""
    yield "null argument", Call(ctx, null=("p",))
    for k in ("state", "clear2", "first", "info"):
        yield "null argument", Call(ctx, null=(k,))
    yield "null goals", Call(ctx, null=("goals",))
    yield "null starts", Call(ctx, starts=((0, 0, 0, 0),), null=("starts",))
    for key, values in (("body_cells", (-1, 256)), ("soft_cells", (-1, 256)), ("near_weight", (-1, 15)), ("unknown_passable", (-1, 2)),
                        ("turn_cells", (0, 17, -1)), ("turn_cost", (-1, 4096)), ("reverse_weight", (-1, 16)),
                        ("max_steps", (-1, (1 << 22) + 1)), ("rounds_per_check", (0, 65)), ("max_rounds", (0, -5))):
        for v in values:
            yield key, Call(ctx, **{key: v})
    # the limits, refused before anything is allocated or read: the planes of these calls are one word
    for nu, nv, G, what in ((4097, 1, 1, "nu outside"), (1, 4097, 1, "nv outside"), (2048, 2049, 1, "2^22"), (2048, 2048, 3, "2^23"), (1024, 1024, 9, "2^23"),
                            (4, 4, 0, "no field")):
        yield what, Call(ctx, nu=nu, nv=nv, G=G, first=(0,) * (G + 1), goals=(), planes=False)
    yield "starts * (max_steps + 1)", Call(ctx, starts=((0, 0, 0, 0),) * 17, max_steps=1 << 22)
    yield "goal_first[0]", Call(ctx, first=(1, 1))
    yield "goal_first falls", Call(ctx, G=2, first=(0, 1, 0))
    for goal in ((5, 0, 0), (0, 4, 0), (-1, 0, 0), (0, -1, 0)):
        yield "a goal outside the window", Call(ctx, goals=(goal,))
    for h in (-2, 8, 255):
        yield "a goal's heading", Call(ctx, goals=((0, 0, h),))
    for start in ((0, 5, 0, 0), (0, 0, 4, 0), (0, -1, 0, 0)):
        yield "a start outside the window", Call(ctx, starts=(start,))
    for start in ((1, 0, 0, 0), (-1, 0, 0, 0)):
        yield "a start's field", Call(ctx, starts=(start,))
    for h in (-1, 8):
        yield "a start's heading", Call(ctx, starts=((0, 0, 0, h),))
    yield "SM_CAR_TILE", Call(ctx, env=dict(SM_CAR_TILE=24))
    yield "SM_CAR_TILE", Call(ctx, env=dict(SM_CAR_TILE=64))
    yield "SM_CAR_TILE=16 with turn_cells above 8", Call(ctx, env=dict(SM_CAR_TILE=16), turn_cells=9)
    yield "SM_CAR_SWEEPS", Call(ctx, env=dict(SM_CAR_SWEEPS=0))


def test_argument_rules_need_no_device():
    from surfelmapping_amd import capi
    L = capi.load()
    assert L.sm_default_route_car_params(None) == capi.SM_E_ARG
    assert L.sm_route_car_stats(None, C.byref(capi.SmRouteCarStats())) == capi.SM_E_ARG
    n = 0
    for what, call in refusals(None):
        assert call.rc == capi.SM_E_ARG and "sm_route_car: " in call.error and what in call.error and call.untouched, (what, call.rc, call.error)
        n += 1
    assert n == 55
    # ... and a call with nothing wrong but its context says so, last of all
    ok = Call(None, starts=((0, 1, 1, 7),), env=dict(SM_CAR_TILE=16, SM_CAR_SWEEPS=3), turn_cells=8)
    assert ok.rc == capi.SM_E_ARG and "null context" in ok.error and ok.untouched
    state = np.ones((2, 2), np.uint8)
    with pytest.raises(KeyError):
        capi.route_car(None, dict(state=state, clear2=state.astype(np.uint32)), [[(0, 0, -1)]], planes=("cost", "prev"))
    with pytest.raises(ValueError):
        capi.route_car(None, dict(state=state, clear2=np.ones(4, np.uint32)), [[(0, 0, -1)]])


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _ctx():
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(64, 48, 40.0, 40.0, 31.5, 23.5, preprocess=0, stereo_border=0.0, max_sqrt_vertices=64))


@pytest.fixture(scope="module")
def m():
    ctx = _ctx()
    yield ctx
    ctx.close()


KEYS = ("cost", "next", "path", "path_len", "path_cost")


def check(got, want, what, keys=KEYS):
    """what the call returned against the restatement, bit for bit"""
    for k in keys:
        if k.startswith("path") and k not in got:
            assert len(want[k]) == 0
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    assert got["info"] == want["info"], (what, got["info"], want["info"])


def with_env(fn, **env):
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return fn()
    finally:
        for k in env:
            os.environ.pop(k, None)


@pytest.mark.gpu
def test_gpu_header_examples(m):
    from surfelmapping_amd import capi
    for ex in cr.examples():
        starts = [(0, 0, 0, 0), (0, ex["state"].shape[1] - 1, 0, 4)]
        want = cr.route_car(ex["state"], ex["clear2"], [ex["goals"]], starts=starts, max_steps=12, **ex["params"])
        got = capi.route_car(m, dict(state=ex["state"], clear2=ex["clear2"]), [ex["goals"]], starts=starts, max_steps=12, **ex["params"])
        cr.check_example(ex, got["cost"][0])
        check(got, want, ex["name"])
        st = capi.route_car_stats(m)
        assert st["rounds"] == 1 and st["tile_visits"] == 1 and st["tile"] == 32 and st["sweep_cap"] == 1024 and st["launches"] == 3 + 4 + 2 and st["total_ms"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,tc,rw,body", RANDOM_CASES)
def test_gpu_random_fields(m, n, tc, rw, body):
    from surfelmapping_amd import capi
    want, args = random_case(n, tc, rw, body)
    got = capi.route_car(m, **args)
    check(got, want, (n, tc, rw, body))
    st = capi.route_car_stats(m)
    assert st["tile"] == 32 and st["rounds"] >= 2 and st["tile_visits"] > 4              # more than the tiles the goals lie in


@pytest.fixture(scope="module")
def wide():
    """130 x 100 cells with a few boxes, one goal: at turn_cells 16 a half turn is 97 cells wide and spans three tiles of 32"""
    state, clear2 = cr.boxes()
    out = {}
    for n in (16, 8):
        # the first start faces away from the goal with room for the half turn, the last two have none at turn_cells 16
        goals, starts = [[(120, 97, 0)]], [(0, 100, 1, 4), (0, 5, 5, 2), (0, 129, 99, 6), (0, 30, 2, 0), (0, 64, 32, 1)]
        out[n] = (state, clear2, goals, starts, cr.route_car(state, clear2, goals, starts=starts, max_steps=400, turn_cells=n, turn_cost=3))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n,tile", ((16, 32), (8, 16)))
def test_gpu_reach_equals_tile(m, wide, n, tile):
    """a move reaches 2 n = T cells: from the first column of a tile into the first of the next, across a whole tile at a corner"""
    from surfelmapping_amd import capi
    state, clear2, goals, starts, want = wide[n]
    exists, _, offset = want["table"]
    assert exists[cr.L].any() and max(abs(offset[cr.L][1][0]), abs(offset[cr.L][1][1])) == 2 * n == tile
    heads = want["path"][0, :want["path_len"][0]] >> 22 & 7
    assert want["info"][0]["reachable_cells"] > 5000 and want["path_len"][0] > 6 * n and sorted(set(heads.tolist())) == [0, 1, 2, 3, 4] and (want["next"][0] == cr.L).any() and (want["next"][0] == cr.R).any()
    got = with_env(lambda: capi.route_car(m, dict(state=state, clear2=clear2), goals, starts=starts, max_steps=400, turn_cells=n, turn_cost=3),
                   **({} if tile == 32 else dict(SM_CAR_TILE=tile)))
    check(got, want, (n, tile))
    assert capi.route_car_stats(m)["tile"] == tile


@pytest.mark.gpu
def test_gpu_schedule_invariance(m):
    from surfelmapping_amd import capi
    want, args = random_case(3, 0, 3, 2)
    base = capi.route_car(m, **args)
    check(base, want, "default")
    s0 = capi.route_car_stats(m)
    for name, env, kw in (("tile 16", dict(SM_CAR_TILE=16), {}), ("one sweep", dict(SM_CAR_SWEEPS=1), {}), ("check every round", {}, dict(rounds_per_check=1))):
        got = with_env(lambda: capi.route_car(m, **dict(args, **kw)), **env)
        for k in KEYS:
            assert got[k].tobytes() == base[k].tobytes(), (name, k)
        assert got["info"] == base["info"]
        st = capi.route_car_stats(m)
        print(name, st)
        if name == "tile 16":
            assert st["tile"] == 16 and st["sweep_cap"] == 256 and st["tile_visits"] > s0["tile_visits"]
        if name == "one sweep":
            assert st["sweep_cap"] == 1 and st["rounds"] > s0["rounds"]
        if name == "check every round":
            assert st["rounds"] >= 2 and st["launches"] >= st["rounds"] + 5


@pytest.mark.gpu
@pytest.mark.parametrize("n,tc,rw,body", (RANDOM_CASES[0], RANDOM_CASES[7]))
def test_gpu_lower_bound_by_route_ground(m, n, tc, rw, body):
    """sm_route_car against sm_route_ground on the same context, planes and goal cells"""
    from surfelmapping_amd import capi
    want, args = random_case(n, tc, rw, body)
    car = capi.route_car(m, **dict(args, starts=None))["cost"]
    cells = [[g[:2] for g in gs] for gs in args["goals"]]
    route = capi.route_ground(m, args["ground"], cells, body_cells=body, **SOFT)["cost"]
    best = car.min(axis=1)
    assert best.shape == route.shape and (best >= route).all() and (best[route == rr.NONE] == cr.NONE).all()
    assert ((best != cr.NONE) & (best > route)).any() and (best == 0).sum() >= 2


@pytest.mark.gpu
def test_gpu_paths_and_null_outputs(m):
    from surfelmapping_amd import capi
    want, args = random_case(2, 7, 0, 0)
    only = capi.route_car(m, planes=(), **args)
    assert only["cost"] is None and only["next"] is None
    check(only, want, "paths only", keys=("path", "path_len", "path_cost"))
    planes = capi.route_car(m, **dict(args, starts=None))
    assert "path" not in planes
    check(planes, want, "planes only", keys=("cost", "next"))
    one = capi.route_car(m, planes=("next",), **dict(args, starts=None))
    assert one["cost"] is None and (one["next"] == want["next"]).all()
    zero = capi.route_car(m, **dict(args, max_steps=0))
    assert zero["path"].shape == (16, 1) and (zero["path_len"] == (want["path_len"] > 0)).all() and (zero["path_cost"] == want["path_cost"]).all()
    assert (zero["path"][:, 0] == np.where(want["path_len"] > 0, want["path"][:, 0], cr.NONE)).all()
    # fields do not see each other: each goal set alone gives its field of the pair
    for f, g in enumerate(args["goals"]):
        alone = capi.route_car(m, args["ground"], [g], **{k: v for k, v in args.items() if k not in ("ground", "goals", "starts")})
        assert (alone["cost"][0] == want["cost"][f]).all() and (alone["next"][0] == want["next"][f]).all() and alone["info"][0] == want["info"][f]


@pytest.mark.gpu
def test_gpu_between_frames_and_other_calls(tmp_path):
    """ground_maps of a small synthetic set, then route_car on its planes; between two identical ground_maps calls and after frames
    the call has a fresh context's bits, the second ground map the first's, and the model is what it was"""
    from surfelmapping_amd import capi, synth
    import ground_ref as gr
    import recall_ref as rc
    import test_ground as tg
    rows = tg.random_rows(600, 5)
    path = str(tmp_path / "set.bin")
    rc.write_map(path, rows)
    gkw = dict(cell_mm=100, nu=64, nv=34, reach_cells=6)
    want_g = gr.ground_set([rows], **gkw)
    ckw = dict(body_cells=1, unknown_passable=1, turn_cells=2, turn_cost=5, reverse_weight=4, max_steps=60, **SOFT)
    mm = rr.multiplier(want_g["state"], want_g["clear2"], **ckw)
    free = np.argwhere(mm > 0)
    assert len(free) > 100
    goals = [[(int(free[0][1]), int(free[0][0]), -1)], [(int(free[-1][1]), int(free[-1][0]), 4)]]
    starts = [(0, int(free[-1][1]), int(free[-1][0]), 0), (1, int(free[len(free) // 2][1]), int(free[len(free) // 2][0]), 6)]
    want = cr.route_car(want_g["state"], want_g["clear2"], goals, starts=starts, **ckw)
    assert want["info"][0]["reachable_cells"] > 50

    fresh = _ctx()
    g1 = fresh.ground_maps([path], **gkw)
    tg.check(g1, want_g, "ground")
    r1 = capi.route_car(fresh, g1, goals, starts=starts, **ckw)
    check(r1, want, "fresh")
    g2 = fresh.ground_maps([path], **gkw)
    tg.check(g2, want_g, "ground again")
    fresh.close()

    cam = dict(width=64, height=48, fx=40.0, fy=40.0, cx=31.5, cy=23.5)
    busy = _ctx()
    for frame in synth.make_sequence(cam, synth.kitti_trajectory(2), seed=3):
        busy.process_frame(*frame)
    counts, model = busy.counts(), np.asarray(busy.download_model()).copy()
    r2 = capi.route_car(busy, g1, goals, starts=starts, **ckw)
    check(r2, want, "after frames")
    assert busy.counts() == counts and np.array_equal(np.asarray(busy.download_model()), model, equal_nan=True)
    g3 = busy.ground_maps([path], **gkw)
    tg.check(g3, want_g, "ground after the car's call")
    busy.close()


@pytest.mark.gpu
def test_gpu_refusals_and_stall(m):
    from surfelmapping_amd import capi
    fresh = _ctx()
    with pytest.raises(capi.SurfelMapError) as e:
        capi.route_car_stats(fresh)
    assert e.value.rc == capi.SM_E_ARG
    fresh.close()
    want, args = random_case(1, 0, 0, 0)
    check(capi.route_car(m, **args), want, "before the refusals")
    before = capi.route_car_stats(m)
    for what, call in refusals(m._h):
        assert call.rc == capi.SM_E_ARG and what in call.error and call.untouched, (what, call.rc, call.error)
    # a call that does not converge within max_rounds: SM_E_STALL, nothing written, the last call's stats left
    state, clear2 = args["ground"]["state"], args["ground"]["clear2"]
    p = capi.route_car_params(nu=NU, nv=NV, turn_cells=1, max_rounds=1, **SOFT)
    cost = np.full((8, NV, NU), 0xA5A5A5A5, np.uint32)
    nxt = np.full((8, NV, NU), 0xA5, np.uint8)
    info = capi.SmRouteCarInfo(7, 7, 7, 7, 7)
    first, flat = np.array([0, 1], np.uint32), np.array(args["goals"][0][0], np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = m._L.sm_route_car(m._h, C.byref(p), ptr(state), ptr(clear2), 1, ptr(first), ptr(flat), 0, None, ptr(cost), ptr(nxt), None, None, None, C.byref(info))
    assert rc == capi.SM_E_STALL and "max_rounds" in m._L.sm_last_error().decode()
    assert (cost == 0xA5A5A5A5).all() and (nxt == 0xA5).all() and info.goals_used == 7 and capi.route_car_stats(m) == before
    check(capi.route_car(m, **args), want, "after the stall")
