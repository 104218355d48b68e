"""A map set as a planner's ground map (sm_ground_maps, sm_ground_stats; SurfelMap.ground_maps; DESIGN.md "4v. Ground map").
CPU: the restatement (ground_ref.py) against the header's example worked by hand, against its own invariances and a brute-force
clearance; the library's symbols, defaults, header and the argument rules that need no device.  GPU: every plane and info of the
HIP path against the restatement, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from surfelmapping_amd.capi import SmGroundParams  # noqa: F401  (the binding's symbol: without it nothing here can run)

import ground_ref as gr
import recall_ref as cr
import test_simplify as ts
from ground_ref import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sm_default_ground_params", "sm_ground_maps", "sm_ground_stats")
UP = dict(n=(0, 1, 0))                                                        # a floor's normal as stored in a world with y down: into the floor


@pytest.fixture(scope="module")
def scene():
    return ts.Scene()


def scene_window(rows, cell_mm):
    """a window of `cell_mm` cells that covers the records' x and z, its low corner on whole metres"""
    lo = np.floor(rows[:, [0, 2]].min(axis=0)) - 1.0
    hi = np.ceil(rows[:, [0, 2]].max(axis=0)) + 1.0
    n = np.ceil((hi - lo) * 1000.0 / cell_mm).astype(int)
    return dict(cell_mm=cell_mm, origin=(float(lo[0]), 0.0, float(lo[1])), nu=int(n[0]), nv=int(n[1]))


def brute_clearance(block, reach):
    nv, nu = block.shape
    bv, bu = np.nonzero(block)
    out = np.full((nv, nu), reach * reach, np.int64)
    for v in range(nv):
        for u in range(nu):
            if len(bv):
                out[v, u] = min(reach * reach, int(((bv - v) ** 2 + (bu - u) ** 2).min()))
    return out.astype(np.uint32)


def check_scene(got, rows, window):
    """what a planner reads off the street: the road is FREE, walls and boxes are OBSTACLE, clearance grows away from them"""
    state, clear2, cls = got["state"], got["clear2"], got["cls"]
    by_state = got["info"]["cells_by_state"]
    assert by_state[gr.FREE] > 50 and by_state[gr.OBSTACLE] > 10, by_state
    road = (cls == 0) & (state != gr.OBSTACLE)
    assert road.sum() > 30 and (state[road] == gr.FREE).mean() > 0.9, (road.sum(), np.bincount(state[road], minlength=4))
    # every cell that holds a wall's record (class 2) and is not UNKNOWN -- one record with no road near it -- is an OBSTACLE; every
    # OBSTACLE cell holds a record of a wall or a box (class 13)
    ok, X, _, _, col = gr.quantities(rows, window["origin"])
    assert ok.all()
    C = gr.q16(window["cell_mm"])
    cu, cv = X[:, 0] // C, X[:, 2] // C
    assert ((cu >= 0) & (cu < window["nu"]) & (cv >= 0) & (cv < window["nv"])).all()
    wall, box = np.zeros(state.shape, bool), np.zeros(state.shape, bool)
    wall[cv[col >> 24 == 2], cu[col >> 24 == 2]] = True
    box[cv[col >> 24 == 13], cu[col >> 24 == 13]] = True
    assert (state[wall & (state != gr.UNKNOWN)] == gr.OBSTACLE).all() and (state[wall] == gr.OBSTACLE).sum() > 30
    assert (wall | box)[state == gr.OBSTACLE].all() and (state[box] == gr.OBSTACLE).sum() >= 5
    assert (clear2[state == gr.OBSTACLE] == 0).all() and (clear2[state == gr.FREE] > 0).all()
    # clearance is 1-Lipschitz in cells: sqrt(clear2) of 4-neighbours differs by at most 1, and it grows away from the obstacles
    r = np.sqrt(clear2.astype(np.float64))
    assert (np.abs(np.diff(r, axis=0)) <= 1.0 + 1e-9).all() and (np.abs(np.diff(r, axis=1)) <= 1.0 + 1e-9).all()
    free = state == gr.FREE
    assert clear2[free].max() >= 9


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_header_example():
    assert (gr.q16(1000), gr.q16(200), gr.q16(150), gr.q16(2000)) == (65536, 13107, 9830, 131072)
    got = gr.ground(gr.EXAMPLE_ROWS, **gr.EXAMPLE_PARAMS)
    assert got["Z"].tolist() == [[-65536, -65536, gr.NONE, -65536, -32768]]
    assert got["R"].tolist() == [[-65536, -65536, -65536, -65536, -32768]]
    assert got["ground"].tolist() == [[-65536, -61440, gr.NONE, -65536, -32768]]
    assert got["top"].tolist() == [[0, 0, 98304, 0, 0]]
    assert got["state"].tolist() == [[1, 1, 2, 3, 3]]
    assert got["cls"].tolist() == [[0, 0, 255, 3, 3]]
    assert got["bgr"][0, 1].tolist() == [10, 100, 200] and got["bgr"][0, 2].tolist() == [0, 0, 0]
    assert got["clear2"].tolist() == [[4, 1, 0, 0, 0]]
    assert got["info"] == dict(records=7, counts_by_kind=[5, 2, 0, 0, 0, 0], cells_by_state=[0, 2, 1, 2])
    # the weights tie in cell 1: the lower id wins the class, whatever the order
    assert gr.ground(gr.EXAMPLE_ROWS[::-1], **gr.EXAMPLE_PARAMS)["cls"][0, 1] == 1
    assert gr.ground(gr.EXAMPLE_ROWS[::-1], ids=np.arange(7)[::-1], **gr.EXAMPLE_PARAMS)["cls"][0, 1] == 0
    # every up direction with the rows moved to suit
    for up in range(6):
        moved = gr.ground(gr.permute_axes(gr.EXAMPLE_ROWS, up), **dict(gr.EXAMPLE_PARAMS, up=up))
        same(moved, got, up)
    # step_mm 0 switches the steps off; unknown_blocks makes no difference without an UNKNOWN cell; min_obstacle 3 frees cell 2
    assert gr.ground(gr.EXAMPLE_ROWS, step_mm=0, **gr.EXAMPLE_PARAMS)["state"].tolist() == [[1, 1, 2, 1, 1]]
    got3 = gr.ground(gr.EXAMPLE_ROWS, min_obstacle=3, **gr.EXAMPLE_PARAMS)
    assert got3["state"].tolist() == [[1, 1, 0, 3, 3]] and got3["clear2"].tolist() == [[9, 4, 1, 0, 0]]
    assert gr.ground(gr.EXAMPLE_ROWS, min_obstacle=3, unknown_blocks=1, **gr.EXAMPLE_PARAMS)["clear2"].tolist() == [[4, 1, 0, 0, 0]]


def same(got, want, what):
    for k in gr.PLANES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    assert got["info"] == want["info"], (what, got["info"], want["info"])


def random_rows(n, seed, span=(6.0, 3.0), classes=6):
    """records over a floor at y = 1 with bumps, walls and clutter above it: every kind of reading 2"""
    rs = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        x, z = rs.rand() * span[0], rs.rand() * span[1]
        kind = rs.randint(0, 4)
        if kind < 2:                                                           # floor, within or above the band
            y, nrm = 1.0 - rs.rand() * (0.1 if kind == 0 else 0.4), (0.2 * rs.rand(), 1, 0.2 * rs.rand())
        elif kind == 2:                                                        # a wall or a box
            y, nrm = 1.0 - rs.rand() * 2.5, (1, 0, 0)
        else:                                                                  # anything: overhangs, below the floor
            y, nrm = 1.5 - rs.rand() * 5.0, tuple(rs.rand(3) - 0.5)
        rows.append(record(x, y, z, n=nrm, sem=int(rs.randint(0, classes)), conf=float(rs.rand() * 20 + 0.01),
                           bgr=tuple(int(v) for v in rs.randint(0, 256, 3)), t0=float(i % 7)))
    return np.stack(rows)


def test_restatement_is_a_function_of_ids_and_records():
    rows = random_rows(3000, 1)
    kw = dict(cell_mm=100, nu=60, nv=30)
    want = gr.ground(rows, **kw)
    assert all(v > 0 for v in want["info"]["counts_by_kind"][:3]) and all(v > 0 for v in want["info"]["cells_by_state"])
    perm = np.random.RandomState(7).permutation(len(rows))
    same(gr.ground(rows[perm], ids=perm, **kw), want, "permuted, ids kept")
    for cuts in ((), (700,), (300, 301, 900, 900)):
        same(gr.ground_set(np.split(rows, list(cuts)), **kw), want, cuts)
    # other ids: only the class of a cell whose heaviest records tie may move
    moved = gr.ground(rows, ids=perm, **kw)
    for k in ("ground", "top", "state", "bgr", "clear2"):
        assert np.array_equal(moved[k], want[k]), k


@pytest.mark.parametrize("reach", (1, 5, 255))
def test_clearance_against_brute_force(reach):
    rs = np.random.RandomState(reach)
    for density in (0.0, 0.002, 0.02, 0.3, 1.0):
        block = rs.rand(33, 40) < density
        got = gr.clearance(block, reach)
        assert got.dtype == np.uint32 and np.array_equal(got, brute_clearance(block, reach)), (reach, density)
    # through the states: OBSTACLE and STEP block, UNKNOWN with unknown_blocks alone
    state = rs.randint(0, 4, (33, 40)).astype(np.uint8)
    state[rs.rand(33, 40) < 0.9] = gr.FREE
    for unknown_blocks in (0, 1):
        block = gr.blocking(state, unknown_blocks)
        assert np.array_equal(block, (state >= 2) | ((state == 0) & bool(unknown_blocks)))
        assert np.array_equal(gr.clearance(block, reach), brute_clearance(block, reach))


def test_fill_tie_breaks():
    # two grounds at equal distance in u: the lower u' wins; in v: the lower v'; across: the lower v' before the lower u'
    def grid(cells, nu=5, nv=5):
        Z, has = np.zeros((nv, nu), np.int64), np.zeros((nv, nu), bool)
        for (u, v), z in cells.items():
            Z[v, u], has[v, u] = z, True
        return Z, has
    R, got = gr.fill(*grid({(1, 2): 10, (3, 2): 20}), 1)
    assert R[2, 2] == 10 and got[2, 2] and not got[0, 2] and R[2, 0] == 10 and R[2, 4] == 20
    R, _ = gr.fill(*grid({(2, 1): 10, (2, 3): 20}), 1)
    assert R[2, 2] == 10
    R, _ = gr.fill(*grid({(3, 2): 10, (2, 3): 20, (1, 2): 30, (2, 1): 40}), 1)   # all at distance 1: v' = 1 first
    assert R[2, 2] == 40
    R, _ = gr.fill(*grid({(3, 2): 10, (1, 2): 30, (2, 3): 20}), 1)              # v' = 2 before v' = 3, then u' = 1 before u' = 3
    assert R[2, 2] == 30
    R, _ = gr.fill(*grid({(3, 3): 10, (1, 1): 20, (3, 1): 30, (2, 4): 40}), 2)  # the diagonals (2) before the straight cell at 2 (4)
    assert R[2, 2] == 20
    R, got = gr.fill(*grid({(0, 0): 10}), 1)                                   # the window is square: |du| <= 1 and |dv| <= 1
    assert got[1, 1] and not got[2, 0] and not got[0, 2]
    R, got = gr.fill(*grid({(0, 0): 10}), 0)
    assert got.sum() == 1
    # through the whole restatement: a wall cell between two floors of other heights
    rows = np.stack([record(0.5, 1.0, 0.5, **UP), record(2.5, 0.5, 0.5, **UP), record(1.5, 0.0, 0.5, n=(1, 0, 0)), record(1.5, -0.5, 0.5, n=(1, 0, 0))])
    got = gr.ground(rows, cell_mm=1000, nu=3, nv=1)
    assert got["R"].tolist() == [[-65536, -65536, -32768]] and got["top"].tolist() == [[0, 98304, 0]]


def test_edge_values():
    kw = dict(cell_mm=1000, nu=2, nv=2)
    C = 65536
    one = lambda *a, **k: gr.ground(record(*a, **dict(UP, **k))[None], **kw)   # noqa: E731
    # -0.0 lies in cell 0; the least negative coordinate floors into cell -1: OUTSIDE
    got = one(-0.0, 1.0, -0.0)
    assert got["info"]["counts_by_kind"] == [1, 0, 0, 0, 0, 0] and got["state"][0, 0] == gr.FREE
    assert one(-1e-6, 1.0, 0.5)["info"]["counts_by_kind"] == [0, 0, 0, 0, 1, 0]
    assert one(0.5, 1.0, -1e-6)["info"]["counts_by_kind"] == [0, 0, 0, 0, 1, 0]
    # the window's edges: in at 0, out at nu * C
    assert one(0.0, 1.0, 0.0)["state"][0, 0] == gr.FREE
    assert one(np.float32(2.0 - 2.0 ** -16), 1.0, 0.5)["state"][0, 1] == gr.FREE
    assert one(2.0, 1.0, 0.5)["info"]["counts_by_kind"][4] == 1 and one(0.5, 1.0, 2.0)["info"]["counts_by_kind"][4] == 1
    # with an origin: the window's low corner; a negative world coordinate inside the window
    got = gr.ground(record(-2.5, 1.0, -0.5, **UP)[None], origin=(-3.0, 0.25, -2.0), **kw)
    assert got["state"].tolist() == [[0, 0], [1, 0]] and got["ground"][1, 0] == -(C * 3 // 4)
    # |H| = 2^30 is OUTSIDE, one step below it is in
    assert one(0.5, 16384.0, 0.5)["info"]["counts_by_kind"][4] == 1 and one(0.5, -16384.0, 0.5)["info"]["counts_by_kind"][4] == 1
    got = one(0.5, np.float32(16384.0 - 2.0 ** -10), 0.5)
    assert got["ground"][0, 0] == -(1 << 30) + 64 and got["info"]["counts_by_kind"][0] == 1
    # loose records: test_simplify's, of which the two that only leave a 10 mm grid are regular here -- x = 3000 is OUTSIDE, y = -3000
    # lies in a cell without a reference height
    loose = ts.loose_rows()
    assert gr.ground(loose, **kw)["info"]["counts_by_kind"] == [0, 0, 0, 1, 1, len(loose) - 2]
    # min_up: 45 degrees is in at the default, a little steeper is out and then an obstacle candidate only
    s = np.float32(np.sqrt(0.5))
    assert one(0.5, 1.0, 0.5, n=(s, s, 0))["info"]["counts_by_kind"][0] == 1
    assert one(0.5, 1.0, 0.5, n=(0.8, 0.6, 0))["info"]["counts_by_kind"] == [0, 0, 0, 1, 0, 0]
    # ground_mask: a class that may not be ground
    mask = [0xFFFFFFFF] * 8
    mask[0] &= ~(1 << 3)
    assert gr.ground(record(0.5, 1.0, 0.5, **UP)[None], ground_mask=mask, **kw)["info"]["counts_by_kind"] == [0, 0, 0, 1, 0, 0]
    # the band's closed end, the body band's open ends, an overhang, a record below the floor; at the defaults the band reaches into
    # the body band, so a ground-like record just above the band is an obstacle candidate
    floor = record(0.5, 1.0, 0.5, **UP)
    at = lambda d: 1.0 - d / 65536.0                                           # noqa: E731
    cases = ((at(6554), True, 0), (at(13107), True, 0), (at(13108), True, 1), (at(9830), False, 2), (at(9831), False, 1), (0.5, False, 1),
             (at(131072), False, 2), (at(131071), False, 1), (-3.0, False, 2), (1.5, False, 2),
             (1.5, True, 1))                                                   # (the lower ground-like record is the ground: the floor is the obstacle)
    for y, like, kind in cases:
        got = gr.ground(np.stack([floor, record(0.5, y, 0.5, n=(0, 1, 0) if like else (1, 0, 0))]), **kw)
        want = [1, 0, 0, 0, 0, 0]
        want[kind] += 1
        assert got["info"]["counts_by_kind"] == want, (y, like, kind, got["info"])
    # band_mm 50 (B = 3277) leaves a slab below clear_lo: IGNORED
    got = gr.ground(np.stack([floor, record(0.5, at(5000), 0.5, **UP)]), band_mm=50, **kw)
    assert got["info"]["counts_by_kind"] == [1, 0, 1, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the library, without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_defaults_and_binding():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None and name in capi.SYMBOLS
    p = capi.default_ground_params()
    got = {k: getattr(p, k) for k, _ in capi.SmGroundParams._fields_}
    got["origin"], got["ground_mask"] = tuple(p.origin), tuple(p.ground_mask)
    assert got == gr.DEFAULTS
    q = capi.ground_params(cell_mm=20, origin=(1, 2, 3), classes=(0, 200), up=4)
    assert q.cell_mm == 20 and q.up == 4 and tuple(q.origin) == (1.0, 2.0, 3.0) and tuple(q.ground_mask) == tuple(capi.segment_class_mask((0, 200)))
    with pytest.raises(KeyError):
        capi.ground_params(cell=1)
    for name in ("ground_maps", "ground_stats"):
        assert callable(getattr(capi.SurfelMap, name))
    assert capi.GROUND_KINDS == gr.KINDS and capi.GROUND_STATES == gr.STATES and capi.GROUND_NONE == gr.NONE and capi.GROUND_PLANES == gr.PLANES
    header = open(os.path.join(ROOT, "include", "sm_c_api.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
    for line in ("typedef struct sm_ground_params {", "typedef struct sm_ground_info {", "typedef struct sm_ground_stats_t {",
                 "#define SM_GROUND_NONE     INT32_MIN", "#define SM_GROUND_STEP     3"):
        assert line in header, line


def test_argument_rules_that_need_no_device():
    from surfelmapping_amd import capi
    L = capi.load()
    p, st, info = capi.default_ground_params(), capi.SmGroundStats(), capi.SmGroundInfo()
    src = capi.map_source([], True)
    plane = np.full(4, 0xA5, np.uint8)
    assert L.sm_default_ground_params(None) == capi.SM_E_ARG
    assert L.sm_ground_maps(None, C.byref(src), C.byref(p), None, None, plane.ctypes.data_as(C.c_void_p), None, None, None, C.byref(info)) == capi.SM_E_ARG
    assert L.sm_ground_stats(None, C.byref(st)) == capi.SM_E_ARG
    assert (plane == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
_ctx = ts._ctx
INFO_KEYS = ("records", "counts_by_kind", "cells_by_state")


def check(got, want, what):
    """every plane and info against the restatement, bit for bit"""
    for k in gr.PLANES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])
    assert {k: got["info"][k] for k in INFO_KEYS} == want["info"], (what, got["info"], want["info"])


def run(m, paths, parts, what, include_model=False, want=None, **kw):
    """ground_maps of `paths` against the restatement of `parts`; -> (what the call returned, the restatement)"""
    got = m.ground_maps(paths, include_model=include_model, **kw)
    want = gr.ground_set(parts, **kw) if want is None else want
    check(got, want, what)
    return got, want


def no_combine(fn):
    os.environ["SM_GROUND_NO_COMBINE"] = "1"
    try:
        return fn()
    finally:
        os.environ.pop("SM_GROUND_NO_COMBINE", None)


@pytest.mark.gpu
@pytest.mark.parametrize("up", range(6))
def test_gpu_header_example(tmp_path, up):
    rows = gr.permute_axes(gr.EXAMPLE_ROWS, up)
    path = str(tmp_path / "e.bin")
    cr.write_map(path, rows)
    m = _ctx()
    got, _ = run(m, [path], [rows], up, want=dict(gr.ground(gr.EXAMPLE_ROWS, **gr.EXAMPLE_PARAMS)), **dict(gr.EXAMPLE_PARAMS, up=up))
    assert got["state"].tolist() == [[1, 1, 2, 3, 3]] and got["clear2"].tolist() == [[4, 1, 0, 0, 0]]
    assert got["info"]["counts"] == dict(GROUND=5, OBSTACLE=2, IGNORED=0, UNREFERENCED=0, OUTSIDE=0, LOOSE=0)
    assert got["info"]["cells"] == dict(UNKNOWN=0, FREE=2, OBSTACLE=1, STEP=2)
    st = m.ground_stats()
    assert st["chunks"] == 2 and st["launches"] == 7 and st["files_skipped"] == 0 and st["total_ms"] > 0
    m.close()


def run_rows():
    """runs of 4 records of one cell one after the other, then 300 of one cell across waves and blocks -- ground, band, wall and
    overhang records of mixed classes, weights and colours --, then more runs of 4"""
    rs = np.random.RandomState(11)
    fours = np.stack([record(0.1 * i + 0.1 * u, 1.0 - 0.05 * h, 0.1 * j + 0.1 * v, conf=c, sem=k, bgr=(int(255 * u), int(255 * v), 7 * i), **UP)
                      for i in range(8) for j in range(8) for u, v, h, c, k in zip(rs.rand(4) * .9 + .05, rs.rand(4) * .9 + .05, rs.rand(4), (0.1, 0.5, 1.0, 20.0),
                                                                                (0, 1, 0, 2))])
    run_300 = random_rows(300, 12, span=(0.09, 0.09))
    run_300[:, 0] += 2.0
    return np.concatenate([fours[:130], run_300, fours[130:]])


@pytest.mark.gpu
def test_gpu_runs_of_one_cell(tmp_path):
    rows = run_rows()
    path = str(tmp_path / "runs.bin")
    cr.write_map(path, rows)
    m = _ctx()
    kw = dict(cell_mm=100, nu=24, nv=9)
    got, want = run(m, [path], [rows], "combined", **kw)
    assert want["info"]["counts_by_kind"][0] > 256 and want["info"]["counts_by_kind"][1] > 20 and want["info"]["counts_by_kind"][2] > 20
    no_combine(lambda: run(m, [path], [rows], "not combined", want=want, **kw))
    m.close()


@pytest.mark.gpu
def test_gpu_257_records_and_the_model(tmp_path):
    """one lane in a second block; the set as a file, as the live model, as both (every cell then holds each record twice)"""
    rows = random_rows(257, 257, span=(2.0, 1.5), classes=256)
    path = str(tmp_path / "s.bin")
    cr.write_map(path, rows)
    m = _ctx(rows)
    kw = dict(cell_mm=100, nu=21, nv=16)
    run(m, [path], [rows], "file", **kw)
    run(m, [], [rows], "model", include_model=True, **kw)
    run(m, [path], [rows, rows], "both", include_model=True, origin=(0.25, -1.0, 0.125), min_obstacle=4, **kw)
    ts.same_rows(m.download_model(), rows, "the live model")
    m.close()


def tile_rows(nu, nv, seed):
    """a floor over the whole window with holes, and walls of two records in the corners of the kernels' tiles (16 x 16 cells for the
    fill, 256 cells of a row for the transform) and on the window's edge"""
    rs = np.random.RandomState(seed)
    rows = []
    for v in range(nv):
        for u in range(nu):
            if rs.rand() < 0.6:
                rows.append(record((u + 0.5) * 0.1, 1.0 - 0.02 * rs.rand(), (v + 0.5) * 0.1, sem=int(rs.randint(0, 3)), **UP))
    walls = {(0, 0), (nu - 1, 0), (0, nv - 1), (nu - 1, nv - 1)}
    walls |= {(u, v) for u in (0, 15, 16, 31, 32, 47, 48, 63, 64) for v in (15, 16, 31, 32, 255, 256, 299) if u < nu and v < nv}
    for u, v in sorted(walls):
        rows += [record((u + 0.5) * 0.1, 0.5 - 0.3 * k, (v + 0.5) * 0.1, n=(1, 0, 0)) for k in range(2)]
    return np.stack(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("nu,nv,cases", ((65, 33, ((0, 1), (16, 17), (3, 255))), (1, 300, ((16, 255), (0, 17), (2, 1)))))
def test_gpu_tile_boundaries(tmp_path, nu, nv, cases):
    rows = tile_rows(nu, nv, nu)
    path = str(tmp_path / "tiles.bin")
    cr.write_map(path, rows)
    m = _ctx()
    for fill_cells, reach_cells in cases:
        for unknown_blocks in (0, 1):
            got, want = run(m, [path], [rows], (fill_cells, reach_cells, unknown_blocks), cell_mm=100, nu=nu, nv=nv, fill_cells=fill_cells,
                            reach_cells=reach_cells, unknown_blocks=unknown_blocks)
            assert np.array_equal(want["clear2"], brute_clearance(gr.blocking(want["state"], unknown_blocks), reach_cells))
    assert want["info"]["cells_by_state"][gr.OBSTACLE] >= 4
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cell_mm", (100, 250))
def test_gpu_scene_shuffled_over_three_files_and_the_model(scene, tmp_path, cell_mm):
    """the synthetic street under other ids in three files (one empty) and the live model: the road is FREE, walls and boxes are
    OBSTACLE, clearance grows away from them -- on the restatement and, bit for bit, on the device.  The default `up` is the sign
    the stored normals have: the road's normals point to -y"""
    window = scene_window(scene.rows, cell_mm)
    straight = gr.ground(scene.rows, **window)
    check_scene(straight, scene.rows, window)
    perm = np.random.RandomState(3).permutation(len(scene.rows))
    parts = np.split(scene.rows[perm], [500, 500, 1200])
    paths = [str(tmp_path / f"p{i}.bin") for i in range(3)]
    for p, part in zip(paths, parts[:3]):
        cr.write_map(p, part)
    m = _ctx(parts[3])
    got, want = run(m, paths, parts, cell_mm, include_model=True, **window)
    for k in ("ground", "top", "state", "bgr", "clear2"):                     # (classes follow the ids where the heaviest records tie)
        assert np.array_equal(want[k], straight[k]), k
    check_scene(got, scene.rows, window)
    assert m.ground_stats()["chunks"] == 6                                    # (two files with records and the model, twice)
    ts.same_rows(m.download_model(), parts[3], "the live model")
    m.close()


@pytest.mark.gpu
def test_gpu_file_index_skips_a_file_outside_the_window(tmp_path):
    near, far = random_rows(400, 5, span=(3.0, 3.0)), random_rows(300, 6, span=(3.0, 3.0))
    far[:, 0] += 100.0
    paths = [str(tmp_path / "near.bin"), str(tmp_path / "far.bin")]
    cr.write_map(paths[0], near)
    cr.write_map(paths[1], far)
    m = _ctx()
    kw = dict(cell_mm=100, nu=30, nv=30)
    got, want = run(m, paths, [near, far], "nothing known yet", **kw)
    assert m.ground_stats()["files_skipped"] == 0 and want["info"]["counts_by_kind"][4] == 300
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (0.0, 0.0, 5000.0)
    assert m.recall(paths, pose=pose, mode="count", radius=8.0) == 0           # (a reading that notes the files' boxes)
    run(m, paths, [near, far], "far.bin skipped", want=want, **kw)
    st = m.ground_stats()
    assert st["files_skipped"] == 1 and st["chunks"] == 2
    os.environ["SM_RECALL_NO_INDEX"] = "1"
    try:
        run(m, paths, [near, far], "no index", want=want, **kw)
        assert m.ground_stats()["files_skipped"] == 0 and m.ground_stats()["chunks"] == 4
    finally:
        os.environ.pop("SM_RECALL_NO_INDEX", None)
    # a window over the far file: the near one is skipped; its records keep their ids (the classes of the far cells follow them)
    kw_far = dict(kw, origin=(100.0, 0.0, 0.0))
    run(m, paths, [near, far], "near.bin skipped", **kw_far)
    assert m.ground_stats()["files_skipped"] == 1
    m.close()


@pytest.mark.gpu
def test_gpu_null_planes(tmp_path):
    rows = random_rows(500, 21, span=(3.0, 3.0))
    path = str(tmp_path / "a.bin")
    cr.write_map(path, rows)
    m = _ctx()
    kw = dict(cell_mm=100, nu=30, nv=30)
    want = gr.ground(rows, **kw)
    launches = {}
    for mask in range(64):
        planes = tuple(k for i, k in enumerate(gr.PLANES) if mask >> i & 1)
        got = m.ground_maps([path], planes=planes, **kw)
        for k in gr.PLANES:
            assert (got[k] is None) if k not in planes else np.array_equal(got[k], want[k]), (planes, k)
        assert {k: got["info"][k] for k in INFO_KEYS} == want["info"]
        launches[mask] = m.ground_stats()["launches"]
    assert launches[63] == launches[32] == launches[0] + 2                     # (without clear2 the transform is not run)
    m.close()


@pytest.mark.gpu
def test_gpu_refusals(tmp_path):
    from surfelmapping_amd import capi
    rows = random_rows(200, 31)
    path = str(tmp_path / "a.bin")
    cr.write_map(path, rows)
    m = _ctx(rows[:50])
    with pytest.raises(capi.SurfelMapError) as e:                            # (no call has succeeded yet: no stats)
        m.ground_stats()
    assert e.value.rc == capi.SM_E_ARG
    bads = (dict(cell_mm=9), dict(cell_mm=10001), dict(up=-1), dict(up=6), dict(origin=(0, float("nan"), 0)), dict(nu=0), dict(nu=8193), dict(nv=0),
            dict(nv=8193), dict(nu=4097, nv=4096), dict(min_up=-1), dict(min_up=16385), dict(band_mm=-1), dict(band_mm=10001),
            dict(clear_lo_mm=-1), dict(clear_lo_mm=2000), dict(clear_hi_mm=100001), dict(min_obstacle=0), dict(fill_cells=-1), dict(fill_cells=17),
            dict(step_mm=-1), dict(step_mm=10001), dict(reach_cells=0), dict(reach_cells=256), dict(unknown_blocks=2), dict(normal_sign=0),
            dict(normal_sign=2))
    for bad in bads:
        with pytest.raises(capi.SurfelMapError) as e:
            m.ground_maps([path], **bad)
        assert e.value.rc == capi.SM_E_ARG and list(bad)[0][:5] in str(e.value), (bad, str(e.value))
    # a missing file: no plane is written, not info
    p, info, src = capi.ground_params(nu=8, nv=8), capi.SmGroundInfo(), capi.map_source([path, str(tmp_path / "nowhere.bin")], False)
    info.records = 12345
    bufs = [np.full(8 * 8 * 4, 0xA5, np.uint8) for _ in range(6)]
    ptrs = [b.ctypes.data_as(C.c_void_p) for b in bufs]
    assert m._L.sm_ground_maps(m._h, C.byref(src), C.byref(p), *ptrs, C.byref(info)) == capi.SM_E_ARG
    assert all((b == 0xA5).all() for b in bufs) and info.records == 12345
    src = capi.map_source([path], False)
    assert m._L.sm_ground_maps(m._h, None, C.byref(p), *ptrs, C.byref(info)) == capi.SM_E_ARG
    assert m._L.sm_ground_maps(m._h, C.byref(src), None, *ptrs, C.byref(info)) == capi.SM_E_ARG
    assert m._L.sm_ground_maps(m._h, C.byref(src), C.byref(p), *ptrs, None) == capi.SM_E_ARG
    assert m._L.sm_ground_stats(m._h, None) == capi.SM_E_ARG
    assert all((b == 0xA5).all() for b in bufs)
    for configure in ("shard_stream_configure", "rig_configure"):
        part = _ctx()
        getattr(part, configure)(0, 1)
        with pytest.raises(capi.SurfelMapError) as e:
            part.ground_maps([path])
        assert e.value.rc == capi.SM_E_UNSUPPORTED
        part.close()
    # the largest window, empty: every cell UNKNOWN, nothing blocks
    got = m.ground_maps([], nu=4096, nv=4096, planes=("state", "clear2"), reach_cells=255)
    assert (got["state"] == 0).all() and (got["clear2"] == 255 * 255).all() and got["info"]["cells"]["UNKNOWN"] == 1 << 24
    # loose records and records on the window's edges
    end = 8 * gr.q16(100) / 65536.0                                          # the window's high edge: 8 cells of 6554, exact in float32
    edge = np.stack([record(-0.0, 1.0, -0.0, **UP), record(-1e-6, 1.0, 0.5, **UP), record(end, 1.0, 0.5, **UP), record(0.5, 16384.0, 0.5, **UP),
                     record(end - 2.0 ** -16, 1.0, 0.5, **UP)] + list(ts.loose_rows()))
    cr.write_map(path, edge)
    got, want = run(m, [path], [edge], "edges", cell_mm=100, nu=8, nv=8)
    assert want["info"]["counts_by_kind"] == [2, 0, 0, 0, 5, len(ts.loose_rows()) - 2]   # (two of those rows are regular and OUTSIDE here)
    ts.same_rows(m.download_model(), rows[:50], "the live model")
    m.close()
