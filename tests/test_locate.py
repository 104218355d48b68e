"""One map set located in another without a guess (sm_locate_maps; DESIGN.md "4ab. Locating").  Without a GPU: the restatement
(tests/locate_ref.py) against the header's hand-derived example, its fast path against the literal triple loop, its status rules at
their thresholds, the record edge values, the scenes (tests/locate_scenes.py), the binding's defaults and the argument rules that
need no device.  On the GPU: every field of the info and the pose, bit for bit against the restatement -- which gets the library's
own rotation table -- over the shapes at which the search takes another path."""
import ctypes as C
import math

import numpy as np
import pytest

from surfelmapping_amd.capi import SmLocateParams  # noqa: F401  (the binding's symbol: without it nothing here can run)

import ground_ref as gr
import locate_ref as lr
import locate_scenes as ls
import recall_ref as cr
import register_ref as rr
import retire_ref as ret
import track_ref as tr

ENTRY_POINTS = ("sm_default_locate_params", "sm_locate_rotations", "sm_locate_maps", "sm_locate_stats")
F32, F64 = np.float32, np.float64
W, H, F = 96, 64, 60.0
INFO_FIELDS = ("status", "row", "du", "dv", "score", "coarse_k", "coarse_du", "coarse_dv", "coarse_score", "runner_up", "n_s", "target_cells",
               "height_pairs", "dh", "source_counts", "target_counts")
# (yaw in degrees, translation) of the yard's truths: any yaw, tens of metres, a height
TRUTHS = ((135.0, (37.0, -52.0, 1.25)), (250.0, (-61.0, 18.0, -0.75)), (33.0, (12.0, 44.0, 0.5)))
MIN_INLIERS = 500            # the yard's source set holds 3000 records
PIVOT = (3.0, -2.0, 1.5)     # the middle of the yard in the target's world


# ---------------------------------------------------------------------------------------------------------------------
# scenes of cells: a structure-like record stands at a cell's centre, so the rasters are known by construction
# ---------------------------------------------------------------------------------------------------------------------
def cell_rows(cells, origin=(0.0, 0.0, 0.0), cell=1.0, reps=1, ground=None):
    """rows of the example's world (up 3): `reps` structure-like records in a row at the centre of every cell (cu, cv) counted from
    `origin`; ground: per cell a height in metres (None: no ground record), a ground-like record there"""
    rows = []
    for i, (cu, cv) in enumerate(cells):
        x, y = origin[0] + (cu + 0.5) * cell, origin[2] + (cv + 0.5) * cell
        rows += [lr.wall(x, y, sem=i % 7)] * reps
        if ground is not None and ground[i] is not None:
            rows.append(gr.record(x, origin[1] - ground[i], y, n=(0, 1, 0)))
    return np.stack(rows) if rows else np.zeros((0, 12), F32)


def cell_scene(seed, n_s, nu, nv, n_yaw, refine, row=None, shift=None, clutter=0.3, reps=2, span=None, heights=True):
    """(source rows, target rows, params): n_s distinct source cells in a square of about twice their number, the target their
    rotation by the fine row `row` moved by `shift` (cut to the window) plus clutter; every cell `reps` records, min_records = reps, and
    a few cells with one record less, which must not count"""
    rng = np.random.default_rng(seed)
    span = span or max(2, int(math.ceil(math.sqrt(2.0 * n_s) / 2)))
    side = 2 * span + 1
    pick = rng.choice(side * side, n_s, replace=False)
    S = np.stack([pick % side - span, pick // side - span], axis=1)
    table = lr.rotations(n_yaw, refine)
    row = refine * int(rng.integers(0, n_yaw)) if row is None else row          # (a coarse row: every cell then matches)
    C = gr.q16(1000)
    ru, rv = lr.rotate(S[:, 0], S[:, 1], int(table[row][0]), int(table[row][1]), C)
    shift = (int(nu // 2), int(nv // 2)) if shift is None else shift
    T = np.stack([ru + shift[0], rv + shift[1]], axis=1)
    extra = rng.integers(0, [nu, nv], (int(clutter * n_s) + 1, 2))
    T = np.concatenate([T, extra])
    T = T[(T[:, 0] >= 0) & (T[:, 0] < nu) & (T[:, 1] >= 0) & (T[:, 1] < nv)]
    hs = [float(rng.integers(-8, 8)) / 16.0 if heights else None for _ in S]
    ht = [float(rng.integers(-8, 8)) / 16.0 + 2.5 if heights else None for _ in T]
    src, tgt = cell_rows(S, reps=reps, ground=hs), cell_rows(T, reps=reps, ground=ht)
    weak = cell_rows(rng.integers(0, [nu, nv], (3, 2)), reps=reps - 1) if reps > 1 else np.zeros((0, 12), F32)
    params = dict(cell_mm=1000, nu=nu, nv=nv, n_yaw=n_yaw, refine=refine, min_records=reps, dilate=0, min_ground=1, sep_yaw=0, sep_cells=1)
    return src, np.concatenate([tgt, weak]), params


def fields(info):
    return {k: info[k] for k in INFO_FIELDS}


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_defaults():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert name in capi.SYMBOLS and hasattr(L, name), name
    p = capi.locate_params()
    d = lr.DEFAULTS
    for k, v in d.items():
        got = getattr(p, k)
        assert (list(got) if hasattr(got, "__len__") else got) == (list(v) if isinstance(v, tuple) else v), k
    assert set(d) == {n for n, _ in capi.SmLocateParams._fields_}
    assert capi.LOCATE_STATUS == lr.STATUS and capi.LOCATE_KINDS == lr.KINDS
    p = capi.locate_params(origin=(1, 2, 3), source_origin=(4, 5, 6), structure_classes=(3, 40), n_yaw=12)
    assert list(p.origin) == [1, 2, 3] and list(p.source_origin) == [4, 5, 6] and p.structure_mask[0] == 8 and p.structure_mask[1] == 256 and p.n_yaw == 12
    with pytest.raises(KeyError):
        capi.locate_params(no_such_field=1)
    assert L.sm_api_version() == 4


def test_rotation_table():
    """the library's table: exact quarter turns, the symmetry of the circle, and the restatement's own within one unit"""
    from surfelmapping_amd import capi
    t = capi.locate_rotations(n_yaw=360, refine=8).astype(np.int64)
    assert t.shape == (2880, 2)
    one = 1 << 30
    assert [tuple(t[j]) for j in (0, 720, 1440, 2160)] == [(one, 0), (0, one), (-one, 0), (0, -one)]
    assert np.abs(t - lr.rotations(360, 8)).max() <= 1
    assert np.abs(t[:, 0] ** 2 + t[:, 1] ** 2 - one * one).max() <= 2 * one
    assert capi.locate_rotations(n_yaw=1, refine=1).tolist() == [[one, 0]]


def test_argument_rules_without_a_device():
    from surfelmapping_amd import capi
    L = capi.load()
    p, src = capi.locate_params(), capi.map_source([], include_model=False)
    out, info, table = np.zeros(16, F32), capi.SmLocateInfo(), np.zeros(2880 * 2, np.int32)
    assert L.sm_default_locate_params(None) == capi.SM_E_ARG
    assert L.sm_locate_rotations(None, table.ctypes.data) == capi.SM_E_ARG and L.sm_locate_rotations(C.byref(p), None) == capi.SM_E_ARG
    assert L.sm_locate_maps(None, C.byref(src), C.byref(src), C.byref(p), out.ctypes.data, C.byref(info)) == capi.SM_E_ARG
    assert L.sm_locate_stats(None, None) == capi.SM_E_ARG and b"sm_locate_stats" in L.sm_last_error()
    for bad in (dict(cell_mm=49), dict(cell_mm=4001), dict(up=6), dict(nu=0), dict(nv=4097), dict(max_up=16385), dict(min_up=-1), dict(normal_sign=0),
                dict(min_records=0), dict(dilate=3), dict(n_yaw=0), dict(n_yaw=1025), dict(refine=0), dict(refine=17), dict(sep_yaw=-1),
                dict(min_ground=-1), dict(min_overlap_256=257), dict(ambiguity_256=-1), dict(max_source_cells=0), dict(max_source_cells=(1 << 20) + 1),
                dict(max_nodes=3), dict(origin=(0.0, float("nan"), 0.0)), dict(source_origin=(float("inf"), 0.0, 0.0))):
        assert L.sm_locate_rotations(C.byref(capi.locate_params(**bad)), table.ctypes.data) == capi.SM_E_ARG, bad
        assert b"sm_locate_rotations: " in L.sm_last_error()
    for good in (dict(cell_mm=50), dict(cell_mm=4000), dict(nu=4096, nv=1), dict(sep_cells=-1), dict(n_yaw=1024, refine=1), dict(max_nodes=4)):
        assert L.sm_locate_rotations(C.byref(capi.locate_params(**good)), table.ctypes.data) == capi.SM_OK, good


def test_ref_header_example():
    """derived by hand in tests/locate_ref.py (and in the header): a tie in score that (k, dv, du) decides, a tie in the refinement that
    (|dj|, dj) decides, a runner-up as good as the winner, two height pairs"""
    r = lr.locate(lr.EXAMPLE_SOURCE, lr.EXAMPLE_TARGET, **lr.EXAMPLE_PARAMS)
    for k, v in lr.EXAMPLE_INFO.items():
        assert r["info"][k] == v, (k, r["info"][k], v)
    table = lr.rotations(4, 8)
    planes = [lr.score_plane(r["S"], r["occ"], table[8 * k], 4, 65536) for k in range(4)]
    assert r["R"] == 4 and [int(p.max()) for p in planes] == [2, 1, 2, 1]
    assert np.argwhere(planes[0] == 2).tolist() == [[1 + 4, 1 + 4], [1 + 4, 4 + 4]]           # (dv + R, du + R): the two tied candidates
    assert np.argwhere(planes[2] == 2).tolist() == [[2 + 4, 3 + 4], [2 + 4, 6 + 4]]
    assert [lr.score_at(r["S"], r["occ"], table[j], 1, 1, 65536) for j in (31, 0, 1)] == [2, 2, 2]       # the refinement's tie
    # source (x, z) -> target (x + 1, z + 1), half a metre up: up is -y
    want = np.eye(4)
    want[:3, 3] = (1.0, -0.5, 1.0)
    assert np.array_equal(r["pose"], want)
    # the runner-up keeps away: 3 cells leave (0, 1, 4) out but not half a turn's (6, 2); 5 cells and every row leave single cells
    assert lr.locate(lr.EXAMPLE_SOURCE, lr.EXAMPLE_TARGET, **dict(lr.EXAMPLE_PARAMS, sep_cells=3))["info"]["runner_up"] == 2     # (k = 2, half a turn)
    assert lr.locate(lr.EXAMPLE_SOURCE, lr.EXAMPLE_TARGET, **dict(lr.EXAMPLE_PARAMS, sep_cells=5, sep_yaw=2))["info"]["runner_up"] == 1


@pytest.mark.parametrize("seed", range(4))
def test_ref_fast_path_is_the_triple_loop(seed):
    """the per-row histogram of cell differences against the definition's loop over every offset, on random rasters"""
    rng = np.random.default_rng(seed)
    nu, nv = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    occ = rng.random((nv, nu)) < 0.4
    S = np.unique(rng.integers(-4, 5, (int(rng.integers(1, 12)), 2)), axis=0)
    C = gr.q16(int(rng.integers(50, 4001)))
    R = lr.search_range(S, C)
    table = lr.rotations(7, 3)
    for j in rng.integers(0, 21, 3):
        assert np.array_equal(lr.score_plane(S, occ, table[j], R, C), lr.score_plane_literal(S, occ, table[j], R, C)), (seed, j)


def test_ref_is_a_function_of_the_records_alone():
    src, tgt, params = cell_scene(3, 40, 30, 20, 12, 2)
    want = lr.locate(src, tgt, **params)
    rng = np.random.default_rng(0)
    ps, pt = rng.permutation(len(src)), rng.permutation(len(tgt))
    got = lr.locate_set(np.split(src[ps], [5, 5, 50]), np.split(tgt[pt], [1, 70]), **params)
    assert fields(got["info"]) == fields(want["info"]) and np.array_equal(got["pose"], want["pose"])
    assert want["info"]["status"] in ("OK", "AMBIGUOUS") and want["info"]["score"] == 40


def _four_cell_source():
    """the example's target; a source of four cells of which two can match at a time: score 2, n_s 4"""
    src = cell_rows([(0, 0), (1, 0), (0, 2), (1, 2)])
    r = lr.locate(src, lr.EXAMPLE_TARGET, **lr.EXAMPLE_PARAMS)
    assert (r["info"]["score"], r["info"]["n_s"], r["info"]["coarse_score"], r["info"]["runner_up"]) == (2, 4, 2, 2)
    return src


def test_ref_status_rules_at_their_thresholds():
    src = _four_cell_source()
    run = lambda **kw: lr.locate(src, lr.EXAMPLE_TARGET, **dict(lr.EXAMPLE_PARAMS, **kw))["info"]["status"]
    # NONE: score * 256 < n_s * min_overlap_256, 512 against 4 * 128
    assert [run(min_overlap_256=v, ambiguity_256=256) for v in (127, 128, 129)] == ["OK", "OK", "NONE"]
    # AMBIGUOUS: runner_up * 256 > coarse_score * ambiguity_256, 512 against 2 * 256
    assert [run(ambiguity_256=v) for v in (255, 256, 257)] == ["AMBIGUOUS", "OK", "OK"]
    # NONE comes first
    assert run(min_overlap_256=129, ambiguity_256=0) == "NONE"
    none = lr.locate(src, lr.EXAMPLE_TARGET, **dict(lr.EXAMPLE_PARAMS, min_overlap_256=129))
    assert np.array_equal(none["pose"], np.eye(4)) and none["info"]["score"] == 2
    # no target, no source: nothing is searched
    empty = np.zeros((0, 12), F32)
    a, b = lr.locate(src, empty, **lr.EXAMPLE_PARAMS), lr.locate(empty, lr.EXAMPLE_TARGET, **lr.EXAMPLE_PARAMS)
    assert (a["info"]["status"], b["info"]["status"]) == ("NO_TARGET", "NO_SOURCE")
    assert lr.locate(empty, empty, **lr.EXAMPLE_PARAMS)["info"]["status"] == "NO_TARGET"
    assert all(a["info"][k] == 0 and b["info"][k] == 0 for k in lr.RESULT_FIELDS) and np.array_equal(a["pose"], np.eye(4))
    assert b["info"]["target_cells"] == 4 and a["info"]["n_s"] == 4


def test_ref_no_runner_up_and_the_height_minimum():
    run = lambda **kw: lr.locate(lr.EXAMPLE_SOURCE, lr.EXAMPLE_TARGET, **dict(lr.EXAMPLE_PARAMS, **kw))["info"]
    i = run(sep_cells=-1)
    assert (i["runner_up"], i["status"]) == (0, "OK")
    # m = 2 pairs: min_ground 3 is m = min_ground - 1, min_ground 2 is m = min_ground
    assert [(run(min_ground=v)["height_pairs"], run(min_ground=v)["dh"]) for v in (3, 2)] == [(2, 0), (2, 32768)]


def test_ref_record_edge_values():
    """a NaN, a zero normal: LOOSE.  |cu| = 4095 is a source cell, 4096 is OUTSIDE.  |ni[a]| = max_up is structure-like, max_up + 1 is not"""
    h = math.sqrt(0.75)
    edge = [lr.wall(4095.5, 0.5), lr.wall(-4094.5, 0.5), lr.wall(4096.5, 0.5), lr.wall(-4095.5, 0.5), lr.wall(0.5, 4095.5), lr.wall(0.5, -4095.5),
            lr.wall(float("nan"), 0.5), lr.wall(2.5, 0.5, n=(0, 0, 0)),
            lr.wall(3.5, 0.5, n=(h, 0.5, 0)), lr.wall(4.5, 0.5, n=(h, -0.5, 0)), lr.wall(5.5, 0.5, n=(h, 0.5 + 2.0 ** -14, 0)),
            lr.wall(6.5, 0.5, n=(h, -0.5 - 2.0 ** -14, 0))]
    S, G, counts = lr.source_cells(np.stack(edge), dict(lr.DEFAULTS, **lr.EXAMPLE_PARAMS))
    assert S.tolist() == [[-4095, 0], [3, 0], [4, 0], [4095, 0], [0, 4095]] and len(G) == 0          # (cv, cu) order
    assert counts == [5, 0, 2, 3, 2]
    r = lr.locate(np.stack(edge), lr.EXAMPLE_TARGET, **lr.EXAMPLE_PARAMS)
    assert r["R"] == (3 * (4095 * 65536 + 32768) // 2) // 65536 + 2 == 6145
    # in the target: the window's last cell, the first one outside
    _, _, _, counts = lr.target_raster(np.stack([lr.wall(5.5, 3.5), lr.wall(6.0, 0.5), lr.wall(0.5, 4.0), lr.wall(-2.0 ** -17, 0.5)]), dict(lr.DEFAULTS, **lr.EXAMPLE_PARAMS))
    assert counts == [1, 0, 0, 3, 0]


@pytest.fixture(scope="module", params=TRUTHS, ids=lambda t: f"yaw{t[0]:.0f}")
def yard(request):
    yaw, t = request.param
    truth = ls.truth_of(yaw, t)
    src, tgt, params = ls.yard_pair(truth)
    return dict(src=src, tgt=tgt, params=params, truth=truth, want=lr.locate(src, tgt, **params))


def test_yard_is_located(yard):
    """with the defaults: OK, the winner within one coarse row and one cell of the truth (its offset to the nearest whole cell), the
    height within 5 cm"""
    i = yard["want"]["info"]
    k, du, dv, height = ls.expected(yard["truth"], yard["params"])
    print(i, (k, du, dv, height))
    assert i["status"] == "OK"
    assert lr.circular(i["coarse_k"] - round(k), 360) <= 1 and lr.circular(i["row"] - round(k * 8), 2880) <= 8
    assert abs(i["du"] - round(du)) <= 1 and abs(i["dv"] - round(dv)) <= 1
    assert abs(i["dh"] * 2.0 ** -16 - height) < 0.05
    assert i["runner_up"] * 256 <= i["coarse_score"] * 200          # (the yard's prototype: 77 of 115)


def test_court_is_ambiguous():
    """the closed rectangle: a half turn about its middle scores as well; the pose is at one of the two placements"""
    truth = ls.truth_of(*TRUTHS[0])
    src, tgt, params = ls.court_pair(truth)
    r = lr.locate(src, tgt, **params)
    i = r["info"]
    assert i["status"] == "AMBIGUOUS" and i["runner_up"] * 256 > i["coarse_score"] * 218
    centre = np.array([3.0, -2.0, 0.5])
    other = truth.copy()
    other[:3, :3] = ls.sc.rigid(rz_deg=180.0)[:3, :3] @ truth[:3, :3]
    other[:3, 3] = centre + ls.sc.rigid(rz_deg=180.0)[:3, :3] @ (truth[:3, 3] - centre)
    errs = [tr.pose_error(r["pose"], T) for T in (truth, other)]
    print(i, errs)
    # a cell and a coarse row: 0.5 m * sqrt(2), 1 degree and its lever of 60 m from the world's origin to the court
    assert min(e[0] for e in errs) < 0.75 + 60.0 * math.radians(1.0) and min(e[1] for e in errs) <= 1.01


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _ctx(rows=None, cap=80):
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, preprocess=0, stereo_border=0.0, max_sqrt_vertices=cap))
    if rows is not None and len(rows):
        m.upload_model(rows)
    return m


def _write(folder, name, rows):
    path = str(folder / name)
    cr.write_map(path, np.ascontiguousarray(rows, F32).reshape(-1, 12), 1, 2)
    return path


def _table(params):
    from surfelmapping_amd import capi
    return capi.locate_rotations(n_yaw=params.get("n_yaw", lr.DEFAULTS["n_yaw"]), refine=params.get("refine", lr.DEFAULTS["refine"]))


def _same(got, want, what):
    """every field of the info, and the pose as the float32 of the restatement's doubles, bit for bit"""
    gi, wi = got["info"], dict(want["info"])
    assert gi["status"] == wi["status"], (what, gi, wi)
    for k in INFO_FIELDS:
        assert gi[k] == wi[k], (what, k, gi[k], wi[k], gi, wi)
    assert np.array_equal(got["pose"].view(np.uint32), want["pose"].astype(F32).view(np.uint32)), (what, got["pose"], want["pose"])


def _check(m, tmp_path, src, tgt, params, what, tag="x"):
    want = lr.locate(src, tgt, _table(params), **params)
    got = m.locate_maps([_write(tmp_path, f"s{tag}.bin", src)], [_write(tmp_path, f"t{tag}.bin", tgt)], **params)
    _same(got, want, what)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("up", range(6))
def test_gpu_header_example_for_every_up(tmp_path, up):
    m = _ctx()
    src, tgt = gr.permute_axes(lr.EXAMPLE_SOURCE, up), gr.permute_axes(lr.EXAMPLE_TARGET, up)
    got, want = _check(m, tmp_path, src, tgt, dict(lr.EXAMPLE_PARAMS, up=up), f"up {up}")
    st = m.locate_stats()
    m.close()
    for k, v in lr.EXAMPLE_INFO.items():
        assert got["info"][k] == v, (k, got["info"][k], v)
    assert st["range"] == 4 and st["rounds"] >= 2 and st["source_records"] == 4 and st["target_records"] == 6 and st["exhaustive"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_s", (1, 63, 64, 65, 257))
def test_gpu_source_cell_counts(tmp_path, n_s):
    """the lanes of k_locate_bound stride over S in steps of 64: one cell, a wave less one, a wave, a wave and one, four and one"""
    src, tgt, params = cell_scene(100 + n_s, n_s, 40, 30, 12, 2)
    m = _ctx()
    got, want = _check(m, tmp_path, src, tgt, params, f"n_s {n_s}")
    m.close()
    assert got["info"]["n_s"] == n_s and got["info"]["score"] == n_s and got["info"]["height_pairs"] >= n_s


@pytest.mark.gpu
@pytest.mark.parametrize("nu,nv", ((86, 48), (1, 300), (300, 1)))
def test_gpu_window_shapes(tmp_path, nu, nv):
    """pyramid depths that differ per axis, sizes off every power of two"""
    src, tgt, params = cell_scene(7, 30, nu, nv, 12, 2, clutter=2.0)
    m = _ctx()
    got, want = _check(m, tmp_path, src, tgt, params, f"{nu} x {nv}")
    st = m.locate_stats()
    m.close()
    assert st["levels"] == max(3, int(math.ceil(math.log2(max(nu, nv) + 2 * st["range"]))))
    assert got["info"]["score"] >= 1


@pytest.mark.gpu
def test_gpu_overlap_across_the_windows_edges(tmp_path):
    """an L of three cells far from source_origin, beside two single cells: only the L's own placement scores 3, and it lies at the
    window's low corner (the winning offsets are negative) or at its high corner (they lie beyond nu and nv)"""
    m = _ctx()
    params = dict(lr.EXAMPLE_PARAMS, nu=6, nv=5, n_yaw=4, refine=1)
    src = cell_rows([(10, 7), (11, 7), (11, 8), (0, 0), (-6, 3)])
    got, want = _check(m, tmp_path, src, cell_rows([(0, 0), (1, 0), (1, 1)]), params, "low corner", "l")
    assert (got["info"]["coarse_k"], got["info"]["du"], got["info"]["dv"], got["info"]["score"], got["info"]["runner_up"]) == (0, -10, -7, 3, 2)
    src = cell_rows([(-10, -7), (-9, -7), (-9, -6), (0, 0), (6, -3)])
    got, want = _check(m, tmp_path, src, cell_rows([(4, 3), (5, 3), (5, 4)]), params, "high corner", "h")
    assert (got["info"]["coarse_k"], got["info"]["du"], got["info"]["dv"], got["info"]["score"], got["info"]["runner_up"]) == (0, 14, 10, 3, 2)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_yaw", (1, 7, 72))
@pytest.mark.parametrize("refine", (1, 8))
def test_gpu_rotation_tables(tmp_path, n_yaw, refine):
    n_fine = n_yaw * refine
    src, tgt, params = cell_scene(11, 50, 48, 40, n_yaw, refine, row=n_fine - 1, span=9)
    m = _ctx()
    got, want = _check(m, tmp_path, src, tgt, params, f"{n_yaw} x {refine}")
    m.close()
    assert 0 <= got["info"]["row"] < n_fine and got["info"]["coarse_k"] < n_yaw


@pytest.mark.gpu
def test_gpu_refinement_wraps_across_row_zero(tmp_path):
    """the target is the source turned by the last fine row: the coarse winner is k = 0 and the refinement steps back across 0"""
    src, tgt, params = cell_scene(5, 120, 64, 64, 24, 8, row=24 * 8 - 2, span=14, clutter=0.0)
    m = _ctx()
    got, want = _check(m, tmp_path, src, tgt, params, "wrap")
    m.close()
    assert want["info"]["coarse_k"] == 0 and want["info"]["row"] > 23 * 8 and want["info"]["score"] > want["info"]["coarse_score"]


@pytest.mark.gpu
def test_gpu_uniform_target_and_few_nodes(tmp_path, monkeypatch):
    """every cell of the window occupied: every score of a placement inside ties and the first in (k, dv, du) order wins -- with the
    default rounds, with rounds of 64 nodes and with every candidate scored"""
    src, _, params = cell_scene(9, 20, 24, 20, 12, 2, heights=False)
    tgt = cell_rows([(u, v) for v in range(20) for u in range(24)], reps=2)
    m = _ctx()
    got, want = _check(m, tmp_path, src, tgt, params, "uniform")
    rounds = m.locate_stats()["rounds"]
    assert got["info"]["score"] == 20 == got["info"]["runner_up"] and got["info"]["status"] == "AMBIGUOUS" and got["info"]["coarse_k"] == 0
    few = m.locate_maps([str(tmp_path / "sx.bin")], [str(tmp_path / "tx.bin")], **dict(params, max_nodes=64))
    st = m.locate_stats()
    _same(few, want, "max_nodes 64")
    assert st["rounds"] >= rounds                       # (the ties are cut so early that 16 parents a round are no limit here)
    monkeypatch.setenv("SM_LOCATE_EXHAUSTIVE", "1")
    every = m.locate_maps([str(tmp_path / "sx.bin")], [str(tmp_path / "tx.bin")], **params)
    st = m.locate_stats()
    m.close()
    _same(every, want, "exhaustive")
    assert st["exhaustive"] == 1 and st["levels"] == 0 and st["nodes"] == 0
    assert st["leaves"] == 2 * 12 * (24 + 2 * st["range"]) * (20 + 2 * st["range"])


@pytest.mark.gpu
@pytest.mark.parametrize("dilate", (0, 1, 2))
def test_gpu_dilation_few_nodes_and_exhaustive(tmp_path, monkeypatch, dilate):
    """a scene with clutter, 257 records in the source file (a workgroup and one record), for every dilation: the search, the search in
    rounds of 64 nodes and the exhaustive form give the restatement's result"""
    src, tgt, params = cell_scene(21 + dilate, 64, 50, 37, 36, 4, clutter=1.5, reps=3, span=8)
    src = np.concatenate([src, cell_rows([(20, 20)])])
    assert len(src) == 257
    params = dict(params, dilate=dilate, sep_yaw=2, sep_cells=3)
    m = _ctx()
    got, want = _check(m, tmp_path, src, tgt, params, f"dilate {dilate}")
    rounds = m.locate_stats()["rounds"]
    paths = ([str(tmp_path / "sx.bin")], [str(tmp_path / "tx.bin")])
    _same(m.locate_maps(*paths, **dict(params, max_nodes=64)), want, "max_nodes 64")
    assert m.locate_stats()["rounds"] >= rounds         # (36 roots fit a round of 64; the yard's 360 rows do not)
    monkeypatch.setenv("SM_LOCATE_EXHAUSTIVE", "1")
    _same(m.locate_maps(*paths, **params), want, "exhaustive")
    m.close()
    assert want["info"]["target_cells"] > 64 and want["info"]["n_s"] == 64 and want["info"]["source_counts"] == [64 * 3 + 1, 64, 0, 0, 0]


@pytest.mark.gpu
def test_gpu_edge_records_and_statuses(tmp_path):
    """the record edge values of test_ref_record_edge_values on the device (R = 6145: the widest range, roots of 4096 cells a side);
    NONE, NO_TARGET and NO_SOURCE return the identity and SM_OK; the stats of a call that was refused stay the last one's"""
    from surfelmapping_amd import capi
    h = math.sqrt(0.75)
    edge = np.stack([lr.wall(4095.5, 0.5), lr.wall(-4094.5, 0.5), lr.wall(4096.5, 0.5), lr.wall(-4095.5, 0.5), lr.wall(0.5, 4095.5), lr.wall(0.5, -4095.5),
                     lr.wall(float("nan"), 0.5), lr.wall(2.5, 0.5, n=(0, 0, 0)), lr.wall(3.5, 0.5, n=(h, 0.5, 0)), lr.wall(4.5, 0.5, n=(h, -0.5, 0)),
                     lr.wall(5.5, 0.5, n=(h, 0.5 + 2.0 ** -14, 0)), lr.wall(6.5, 0.5, n=(h, -0.5 - 2.0 ** -14, 0))])
    m = _ctx()
    with pytest.raises(capi.SurfelMapError) as e:
        m.locate_stats()
    assert e.value.rc == capi.SM_E_ARG and "no sm_locate_maps call yet" in str(e.value)
    got, want = _check(m, tmp_path, edge, lr.EXAMPLE_TARGET, lr.EXAMPLE_PARAMS, "edge", "e")
    assert got["info"]["source_counts"] == [5, 0, 2, 3, 2] and m.locate_stats()["range"] == 6145
    src = _four_cell_source()
    empty = np.zeros((0, 12), F32)
    for what, s, t, kw, status in (("none", src, lr.EXAMPLE_TARGET, dict(min_overlap_256=129), "NONE"), ("at the threshold", src, lr.EXAMPLE_TARGET, dict(min_overlap_256=128), "AMBIGUOUS"),
                                   ("ambiguity at the threshold", src, lr.EXAMPLE_TARGET, dict(ambiguity_256=256), "OK"),
                                   ("no target", src, empty, {}, "NO_TARGET"), ("no source", empty, lr.EXAMPLE_TARGET, {}, "NO_SOURCE"),
                                   ("no runner-up", lr.EXAMPLE_SOURCE, lr.EXAMPLE_TARGET, dict(sep_cells=-1), "OK"),
                                   ("too few pairs", lr.EXAMPLE_SOURCE, lr.EXAMPLE_TARGET, dict(min_ground=3), "AMBIGUOUS")):
        got, want = _check(m, tmp_path, s, t, dict(lr.EXAMPLE_PARAMS, **kw), what, "q")
        assert got["info"]["status"] == status, what
        if status in ("NONE", "NO_TARGET", "NO_SOURCE"):
            assert np.array_equal(got["pose"], np.eye(4, dtype=F32))
    last = m.locate_stats()
    s, t = str(tmp_path / "sq.bin"), str(tmp_path / "tq.bin")
    for what, call, rc in (("a path in both sets", lambda: m.locate_maps([s, t], [t]), capi.SM_E_ARG), ("a missing file", lambda: m.locate_maps([s + ".none"], [t]), capi.SM_E_ARG),
                           ("a parameter", lambda: m.locate_maps([s], [t], dilate=3), capi.SM_E_ARG),
                           ("the capacity", lambda: m.locate_maps([_write(tmp_path, "four.bin", src)], [t], **dict(lr.EXAMPLE_PARAMS, max_source_cells=3)), capi.SM_E_CAPACITY)):
        with pytest.raises(capi.SurfelMapError) as e:
            call()
        assert e.value.rc == rc, what
    assert m.locate_stats() == last
    m.close()


@pytest.mark.gpu
def test_gpu_exhaustive_is_refused_above_its_limit(tmp_path, monkeypatch):
    from surfelmapping_amd import capi
    m = _ctx()
    s, t = _write(tmp_path, "s.bin", cell_rows([(4095, 0), (0, 0)])), _write(tmp_path, "t.bin", lr.EXAMPLE_TARGET)
    monkeypatch.setenv("SM_LOCATE_EXHAUSTIVE", "1")
    with pytest.raises(capi.SurfelMapError) as e:                   # 360 rows * 12296 * 12294 offsets * 2 cells > 2^36
        m.locate_maps([s], [t], **dict(lr.EXAMPLE_PARAMS, n_yaw=360))
    m.close()
    assert e.value.rc == capi.SM_E_ARG and "2^36" in str(e.value)


@pytest.mark.gpu
def test_gpu_sharded_and_rig_contexts_are_refused(tmp_path):
    from surfelmapping_amd import capi
    s, t = _write(tmp_path, "s.bin", lr.EXAMPLE_SOURCE), _write(tmp_path, "t.bin", lr.EXAMPLE_TARGET)
    m = _ctx()
    m._chk(m._L.sm_shard_stream_configure(m._h, 0, 1), "sm_shard_stream_configure")
    with pytest.raises(capi.SurfelMapError) as e:
        m.locate_maps([s], [t], **lr.EXAMPLE_PARAMS)
    m.close()
    assert e.value.rc == capi.SM_E_UNSUPPORTED
    m = _ctx()
    m._chk(m._L.sm_rig_configure(m._h, 0, 1), "sm_rig_configure")
    with pytest.raises(capi.SurfelMapError) as e:
        m.locate_maps([s], [t], **lr.EXAMPLE_PARAMS)
    m.close()
    assert e.value.rc == capi.SM_E_UNSUPPORTED


@pytest.mark.gpu
def test_gpu_refused_between_conflict_and_cull(tmp_path):
    from surfelmapping_amd import capi, synth
    s, t = _write(tmp_path, "s.bin", lr.EXAMPLE_SOURCE), _write(tmp_path, "t.bin", lr.EXAMPLE_TARGET)
    cam = dict(width=W, height=H, fx=F, fy=F, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    rgb, depth, sem, pose = next(iter(synth.make_sequence(cam, synth.kitti_trajectory(1), seed=3)))
    m = _ctx()
    m.process_frame(rgb, depth, sem, pose)
    m.stage_conflict(pose, 1.0, 30.0)
    with pytest.raises(capi.SurfelMapError) as e:
        m.locate_maps([s], [t], **lr.EXAMPLE_PARAMS)
    assert e.value.rc == capi.SM_E_ARG and "between sm_stage_conflict and sm_stage_cull" in str(e.value)
    m.stage_cull()
    got = m.locate_maps([s], [t], **lr.EXAMPLE_PARAMS)
    m.close()
    assert got["info"]["status"] == "AMBIGUOUS" and got["info"]["score"] == 2


@pytest.fixture(scope="module")
def yard0():
    truth = ls.truth_of(*TRUTHS[0])
    src, tgt, params = ls.yard_pair(truth)
    return dict(src=src, tgt=tgt, params=params, truth=truth)


@pytest.mark.gpu
def test_gpu_yard_over_files_packed_file_and_model(yard0, tmp_path, monkeypatch):
    """the yard as one file a set; then both sets shuffled over three files, one of the source's packed, plus the live model for the
    target's remainder: no bit changes.  (A packed file holds positions on a grid of 2^-10 m: the one-file set holds that part as the
    packed file decodes it.)  The exhaustive form of the same call agrees as well.  Nothing is modified"""
    src, tgt, params = yard0["src"], yard0["tgt"], yard0["params"]
    rng = np.random.default_rng(3)
    ps, pt = rng.permutation(len(src)), rng.permutation(len(tgt))
    sparts, tparts = np.split(src[ps], [700, 957]), np.split(tgt[pt], [6000, 6001, 15000])
    m = _ctx()
    packed = m.pack_maps([_write(tmp_path, "s1.bin", sparts[1])], str(tmp_path / "p"))
    sparts[1] = ret.read_map(m.unpack_maps(packed, str(tmp_path / "u"))[0])[0]
    assert len(sparts[1]) == 257 and not np.array_equal(sparts[1], src[ps][700:957])
    src = np.concatenate(sparts)
    got, want = _check(m, tmp_path, src, tgt, params, "yard")
    st = m.locate_stats()
    print(got["info"], st)
    assert got["info"]["status"] == "OK" and st["chunks"] == 2 and st["nodes"] > 0 and st["leaves"] > 0
    _same(m.locate_maps([str(tmp_path / "sx.bin")], [str(tmp_path / "tx.bin")], **dict(params, max_nodes=64)), want, "max_nodes 64")
    few = m.locate_stats()
    print(few)
    assert few["rounds"] > st["rounds"]                 # the frontier waits: 16 parents a round, the same result
    sp = [_write(tmp_path, "s0.bin", sparts[0]), packed[0], _write(tmp_path, "s2.bin", sparts[2])]
    tp = [_write(tmp_path, f"t{i}.bin", q) for i, q in enumerate(tparts[:3])]
    before = {p: open(p, "rb").read() for p in sp + tp}
    m.upload_model(tparts[3])
    counts = m.counts()
    _same(m.locate_maps(sp, tp, target_model=True, **params), want, "three files, one packed, and the model")
    assert {p: open(p, "rb").read() for p in sp + tp} == before and m.counts() == counts
    monkeypatch.setenv("SM_LOCATE_EXHAUSTIVE", "1")
    _same(m.locate_maps(sp, tp, target_model=True, **params), want, "exhaustive")
    m.close()


@pytest.mark.gpu
def test_gpu_locate_then_register(yard0, tmp_path):
    """end to end: the located pose as the guess of register_maps, the pivot inside the overlap: OK and the truth recovered"""
    src, tgt, params, truth = yard0["src"], yard0["tgt"], yard0["params"], yard0["truth"]
    m = _ctx()
    sp, tp = [_write(tmp_path, "s.bin", src)], [_write(tmp_path, "t.bin", tgt)]
    found = m.locate_maps(sp, tp, **params)
    assert found["info"]["status"] == "OK"
    # the restatement of the registration from the located guess, on the CPU
    T, want = rr.register(src, tgt, guess=found["pose"].astype(F64), min_inliers=MIN_INLIERS, pivot=PIVOT)
    ref_dt, ref_dr = tr.pose_error(T, truth)
    pose, info = m.register_maps(sp, tp, guess=found["pose"], min_inliers=MIN_INLIERS, pivot=PIVOT)
    m.close()
    dt, dr = tr.pose_error(pose.astype(F64), truth)
    print(found["info"], tr.pose_error(found["pose"].astype(F64), truth), want["status"], (ref_dt, ref_dr), info["status"], (dt, dr))
    assert want["status"] == "OK" and info["status"] == "OK"
    # tests/test_register.py's bound for a guessed start.  The restatement reaches 0.0079 m and 0.0077 degrees from the located
    # guess (1.5 m and 1 degree off at the world's origin, 60 m from the yard): inside the bound, so the bound stays as it is
    assert ref_dt < 0.01 and ref_dr < 0.03
    assert dt < 0.01 and dr < 0.03
