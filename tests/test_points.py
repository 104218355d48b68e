"""Point queries (sm_query_points_maps, sm_default_points_params, sm_query_points_stats; SurfelMap.query_points / query_points_stats,
capi.body_points; DESIGN.md "4y. Point queries").  CPU: the symbols, the struct sizes against the compiled header, the defaults,
body_points against a float64 restatement, the restated rule on hand-made cases.  GPU: every plane bit for bit against the
brute-force restatement of tests/points_ref.py -- on the street of tests/retire_ref.py and on small sets made for a rule each."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import points_ref as pr
import rays_ref as rf
import retire_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CAM, OVER = rr.CAM, rr.OVER
NEW = ("sm_default_points_params", "sm_query_points_maps", "sm_query_points_stats")
PLANES = pr.PLANES
CUTS = [0, 9000, 9300, 27011]
INF, NAN = float("inf"), float("nan")


def _assert_equal(got, want, what="", planes=PLANES):
    for k in planes:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        same = g.view(np.uint32) == w.view(np.uint32) if g.dtype == f32 else g == w
        assert same.all(), (what, k, int((~same).sum()), np.argwhere(~same)[:4], g[~same][:4], w[~same][:4])


def _row(c, n, r, conf=1.0, colour=0x01406080):
    m = np.zeros(12, f32)
    m[0:3], m[3], m[8:11], m[11] = c, conf, n, r
    m[4] = np.array([colour], np.uint32).view(f32)[0]
    return m


def _pt(x, R):
    return np.array([x[0], x[1], x[2], R], f32)


def _write_map(path, rows, a=0, b=0):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([a, b], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, f32).tobytes())


def _street_points(model, n, seed):
    """half on the surface, jittered by centimetres, reaches 0.05 .. 1 m; a quarter inside and outside the box, reaches 0 .. 30 m;
    the rest: R = +inf, R = 0 (every other one exactly at a record's centre), or exactly at a centre with a small reach"""
    rng = np.random.default_rng(seed)
    lo, hi = model[:, 0:3].min(axis=0), model[:, 0:3].max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    pts = np.zeros((n, 4), f32)
    a, b = n // 2, n // 2 + n // 4
    pick = rng.integers(0, len(model), n)
    pts[:a, 0:3] = model[pick[:a], 0:3] + rng.normal(0.0, 0.02, (a, 3))
    pts[:a, 3] = rng.uniform(0.05, 1.0, a)
    pts[a:b, 0:3] = mid + rng.uniform(-1.5, 1.5, (b - a, 3)) * half
    pts[a:b, 3] = rng.uniform(0.0, 30.0, b - a)
    pts[a:b:8, 3] = 0.0
    rest = np.arange(b, n)
    pts[rest, 0:3] = mid + rng.uniform(-1.2, 1.2, (len(rest), 3)) * half
    at_centre = rest[1::2]
    pts[at_centre, 0:3] = model[pick[at_centre], 0:3]
    pts[rest[0::3], 3] = INF
    pts[rest[1::3], 3] = 0.0
    pts[rest[2::3], 3] = rng.uniform(0.0, 0.02, len(rest[2::3]))
    return pts


@pytest.fixture(scope="module")
def scene():
    """the street of tests/test_rays.py: the model of frames 0..9 on the CPU oracle, 2048 points and the restatement's answers,
    computed once"""
    import oracle_lib as ol
    seq = rr.sequence(11)
    cpu = ol.Oracle(ol.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=440))
    for fr in seq[:10]:
        cpu.process_frame(*fr)
    model = cpu.download_model()
    assert len(model) > 30000
    pts = _street_points(model, 2048, 11)
    return dict(seq=seq, model=model, pts=pts, want=pr.query(model, pts))


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_point_symbols_and_defaults():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.sm_api_version() == 4
    p = capi.points_params()
    assert (p.cell_mm, list(p.origin), p.min_conf, list(p.reserved)) == (250, [0.0, 0.0, 0.0], 0.0, [0, 0, 0])
    q = capi.points_params(cell_mm=100, origin=(1.0, 2.0, 3.5), min_conf=2.0)
    assert (q.cell_mm, list(q.origin), q.min_conf) == (100, [1.0, 2.0, 3.5], 2.0)
    with pytest.raises(KeyError):
        capi.points_params(cell=3)


def test_null_arguments_are_rejected_without_a_context():
    from surfelmapping_amd import capi
    L = capi.load()
    p, src, st = capi.points_params(), capi.map_source([]), capi.SmPointsStats()
    pts, d2 = np.zeros((4, 4), f32), np.zeros(4, f32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sm_default_points_params(None) == capi.SM_E_ARG
    assert L.sm_query_points_maps(None, C.byref(src), C.byref(p), vp(pts), 4, vp(d2), None, None, None, None, None, None) == capi.SM_E_ARG
    assert L.sm_query_points_stats(None, C.byref(st)) == capi.SM_E_ARG


def test_point_size_and_limit_against_the_compiled_header(tmp_path):
    from surfelmapping_amd import capi
    src = tmp_path / "points.c"
    src.write_text('#include <stdio.h>\n#include "sm_c_api.h"\nint main(void) { printf("%zu %lld %zu %zu\\n", sizeof(sm_point), '
                   "(long long)SM_POINTS_MAX, sizeof(sm_points_params), sizeof(sm_points_stats_t)); return 0; }\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "points"), str(src)])
    size, limit, params, stats = (int(v) for v in subprocess.check_output([str(tmp_path / "points")]).split())
    assert size == 16 == C.sizeof(capi.SmPoint) and limit == 1 << 24 == capi.POINTS_MAX
    assert params == C.sizeof(capi.SmPointsParams) and stats == C.sizeof(capi.SmPointsStats)


def _body_points64(pose44, spheres):
    """R * c + t in double, ((R0 cx + R1 cy) + R2 cz) + t, a term with a zero coefficient left out, rounded once"""
    M = np.asarray(pose44, f32).astype(np.float64)
    out = np.zeros((len(spheres), 4), f32)
    for i, s in enumerate(np.asarray(spheres, f32)):
        for r in range(3):
            term = [M[r, c] * float(s[c]) if M[r, c] != 0.0 else -0.0 for c in range(3)]
            out[i, r] = f32(((term[0] + term[1]) + term[2]) + M[r, 3])
        out[i, 3] = s[3]
    return out


def test_body_points_against_a_float64_restatement():
    from surfelmapping_amd import capi
    rng = np.random.default_rng(2)
    spheres = np.concatenate([rng.uniform(-2.0, 2.0, (5, 3)), rng.uniform(0.1, 0.9, (5, 1))], axis=1).astype(f32)
    poses = []
    for j in range(4):
        a = 0.3 * j + 0.1
        poses.append(np.array([[np.cos(a), 0, np.sin(a), 10.0 * j], [0, 1, 0, 2.5 * j], [-np.sin(a), 0, np.cos(a), -1e3 * j], [0, 0, 0, 1]]).astype(f32))
    for M in poses:
        want = _body_points64(M, spheres)
        for given in (M, M.T.reshape(16)):                                                # a 4x4 matrix, or 16 floats column-major
            got = capi.body_points(given, spheres)
            assert got.shape == (5, 4) and got.dtype == f32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got = capi.body_points(np.stack([M.T.reshape(16) for M in poses]), spheres)
    want = np.concatenate([_body_points64(M, spheres) for M in poses])
    assert got.shape == (20, 4) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(capi.body_points(np.stack(poses), spheres).view(np.uint32), want.view(np.uint32))
    # an identity rotation adds the translation to the centres, rounded once: no term of a zero coefficient takes part
    M = np.eye(4, dtype=f32)
    M[0:3, 3] = (1.5, -2.25, 1e3)
    odd = np.array([[-0.0, 1e-30, 3.0, 0.5], [7.0, -0.0, 0.0, 0.0]], f32)
    got = capi.body_points(M, odd)
    assert np.array_equal(got[:, 0:3], (odd[:, 0:3].astype(np.float64) + M[0:3, 3].astype(np.float64)).astype(f32)) and (got[:, 3] == odd[:, 3]).all()
    with pytest.raises(ValueError):
        capi.body_points(M, np.zeros((3, 3), f32))


def test_restatement_on_hand_made_points():
    """the reference itself: one disc of radius 0.5 at the origin with normal +z; these dd are exact in float32"""
    model = _row((0, 0, 0), (0, 0, 1), 0.5)[None]
    pts = np.stack([_pt((0, 0, 2), INF), _pt((1.5, 0, 0), INF), _pt((0.25, -0.125, 0), INF), _pt((1.5, 0, 2), INF),
                    _pt((0, 0, 2), 2.0), _pt((0, 0, 2), 1.9999999), _pt((0, 0, 2), -1.0), _pt((NAN, 0, 2), 5.0)])
    out = pr.query(model, pts)
    assert out["d2"].tolist() == [4.0, 1.0, 0.0, 5.0, 4.0, INF, INF, INF] and out["id"].tolist() == [0, 0, 0, 0, 0, -1, -1, -1]
    assert out["sem"].tolist() == [2] * 5 + [0] * 3 and out["rgb"][0].tolist() == [0x40, 0x60, 0x80] and out["radius"].tolist() == [0.5] * 5 + [0.0] * 3
    assert pr.valid(pts).tolist() == [True] * 6 + [False, False]
    # a normal that is not normalised, a negative radius, the gate, a zero normal, an infinite radius: the whole plane
    for row, want in ((_row((0, 0, 0), (0, 0, -4), 0.5), 5.0), (_row((0, 0, 0), (0, 0, 1), -0.5), 5.0), (_row((0, 0, 0), (0, 0, 1), 0.5, conf=-1.0), INF),
                      (_row((0, 0, 0), (0, 0, 0), 0.5), INF), (_row((0, 0, 0), (0, 0, 2), INF), 4.0), (_row((0, 0, 0), (0, NAN, 2), 0.5), INF),
                      (_row((0, 0, 0), (0, 0, 1), NAN), INF)):
        assert pr.query(row[None], pts[3:4])["d2"][0] == f32(want), row
    # two records: the nearer wins, equal ones go to the lower id
    two = np.stack([_row((0, 0, 5), (0, 0, 1), 0.5), _row((0, 0, 0), (0, 0, 1), 0.5), _row((0, 0, 0), (0, 0, 1), 0.5)])
    assert pr.query(two, pts[:1])["id"].tolist() == [1] and pr.query(two, np.stack([_pt((0, 0, 2.5), INF)]))["id"].tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _gpu(**over):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=440, **over))


@pytest.fixture(scope="module")
def held(scene):
    """a context whose model is the street's, row = slot"""
    m = _gpu()
    m.upload_model(scene["model"])
    return m


@pytest.fixture(scope="module")
def bench():
    """a context for the small sets: every test uploads its own"""
    return _gpu()


def _query(m, model, pts, **kw):
    m.upload_model(np.ascontiguousarray(model, f32))
    return m.query_points(pts, **kw)


@pytest.fixture(scope="module")
def map_set(scene, tmp_path_factory):
    """the street's model as three files of unequal length and a live remainder, and as one file"""
    d = tmp_path_factory.mktemp("points_maps")
    cuts = CUTS + [len(scene["model"])]
    paths = []
    for i in range(3):
        paths.append(str(d / f"part_{i}.bin"))
        _write_map(paths[-1], scene["model"][cuts[i]:cuts[i + 1]])
    whole = str(d / "whole.bin")
    _write_map(whole, scene["model"])
    live = _gpu()
    live.upload_model(scene["model"][cuts[3]:])
    return dict(paths=paths, whole=whole, live=live, dir=d)


@pytest.mark.gpu
def test_street_points_equal_the_restatement(scene, held):
    before = held.counts()
    got = held.query_points(scene["pts"])
    st = held.query_points_stats()
    want = scene["want"]
    n = int((want["id"] >= 0).sum())
    print(f"{n} of 2048 points have a disc within reach; stats {st}")
    assert 1000 < n < 2048
    _assert_equal(got, want)
    assert np.array_equal(got["dist"].view(np.uint32), np.sqrt(want["d2"]).view(np.uint32))
    assert st["points"] == 2048 and st["bad_points"] == 0 and st["records"] == len(scene["model"]) and st["chunks"] == 1 and st["files_skipped"] == 0
    assert st["tests"] >= n and st["probes"] > 0 and 0 < st["cells"] <= st["pairs"] <= 8 * len(scene["model"]) and st["no_slot"] == 0
    assert held.counts() == before                                            # the model, the counters and the tick are untouched
    assert np.array_equal(held.download_model().view(np.uint32), scene["model"].view(np.uint32))
    # only d2 asked for; then planes by name
    from surfelmapping_amd import capi
    d2 = np.zeros(2048, f32)
    p, src = capi.points_params(), capi.map_source([])
    assert held._L.sm_query_points_maps(held._h, C.byref(src), C.byref(p), scene["pts"].ctypes.data_as(C.c_void_p), 2048, d2.ctypes.data_as(C.c_void_p),
                                        None, None, None, None, None, None) == 0
    assert np.array_equal(d2.view(np.uint32), want["d2"].view(np.uint32))
    some = held.query_points(scene["pts"], planes=("radius", "sem"))
    assert sorted(some) == ["d2", "dist", "id", "radius", "sem"]
    _assert_equal(some, want, "two planes", ("d2", "id", "radius", "sem"))
    with pytest.raises(KeyError):
        held.query_points(scene["pts"], planes=("colour",))


@pytest.mark.gpu
def test_answer_does_not_depend_on_split_cells_origin_or_index(scene, held, map_set, tmp_path, monkeypatch):
    monkeypatch.delenv("SM_POINTS_NO_INDEX", raising=False)
    pts, want = scene["pts"], scene["want"]
    live = map_set["live"]
    _assert_equal(live.query_points(pts, map_set["paths"]), want, "three files and the live remainder")
    st = live.query_points_stats()
    assert st["chunks"] == 4 and st["records"] == len(scene["model"])
    files_only = live.query_points(pts, map_set["paths"], include_model=False)
    assert (want["id"] >= CUTS[3]).any() and (files_only["id"] < CUTS[3]).all()
    _assert_equal(live.query_points(pts, [map_set["whole"]], include_model=False), want, "one file")
    assert live.query_points_stats()["chunks"] == 1
    _assert_equal(held.query_points(pts), want, "the model alone")
    tests = {}
    for cell_mm in (50, 250, 1000, 20000):
        for origin in ((0.0, 0.0, 0.0), (0.1234, -7.001, 3.3)):
            _assert_equal(held.query_points(pts, cell_mm=cell_mm, origin=origin), want, f"cell_mm {cell_mm} origin {origin}")
            tests[cell_mm] = held.query_points_stats()["tests"]
    print("exact tests by cell_mm:", tests)
    # every record on the wide path, in a fresh process
    sub = pts[::4]
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, model=scene["model"], points=sub, cell_mm=250)
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), SM_POINTS_NO_INDEX="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "points_child.py"), src, dst], capture_output=True, text=True, env=e, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    child = dict(np.load(dst))
    _assert_equal(child, {k: v[::4] for k, v in want.items()}, "SM_POINTS_NO_INDEX=1")
    takes = int(pr.takes_part(scene["model"]).sum())
    assert takes == int((scene["model"][:, 3] >= 0).sum())                     # (the street has no record the normal's rule leaves out)
    assert int(child["stat_wide"]) == takes and int(child["stat_tests"]) == takes * int(pr.valid(sub).sum()) and int(child["stat_probes"]) == 0


def _aimed(rng, model, idx):
    """points at the distance g from the rim of the discs idx, in their planes, and at the height g over them, with reaches just
    inside and just outside g"""
    pts = []
    for j in idx:
        c, nn, r = model[j, 0:3].astype(np.float64), model[j, 8:11].astype(np.float64), abs(float(model[j, 11]))
        nn = nn / np.linalg.norm(nn)
        e = np.cross(nn, rng.normal(size=3))
        e /= np.linalg.norm(e)
        g = rng.uniform(0.01, 0.3)
        for x in (c + e * (r + g), c + e * (0.5 * r) + nn * g, c + e * (0.5 * r) - nn * g):
            for k in (1 - 1e-3, 1 - 1e-6, 1.0, 1 + 1e-6, 1 + 1e-3):
                pts.append(_pt(x, g * k))
    return np.stack(pts)


@pytest.mark.gpu
def test_wide_and_boundary_registration(bench):
    rng = np.random.default_rng(21)
    n = 600
    model = np.zeros((n, 12), f32)
    model[:, 0:3] = rng.uniform(-4.0, 4.0, (n, 3))
    model[:, 3] = 1.0
    model[:, 4] = rng.integers(0, 1 << 29, n).astype(np.uint32).view(f32)
    model[:, 8:11] = rng.normal(size=(n, 3))
    model[:, 11] = rng.uniform(0.005, 0.04, n)
    big = np.arange(0, n, 50)
    model[big, 11] = 2.0                                                      # 40 cells of 100 mm across: wide
    # cubes over exactly 2 x 2 x 2 = 8 cells (regular) and 3 x 1 x 3 = 9 (wide), by the restated rule
    model[7] = _row((0.1, 0.1, 0.1), (0.2, 0.1, 1), 0.04)
    model[8] = _row((0.15, 0.05, 0.15), (0.1, 1, 0.3), 0.06)
    V = pr.cell_edge(100)
    k7, c0, c1 = pr.classify(model[7], V, (0, 0, 0))
    assert k7 == pr.REG and len(pr.registered(c0, c1)) == 8 and pr.classify(model[8], V, (0, 0, 0))[0] == pr.WIDE
    pts = np.concatenate([_aimed(rng, model, list(big) + [7, 8] + list(range(100, 160))), _street_points(model, 512, 5)])
    got = _query(bench, model, pts, cell_mm=100)
    st = bench.query_points_stats()
    want = pr.query(model, pts)
    print("found:", int((want["id"] >= 0).sum()), "of", len(pts), "stats:", st)
    assert np.isin([7, 8, big[0], big[3]], want["id"]).all() and (want["id"] == -1).sum() > 100
    _assert_equal(got, want)
    assert st["wide"] == pr.wide_count(model, 100) == len(big) + 1
    _assert_equal(bench.query_points(pts, cell_mm=5000), want, "5 m cells")
    assert bench.query_points_stats()["wide"] == pr.wide_count(model, 5000) == 0


@pytest.mark.gpu
def test_hostile_records_and_dead_slots(scene, bench):
    c = scene["model"][1000, 0:3]
    bad = np.stack([
        _row((NAN, c[1], c[2]), (0, 0, 1), 0.3), _row((c[0], INF, c[2]), (0, 0, 1), 0.3), _row((c[0], c[1], -INF), (0, 0, 1), 0.3),
        _row((1e10, c[1], c[2]), (0, 0, 1), 0.3), _row((c[0], -1e10, 1e10), (0, 1, 0), 1e10), _row(c, (0, 0, 0), 0.3),
        _row(c, (0, 0, 1), -0.3), _row(c + 0.5, (0, 1, 1), INF), _row(c - 0.5, (1, 0, 1), -INF), _row(c, (0, 0, 1), NAN),
        _row(c, (NAN, 0, 1), 0.3), _row(c, (0, INF, 1), 0.3), _row(c + 0.1, (0, 0, 1), 0.3, conf=NAN), _row(c + 0.2, (0, 0, 1), 0.3, conf=0.25),
        _row(c + 0.3, (0, 0, 1), 0.3, conf=INF), _row((3e38, 3e38, 3e38), (1, 1, 1), 3e38), _row(c, (1e38, 1e38, 1e38), 0.3),
        _row((0, 0, 0), (0, 0, 0), 0.0), _row(c, (0.1, 0, 1), 1e30), _row(c + 0.05, (1e-20, 0, 1e-21), 0.2), _row(c - 0.05, (1e-23, 0, 0), 0.2)])
    rng = np.random.default_rng(9)
    model = scene["model"][:12000]
    at = np.sort(rng.choice(len(model), len(bad), replace=False))
    model = np.insert(model, at, bad, axis=0)
    hostile = [int(x) for x in at + np.arange(len(bad))]
    close = [j for j in hostile if np.isfinite(model[j, 0:3]).all() and abs(model[j, 0]) < 1e9]
    around = np.concatenate([np.concatenate([model[close, 0:3] + rng.normal(0, 0.2, (len(close), 3)), rng.uniform(0.1, 1.0, (len(close), 1))], axis=1)
                             for _ in range(6)]).astype(f32)
    pts = np.concatenate([scene["pts"][:768], around, np.stack([_pt(c, INF), _pt(c + 40.0, INF), _pt((1e10, c[1], c[2]), 1.0), _pt((0, 0, 0), 1e30)])])
    for min_conf in (0.0, 0.5):
        got = _query(bench, model, pts, min_conf=min_conf)
        want = pr.query(model, pts, min_conf=min_conf)
        _assert_equal(got, want, f"min_conf {min_conf}")
    seen = set(np.unique(want["id"])) - {-1}
    out = set(int(j) for j in np.flatnonzero(~pr.takes_part(model, 0.5)))
    assert len(seen - set(hostile)) > 50 and len(seen & set(hostile)) >= 3 and not (seen & out)
    assert (bench.query_points(pts, min_conf=NAN)["id"] == -1).all()
    # the hostile records among themselves: an infinite radius is the whole plane and takes part
    got = _query(bench, bad, around)
    want = pr.query(bad, around)
    _assert_equal(got, want, "the hostile records alone")
    assert {7, 8} <= set(np.unique(want["id"])) and not set(np.unique(want["id"])) & {0, 1, 2, 5, 9, 10, 11, 12, 15, 16, 17}
    # dead slots: frames with the compaction deferred leave dead slots among the occupied ones; the query sees the compacted model
    m = _gpu(compact_period=1000)
    for fr in scene["seq"][:11]:
        m.process_frame(*fr)
    assert int(m.read_frame_log()["n_kill"].sum()) > 0
    got = m.query_points(scene["pts"][:1024])
    after = m.download_model()
    m.close()
    _assert_equal(got, pr.query(after, scene["pts"][:1024]), "dead slots")


@pytest.mark.gpu
def test_hostile_points(scene, held):
    c = scene["model"][2000, 0:3].astype(np.float64)
    bad = np.stack([_pt((NAN, c[1], c[2]), 1.0), _pt((c[0], NAN, c[2]), INF), _pt((c[0], c[1], NAN), 1.0), _pt((INF, c[1], c[2]), 1.0),
                    _pt((c[0], -INF, c[2]), INF), _pt(c, -1.0), _pt(c, -1e-30), _pt(c, NAN), _pt(c, -INF), _pt((NAN, NAN, NAN), NAN)])
    huge = np.stack([_pt(c + 0.01, 1e20), _pt(c + 100.0, 3e38), _pt((1e4, -1e4, 1e4), 1.9e19), _pt((3e38, 0, 0), INF), _pt((-1e30, 1e30, 0), 3e38)])
    same = huge.copy()
    same[:, 3] = INF                                                          # a reach whose square overflows behaves as +inf
    good = scene["pts"][:500].copy()
    good[::7, 3] = -0.0                                                       # R = -0 is valid: R >= 0
    pts = np.concatenate([bad, huge, same, good])
    order = np.random.default_rng(1).permutation(len(pts))
    pts = pts[order]
    assert int((~pr.valid(pts)).sum()) == len(bad)
    got = held.query_points(pts)
    st = held.query_points_stats()
    want = pr.query(scene["model"], pts)
    _assert_equal(got, want)
    is_bad = ~pr.valid(pts)
    assert st["bad_points"] == len(bad) and (got["id"][is_bad] == -1).all() and np.isinf(got["d2"][is_bad]).all() and (got["sem"][is_bad] == 0).all()
    back = np.argsort(order)
    h, s = back[len(bad):len(bad) + len(huge)], back[len(bad) + len(huge):len(bad) + 2 * len(huge)]
    assert np.array_equal(got["id"][h], got["id"][s]) and np.array_equal(got["d2"][h].view(np.uint32), got["d2"][s].view(np.uint32))
    assert (got["id"][h][:3] >= 0).all()


@pytest.mark.gpu
def test_ties_go_to_the_lower_id(bench, tmp_path):
    model = np.stack([_row((5, 5, 5), (1, 0, 0), 0.1),                                   # padding: ids 1 and 2 are the twins
                      _row((0, 0, 2), (0, 0, 1), 0.5, colour=0x02010203), _row((0, 0, 2), (0, 0, 1), 0.5, colour=0x03040506),
                      _row((0, 0, -2), (0, 0, 3), 0.5), _row((-3, 0, 0), (0, 1, 0), 0.25), _row((-3, 0, 1), (0, 1, 0), 0.75)])
    pts = np.stack([_pt((0, 0, 1), 5.0),                           # the twins: the lower id wins
                    _pt((0, 0, 0), INF),                           # equidistant from two different discs (ids 1 and 3): dd = 4 both, the lower id
                    _pt((0.25, 0, -0.125), INF),                   # nearer to id 3
                    _pt((-3, 0, 0.25), INF),                       # on id 4's rim, inside id 5: dd = 0 both
                    _pt((-3, 0, 0.0), 0.0), _pt((0, 0, 1), 0.999)])
    got = _query(bench, model, pts)
    want = pr.query(model, pts)
    _assert_equal(got, want)
    assert got["id"].tolist() == [1, 1, 3, 4, 4, -1] and got["d2"].tolist() == [1.0, 4.0, 3.515625, 0.0, 0.0, INF]
    assert got["rgb"][0].tolist() == [1, 2, 3] and got["sem"][0] == 3 and got["normal"][2].tolist() == [0, 0, 3] and got["centre"][2].tolist() == [0, 0, -2]
    # across a file boundary: the file's copy has the lower id
    path = str(tmp_path / "twin.bin")
    _write_map(path, model[2:3])
    bench.upload_model(np.ascontiguousarray(model[1:3]))
    got = bench.query_points(pts[:1], [path])
    assert got["id"].tolist() == [0] and got["rgb"][0].tolist() == [4, 5, 6]
    got = bench.query_points(pts[:1], [path], cell_mm=20000)
    assert got["id"].tolist() == [0]


def _small_set(seed=17, n=600):
    rng = np.random.default_rng(seed)
    model = np.zeros((n, 12), f32)
    model[:, 0:3] = rng.uniform(-4.0, 4.0, (n, 3))
    model[:, 3] = 1.0
    model[:, 4] = rng.integers(0, 1 << 29, n).astype(np.uint32).view(f32)
    model[:, 8:11] = rng.normal(size=(n, 3))
    model[:, 11] = rng.uniform(0.005, 0.04, n)
    return rng, model


@pytest.mark.gpu
def test_walk_that_is_given_up_still_finds_the_nearest(bench):
    rng, model = _small_set()
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    far = np.concatenate([d * 1000.0, np.full((200, 1), 2000.0)], axis=1).astype(f32)   # 1 km away, reach 2 km
    V = pr.cell_edge(250)
    box, _ = pr.box_of(model, V, (0.0, 0.0, 0.0))
    assert all(pr.visited(p, V, (0.0, 0.0, 0.0), box, len(model)) is None for p in far[:5])
    got = _query(bench, model, far, cell_mm=250)
    st = bench.query_points_stats()
    want = pr.query(model, far)
    assert (want["id"] >= 0).all()
    _assert_equal(got, want, "1 km away")
    assert st["gave_up"] == 200 and st["wide"] == 0 and st["tests"] == 200 * len(model) and st["probes"] == 0, st
    inside = np.concatenate([rng.uniform(-5.0, 5.0, (200, 3)), np.full((200, 1), INF)], axis=1).astype(f32)
    got = bench.query_points(inside, cell_mm=50)
    st = bench.query_points_stats()
    _assert_equal(got, pr.query(model, inside), "R = +inf at 50 mm cells")
    assert st["gave_up"] == 200 and st["tests"] <= 200 * len(model), st


@pytest.mark.gpu
def test_points_out_of_reach_cost_no_test(bench):
    rng = np.random.default_rng(4)
    n = 2000
    model = np.zeros((n, 12), f32)
    model[:, 0:3] = rng.uniform((10.5, -5, -5), (30, 5, 5), (n, 3))
    model[:, 3], model[:, 11] = 1.0, rng.uniform(0.01, 0.1, n)
    model[:, 8:11] = rng.normal(size=(n, 3))
    pts = np.zeros((600, 4), f32)
    pts[:, 0:3] = rng.uniform((-30, -5, -5), (-0.5, 5, 5), (600, 3))
    pts[:, 3] = rng.uniform(0.0, 10.0, 600)                                    # the nearest disc is 0.9 m past every reach: more than a cell
    got = _query(bench, model, pts, cell_mm=250)
    st = bench.query_points_stats()
    assert (got["id"] == -1).all() and np.isinf(got["d2"]).all() and st["tests"] == 0 and st["probes"] == 0 and st["wide"] == 0, st
    # the same points with longer reaches do find them
    pts[:, 3] += 12.0
    got = bench.query_points(pts, cell_mm=250)
    want = pr.query(model, pts)
    assert (want["id"] >= 0).sum() > 100
    _assert_equal(got, want)


@pytest.mark.gpu
def test_argument_rules(scene, map_set):
    from surfelmapping_amd import capi
    L = capi.load()
    E = capi.SM_E_ARG
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    m = _gpu()
    st = capi.SmPointsStats()
    assert L.sm_query_points_stats(m._h, C.byref(st)) == E and b"no sm_query_points_maps call yet" in L.sm_last_error()
    m.process_frame(*scene["seq"][0])
    pts = np.ascontiguousarray(scene["pts"][:64])
    outs = dict(d2=np.full(64, 7.0, f32), id=np.full(64, 7, np.int32), centre=np.full((64, 3), 7.0, f32), normal=np.full((64, 3), 7.0, f32),
                radius=np.full(64, 7.0, f32), rgb=np.full((64, 3), 7, np.uint8), sem=np.full(64, 7, np.uint8))
    ptrs = [vp(outs[k]) for k in PLANES]
    p, src = capi.points_params(), capi.map_source(map_set["paths"])
    call = lambda p_=p, src_=src, pts_=pts, n=64, ptrs_=ptrs: L.sm_query_points_maps(m._h, None if src_ is None else C.byref(src_),
                                                                                       None if p_ is None else C.byref(p_), vp(pts_), n, *ptrs_)
    unwritten = lambda: all((outs[k] == 7).all() for k in PLANES)
    assert call(src_=None) == E and call(p_=None) == E and call(pts_=None) == E and call(ptrs_=[None] + ptrs[1:]) == E
    assert call(p_=capi.points_params(cell_mm=0)) == E and call(p_=capi.points_params(cell_mm=-5)) == E
    assert call(p_=capi.points_params(cell_mm=(1 << 24) + 1)) == E
    assert call(p_=capi.points_params(origin=(0.0, NAN, 0.0))) == E and call(p_=capi.points_params(origin=(INF, 0.0, 0.0))) == E
    assert call(n=capi.POINTS_MAX + 1) == E and b"2^24" in L.sm_last_error()
    null_paths = capi.SmMapSource(None, 2, 1)
    assert call(src_=null_paths) == E
    m.stage_conflict(scene["seq"][1][3], 1.0, 30.0)
    assert call() == E and b"between sm_stage_conflict and sm_stage_cull" in L.sm_last_error()
    m.stage_cull()
    short = str(map_set["dir"] / "short.bin")
    with open(short, "wb") as f:
        f.write(open(map_set["paths"][1], "rb").read()[:-20])
    for bad in ([map_set["paths"][0], short, map_set["paths"][2]], [map_set["paths"][0], str(map_set["dir"] / "missing.bin")]):
        assert call(src_=capi.map_source(bad)) == E and os.path.basename(bad[1]).encode() in L.sm_last_error()
    assert unwritten()
    assert L.sm_query_points_stats(m._h, C.byref(st)) == E                    # no call has succeeded yet
    assert call(n=0, pts_=None, ptrs_=[None] * 7) == 0 and unwritten()         # n_pts == 0 checks the set only
    assert L.sm_query_points_stats(m._h, C.byref(st)) == 0 and st.points == 0 and st.records == CUTS[3] + m.counts()["count"]
    assert call(n=0, src_=capi.map_source([short])) == E
    assert call() == 0 and not unwritten()
    m.close()
    for configure in ("shard_stream_configure", "rig_configure"):
        part = _gpu()
        getattr(part, configure)(0, 1)
        with pytest.raises(capi.SurfelMapError) as e:
            part.query_points(pts)
        assert e.value.rc == capi.SM_E_UNSUPPORTED
        part.close()
