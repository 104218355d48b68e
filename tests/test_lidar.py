"""Lidar sweeps (sm_lidar_sweep, sm_lidar_sweep_maps, sm_lidar_directions, sm_lidar_stats; SurfelMap.lidar_sweep / lidar_sweep_maps;
DESIGN.md "4k. Lidar sweeps").  CPU: the symbols, the struct layouts, the argument rules, the direction table against numpy's.  GPU:
every plane bit for bit against the brute-force restatement of tests/lidar_ref.py on the street of tests/retire_ref.py, the seam, a
partial sweep, wide footprints on both work paths, hostile records, dead slots, the confidence gate, map sets against the
concatenation, and the facade's velodyne files."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lidar_ref as lr
import retire_ref as rr
import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
DEMO = os.path.join(ROOT, "tests", "cpp", "lidar_demo.cpp")
f32 = np.float32
CAM, OVER = rr.CAM, rr.OVER
NEW = ("sm_default_lidar_sensor", "sm_lidar_directions", "sm_lidar_sweep", "sm_lidar_sweep_maps", "sm_lidar_stats")
PLANES = ("range", "id", "rgb", "sem")
# the sweep of the street: 180 x 8 at 2 degrees over the odd azimuths -179 .. 179 (the seam lies behind the sensor), el = -14 .. 0
STREET = dict(n_az=180, az0=-179.0, step=2.0, el=np.arange(-14, 1, 2, dtype=f32), min_range=1.0, max_range=60.0, min_conf=0.0)


def _ref_sensor(d):
    return lr.sensor(n_az=d["n_az"], n_el=len(d["el"]), az0=d["az0"], step=d["step"], el=d["el"], min_range=d["min_range"],
                     max_range=d["max_range"], min_conf=d["min_conf"])


def _c_sensor(d):
    from surfelmapping_amd import capi
    return capi.lidar_sensor(n_az=d["n_az"], az0_deg=d["az0"], az_step_deg=d["step"], el_deg=d["el"], min_range=d["min_range"],
                             max_range=d["max_range"], min_conf=d["min_conf"])


def _assert_planes_equal(got, want, what=""):
    for k in PLANES:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        same = g.view(np.uint32) == w.view(np.uint32) if k == "range" else g == w
        assert same.all(), (what, k, int((~same).sum()), np.argwhere(~same)[:4])


def _turned(pose16, deg):
    """the pose turned about its own y axis"""
    a = np.radians(deg)
    D = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    return tr.colmajor((np.asarray(pose16, np.float64).reshape(4, 4).T @ D).astype(f32))


@pytest.fixture(scope="module")
def scene():
    """frames 0..10 of the street; the model of frames 0..9 on the CPU oracle (bit-equal to the GPU's: test_gpu_parity.py); the
    restatement's sweep of it from frame 10's pose, computed once"""
    import oracle_lib as ol
    seq = rr.sequence(11)
    cpu = ol.Oracle(ol.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=440))
    for fr in seq[:10]:
        cpu.process_frame(*fr)
    model = cpu.download_model()
    assert len(model) > 30000
    pose = np.asarray(seq[10][3], f32).reshape(16)
    from surfelmapping_amd import capi
    sn = _ref_sensor(STREET)
    dirs = capi.lidar_directions(_c_sensor(STREET))       # the library's table (host only; within 1 ulp of numpy's, tested below)
    return dict(seq=seq, model=model, pose=pose, sn=sn, dirs=dirs, want=lr.sweep(model, pose, sn, dirs))


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_lidar_symbols():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.sm_api_version() == 4
    p = capi.lidar_sensor()
    assert (p.n_az, p.n_el, p.az0_deg, p.az_step_deg, p.min_range, p.max_range, p.min_conf) == (360, 16, 0.0, 1.0, 1.0, 60.0, 0.0)
    assert [p.el_deg[i] for i in range(16)] == list(range(-15, 1))
    q = capi.lidar_sensor(n_az=90, az_step_deg=4.0, el_deg=[-3.0, 0.5, 2.0])
    assert (q.n_az, q.n_el, q.az_step_deg, q.max_range) == (90, 3, 4.0, 60.0) and [q.el_deg[i] for i in range(3)] == [-3.0, 0.5, 2.0]


def test_ctypes_mirrors_have_the_header_layout(tmp_path):
    from surfelmapping_amd import capi
    mirrors = {"sm_lidar_sensor": capi.SmLidarSensor, "sm_lidar_stats_t": capi.SmLidarStats}
    lines = []
    for cname, cls in mirrors.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("version %d %u\\n", SM_API_VERSION, SM_LIDAR_MAX_BEAMS);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sm_c_api.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    assert got["version"] == f"4 {capi.LIDAR_MAX_BEAMS}"
    for cname, cls in mirrors.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_arguments_are_rejected_before_any_device_call():
    from surfelmapping_amd import capi
    L = capi.load()
    E = capi.SM_E_ARG
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    sn = capi.lidar_sensor()
    pose = np.eye(4, dtype=f32).reshape(16)
    rng, st = np.zeros(360 * 16, f32), capi.SmLidarStats()
    src = capi.map_source([])
    assert L.sm_default_lidar_sensor(None) == E
    assert L.sm_lidar_sweep(None, C.byref(sn), vp(pose), vp(rng), None, None, None) == E
    assert L.sm_lidar_sweep_maps(None, C.byref(src), C.byref(sn), vp(pose), 1, vp(rng), None, None, None) == E
    assert L.sm_lidar_stats(None, C.byref(st)) == E
    assert L.sm_lidar_directions(None, vp(rng)) == E and L.sm_lidar_directions(C.byref(sn), None) == E
    # the sensor's limits, through the entry point that needs no context
    out = np.zeros(360 * 16 * 3, f32)
    assert L.sm_lidar_directions(C.byref(sn), vp(out)) == 0
    bad = [dict(n_az=0), dict(n_el=0), dict(n_az=4096, n_el=1025, az_step_deg=0.01, el_deg=np.linspace(-80, 80, 1025)), dict(az_step_deg=0.0),
           dict(az_step_deg=-1.0), dict(az_step_deg=float("nan")), dict(az0_deg=float("inf")), dict(n_az=361), dict(az_step_deg=1.001),
           dict(el_deg=[-1.0, -1.0]), dict(el_deg=[0.0, -1.0]), dict(el_deg=[-90.0, 0.0]), dict(el_deg=[0.0, 90.0]), dict(el_deg=[float("nan")]),
           dict(min_range=0.0), dict(min_range=-1.0), dict(min_range=61.0), dict(max_range=float("inf")), dict(min_range=float("nan"))]
    for kw in bad:
        assert L.sm_lidar_directions(C.byref(capi.lidar_sensor(**kw)), vp(np.zeros(1 << 24, f32) if kw.get("n_az") == 4096 else out)) == E, kw
        assert b"sm_lidar_directions" in L.sm_last_error()
    null_el = capi.lidar_sensor()
    null_el.el_deg = None
    assert L.sm_lidar_directions(C.byref(null_el), vp(out)) == E
    # the limits themselves are allowed: n_az * step = 360, min_range = max_range
    assert L.sm_lidar_directions(C.byref(capi.lidar_sensor(n_az=360, az_step_deg=1.0, min_range=5.0, max_range=5.0)), vp(out)) == 0


def test_lidar_demo_compiles_against_c_abi_only(tmp_path):
    exe = str(tmp_path / "lidar_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, DEMO, "-L" + LIBDIR, "-lsurfelmapping_hip",
                           "-Wl,-rpath," + LIBDIR])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def _ulps(a, b):
    """distance in float32 steps, signs included (-0 and +0 are 0 apart)"""
    def lin(x):
        i = np.ascontiguousarray(x, f32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(lin(a) - lin(b))


def test_direction_table_is_numpys_to_one_ulp():
    from surfelmapping_amd import capi
    # double sin / cos are good to under 1 ulp of a double, so the one rounding to float can differ by at most one float ulp
    for kw in (dict(), dict(n_az=2048, az_step_deg=360.0 / 2048, az0_deg=-180.0, el_deg=np.linspace(-24.8, 2.0, 64)),
               dict(n_az=45, az0_deg=-45.0, az_step_deg=1.0, el_deg=[-88.5, -30.25, 0.0, 0.125, 89.0]), dict(n_az=7, az0_deg=1234.5, az_step_deg=51.0)):
        sn = capi.lidar_sensor(**kw)
        got = capi.lidar_directions(sn)
        el = np.array([sn.el_deg[i] for i in range(sn.n_el)], f32)
        want = lr.directions(lr.sensor(n_az=sn.n_az, n_el=sn.n_el, az0=sn.az0_deg, step=sn.az_step_deg, el=el))
        assert got.shape == want.shape == (sn.n_el, sn.n_az, 3) and got.dtype == f32
        assert _ulps(got, want).max() <= 1, kw
        np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=2), 1.0, atol=2e-7)
    d = capi.lidar_directions(capi.lidar_sensor(n_az=4, az0_deg=0.0, az_step_deg=90.0, el_deg=[0.0]))
    assert d[0, 0, 0] == 0 and d[0, 0, 1] == 0 and d[0, 0, 2] == 1 and d[0, 1, 0] == 1           # column 0: exactly (0, -0 or 0, 1)


def test_lidar_points_layout():
    from surfelmapping_amd import capi
    rng = np.array([[2.0, 0.0], [4.0, 1.0]], f32)
    dirs = np.array([[[0, 0, 1], [1, 0, 0]], [[0, -1, 0], [0.6, 0, 0.8]]], f32)
    rgb = np.array([[[255, 255, 255], [9, 9, 9]], [[255, 0, 0], [0, 0, 255]]], np.uint8)
    p = capi.lidar_points(rng, dirs, rgb)
    assert p.dtype == f32 and p.shape == (3, 4)
    # forward 2 m -> x = 2; up 4 m (d.y = -1) -> z = 4; (0.6, 0, 0.8): 0.8 forward, 0.6 to the right = y -0.6
    assert np.allclose(p[:, :3], [[2, 0, 0], [0, 0, 4], [0.8, -0.6, 0]], atol=1e-7)
    assert p[0, 3] == f32(1.0) and p[1, 3] == f32(f32(0.299) * f32(255)) / f32(255) and abs(p[2, 3] - 0.114) < 1e-6
    assert (capi.lidar_points(rng, dirs)[:, 3] == 0).all()


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


@pytest.mark.gpu
def test_sweep_equals_the_restatement(scene, held):
    sn = _c_sensor(STREET)
    want = scene["want"]
    before = held.counts()
    got = held.lidar_sweep(scene["pose"], sn)
    n = int((want["id"] >= 0).sum())
    print(f"{n} of {want['id'].size} beams return; stats {held.lidar_stats()}")
    assert 300 < n < want["id"].size
    _assert_planes_equal(got, want)
    st = held.lidar_stats()
    assert st["surfels"] == len(scene["model"]) and st["tests"] >= n and st["passes"] == 1 and st["chunks"] == 0
    assert held.counts() == before                                    # the model, the counters and the tick are untouched
    assert np.array_equal(held.download_model().view(np.uint32), scene["model"].view(np.uint32))


@pytest.mark.gpu
def test_seam_faces_the_street(scene, held):
    from surfelmapping_amd import capi
    sn = _c_sensor(STREET)
    pose = _turned(scene["pose"], 180.0)
    want = lr.sweep(scene["model"], pose, scene["sn"], capi.lidar_directions(sn))
    got = held.lidar_sweep(pose, sn)
    _assert_planes_equal(got, want)
    # returns on both sides of the seam: the first and the last columns
    assert (want["id"][:, :3] >= 0).any() and (want["id"][:, -3:] >= 0).any()


@pytest.mark.gpu
def test_partial_sweep_is_a_cut_of_the_full_one(scene, held):
    full = held.lidar_sweep(scene["pose"], _c_sensor(STREET))
    part = held.lidar_sweep(scene["pose"], _c_sensor(dict(STREET, n_az=45, az0=-45.0)))     # azimuths -45 .. 43: columns 67 .. 111 of the full sweep
    _assert_planes_equal(part, {k: np.ascontiguousarray(full[k][:, 67:112]) for k in PLANES})
    assert (part["id"] >= 0).any()
    # turned round, the street lies behind the partial sweep: nothing may wrap into its edge columns
    back = _turned(scene["pose"], 180.0)
    full_b = held.lidar_sweep(back, _c_sensor(STREET))
    part_b = held.lidar_sweep(back, _c_sensor(dict(STREET, n_az=45, az0=-45.0)))
    _assert_planes_equal(part_b, {k: np.ascontiguousarray(full_b[k][:, 67:112]) for k in PLANES})


def _child(tmp_path, name, model, pose, sensor, env, timeout=120):
    src, dst = str(tmp_path / f"{name}_in.npz"), str(tmp_path / f"{name}_out.npz")
    np.savez(src, model=model, pose=pose, **sensor)
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env)
    for k in ("SM_LIDAR_LANE_BEAMS", "SM_LIDAR_NO_CULL", "SM_LIDAR_KEY_MB"):
        if k not in env:
            e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lidar_child.py"), src, dst], capture_output=True, text=True, env=e, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(np.load(dst))


def _row(c, n, r, conf=1.0, colour=0x01406080):
    m = np.zeros(12, f32)
    m[0:3], m[3], m[8:11], m[11] = c, conf, n, r
    m[4] = np.array([colour], np.uint32).view(f32)[0]
    return m


def _ordinary(n, seed):
    """n small discs 2..30 m around the origin, half of them facing it"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    nrm = rng.normal(size=(n, 3))
    face = rng.random(n) < 0.5
    nrm[face] = -d[face] + 0.2 * nrm[face]
    m = np.zeros((n, 12), f32)
    m[:, 0:3] = d * rng.uniform(2.0, 30.0, n)[:, None]
    m[:, 3] = rng.uniform(0.0, 20.0, n)
    m[:, 4] = rng.integers(0, 1 << 29, n).astype(np.uint32).view(f32)
    m[:, 7] = rng.integers(0, 10, n)
    m[:, 8:11] = nrm
    m[:, 11] = rng.uniform(0.05, 0.6, n)
    return m


WIDE = dict(n_az=64, az0=-180.0, step=360.0 / 64, el=np.array([-85, -70, -50, -30, -29, -12, -5, 0, 2, 9, 20, 45], f32), min_range=0.2,
            max_range=40.0, min_conf=0.0)
IDENT = np.eye(4, dtype=f32).reshape(16)


def _wide_model():
    wide = np.stack([
        _row((0.0, 0.5, 0.0), (0, 1, 0), 2.0),             # the sensor 0.5 m above a ground disc of r = 2
        _row((0.3, -0.2, 0.4), (0.3, 0.2, 1), 1.5),        # the sensor inside a disc's sphere, the disc tilted
        _row((0.1, 3.0, -0.2), (0, 1, 0.1), 1.2),          # a disc over the pole of the grid
        _row((0.05, 0.5, -6.0), (0, 0, 1), 3.5),           # across the seam
        _row((4.0, 1.0, 4.0), (1, 0, 1), 3.0)])            # large and to the side
    return np.concatenate([_ordinary(400, 5), wide, _ordinary(400, 6)]), np.arange(400, 405)


def test_wide_scenario_on_the_restatement():
    """guards the scenario of the GPU test below: each wide disc is hit, and its footprint is beyond a lane's budget"""
    from surfelmapping_amd import capi
    model, w = _wide_model()
    sn = _ref_sensor(WIDE)
    c, m, r = lr.surfels(model, IDENT)
    hit, _ = lr.hits(c, m, r, sn, capi.lidar_directions(_c_sensor(WIDE)))
    rows, cols = lr.footprint(c, r, sn)
    fp = rows.sum(axis=1) * cols.sum(axis=1)
    assert hit[w].any(axis=1).all() and (fp[w] > 80).all() and (fp[w[:2]] == 768).all()
    assert not (hit & ~(rows[:, :, None] & cols[:, None, :]).reshape(len(model), -1)).any()
    assert (fp > 0).sum() > 100 and hit.any(axis=1).sum() > 40


@pytest.mark.gpu
def test_wide_footprints_on_both_work_paths(tmp_path):
    model, _ = _wide_model()
    sn = _ref_sensor(WIDE)
    one = _child(tmp_path, "lane1", model, IDENT, WIDE, dict(SM_LIDAR_LANE_BEAMS="1"))
    dflt = _child(tmp_path, "default", model, IDENT, WIDE, {})
    from surfelmapping_amd import capi
    want = lr.sweep(model, IDENT, sn, capi.lidar_directions(_c_sensor(WIDE)))
    _assert_planes_equal(one, dflt, "SM_LIDAR_LANE_BEAMS=1 against the default")
    _assert_planes_equal(dflt, want, "default against the restatement")
    # the work split and the tests made are the restated footprint's, up to a beam at a boundary where two maths libraries round apart
    c, _, r = lr.surfels(model, IDENT)
    rows, cols = lr.footprint(c, r, sn)
    fp = rows.sum(axis=1) * cols.sum(axis=1)
    print("wide:", int(one["stat_wide"]), int(dflt["stat_wide"]), "tests:", int(one["stat_tests"]), int(dflt["stat_tests"]), "restated:", int(fp.sum()))
    assert (fp > 80).sum() <= int(dflt["stat_wide"]) <= (fp > 50).sum()
    assert (fp > 2).sum() <= int(one["stat_wide"]) <= (fp > 0).sum()
    assert int(one["stat_tests"]) == int(dflt["stat_tests"]) and abs(int(dflt["stat_tests"]) - int(fp.sum())) <= 0.02 * fp.sum()


@pytest.mark.gpu
def test_hostile_records(tmp_path):
    nan, inf = float("nan"), float("inf")
    bad = np.stack([
        _row((nan, 0, 5), (0, 0, 1), 0.3), _row((0, inf, 5), (0, 0, 1), 0.3), _row((0, 0, -inf), (0, 0, 1), 0.3),
        _row((0, 1, 5), (nan, 0, 1), 0.3), _row((0, 1, 5), (0, inf, 1), 0.3), _row((0, 1, 5), (0, 0, 1), nan),
        _row((0, 1, -5), (0, 0, 1), inf), _row((0, 1, -5), (0, 0, 1), -inf), _row((1, 1, 35), (0.1, 0, 1), 1e30),
        _row((0, 1, 5), (0, 0, 1), 0.3, conf=nan), _row((0, 1, 5), (0, 0, 1), 0.3, conf=inf), _row((1e30, 0, 5), (0, 0, 1), 1e30),
        _row((3e38, 3e38, 3e38), (1, 1, 1), 3e38), _row((0, 1, 5), (1e38, 1e38, 1e38), 0.3), _row((0, 0, 0), (0, 0, 0), 0.0)])
    rng = np.random.default_rng(9)
    model = _ordinary(1000, 7)
    at = np.sort(rng.choice(len(model), len(bad), replace=False))
    model = np.insert(model, at, bad, axis=0)
    got = _child(tmp_path, "hostile", model, IDENT, WIDE, {}, timeout=120)
    from surfelmapping_amd import capi
    want = lr.sweep(model, IDENT, _ref_sensor(WIDE), capi.lidar_directions(_c_sensor(WIDE)))
    _assert_planes_equal(got, want)
    seen = set(np.unique(want["id"])) - {-1}
    hostile = set(int(x) for x in at + np.arange(len(bad)))
    with_nan = set(int(x) for x in np.flatnonzero(np.isnan(model[:, [0, 1, 2, 3, 8, 9, 10, 11]]).any(axis=1)))
    assert len(seen - hostile) > 20 and len(seen & hostile) >= 2 and not (seen & with_nan)     # unbounded discs are hit, rows with a NaN never


@pytest.mark.gpu
def test_dead_slots_are_no_surfels(scene):
    """the same frames with the compaction deferred (dead slots among the occupied ones at the time of the call) and with a
    compaction in every frame: the same planes, the same ids"""
    sn = _c_sensor(STREET)
    outs = []
    for period in (1000, 1):
        m = _gpu(compact_period=period)
        for fr in scene["seq"][:11]:
            m.process_frame(*fr)
        log = m.read_frame_log()
        assert int(log["n_kill"].sum()) > 0                         # frames that culled
        outs.append((m.lidar_sweep(scene["pose"], sn), m.download_model()))
        m.close()
    _assert_planes_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    want = lr.sweep(outs[0][1], scene["pose"], scene["sn"], scene["dirs"])
    _assert_planes_equal(outs[0][0], want)


@pytest.mark.gpu
def test_min_conf_removes_exactly_the_unstable(scene):
    """after ten frames nearly every surfel of the street is still unstable (confidence 0.9), so two thirds of the rows are given a
    stable surfel's confidence here; min_conf between the two values must remove the other third and nothing else"""
    from surfelmapping_amd import capi
    model = scene["model"].copy()
    model[:, 3] = np.where(np.arange(len(model)) % 3 == 0, f32(0.9), f32(10.0))
    conf, thresh = model[:, 3], 5.0
    m = _gpu()
    m.upload_model(model)
    sn = _c_sensor(dict(STREET, min_conf=thresh))
    got = m.lidar_sweep(scene["pose"], sn)
    want = lr.sweep(model, scene["pose"], _ref_sensor(dict(STREET, min_conf=thresh)), scene["dirs"])
    _assert_planes_equal(got, want)
    seen = got["id"][got["id"] >= 0]
    assert len(seen) > 300 and (conf[seen] >= thresh).all() and not np.array_equal(got["id"], scene["want"]["id"])
    # a NaN threshold: nobody takes part
    assert (m.lidar_sweep(scene["pose"], _c_sensor(dict(STREET, min_conf=float("nan"))))["id"] == -1).all()
    # ... and the same as a model without them, up to the ids
    keep = np.flatnonzero(conf >= thresh)
    m.upload_model(model[keep])
    cut = m.lidar_sweep(scene["pose"], _c_sensor(STREET))
    m.close()
    assert np.array_equal(cut["range"].view(np.uint32), got["range"].view(np.uint32))
    assert np.array_equal(np.where(cut["id"] >= 0, keep[np.maximum(cut["id"], 0)], -1), got["id"])


def _write_map(path, rows, a=0, b=0):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([a, b], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, f32).tobytes())


@pytest.fixture(scope="module")
def map_set(scene, tmp_path_factory):
    """the street's model as three files of unequal length and a live remainder"""
    d = tmp_path_factory.mktemp("lidar_maps")
    cuts = [0, 9000, 9300, 27011, len(scene["model"])]
    paths = []
    for i in range(3):
        paths.append(str(d / f"part_{i}.bin"))
        _write_map(paths[-1], scene["model"][cuts[i]:cuts[i + 1]])
    live = _gpu()
    live.upload_model(scene["model"][cuts[3]:])
    poses = np.stack([scene["pose"], _turned(scene["pose"], 180.0), _turned(scene["pose"], 75.0)])
    return dict(paths=paths, live=live, poses=poses, dir=d)


@pytest.mark.gpu
def test_map_set_equals_the_concatenation(scene, held, map_set, monkeypatch):
    for k in ("SM_LIDAR_KEY_MB", "SM_LIDAR_NO_CULL", "SM_LIDAR_LANE_BEAMS"):
        monkeypatch.delenv(k, raising=False)
    live, paths, poses = map_set["live"], map_set["paths"], map_set["poses"]
    near = dict(STREET, max_range=4.0)                                # most of the street lies beyond it
    # blocks of 256 records whose box lies beyond max_range + the largest radius from the first pose, with room to spare for the
    # box test's own slack (the pose is turned by a quarter of a degree only, so the box in the sensor frame is hardly larger)
    cuts, p0, blocks_beyond = [0, 9000, 9300, 27011], np.asarray(poses[0], np.float64)[12:15], 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        for k in range(a, b, 256):
            rows = scene["model"][k:min(k + 256, b)].astype(np.float64)
            lo, hi = rows[:, :3].min(axis=0), rows[:, :3].max(axis=0)
            gap = np.linalg.norm(np.maximum(np.maximum(lo - p0, p0 - hi), 0.0))
            blocks_beyond += gap > (4.0 + np.abs(rows[:, 11]).max()) * 1.01 + 0.1
    assert blocks_beyond > 10
    for sensor in (STREET, near):
        sn = _c_sensor(sensor)
        want = {k: np.stack([held.lidar_sweep(p, sn)[k] for p in poses]) for k in PLANES}
        assert (want["id"] >= 0).any(axis=(1, 2)).all()
        got = live.lidar_sweep_maps(paths, poses, sn)
        _assert_planes_equal(got, want, "files + model")
        st = live.lidar_stats()
        assert st["passes"] == 1 and st["chunks"] == 3 and st["surfels"] == len(scene["model"])
        if sensor is near:
            print("near:", st)
            assert st["blocks_skipped"] >= blocks_beyond
        monkeypatch.setenv("SM_LIDAR_NO_CULL", "1")
        _assert_planes_equal(live.lidar_sweep_maps(paths, poses, sn), want, "no cull")
        assert live.lidar_stats()["blocks_skipped"] == 0
        monkeypatch.delenv("SM_LIDAR_NO_CULL")
    # ids above the files' rows come from the live model; without it they are gone and nothing else changes
    sn = _c_sensor(STREET)
    full = live.lidar_sweep_maps(paths, poses, sn)
    files_only = live.lidar_sweep_maps(paths, poses, sn, include_model=False)
    assert (full["id"] >= 27011).any() and (files_only["id"] < 27011).all()
    # the model alone through the map-set call equals the plain call
    _assert_planes_equal({k: v[0] for k, v in live.lidar_sweep_maps([], poses[:1], sn).items()}, live.lidar_sweep(poses[0], sn))
    # n_sweeps == 0 checks the set only
    assert live.lidar_sweep_maps(paths, np.zeros((0, 16), f32), sn)["range"].shape == (0, 8, 180)


@pytest.mark.gpu
def test_map_set_one_sweep_per_pass(scene, held, map_set, monkeypatch):
    """1 MiB of keys holds one sweep of 1100 x 64 beams (8 bytes each): three passes over the files, the same planes"""
    live, paths, poses = map_set["live"], map_set["paths"], map_set["poses"]
    big = dict(STREET, n_az=1100, az0=-180.0, step=f32(360.0 / 1100), el=np.linspace(-24.0, 2.0, 64).astype(f32))
    if f32(big["step"]) * 1100 > 360:
        big["step"] = np.nextafter(f32(big["step"]), f32(0))
    sn = _c_sensor(big)
    monkeypatch.delenv("SM_LIDAR_KEY_MB", raising=False)
    want = live.lidar_sweep_maps(paths, poses, sn)
    assert live.lidar_stats()["passes"] == 1
    _assert_planes_equal({k: v[1] for k, v in want.items()}, held.lidar_sweep(poses[1], sn))
    monkeypatch.setenv("SM_LIDAR_KEY_MB", "1")
    got = live.lidar_sweep_maps(paths, poses, sn)
    st = live.lidar_stats()
    assert st["passes"] == 3 and st["chunks"] == 9
    _assert_planes_equal(got, want)


@pytest.mark.gpu
def test_truncated_file_is_refused_with_the_outputs_unwritten(scene, map_set):
    from surfelmapping_amd import capi
    live, paths, poses = map_set["live"], map_set["paths"], map_set["poses"]
    short = str(map_set["dir"] / "short.bin")
    with open(short, "wb") as f:
        f.write(open(paths[1], "rb").read()[:-20])
    sn = _c_sensor(STREET)
    L = capi.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rng, ids = np.full((3, 8, 180), 7.0, f32), np.full((3, 8, 180), 7, np.int32)
    rgb, sem = np.full((3, 8, 180, 3), 7, np.uint8), np.full((3, 8, 180), 7, np.uint8)
    for bad in ([paths[0], short, paths[2]], [paths[0], str(map_set["dir"] / "missing.bin")]):
        src = capi.map_source(bad)
        rc = L.sm_lidar_sweep_maps(live._h, C.byref(src), C.byref(sn), vp(np.ascontiguousarray(poses)), 3, vp(rng), vp(ids), vp(rgb), vp(sem))
        assert rc == capi.SM_E_ARG and os.path.basename(bad[1]).encode() in L.sm_last_error()
        assert (rng == 7).all() and (ids == 7).all() and (rgb == 7).all() and (sem == 7).all()
    with pytest.raises(capi.SurfelMapError):
        live.lidar_sweep(np.full(16, np.nan, f32), sn)


@pytest.mark.gpu
def test_facade_velodyne_files_equal_python(scene, map_set, tmp_path):
    from surfelmapping_amd import capi
    exe = str(tmp_path / "lidar_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, DEMO, "-L" + LIBDIR, "-lsurfelmapping_hip",
                           "-Wl,-rpath," + LIBDIR])
    live_map = str(tmp_path / "live.bin")
    _write_map(live_map, scene["model"][27011:])
    poses = map_set["poses"]
    with open(tmp_path / "poses.bin", "wb") as f:
        f.write(np.array([len(poses)], np.uint32).tobytes() + np.ascontiguousarray(poses, f32).tobytes())
    r = subprocess.run([exe, live_map, "440", str(tmp_path / "poses.bin"), str(tmp_path), "180", "8", "-179", "2", "-14", "2", "60"] + map_set["paths"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sn = _c_sensor(STREET)
    dirs = capi.lidar_directions(sn)
    out = map_set["live"].lidar_sweep_maps(map_set["paths"], poses, sn)
    for k in range(len(poses)):
        pts = np.fromfile(tmp_path / "velodyne" / f"{k:06d}.bin", f32).reshape(-1, 4)
        want = capi.lidar_points(out["range"][k], dirs, out["rgb"][k])
        assert len(want) > 100 and np.array_equal(pts.view(np.uint32), want.view(np.uint32)), k
    n0 = int((out["id"][0] >= 27011).sum())
    alone = map_set["live"].lidar_sweep(poses[0], sn)
    assert f"model returns {int((alone['id'] >= 0).sum())} of 1440" in r.stdout and n0 > 0, r.stdout
