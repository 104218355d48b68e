"""Ray casts (sm_cast_rays_maps, sm_default_rays_params, sm_cast_rays_stats; SurfelMap.cast_rays / cast_rays_stats, capi.lidar_rays;
DESIGN.md "4x. Ray casts").  CPU: the symbols, the struct layouts, the defaults, lidar_rays against the direction table.  GPU: every
plane bit for bit against the brute-force restatement of tests/rays_ref.py and, where the rays are a sweep's beams from a pose that
does not rotate, against sm_lidar_sweep -- on the street of tests/retire_ref.py and on small sets made for a rule each."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rays_ref as rf
import retire_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CAM, OVER = rr.CAM, rr.OVER
NEW = ("sm_default_rays_params", "sm_cast_rays_maps", "sm_cast_rays_stats")
PLANES = ("t", "id", "rgb", "sem", "normal")
STREET = dict(n_az=180, az0_deg=-179.0, az_step_deg=2.0, el_deg=np.arange(-14, 1, 2, dtype=f32), min_range=1.0, max_range=60.0, min_conf=0.0)
CUTS = [0, 9000, 9300, 27011]


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


def _ray(o, d, t_min=0.0, t_max=1e30):
    return np.array([o[0], o[1], o[2], t_min, d[0], d[1], d[2], t_max], f32)


def _write_map(path, rows, a=0, b=0):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([a, b], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, f32).tobytes())


def _street_rays(model, n, seed):
    """n rays with origins inside and outside the model's box, directions of lengths 1e-3 .. 1e3, random [t_min, t_max] in units of
    those lengths, every eighth with t_min == t_max"""
    rng = np.random.default_rng(seed)
    lo, hi = model[:, 0:3].min(axis=0), model[:, 0:3].max(axis=0)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    o = mid + rng.uniform(-1.5, 1.5, (n, 3)) * half
    d = rng.normal(size=(n, 3))
    d[::16, 1] = 0.0
    length = 10.0 ** rng.uniform(-3, 3, n)
    d = d / np.linalg.norm(d, axis=1)[:, None] * length[:, None]
    t0 = rng.uniform(0.0, 5.0, n) / length
    t0[::3] = 0.0
    t1 = t0 + rng.uniform(0.0, 60.0, n) / length
    t1[::8] = t0[::8]
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, t0, d, t1
    rays[:, 7] = np.maximum(rays[:, 7], rays[:, 3])
    return rays


@pytest.fixture(scope="module")
def scene():
    """the street of tests/test_lidar.py: the model of frames 0..9 on the CPU oracle, an identity-rotation pose at frame 10's position,
    the sweep's beams as rays and 2048 general rays, with the restatement's answers, computed once"""
    import oracle_lib as ol
    from surfelmapping_amd import capi
    seq = rr.sequence(11)
    cpu = ol.Oracle(ol.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=440))
    for fr in seq[:10]:
        cpu.process_frame(*fr)
    model = cpu.download_model()
    assert len(model) > 30000
    pose = np.eye(4, dtype=f32)
    pose[0:3, 3] = np.asarray(seq[10][3], f32).reshape(16)[12:15]
    sn = capi.lidar_sensor(**STREET)
    beams = capi.lidar_rays(sn, pose)
    general = _street_rays(model, 2048, 11)
    return dict(seq=seq, model=model, pose=pose, sn=sn, beams=beams, want_beams=rf.cast(model, beams), general=general,
                want_general=rf.cast(model, general))


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_ray_symbols_and_defaults():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.sm_api_version() == 4
    p = capi.rays_params()
    assert (p.cell_mm, list(p.origin), p.min_conf, list(p.reserved)) == (250, [0.0, 0.0, 0.0], 0.0, [0, 0, 0])
    q = capi.rays_params(cell_mm=100, origin=(1.0, 2.0, 3.5), min_conf=2.0)
    assert (q.cell_mm, list(q.origin), q.min_conf) == (100, [1.0, 2.0, 3.5], 2.0)
    with pytest.raises(KeyError):
        capi.rays_params(cell=3)


def test_null_arguments_are_rejected_without_a_context():
    from surfelmapping_amd import capi
    L = capi.load()
    p, src, st = capi.rays_params(), capi.map_source([]), capi.SmRaysStats()
    rays, t = np.zeros((4, 8), f32), np.zeros(4, f32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sm_default_rays_params(None) == capi.SM_E_ARG
    assert L.sm_cast_rays_maps(None, C.byref(src), C.byref(p), vp(rays), 4, vp(t), None, None, None, None) == capi.SM_E_ARG
    assert L.sm_cast_rays_stats(None, C.byref(st)) == capi.SM_E_ARG


def test_lidar_rays_of_an_unrotated_pose_are_the_direction_table():
    from surfelmapping_amd import capi
    for kw in (dict(), STREET, dict(n_az=7, az0_deg=12.5, az_step_deg=51.0, el_deg=[-88.5, 0.0, 0.125, 89.0], min_range=0.5, max_range=7.0)):
        sn = capi.lidar_sensor(**kw)
        d = capi.lidar_directions(sn)
        pose = np.eye(4, dtype=f32)
        pose[0:3, 3] = (1.5, -2.25, 1e3)
        for given in (pose, pose.T.reshape(16), np.broadcast_to(pose.T.reshape(16), (sn.n_az, 16))):
            rays = capi.lidar_rays(sn, given)
            assert rays.shape == (sn.n_el * sn.n_az, 8) and rays.dtype == f32
            assert np.array_equal(rays[:, 4:7].view(np.uint32), d.reshape(-1, 3).view(np.uint32))          # bit for bit, -0 included
            assert (rays[:, 0:3] == pose[0:3, 3]).all() and (rays[:, 3] == f32(sn.min_range)).all() and (rays[:, 7] == f32(sn.max_range)).all()
    # a pose per column: column j's beams turn with pose j, in double, rounded once
    sn = capi.lidar_sensor(n_az=4, az0_deg=0.0, az_step_deg=90.0, el_deg=[-10.0, 0.0])
    d = capi.lidar_directions(sn).astype(np.float64)
    poses = []
    for j in range(4):
        a = 0.3 * j + 0.1
        M = np.array([[np.cos(a), 0, np.sin(a), j], [0, 1, 0, 2 * j], [-np.sin(a), 0, np.cos(a), -j], [0, 0, 0, 1]]).astype(f32)
        poses.append(M.T.reshape(16))
    rays = capi.lidar_rays(sn, np.stack(poses)).reshape(2, 4, 8)
    for j in range(4):
        R = poses[j].reshape(4, 4).T[:3, :3].astype(np.float64)
        assert np.allclose(rays[:, j, 4:7], d[:, j] @ R.T, atol=1e-7) and (rays[:, j, 0:3] == poses[j][12:15]).all()
    with pytest.raises(ValueError):
        capi.lidar_rays(sn, np.stack(poses[:3]))


def test_restatement_on_hand_made_rays():
    """the reference itself: a disc straight ahead, ties, a grazing ray, the gate, an invalid ray"""
    model = np.stack([_row((0, 0, 5), (0, 0, 1), 0.5), _row((0, 0, 5), (0, 0, 1), 0.5), _row((0, 0, 3), (0, 0, -2), 0.1, conf=0.5)])
    rays = np.stack([_ray((0, 0, 0), (0, 0, 1)), _ray((0, 0, 0), (0, 0, 2)), _ray((0.3, 0, 0), (0, 0, 1)), _ray((0, 0, 5), (1, 0, 0)),
                     _ray((0, 0, 0), (0, 0, 0)), _ray((0, 0, 0), (0, 0, 1), 3.5, 4.0)])
    out = rf.cast(model, rays)
    assert out["id"].tolist() == [2, 2, 0, -1, -1, -1] and out["t"].tolist() == [3.0, 1.5, 5.0, 0.0, 0.0, 0.0]
    assert rf.cast(model, rays, min_conf=1.0)["id"].tolist() == [0, 0, 0, -1, -1, -1]
    assert out["sem"].tolist() == [2, 2, 2, 0, 0, 0] and out["rgb"][0].tolist() == [0x40, 0x60, 0x80] and out["normal"][0].tolist() == [0, 0, -2]
    assert rf.valid(rays).tolist() == [True, True, True, True, False, True]


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


def _cast(m, model, rays, **kw):
    m.upload_model(np.ascontiguousarray(model, f32))
    return m.cast_rays(rays, normal=True, **kw)


@pytest.mark.gpu
def test_sweep_beams_equal_the_restatement_and_the_lidar(scene, held):
    before = held.counts()
    got = held.cast_rays(scene["beams"], normal=True)
    st = held.cast_rays_stats()
    want = scene["want_beams"]
    n = int((want["id"] >= 0).sum())
    print(f"{n} of {len(want['id'])} beams return; stats {st}")
    assert 300 < n < len(want["id"])
    _assert_equal(got, want, "restatement")
    lid = held.lidar_sweep(scene["pose"], scene["sn"])
    _assert_equal(dict(t=got["t"].reshape(8, 180), id=got["id"].reshape(8, 180), rgb=got["rgb"].reshape(8, 180, 3), sem=got["sem"].reshape(8, 180)),
                  dict(t=lid["range"], id=lid["id"], rgb=lid["rgb"], sem=lid["sem"]), "lidar", ("t", "id", "rgb", "sem"))
    assert st["rays"] == 1440 and st["bad_rays"] == 0 and st["records"] == len(scene["model"]) and st["chunks"] == 1 and st["files_skipped"] == 0
    assert st["tests"] >= n and st["probes"] > 0 and 0 < st["cells"] <= st["pairs"] <= 8 * len(scene["model"])
    assert st["no_slot"] == 0 and st["gave_up"] == 0
    indexed = st["tests"] - st["wide"] * 1440                                  # every valid ray tests every wide record; the rest came through the index
    assert 0 < indexed < 0.02 * 1440 * (len(scene["model"]) - st["wide"])      # ... which does save tests
    assert held.counts() == before                                            # the model, the counters and the tick are untouched
    assert np.array_equal(held.download_model().view(np.uint32), scene["model"].view(np.uint32))
    # only t asked for
    L = held._L
    from surfelmapping_amd import capi
    t = np.zeros(1440, f32)
    p, src = capi.rays_params(), capi.map_source([])
    assert L.sm_cast_rays_maps(held._h, C.byref(src), C.byref(p), scene["beams"].ctypes.data_as(C.c_void_p), 1440, t.ctypes.data_as(C.c_void_p),
                               None, None, None, None) == 0
    assert np.array_equal(t.view(np.uint32), want["t"].view(np.uint32))


@pytest.mark.gpu
def test_general_rays_equal_the_restatement(scene, held):
    got = held.cast_rays(scene["general"], normal=True)
    want = scene["want_general"]
    n = int((want["id"] >= 0).sum())
    print(f"{n} of 2048 rays return; stats {held.cast_rays_stats()}")
    assert 100 < n < 2048
    _assert_equal(got, want)


@pytest.fixture(scope="module")
def map_set(scene, tmp_path_factory):
    """the street's model as three files of unequal length and a live remainder, and as one file"""
    d = tmp_path_factory.mktemp("rays_maps")
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
def test_answer_does_not_depend_on_split_cells_origin_or_index(scene, held, map_set, tmp_path, monkeypatch):
    monkeypatch.delenv("SM_RAYS_NO_INDEX", raising=False)
    rays = np.concatenate([scene["beams"][::3], scene["general"][:1024]])
    want = {k: np.concatenate([scene["want_beams"][k][::3], scene["want_general"][k][:1024]]) for k in PLANES}
    live = map_set["live"]
    _assert_equal(live.cast_rays(rays, map_set["paths"], normal=True), want, "three files and the live remainder")
    st = live.cast_rays_stats()
    assert st["chunks"] == 4 and st["records"] == len(scene["model"])
    files_only = live.cast_rays(rays, map_set["paths"], include_model=False, normal=True)
    full_ids = want["id"]
    assert (full_ids >= CUTS[3]).any() and (files_only["id"] < CUTS[3]).all()
    _assert_equal(live.cast_rays(rays, [map_set["whole"]], include_model=False, normal=True), want, "one file")
    _assert_equal(held.cast_rays(rays, normal=True), want, "the model alone")
    tests = {}
    for cell_mm in (50, 250, 1000, 20000):
        for origin in ((0.0, 0.0, 0.0), (0.1234, -7.001, 3.3)):
            _assert_equal(held.cast_rays(rays, cell_mm=cell_mm, origin=origin, normal=True), want, f"cell_mm {cell_mm} origin {origin}")
            tests[cell_mm] = held.cast_rays_stats()["tests"]
    print("exact tests by cell_mm:", tests)
    assert tests[1000] < tests[20000]                                         # (in 20 m cells a ray meets most of the street)
    # every record on the wide path, in a fresh process
    sub = rays[::4]
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, model=scene["model"], rays=sub, cell_mm=250)
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), SM_RAYS_NO_INDEX="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rays_child.py"), src, dst], capture_output=True, text=True, env=e, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    child = dict(np.load(dst))
    _assert_equal(child, {k: v[::4] for k, v in want.items()}, "SM_RAYS_NO_INDEX=1")
    takes = int((scene["model"][:, 3] >= 0).sum())
    assert int(child["stat_wide"]) == takes and int(child["stat_tests"]) == takes * int(rf.valid(sub).sum()) and int(child["stat_probes"]) == 0


def _targets(rng, model, idx, n_each=3):
    """rays aimed at points of the discs idx from random sides"""
    rays = []
    for j in idx:
        c, nn, r = model[j, 0:3].astype(np.float64), model[j, 8:11].astype(np.float64), abs(float(model[j, 11]))
        for _ in range(n_each):
            e = np.cross(nn, rng.normal(size=3))
            e /= max(np.linalg.norm(e), 1e-30) if np.isfinite(e).all() else 1.0
            target = c + e * min(r, 5.0) * rng.uniform(0.0, 1.1)
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            rays.append(_ray(target - d * rng.uniform(0.5, 6.0), d * rng.uniform(0.5, 2.0)))
    return np.stack(rays)


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
    V = rf.cell_edge(100)
    k7, c0, c1 = rf.classify(model[7], V, (0, 0, 0))
    assert k7 == rf.REG and len(rf.registered(c0, c1)) == 8 and rf.classify(model[8], V, (0, 0, 0))[0] == rf.WIDE
    rays = np.concatenate([_targets(rng, model, list(big) + [7, 8] + list(range(100, 160))), _street_rays(model, 512, 5)])
    got = _cast(bench, model, rays, cell_mm=100)
    st = bench.cast_rays_stats()
    want = rf.cast(model, rays)
    print("hits:", int((want["id"] >= 0).sum()), "stats:", st)
    assert np.isin([7, 8, big[0], big[3]], want["id"]).all()
    _assert_equal(got, want)
    assert st["wide"] == rf.wide_count(model, 100) == len(big) + 1
    _assert_equal(bench.cast_rays(rays, cell_mm=5000, normal=True), want, "5 m cells")
    assert bench.cast_rays_stats()["wide"] == rf.wide_count(model, 5000) == 0


@pytest.mark.gpu
def test_hostile_records_and_dead_slots(scene, bench):
    nan, inf = float("nan"), float("inf")
    c = scene["model"][1000, 0:3]
    bad = np.stack([
        _row((nan, c[1], c[2]), (0, 0, 1), 0.3), _row((c[0], inf, c[2]), (0, 0, 1), 0.3), _row((c[0], c[1], -inf), (0, 0, 1), 0.3),
        _row((1e10, c[1], c[2]), (0, 0, 1), 0.3), _row((c[0], -1e10, 1e10), (0, 1, 0), 1e10), _row(c, (0, 0, 0), 0.3),
        _row(c, (0, 0, 1), -0.3), _row(c + 0.5, (0, 1, 1), inf), _row(c - 0.5, (1, 0, 1), -inf), _row(c, (0, 0, 1), nan),
        _row(c, (nan, 0, 1), 0.3), _row(c, (0, inf, 1), 0.3), _row(c + 0.1, (0, 0, 1), 0.3, conf=nan), _row(c + 0.2, (0, 0, 1), 0.3, conf=0.25),
        _row(c + 0.3, (0, 0, 1), 0.3, conf=inf), _row((3e38, 3e38, 3e38), (1, 1, 1), 3e38), _row(c, (1e38, 1e38, 1e38), 0.3),
        _row((0, 0, 0), (0, 0, 0), 0.0), _row(c, (0.1, 0, 1), 1e30)])
    rng = np.random.default_rng(9)
    model = scene["model"][:12000]
    at = np.sort(rng.choice(len(model), len(bad), replace=False))
    model = np.insert(model, at, bad, axis=0)
    rays = np.concatenate([scene["beams"][::2], scene["general"][:512], _targets(rng, model, [int(x) for x in at + np.arange(len(bad))
                                                                                               if np.isfinite(model[int(x), 0:3]).all() and abs(model[int(x), 0]) < 1e9], 2)])
    for min_conf in (0.0, 0.5):
        got = _cast(bench, model, rays, min_conf=min_conf)
        want = rf.cast(model, rays, min_conf=min_conf)
        _assert_equal(got, want, f"min_conf {min_conf}")
    hostile = set(int(x) for x in at + np.arange(len(bad)))
    seen = set(np.unique(want["id"])) - {-1}
    with_nan = set(int(x) for x in np.flatnonzero(np.isnan(model[:, [0, 1, 2, 3, 11]]).any(axis=1)))
    assert len(seen - hostile) > 50 and len(seen & hostile) >= 2 and not (seen & with_nan)
    assert (bench.cast_rays(rays, min_conf=nan)["id"] == -1).all()
    # dead slots: frames with the compaction deferred leave dead slots among the occupied ones; the cast sees the compacted model
    m = _gpu(compact_period=1000)
    for fr in scene["seq"][:11]:
        m.process_frame(*fr)
    assert int(m.read_frame_log()["n_kill"].sum()) > 0
    got = m.cast_rays(scene["beams"], normal=True)
    lid = m.lidar_sweep(scene["pose"], scene["sn"])
    after = m.download_model()
    m.close()
    _assert_equal(got, rf.cast(after, scene["beams"]), "dead slots")
    assert np.array_equal(got["id"].reshape(8, 180), lid["id"]) and np.array_equal(got["t"].reshape(8, 180).view(np.uint32), lid["range"].view(np.uint32))


@pytest.mark.gpu
def test_hostile_rays(scene, held):
    nan, inf = float("nan"), float("inf")
    o = scene["pose"][0:3, 3]
    bad = np.stack([_ray((nan, 0, 0), (0, 0, 1)), _ray(o, (0, nan, 1)), _ray(o, (0, 0, 1), nan, 5.0), _ray(o, (0, 0, 1), 0.0, nan),
                    _ray((inf, 0, 0), (0, 0, 1)), _ray(o, (0, -inf, 1)), _ray(o, (0, 0, 1), 0.0, inf), _ray(o, (0, 0, 1), inf, inf),
                    _ray(o, (0, 0, 0)), _ray(o, (0.0, -0.0, 0.0)), _ray(o, (0, 0, 1), -1e-30, 5.0), _ray(o, (0, 0, 1), 5.0, 4.999)])
    good = scene["beams"][::5].copy()
    good[:, 7] = 1e30
    good[:, 3] = 0.0
    # rays lying exactly in lattice planes and through lattice corners of the 250 mm grid (0.25 m exactly), along the street
    lo, hi = scene["model"][:, 0:3].min(axis=0), scene["model"][:, 0:3].max(axis=0)
    snap = lambda p: np.round(np.asarray(p, np.float64) * 4) / 4
    lattice = []
    for k in range(40):
        c = snap(lo + (hi - lo) * np.random.default_rng(k).uniform(0, 1, 3))
        lattice += [_ray(c - np.eye(3)[k % 3] * 8.0, np.eye(3)[k % 3]), _ray(c, (1, 1, 1), 0.0, 40.0), _ray(c - (8, 0, 8), (0.25, 0, 0.25)),
                    _ray((c[0], lo[1] - 1.0, c[2]), (0, 1, 0))]
    rays = np.concatenate([bad, good, np.stack(lattice)])
    order = np.random.default_rng(1).permutation(len(rays))
    rays = rays[order]
    assert int((~rf.valid(rays)).sum()) == len(bad)
    got = held.cast_rays(rays, normal=True)
    st = held.cast_rays_stats()
    want = rf.cast(scene["model"], rays)
    _assert_equal(got, want)
    is_bad = ~rf.valid(rays)
    assert st["bad_rays"] == len(bad) and (got["id"][is_bad] == -1).all() and (got["t"][is_bad] == 0).all() and (got["sem"][is_bad] == 0).all()
    assert (want["id"][~is_bad] >= 0).sum() > 100


@pytest.mark.gpu
def test_ties_signs_and_grazing(bench):
    model = np.stack([_row((5, 5, 5), (1, 0, 0), 0.1),                                   # padding: ids 1 and 2 are the twins
                      _row((0, 0, 2), (0, 0, 1), 0.5, colour=0x02010203), _row((0, 0, 2), (0, 0, 1), 0.5, colour=0x03040506),
                      _row((1, 1, 0), (0, 0, -1), 0.5), _row((-3, 0, 0), (0, 1, 0), 0.5)])
    rays = np.stack([_ray((0, 0, 0), (0, 0, 1)),                    # the twins: the lower id wins
                     _ray((1.2, 1.1, 0), (0, 0, 1)),                # the origin on the disc's plane: num = -0, t = -0 -> bits 0
                     _ray((1.2, 1.1, 0), (0, 0, -1)),               # ... num = -0 / den = +1
                     _ray((1.2, 1.1, 0), (1, 0, 0)),                # in the plane: den = 0, 0 / 0
                     _ray((-3, -2, 0.1), (0, 1, 0)), _ray((-5, 0, 0), (1, 0, 0)),     # one through the disc; one grazing in its plane: den = 0
                     _ray((-5, 1e-3, 0), (1, 0, 0))])               # parallel to it, just off the plane: den = 0, num != 0 -> inf
    got = _cast(bench, model, rays)
    want = rf.cast(model, rays)
    _assert_equal(got, want)
    assert got["id"].tolist() == [1, 3, 3, -1, 4, -1, -1]
    assert got["t"].view(np.uint32)[1] == 0 and got["t"].view(np.uint32)[2] == 0 and got["t"][0] == 2.0
    assert got["rgb"][0].tolist() == [1, 2, 3] and got["sem"][0] == 3 and got["normal"][1].tolist() == [0, 0, -1]


@pytest.mark.gpu
def test_rays_that_cannot_reach_the_records_cost_no_test(bench):
    rng = np.random.default_rng(4)
    n = 2000
    model = np.zeros((n, 12), f32)
    model[:, 0:3] = rng.uniform((10.5, -5, -5), (30, 5, 5), (n, 3))
    model[:, 3], model[:, 11] = 1.0, rng.uniform(0.01, 0.1, n)
    model[:, 8:11] = rng.normal(size=(n, 3))
    o = rng.uniform((-30, -5, -5), (-0.5, 5, 5), (600, 3))
    e = rng.uniform((-30, -5, -5), (-0.5, 5, 5), (600, 3))
    rays = np.zeros((600, 8), f32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = o, e - o, 1.0                                 # segments from o to e, both at x < 0
    got = _cast(bench, model, rays, cell_mm=250)
    st = bench.cast_rays_stats()
    assert (got["id"] == -1).all() and (got["t"] == 0).all() and st["tests"] == 0 and st["wide"] == 0, st
    # the same rays prolonged do reach them
    rays[:, 7] = 1e3
    got = bench.cast_rays(rays, cell_mm=250, normal=True)
    _assert_equal(got, rf.cast(model, rays))


def _far_origin_case():
    """100 discs of about 1 mm in a 0.2 m box, 2000 rays from 30 km away: there a float32 coordinate is 2 mm coarse and the ray's
    slack S is 15 mm, 7 cells of 2 mm -- more cells in the first slab than a walk may visit (64 + n / 8 = 76)"""
    rng = np.random.default_rng(17)
    n = 100
    model = np.zeros((n, 12), f32)
    model[:, 0:3] = rng.uniform(-0.1, 0.1, (n, 3))
    model[:, 3] = 1.0
    model[:, 4] = rng.integers(0, 1 << 29, n).astype(np.uint32).view(f32)
    model[:, 8:11] = rng.normal(size=(n, 3))
    model[:, 11] = rng.uniform(0.0005, 0.0009, n)
    rays = []
    for j in range(n):
        for _ in range(20):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            rays.append(_ray(model[j, 0:3].astype(np.float64) - d * 3.0e4, d))
    return model, np.stack(rays)


def test_far_origin_case_on_the_restatement():
    """guards the scenario of the GPU test below: some rays do hit, their records are regular, and the restated walk of a hitting
    ray visits more cells than the budget"""
    model, rays = _far_origin_case()
    want = rf.cast(model, rays)
    hit = np.flatnonzero(want["id"] >= 0)
    V = rf.cell_edge(2)
    box, kinds = rf.box_of(model, V, (0.0, 0.0, 0.0))
    assert len(hit) >= 5 and sum(k == rf.REG for k, _, _ in kinds) >= 60
    assert all(kinds[want["id"][i]][0] == rf.REG for i in hit[:5])
    assert all(len(rf.visited(rays[i], V, (0.0, 0.0, 0.0), box)) > rf.budget(len(model)) for i in hit[:5])


@pytest.mark.gpu
def test_walk_that_is_given_up_still_finds_the_hits(bench):
    model, rays = _far_origin_case()
    got = _cast(bench, model, rays, cell_mm=2)
    st = bench.cast_rays_stats()
    want = rf.cast(model, rays)
    print("hits:", int((want["id"] >= 0).sum()), "stats:", st)
    _assert_equal(got, want)
    assert st["gave_up"] > 0 and st["no_slot"] == 0 and st["wide"] == rf.wide_count(model, 2)
    _assert_equal(bench.cast_rays(rays, cell_mm=250, normal=True), want, "250 mm cells")
    assert bench.cast_rays_stats()["gave_up"] == 0



@pytest.mark.gpu
def test_moving_sweep(scene, held):
    from surfelmapping_amd import capi
    sn = scene["sn"]
    base = scene["pose"].astype(np.float64)
    poses = []
    for j in range(180):                                                                  # the vehicle drives and yaws while the sensor turns
        a = np.radians(0.05 * j)
        M = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
        M[0:3, 3] = base[0:3, 3] + np.array([0.002 * j, 0.0, 0.01 * j])
        poses.append(M.astype(f32).T.reshape(16))
    rays = capi.lidar_rays(sn, np.stack(poses))
    assert len(np.unique(rays[:, 0:3], axis=0)) == 180
    got = held.cast_rays(rays, normal=True)
    want = rf.cast(scene["model"], rays)
    assert (want["id"] >= 0).sum() > 300
    _assert_equal(got, want)
    same = capi.lidar_rays(sn, np.broadcast_to(scene["pose"].T.reshape(16), (180, 16)))
    got = held.cast_rays(same)
    lid = held.lidar_sweep(scene["pose"], sn)
    assert np.array_equal(got["t"].reshape(8, 180).view(np.uint32), lid["range"].view(np.uint32)) and np.array_equal(got["id"].reshape(8, 180), lid["id"])
    assert np.array_equal(got["rgb"].reshape(8, 180, 3), lid["rgb"]) and np.array_equal(got["sem"].reshape(8, 180), lid["sem"])


@pytest.mark.gpu
def test_argument_rules(scene, map_set):
    from surfelmapping_amd import capi
    L = capi.load()
    E = capi.SM_E_ARG
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    m = _gpu()
    st = capi.SmRaysStats()
    assert L.sm_cast_rays_stats(m._h, C.byref(st)) == E and b"no sm_cast_rays_maps call yet" in L.sm_last_error()
    m.process_frame(*scene["seq"][0])
    rays = np.ascontiguousarray(scene["beams"][:64])
    outs = dict(t=np.full(64, 7.0, f32), id=np.full(64, 7, np.int32), rgb=np.full((64, 3), 7, np.uint8), sem=np.full(64, 7, np.uint8),
                normal=np.full((64, 3), 7.0, f32))
    ptrs = [vp(outs[k]) for k in PLANES]
    p, src = capi.rays_params(), capi.map_source(map_set["paths"])
    call = lambda p_=p, src_=src, rays_=rays, n=64, ptrs_=ptrs: L.sm_cast_rays_maps(m._h, None if src_ is None else C.byref(src_),
                                                                                      None if p_ is None else C.byref(p_), vp(rays_), n, *ptrs_)
    unwritten = lambda: all((outs[k] == 7).all() for k in PLANES)
    assert call(src_=None) == E and call(p_=None) == E and call(rays_=None) == E and call(ptrs_=[None] + ptrs[1:]) == E
    assert call(p_=capi.rays_params(cell_mm=0)) == E and call(p_=capi.rays_params(cell_mm=-5)) == E
    assert call(p_=capi.rays_params(origin=(0.0, float("nan"), 0.0))) == E and call(p_=capi.rays_params(origin=(float("inf"), 0.0, 0.0))) == E
    assert call(n=capi.RAYS_MAX + 1) == E and b"2^24" in L.sm_last_error()
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
    assert L.sm_cast_rays_stats(m._h, C.byref(st)) == E                       # no call has succeeded yet
    assert call(n=0, rays_=None, ptrs_=[None] * 5) == 0 and unwritten()        # n_rays == 0 checks the set only
    assert L.sm_cast_rays_stats(m._h, C.byref(st)) == 0 and st.rays == 0 and st.records == CUTS[3] + m.counts()["count"]
    assert call(n=0, src_=capi.map_source([short])) == E
    assert call() == 0 and not unwritten()
    m.close()
    for configure in ("shard_stream_configure", "rig_configure"):
        part = _gpu()
        getattr(part, configure)(0, 1)
        with pytest.raises(capi.SurfelMapError) as e:
            part.cast_rays(rays)
        assert e.value.rc == capi.SM_E_UNSUPPORTED
        part.close()
