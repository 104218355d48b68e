"""Scenes (sm_render_image_scene, sm_lidar_sweep_scene, sm_scene_place_rows, sm_scene_stats; SurfelMap.render_scene /
lidar_sweep_scene; DESIGN.md "4w. Scenes").  CPU: the symbols, the struct layouts, the placed row against numpy, the argument
rules, the restatement's own arithmetic.  GPU: the definition -- every plane of every view bit for bit against the EXISTING entry
points (render_image_maps / lidar_sweep_maps per view over the static files plus actor files placed on the host, or by
sm_warp_by_time itself) --, ties, batching, culling, wide footprints, hostile rows, the live model, the empty scene."""
import ctypes as C
import os

import numpy as np
import pytest

import retire_ref as rr
import scene_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CAM, OVER = rr.CAM, rr.OVER
IMG = (CAM["width"], CAM["height"], CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])
NEW = ("sm_render_image_scene", "sm_lidar_sweep_scene", "sm_scene_place_rows", "sm_scene_stats")
LIDAR_PLANES = ("range", "id", "rgb", "sem")
# test_lidar.py's sweep of the street: 180 x 8 at 2 degrees, el = -14 .. 0
STREET = dict(n_az=180, az0_deg=-179.0, az_step_deg=2.0, el_deg=np.arange(-14, 1, 2, dtype=f32), min_range=1.0, max_range=60.0, min_conf=0.0)
ACTOR_SEM = sr.ACTOR_CLASS + 1
ENV = ("SM_RENDER_MAPS_KEY_MB", "SM_RENDER_MAPS_NO_CULL", "SM_LIDAR_KEY_MB", "SM_LIDAR_NO_CULL", "SM_LIDAR_LANE_BEAMS", "SM_SCENE_NO_CULL")


def write_map(path, rows, a=0, b=0):
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 12)
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([a, b], np.int32).tobytes())
        f.write(rows.tobytes())
    return str(path)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    eq = a.view(np.uint8) == b.view(np.uint8)
    assert eq.all(), (what, int((~eq).sum()), np.argwhere(~eq)[:4])


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_scene_symbols():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.sm_api_version() == 4 and capi.API_VERSION == 4
    for name in ("render_scene", "lidar_sweep_scene", "scene_stats"):
        assert callable(getattr(capi.SurfelMap, name))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_place_rows_is_the_stated_rule_bit_for_bit():
    from surfelmapping_amd import capi
    rng = np.random.default_rng(11)
    rows = rng.normal(0, 30, (4096, 12)).astype(f32)
    # a near-rigid pose with every entry busy, and a large translation
    a, b = 0.7, -0.4
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    pose = np.concatenate([R, [[1234.5], [-6.25], [9876.0]]], axis=1).astype(f32).reshape(12)
    got = capi.scene_place_rows(pose, rows)
    want = sr.place_rows(pose, rows)
    assert np.array_equal(_bits(got), _bits(want))
    # the inputs would catch a contracted build: the fused restatement differs on them
    fused = sr.place_rows_contracted(pose, rows)
    n_diff = int((_bits(fused) != _bits(want)).any(axis=1).sum())
    assert n_diff > 100, n_diff
    assert not np.array_equal(_bits(got), _bits(fused))
    # every field but the centre and the normal passes through
    keep = [3, 4, 5, 6, 7, 11]
    assert np.array_equal(_bits(got[:, keep]), _bits(rows[:, keep]))
    # hostile values: NaN, +-inf, denormals, -0 -- NaNs compared as NaNs (their payloads are the hardware's), the rest by bits
    hostile = rows[:64].copy()
    vals = np.array([np.nan, np.inf, -np.inf, 1e-42, -1e-45, -0.0, 0.0, 3e38], f32)
    for k in range(64):
        hostile[k, [0, 1, 2, 8, 9, 10, 11, 3][k % 8]] = vals[(k // 8) % 8]
    with np.errstate(all="ignore"):
        got, want = capi.scene_place_rows(pose, hostile), sr.place_rows(pose, hostile)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.any() and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])
    # the identity: output == input bit for bit on finite rows; -0 as the rule gives it ((1 * -0 + 0 * y) + 0 * z) + 0 = +0
    ident = np.eye(4, dtype=f32)
    assert np.array_equal(_bits(capi.scene_place_rows(ident, rows)), _bits(rows))
    neg0 = np.zeros((1, 12), f32)
    neg0[0, [0, 8]] = -0.0
    got = capi.scene_place_rows(ident, neg0)
    assert np.array_equal(_bits(got), _bits(sr.place_rows(ident, neg0))) and _bits(got)[0, 0] == 0 and _bits(got)[0, 8] == 0
    # in place, and n == 0
    L = capi.load()
    buf = rows[:8].copy()
    p12 = sr.pose12(pose)
    assert L.sm_scene_place_rows(p12.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), 8, buf.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(_bits(buf), _bits(sr.place_rows(pose, rows[:8])))
    assert L.sm_scene_place_rows(p12.ctypes.data_as(C.c_void_p), None, 0, None) == 0
    assert L.sm_scene_place_rows(None, None, 0, None) == capi.SM_E_ARG


def test_scene_arguments_are_rejected_before_any_device_call(tmp_path):
    """with a NULL context: a scene the checks refuse is named in the message; one they accept gets as far as "null context" """
    from surfelmapping_amd import capi
    L = capi.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    good = write_map(tmp_path / "good.bin", sr.actor_box(5))
    short = str(tmp_path / "short.bin")
    with open(short, "wb") as f:
        f.write(open(good, "rb").read()[:-4])
    big, big2 = str(tmp_path / "big.bin"), str(tmp_path / "big2.bin")   # 2^21 + 1 records each (sparse files: only the headers are written)
    for path in (big, big2):
        with open(path, "wb") as f:
            f.write(np.array([(1 << 21) + 1, 0, 0], np.uint32).tobytes())
            f.truncate(12 + 48 * ((1 << 21) + 1))
    I = np.stack([sr.rigid(0, 0, 5), sr.rigid(1, 0, 6, 30.0)])
    nan = I.copy(); nan[1, 3] = np.nan
    inf = I.copy(); inf[0, 0] = np.inf
    scaled = I.copy(); scaled[1, [0, 2, 8, 10]] *= f32(1.002)         # R^T R - I = 4e-3
    at_limit = I.copy(); at_limit[1, [0, 2, 8, 10]] *= f32(1.0004)    # 8e-4: allowed
    mirror = I.copy(); mirror[0, 5] = -1.0
    src = capi.map_source([])
    sn = capi.lidar_sensor()
    buf = np.zeros(1 << 16, np.uint8)
    views = np.tile(np.eye(4, dtype=f32).reshape(16), (2, 1))

    def calls(sc):
        yield "sm_render_image_scene", L.sm_render_image_scene(None, C.byref(src), sc, vp(views), 2, 8, 8, 5.0, 5.0, 4.0, 4.0, None, vp(buf), vp(buf), None)
        yield "sm_lidar_sweep_scene", L.sm_lidar_sweep_scene(None, C.byref(src), sc, C.byref(sn), vp(views), 2, vp(buf), None, None, None)

    def expect(actors, rc, text):
        sc = capi.scene(actors)
        for fn, got in calls(C.byref(sc)):
            msg = L.sm_last_error().decode()
            assert got == rc and text in msg and fn in msg, (fn, got, msg)

    E, CAP = capi.SM_E_ARG, capi.SM_E_CAPACITY
    expect([(good, I)], E, "null context")                             # a good scene: only the context is missing
    expect([], E, "null context")
    for fn, got in calls(None):
        assert got == E and "null context" in L.sm_last_error().decode()
    expect([(good, nan)], E, "non-finite pose")
    expect([(good, inf)], E, "non-finite pose")
    expect([(good, nan, [1, 0])], E, "null context")                   # rows of absent views are not read
    expect([(good, scaled)], E, "not orthonormal")
    expect([(good, scaled, [1, 0])], E, "null context")
    expect([(good, at_limit)], E, "null context")
    expect([(good, mirror)], E, "not orthonormal")
    expect([(good, I), (short, I)], E, "short.bin")
    expect([(good, I), (str(tmp_path / "missing.bin"), I)], E, "missing.bin")
    expect([(good, I)] * 4096, E, "null context")
    expect([(good, I)] * 4097, CAP, "4097 actors")
    expect([(big, I), (big, I), (good, I)], E, "null context")        # one resident copy: 2^21 + 6 records
    expect([(big, I), (big2, I)], CAP, "records")                      # two distinct files: 2^22 + 2
    # NULL members
    sc = capi.scene([(good, I)])
    sc.actors[0].path = None
    for fn, got in calls(C.byref(sc)):
        assert got == E and "null path" in L.sm_last_error().decode()
    sc = capi.scene([(good, I)])
    sc.actors[0].poses12 = None
    for fn, got in calls(C.byref(sc)):
        assert got == E and "null poses12" in L.sm_last_error().decode()
    sc = capi.SmScene(None, 3)
    for fn, got in calls(C.byref(sc)):
        assert got == E and "null actors" in L.sm_last_error().decode()
    st = capi.SmSceneStats()
    assert L.sm_scene_stats(None, C.byref(st)) == E


def test_the_restatements_own_arithmetic():
    # ids: an absent actor, a 0-record actor and a shared file all keep their places
    assert sr.id_bases(1000, [600, 1, 0, 600, 600]) == [1000, 1600, 1601, 1601, 2201]
    static = np.arange(36, dtype=f32).reshape(3, 12)
    A = np.ones((2, 12), f32); B = np.full((1, 12), 2, f32); Z = np.zeros((0, 12), f32)
    I2 = np.stack([sr.rigid(0, 0, 0), sr.rigid(10, 0, 0)])
    actors = [(A, I2, np.array([1, 0], np.uint8)), (Z, I2, None), (B, I2, None), (A, I2, None)]
    rows0, ids0 = sr.scene_rows(static, actors, 0)
    rows1, ids1 = sr.scene_rows(static, actors, 1)
    assert ids0.tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and ids1.tolist() == [0, 1, 2, 5, 6, 7]
    assert len(rows0) == 8 and len(rows1) == 6
    assert np.array_equal(rows0[:3], static) and np.array_equal(rows0[3:5], A) and np.array_equal(rows0[5], B[0])
    # view 1: the placed rows moved by 10 along x, nothing else
    assert np.array_equal(rows1[3], np.array([12, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2], f32)) and np.array_equal(rows1[4, 1:], A[0, 1:]) and rows1[4, 0] == 11
    # a yaw of 90 degrees takes +z to +x, for centres and normals alike
    r = np.zeros((1, 12), f32); r[0, 2] = 2; r[0, 10] = 1
    out = sr.place_rows(sr.rigid(5, 6, 7, 90.0), r)
    assert np.allclose(out[0, 0:3], [7, 6, 7], atol=1e-6) and np.allclose(out[0, 8:11], [1, 0, 0], atol=1e-6)
    # pose forms
    M = np.eye(4, dtype=f32); M[:3, 3] = (1, 2, 3)
    assert np.array_equal(sr.pose12(M), sr.rigid(1, 2, 3))
    # S_i built with the library's own placement (sm_scene_place_rows) is the restatement's, bit for bit
    from surfelmapping_amd import capi
    rng = np.random.default_rng(5)
    static = rng.normal(0, 20, (7, 12)).astype(f32)
    P, Q = rng.normal(0, 3, (300, 12)).astype(f32), rng.normal(0, 3, (1, 12)).astype(f32)
    poses = np.stack([sr.rigid(3.5, -1.25, 40.0, 33.0), sr.rigid(-7.0, 0.5, 12.0, -120.0), sr.rigid(0.1, 0.2, 0.3, 5.0)])
    actors = [(P, poses, np.array([1, 0, 1], np.uint8)), (Z, poses, None), (Q, poses[::-1], None), (P, poses[[1, 2, 0]], np.array([0, 1, 1], np.uint8))]
    bases = sr.id_bases(len(static), [300, 0, 1, 300])
    for i in range(3):
        parts, ids = [static], [np.arange(7)]
        for (rows, ps, present), base in zip(actors, bases):
            if present is None or present[i]:
                parts.append(capi.scene_place_rows(ps[i], rows))
                ids.append(base + np.arange(len(rows)))
        want_rows, want_ids = sr.scene_rows(static, actors, i)
        assert np.array_equal(_bits(np.concatenate(parts)), _bits(want_rows)) and np.array_equal(np.concatenate(ids), want_ids), i


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _gpu(cap=440):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=cap))


def _sensor(**over):
    from surfelmapping_amd import capi
    return capi.lidar_sensor(**dict(STREET, **over))


class World:
    """the shared scenario on disk, a context without a model, and the references by the EXISTING entry points"""

    def __init__(self, d):
        import oracle_lib as ol
        self.dir = d
        self.seq = rr.sequence(10)
        cpu = ol.Oracle(ol.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=440))
        for fr in self.seq:
            cpu.process_frame(*fr)
        S = sr.street_setup(cpu.download_model(), [fr[3] for fr in self.seq])
        self.static_rows = S["static"]
        self.static = [write_map(d / f"static_{i}.bin", r) for i, r in enumerate(S["static"])]
        self.A = sum(len(r) for r in S["static"])
        self.views = S["views"]
        self.rows = {n: r for n, r, _, _ in S["actors"]}
        self.files = {n: write_map(d / f"actor_{n}.bin", r) for n, r in self.rows.items()}
        self.actors = S["actors"]                        # (name, rows, poses, present)
        self.ctx = _gpu()
        self.n = 0

    def call_actors(self, actors=None):
        return [(self.files[n], p, pr) for n, _, p, pr in (self.actors if actors is None else actors)]

    def placed_files(self, actors, view, place=None):
        """the files of S_i behind the static ones, and the scene id of every row of the concatenation"""
        paths, ids = [], [np.arange(self.A, dtype=np.int64)]
        bases = sr.id_bases(self.A, [len(r) for _, r, _, _ in actors])
        for (name, rows, poses, present), base in zip(actors, bases):
            if present is not None and not present[view]:
                continue
            self.n += 1
            path = str(self.dir / f"placed_{self.n}.bin")
            if place is None:
                write_map(path, sr.place_rows(poses[view], rows))
            else:
                place(write_map(path, rows), poses[view])
            paths.append(path)
            ids.append(base + np.arange(len(rows), dtype=np.int64))
        return paths, np.concatenate(ids)

    def ref_images(self, actors, views, fill, place=None, static=None):
        static = self.static if static is None else static
        out = [self.ctx.render_image_maps(static + self.placed_files(actors, i, place)[0], views[i:i + 1], *IMG, include_model=False, fill=fill, depth=True)
               for i in range(len(views))]
        return tuple(np.concatenate([o[k] for o in out]) for k in range(3))

    def ref_sweeps(self, actors, poses, sn, place=None):
        out = []
        for i in range(len(poses)):
            paths, ids = self.placed_files(actors, i, place)
            o = self.ctx.lidar_sweep_maps(self.static + paths, poses[i:i + 1], sn, include_model=False)
            o["id"] = np.where(o["id"] >= 0, ids[np.maximum(o["id"], 0)], -1).astype(np.int32)
            out.append(o)
        return {k: np.concatenate([o[k] for o in out]) for k in LIDAR_PLANES}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("scene"))
    yield w
    w.ctx.close()


def _same_sweeps(got, want, what):
    for k in LIDAR_PLANES:
        same(got[k], want[k], f"{what}: {k}")


@pytest.mark.gpu
def test_every_view_equals_the_existing_entry_points(world):
    """the definition, fill off and on, depth on; the lidar planes with the ids of the id rule"""
    w = world
    sn = _sensor()
    for fill in (None, True):
        want = w.ref_images(w.actors, w.views, fill)
        got = w.ctx.render_scene(w.static, w.call_actors(), w.views, *IMG, include_model=False, fill=fill, depth=True)
        for k, name in enumerate(("bgr", "sem", "depth_mm")):
            same(got[k], want[k], f"fill {fill}: {name}")
        st = w.ctx.scene_stats()
        print(f"fill {fill}: scene stats {st}")
        assert st["actors"] == 5 and st["files"] == 3 and st["records"] == 601 and st["pairs_tested"] == 3 * 3 + 2 * 1 + 2 * 3 + 2 * 3
        ms = w.ctx.render_maps_stats()
        assert ms["passes"] == 1 and ms["chunks"] == 2 and ms["surfels_read"] == w.A
    # without fill and depth: the plain form of the call
    same(w.ctx.render_scene(w.static, w.call_actors(), w.views, *IMG, include_model=False)[0], w.ref_images(w.actors, w.views, None)[0], "plain: bgr")
    want = w.ref_sweeps(w.actors, w.views, sn)
    got = w.ctx.lidar_sweep_scene(w.static, w.call_actors(), w.views, sn, include_model=False)
    _same_sweeps(got, want, "lidar")
    assert (want["id"] >= w.A).any(axis=(1, 2)).all() and (want["id"] < w.A).any() and (want["id"] == -1).any()
    assert w.ctx.lidar_stats()["passes"] == 1 and w.ctx.lidar_stats()["surfels"] == w.A

    # ---- what the inputs must show, asserted on the references
    sem = w.ref_images(w.actors, w.views, None)[1]
    base = w.ctx.render_image_maps(w.static, w.views, *IMG, include_model=False)[1]
    hidden_partly = hides = False
    for j, a in enumerate(w.actors):
        name, rows, poses, present = a
        if not len(rows):
            continue
        for i in range(len(w.views)):
            if present is not None and not present[i]:
                continue
            one = [(name, rows, poses[i:i + 1], None)]
            with_static = w.ref_images(one, w.views[i:i + 1], None)[1][0]
            alone = w.ref_images(one, w.views[i:i + 1], None, static=[])[1][0]
            n_with, n_alone = int((with_static == ACTOR_SEM).sum()), int((alone == ACTOR_SEM).sum())
            print(f"actor {j} ({name}) view {i}: {n_with} pixels, {n_alone} drawn alone")
            assert n_with >= 50
            hidden_partly |= n_with < n_alone
            hides |= bool(((base[i] > 0) & (with_static == ACTOR_SEM)).any())
    assert hidden_partly and hides
    assert (base != ACTOR_SEM).all() and (sem == ACTOR_SEM).any(axis=(1, 2)).all()


@pytest.mark.gpu
def test_rows_placed_by_the_warp_itself_give_the_same_views(world):
    """the expectation's files are moved by sm_warp_by_time (t0 = 0, a one-row table) instead of numpy"""
    w = world
    mover = _gpu()

    def place(path, pose):
        mover.warp_by_time([path], 0, sr.pose12(pose).reshape(1, 12), include_model=False)
        assert mover.warp_stats()["records_moved"] == (os.path.getsize(path) - 12) // 48

    try:
        want = w.ref_images(w.actors, w.views, True, place)
        got = w.ctx.render_scene(w.static, w.call_actors(), w.views, *IMG, include_model=False, fill=True, depth=True)
        for k, name in enumerate(("bgr", "sem", "depth_mm")):
            same(got[k], want[k], name)
        sn = _sensor()
        _same_sweeps(w.ctx.lidar_sweep_scene(w.static, w.call_actors(), w.views, sn, include_model=False), w.ref_sweeps(w.actors, w.views, sn, place), "lidar")
    finally:
        mover.close()


@pytest.mark.gpu
def test_ties_go_to_the_earlier_source(world):
    w = world
    sn = _sensor()
    # an actor that IS a part of the static set (identity pose), in another colour and class: the static colour wins every pixel
    twin = w.static_rows[1][:900].copy()
    twin[:, 4] = w.rows["P"][0, 4]
    twin_path = write_map(w.dir / "twin.bin", twin)
    ident = np.tile(sr.rigid(0, 0, 0), (len(w.views), 1))
    base = w.ctx.render_image_maps(w.static, w.views, *IMG, include_model=False, depth=True)
    got = w.ctx.render_scene(w.static, [(twin_path, ident)], w.views, *IMG, include_model=False, depth=True)
    for k in range(3):
        same(got[k], base[k], f"twin: plane {k}")
    alone = w.ctx.render_scene([], [(twin_path, ident)], w.views, *IMG, include_model=False)
    assert (alone[1] == ACTOR_SEM).sum() > 500                            # (the twin is in view: drawn alone it shows)
    lb = w.ctx.lidar_sweep_maps(w.static, w.views, sn, include_model=False)
    _same_sweeps(w.ctx.lidar_sweep_scene(w.static, [(twin_path, ident)], w.views, sn, include_model=False), lb, "twin lidar")
    # two instances of P at one pose: the earlier one's ids
    name, rows, poses, _ = w.actors[0]
    got = w.ctx.lidar_sweep_scene(w.static, [(w.files["P"], poses), (w.files["P"], poses)], w.views, sn, include_model=False)
    ids = got["id"]
    assert ((ids >= w.A) & (ids < w.A + 600)).sum() > 30 and not (ids >= w.A + 600).any()
    one = w.ctx.lidar_sweep_scene(w.static, [(w.files["P"], poses)], w.views, sn, include_model=False)
    _same_sweeps(got, one, "two instances at one pose")
    a = w.ctx.render_scene(w.static, [(w.files["P"], poses), (w.files["P"], poses)], w.views, *IMG, include_model=False, depth=True)
    b = w.ctx.render_scene(w.static, [(w.files["P"], poses)], w.views, *IMG, include_model=False, depth=True)
    for k in range(3):
        same(a[k], b[k], f"two instances: plane {k}")


@pytest.mark.gpu
def test_one_view_per_pass_gives_the_same_planes(world, monkeypatch):
    """1 MiB of keys holds one view of 624 x 188 (8 bytes a pixel) and one sweep of 1100 x 64 beams: three passes over the two
    static files (one chunk each; test_chunked_static_files_and_one_view_per_pass has more), the actors drawn once per pass under that
    pass's poses"""
    w = world
    big = (624, 188, 360.0, 360.0, 311.5, 93.5)
    want = w.ctx.render_scene(w.static, w.call_actors(), w.views, *big, include_model=False, fill=True, depth=True)
    assert w.ctx.render_maps_stats()["passes"] == 1
    assert (want[1] == ACTOR_SEM).any(axis=(1, 2)).all()
    monkeypatch.setenv("SM_RENDER_MAPS_KEY_MB", "1")
    got = w.ctx.render_scene(w.static, w.call_actors(), w.views, *big, include_model=False, fill=True, depth=True)
    st = w.ctx.render_maps_stats()
    assert st["passes"] == 3 and st["chunks"] == 6
    for k in range(3):
        same(got[k], want[k], f"plane {k}")
    # the last view alone, by the existing entry point (its pose row is the third of every actor's)
    ref = w.ctx.render_image_maps(w.static + w.placed_files(w.actors, 2)[0], w.views[2:3], *big, include_model=False, fill=True, depth=True)
    for k in range(3):
        same(got[k][2:3], ref[k], f"view 2: plane {k}")
    step = f32(360.0 / 1100)
    if step * 1100 > 360:
        step = np.nextafter(step, f32(0))
    sn = _sensor(n_az=1100, az0_deg=-180.0, az_step_deg=float(step), el_deg=np.linspace(-24.0, 2.0, 64).astype(f32))
    want = w.ctx.lidar_sweep_scene(w.static, w.call_actors(), w.views, sn, include_model=False)
    assert w.ctx.lidar_stats()["passes"] == 1 and (want["id"] >= w.A).any(axis=(1, 2)).all()
    monkeypatch.setenv("SM_LIDAR_KEY_MB", "1")
    got = w.ctx.lidar_sweep_scene(w.static, w.call_actors(), w.views, sn, include_model=False)
    assert w.ctx.lidar_stats()["passes"] == 3
    _same_sweeps(got, want, "lidar")


@pytest.mark.gpu
def test_actors_outside_every_view_are_skipped_and_change_nothing(world, monkeypatch):
    w = world
    sn = _sensor()
    V = len(w.views)
    far = [("P", w.rows["P"], np.stack([sr.rigid(0.0, 0.9, float(v[14]) - 40.0, 15.0) for v in w.views]), None),      # behind every camera
           ("P", w.rows["P"], np.stack([sr.rigid(700.0, 0.9, float(v[14]) + 10.0) for v in w.views]), None)]          # far to the side, out of range
    actors = w.actors + far
    img = w.ctx.render_scene(w.static, w.call_actors(actors), w.views, *IMG, include_model=False, fill=True, depth=True)
    st = w.ctx.scene_stats()
    print("image:", st)
    assert st["pairs_skipped"] >= 2 * 3 * V and st["pairs_tested"] == 23 + 2 * 3 * V
    near = w.ctx.render_scene(w.static, w.call_actors(), w.views, *IMG, include_model=False, fill=True, depth=True)
    sweep = w.ctx.lidar_sweep_scene(w.static, w.call_actors(actors), w.views, sn, include_model=False)
    st = w.ctx.scene_stats()
    print("lidar:", st)
    assert st["pairs_skipped"] >= 3 * V                                   # (the one behind the camera is in the lidar's range)
    monkeypatch.setenv("SM_SCENE_NO_CULL", "1")
    img2 = w.ctx.render_scene(w.static, w.call_actors(actors), w.views, *IMG, include_model=False, fill=True, depth=True)
    st = w.ctx.scene_stats()
    assert st["pairs_skipped"] == 0 and st["pairs_tested"] == 0
    sweep2 = w.ctx.lidar_sweep_scene(w.static, w.call_actors(actors), w.views, sn, include_model=False)
    assert w.ctx.scene_stats()["pairs_skipped"] == 0
    for k in range(3):
        same(img[k], img2[k], f"cull / no cull: plane {k}")
        same(img[k], near[k], f"far actors: plane {k}")
    _same_sweeps(sweep, sweep2, "cull / no cull")
    assert not (sweep["id"] >= w.A + 1801 + 600).any() and (sweep["id"] >= w.A + 1801).any()     # the one behind is seen by the lidar, the far one is not


@pytest.mark.gpu
def test_discs_close_to_the_sensor_take_the_wide_path(world):
    """Q, a disc of 0.45 m, 1.5 m in front of the sensor: its footprint on the 2-degree grid is far above the 64 beams a lane
    tests by itself; in the image it covers thousands of pixels"""
    w = world
    sn = _sensor()
    poses = np.stack([sr.rigid(0.1, 0.25, float(v[14]) + 1.5) for v in w.views])
    actors = [("Q", w.rows["Q"], poses, None), ("P", w.rows["P"], w.actors[0][2], None)]
    want = w.ref_sweeps(actors, w.views, sn)
    n_q = (want["id"] == w.A).sum(axis=(1, 2))
    print("beams on Q per sweep:", n_q)
    assert (n_q > 64).all()
    _same_sweeps(w.ctx.lidar_sweep_scene(w.static, w.call_actors(actors), w.views, sn, include_model=False), want, "lidar")
    want = w.ref_images(actors, w.views, True)
    assert ((want[1] == ACTOR_SEM).sum(axis=(1, 2)) > 3000).all()
    got = w.ctx.render_scene(w.static, w.call_actors(actors), w.views, *IMG, include_model=False, fill=True, depth=True)
    for k in range(3):
        same(got[k], want[k], f"image plane {k}")


@pytest.mark.gpu
def test_hostile_actor_rows(world):
    """NaN / inf centres, normals and radii, zero normals, an actor behind the camera: equal to the reference, and no pixel
    changes but those the good rows of the actor take"""
    w = world
    sn = _sensor()
    H = w.rows["P"][:300].copy()
    bad = np.array([np.nan, np.inf, -np.inf], f32)
    for k in range(120):
        H[k, [0, 1, 2, 8, 9, 10, 11][k % 7]] = bad[k % 3]
    H[120:140, 8:11] = 0.0                                                  # zero normals
    H[140:150, 11] = [0.0, -0.12, 1e-30, 3e38, -3e38, 1e19, 1e-45, 0.5, 2.0, -0.0]
    h_path = write_map(w.dir / "hostile.bin", H)
    w.files["H"] = h_path
    behind = np.stack([sr.rigid(0.0, 0.9, float(v[14]) - 6.0) for v in w.views])
    actors = [("H", H, w.actors[0][2], None), ("P", w.rows["P"], behind, None)]
    want = w.ref_images(actors, w.views, None)
    got = w.ctx.render_scene(w.static, w.call_actors(actors), w.views, *IMG, include_model=False, depth=True)
    for k in range(3):
        same(got[k], want[k], f"image plane {k}")
    base = w.ctx.render_image_maps(w.static, w.views, *IMG, include_model=False, depth=True)
    changed = (got[0] != base[0]).any(axis=3) | (got[1] != base[1]) | (got[2] != base[2])
    assert changed.any() and (got[1][changed] == ACTOR_SEM).all()
    wl = w.ref_sweeps(actors, w.views, sn)
    gl = w.ctx.lidar_sweep_scene(w.static, w.call_actors(actors), w.views, sn, include_model=False)
    _same_sweeps(gl, wl, "lidar")
    bl = w.ctx.lidar_sweep_maps(w.static, w.views, sn, include_model=False)
    changed = gl["range"].view(np.uint32) != bl["range"].view(np.uint32)
    assert changed.any() and (gl["id"][changed] >= w.A).all() and (gl["id"][~changed] == bl["id"][~changed]).all()


@pytest.mark.gpu
def test_live_model_takes_part(world):
    """include_model = 1 after three fused frames: the static files, the live model, the actors -- against a context that holds
    the concatenation"""
    w = world
    sn = _sensor()
    live = _gpu()
    big = _gpu()
    try:
        for fr in w.seq[:3]:
            live.process_frame(*fr)
        model = live.download_model()
        assert len(model) > 10000
        before = live.counts()
        static = np.concatenate(list(w.static_rows) + [model])
        A = len(static)
        got = live.render_scene(w.static, w.call_actors(), w.views, *IMG, include_model=True, fill=True, depth=True)
        gl = live.lidar_sweep_scene(w.static, w.call_actors(), w.views, sn, include_model=True)
        assert live.counts() == before
        acts = [(r, p, pr) for _, r, p, pr in w.actors]
        saw_model = saw_actor = False
        for i in range(len(w.views)):
            rows, ids = sr.scene_rows(static, acts, i)
            big.upload_model(rows)
            want = big.render_image(w.views[i], *IMG, fill=True, depth=True)
            for k in range(3):
                same(got[k][i], want[k], f"view {i}: plane {k}")
            wl = big.lidar_sweep(w.views[i], sn)
            wl["id"] = np.where(wl["id"] >= 0, ids[np.maximum(wl["id"], 0)], -1).astype(np.int32)
            _same_sweeps({k: gl[k][i] for k in LIDAR_PLANES}, wl, f"sweep {i}")
            saw_model |= bool(((wl["id"] >= w.A) & (wl["id"] < A)).any())
            saw_actor |= bool((wl["id"] >= A).any())
        assert saw_model and saw_actor
    finally:
        live.close()
        big.close()


@pytest.mark.gpu
def test_empty_scene_is_the_maps_call(world):
    from surfelmapping_amd import capi
    w = world
    sn = _sensor()
    want = w.ctx.render_image_maps(w.static, w.views, *IMG, include_model=False, fill=True, depth=True)
    got = w.ctx.render_scene(w.static, [], w.views, *IMG, include_model=False, fill=True, depth=True)
    for k in range(3):
        same(got[k], want[k], f"plane {k}")
    ms, fs, ss = w.ctx.render_maps_stats(), w.ctx.fill_stats(), w.ctx.scene_stats()
    assert ms["passes"] == 1 and ms["chunks"] == 2 and ms["surfels_read"] == w.A and fs["launches"] > 0 and fs["filled"] > 0
    assert ss["actors"] == 0 and ss["records"] == 0 and ss["pairs_tested"] == 0
    _same_sweeps(w.ctx.lidar_sweep_scene(w.static, [], w.views, sn, include_model=False), w.ctx.lidar_sweep_maps(w.static, w.views, sn, include_model=False), "lidar")
    assert w.ctx.lidar_stats()["surfels"] == w.A and w.ctx.scene_stats()["actors"] == 0
    # scene == NULL
    L, vp = capi.load(), lambda a: a.ctypes.data_as(C.c_void_p)
    src = capi.map_source(w.static, False)
    bgr, sem = np.zeros_like(want[0]), np.zeros_like(want[1])
    views = np.ascontiguousarray(w.views, f32)
    assert L.sm_render_image_scene(w.ctx._h, C.byref(src), None, vp(views), len(views), *IMG, None, vp(bgr), vp(sem), None) == 0
    plain = w.ctx.render_image_maps(w.static, w.views, *IMG, include_model=False)
    same(bgr, plain[0], "NULL scene: bgr")
    same(sem, plain[1], "NULL scene: sem")
    # an actor of 0 records alone, and n_views == 0
    z = [(w.files["Z"], w.actors[2][2], None)]
    same(w.ctx.render_scene(w.static, z, w.views, *IMG, include_model=False)[0], plain[0], "Z alone")
    _same_sweeps(w.ctx.lidar_sweep_scene(w.static, z, w.views, sn, include_model=False), w.ctx.lidar_sweep_maps(w.static, w.views, sn, include_model=False), "Z alone, lidar")
    none = [(w.files["P"], np.zeros((0, 12), f32))]
    assert w.ctx.render_scene(w.static, none, np.zeros((0, 16), f32), *IMG, include_model=False)[0].shape == (0, CAM["height"], CAM["width"], 3)
    assert w.ctx.lidar_sweep_scene(w.static, none, np.zeros((0, 16), f32), sn, include_model=False)["range"].shape == (0, 8, 180)


@pytest.mark.gpu
def test_a_bad_actor_file_leaves_the_outputs_unwritten(world):
    from surfelmapping_amd import capi
    w = world
    L, vp = capi.load(), lambda a: a.ctypes.data_as(C.c_void_p)
    short = str(w.dir / "short_actor.bin")
    with open(short, "wb") as f:
        f.write(open(w.files["P"], "rb").read()[:-8])
    sc = capi.scene([(w.files["P"], w.actors[0][2]), (short, w.actors[0][2])], 3)
    src = capi.map_source(w.static, False)
    views = np.ascontiguousarray(w.views, f32)
    bgr, sem = np.full((3, CAM["height"], CAM["width"], 3), 7, np.uint8), np.full((3, CAM["height"], CAM["width"]), 7, np.uint8)
    rc = L.sm_render_image_scene(w.ctx._h, C.byref(src), C.byref(sc), vp(views), 3, *IMG, None, vp(bgr), vp(sem), None)
    assert rc == capi.SM_E_ARG and b"short_actor.bin" in L.sm_last_error() and (bgr == 7).all() and (sem == 7).all()
    # the set's own files are checked too, with the actors', before any work
    bad_src = capi.map_source(w.static + [str(w.dir / "missing_static.bin")], False)
    good = capi.scene(w.call_actors(), 3)
    rc = L.sm_render_image_scene(w.ctx._h, C.byref(bad_src), C.byref(good), vp(views), 3, *IMG, None, vp(bgr), vp(sem), None)
    assert rc == capi.SM_E_ARG and b"missing_static.bin" in L.sm_last_error() and (bgr == 7).all()


def _ahead(view16, d, side=0.0, y=0.9, yaw=0.0):
    """a pose `d` metres in front of the camera of `view16` (and `side` to its right), turned by yaw against it"""
    v = np.asarray(view16, np.float64).reshape(4, 4).T                      # camera -> world
    p = v[:3, 3] + d * v[:3, 2] + side * v[:3, 0]
    cam_yaw = np.degrees(np.arctan2(v[0, 2], v[2, 2]))
    return sr.rigid(p[0], y, p[2], cam_yaw + yaw)


@pytest.mark.gpu
def test_chunked_static_files_and_one_view_per_pass(world, tmp_path, monkeypatch):
    """a static file of 2^20 + 70001 records streams as two chunks (test_render_maps.py's way to chunk: the chunk size is fixed),
    a small one follows: ids A + off_j + r with A spanning three chunks, the actors drawn once per batch after the last chunk;
    then 1 MiB of keys, one view per pass: three passes over three chunks.  Against the existing calls over the placed files."""
    from surfelmapping_amd import synth
    w = world
    n0, n2 = (1 << 20) + 70001, 12345
    rows = synth.seeded_model(n0 + n2, 50, seed=4)
    static = [write_map(tmp_path / "a.bin", rows[:n0]), write_map(tmp_path / "c.bin", rows[n0:])]
    A = n0 + n2
    P = synth.pose_matrix
    views = np.stack([synth.pose_to_colmajor(p) for p in (P(0, 0, 0), P(10, 0, 100, 40.0), P(5, 0, 50, 10.0))])
    actors = [("P", w.rows["P"], np.stack([_ahead(v, 9.0, -1.5, yaw=20.0 * i) for i, v in enumerate(views)]), None),
              ("Q", w.rows["Q"], np.stack([_ahead(v, 4.0, 1.0, y=0.3) for v in views]), np.array([1, 1, 0], np.uint8)),
              ("Z", w.rows["Z"], np.stack([_ahead(v, 5.0) for v in views]), None),
              ("P", w.rows["P"], np.stack([_ahead(v, 15.0, 2.5, yaw=-30.0) for v in views]), np.array([0, 1, 1], np.uint8))]
    call = [(w.files[n], p, pr) for n, _, p, pr in actors]
    bases = sr.id_bases(A, [len(r) for _, r, _, _ in actors])

    def placed(i):
        paths, ids = [], [np.arange(A, dtype=np.int64)]
        for j, ((name, r, poses, present), base) in enumerate(zip(actors, bases)):
            if present is None or present[i]:
                paths.append(write_map(tmp_path / f"placed_{i}_{j}.bin", sr.place_rows(poses[i], r)))
                ids.append(base + np.arange(len(r), dtype=np.int64))
        return paths, np.concatenate(ids)

    big = (624, 188, 360.0, 360.0, 311.5, 93.5)
    ref = [w.ctx.render_image_maps(static + placed(i)[0], views[i:i + 1], *big, include_model=False, fill=True, depth=True) for i in range(3)]
    want = tuple(np.concatenate([o[k] for o in ref]) for k in range(3))
    base = w.ctx.render_image_maps(static, views, *big, include_model=False, fill=True, depth=True)
    changed = (want[2] != base[2]).sum(axis=(1, 2))                          # (the seeded records have every class: the actors show in the depth)
    print("pixels the actors change per view:", changed, "of", int((base[1] > 0).sum()), "drawn")
    assert (changed > 500).all() and (base[1] > 0).any(axis=(1, 2)).all()
    got = w.ctx.render_scene(static, call, views, *big, include_model=False, fill=True, depth=True)
    st = w.ctx.render_maps_stats()
    assert st["passes"] == 1 and st["chunks"] == 3 and st["chunks"] > len(static) and st["surfels_read"] == A
    for k in range(3):
        same(got[k], want[k], f"one pass: plane {k}")
    monkeypatch.setenv("SM_RENDER_MAPS_KEY_MB", "1")
    got = w.ctx.render_scene(static, call, views, *big, include_model=False, fill=True, depth=True)
    st = w.ctx.render_maps_stats()
    assert st["passes"] == 3 and st["chunks"] == 9 and st["surfels_read"] == 3 * A
    for k in range(3):
        same(got[k], want[k], f"three passes: plane {k}")

    step = f32(360.0 / 1100)
    if step * 1100 > 360:
        step = np.nextafter(step, f32(0))
    sn = _sensor(n_az=1100, az0_deg=-180.0, az_step_deg=float(step), el_deg=np.linspace(-24.0, 2.0, 64).astype(f32))
    ref = []
    for i in range(3):
        paths, ids = placed(i)
        o = w.ctx.lidar_sweep_maps(static + paths, views[i:i + 1], sn, include_model=False)
        o["id"] = np.where(o["id"] >= 0, ids[np.maximum(o["id"], 0)], -1).astype(np.int32)
        ref.append(o)
    want = {k: np.concatenate([o[k] for o in ref]) for k in LIDAR_PLANES}
    assert (want["id"] >= A).any(axis=(1, 2)).all() and (want["id"] >= n0).any() and ((want["id"] >= 0) & (want["id"] < (1 << 20))).any()
    assert ((want["id"] >= (1 << 20)) & (want["id"] < n0)).any()            # returns from each of the three chunks and from the actors
    got = w.ctx.lidar_sweep_scene(static, call, views, sn, include_model=False)
    st = w.ctx.lidar_stats()
    assert st["passes"] == 1 and st["chunks"] == 3
    _same_sweeps(got, want, "one pass")
    monkeypatch.setenv("SM_LIDAR_KEY_MB", "1")
    got = w.ctx.lidar_sweep_scene(static, call, views, sn, include_model=False)
    st = w.ctx.lidar_stats()
    assert st["passes"] == 3 and st["chunks"] == 9
    _same_sweeps(got, want, "three passes")


@pytest.mark.gpu
def test_the_last_of_4096_actors_is_found(world):
    """SM_SCENE_MAX_ACTORS instances of Q, three of them present -- the first, one in the middle, the last: the searches over the
    first workgroups and over the id bases reach every index"""
    w = world
    sn = _sensor()
    V = len(w.views)
    spots = {0: (-1.5, 3.0), 2047: (0.0, 4.0), 4095: (1.5, 5.0)}
    absent, nowhere = np.zeros(V, np.uint8), np.tile(sr.rigid(0, 0, 0), (V, 1))
    many, few = [], []
    for j in range(4096):
        if j in spots:
            side, d = spots[j]
            a = (w.files["Q"], np.stack([_ahead(v, d, side, y=0.3) for v in w.views]), None)
            few.append(a)
        else:
            a = (w.files["Q"], nowhere, absent)
        many.append(a)
    got = w.ctx.lidar_sweep_scene(w.static, many, w.views, sn, include_model=False)
    st = w.ctx.scene_stats()
    assert st["actors"] == 4096 and st["files"] == 1 and st["records"] == 1 and st["pairs_tested"] == 3 * V
    want = w.ctx.lidar_sweep_scene(w.static, few, w.views, sn, include_model=False)
    remap = np.array([0, 2047, 4095])
    want["id"] = np.where(want["id"] >= w.A, w.A + remap[np.clip(want["id"] - w.A, 0, 2)], want["id"]).astype(np.int32)
    _same_sweeps(got, want, "lidar")
    for j in spots:
        assert (got["id"] == w.A + j).sum() > 2 * V, j
    a = w.ctx.render_scene(w.static, many, w.views, *IMG, include_model=False, depth=True)
    b = w.ctx.render_scene(w.static, few, w.views, *IMG, include_model=False, depth=True)
    for k in range(3):
        same(a[k], b[k], f"image plane {k}")
    assert ((a[1] == ACTOR_SEM).sum(axis=(1, 2)) > 500).all()


@pytest.mark.gpu
def test_the_id_limit_and_partial_contexts_are_refused(world, tmp_path):
    from surfelmapping_amd import capi
    w = world
    L, vp = capi.load(), lambda a: a.ctypes.data_as(C.c_void_p)
    sn = _sensor()
    views = np.ascontiguousarray(w.views, f32)
    V = len(views)
    bgr, sem = np.full((V, CAM["height"], CAM["width"], 3), 7, np.uint8), np.full((V, CAM["height"], CAM["width"]), 7, np.uint8)
    rng, ids = np.full((V, 8, 180), 7.0, f32), np.full((V, 8, 180), 7, np.int32)
    src = capi.map_source(w.static, False)

    def both(ctx, sc):
        yield L.sm_render_image_scene(ctx._h, C.byref(src), C.byref(sc), vp(views), V, *IMG, None, vp(bgr), vp(sem), None)
        yield L.sm_lidar_sweep_scene(ctx._h, C.byref(src), C.byref(sc), C.byref(sn), vp(views), V, vp(rng), vp(ids), None, None)

    # 2048 instances of a file of 2^20 records (a sparse file: only its header is written; one resident copy, within the limits)
    # take 2^31 ids: one too many, with or without the static set's
    mega = str(tmp_path / "mega.bin")
    with open(mega, "wb") as f:
        f.write(np.array([1 << 20, 0, 0], np.uint32).tobytes())
        f.truncate(12 + 48 * (1 << 20))
    poses = np.tile(sr.rigid(0, 0, 500.0), (V, 1))
    sc = capi.scene([(mega, poses)] * 2048, V)
    for rc in both(w.ctx, sc):
        assert rc == capi.SM_E_CAPACITY and b"2^31 - 1" in L.sm_last_error(), L.sm_last_error()
    assert (bgr == 7).all() and (sem == 7).all() and (rng == 7).all() and (ids == 7).all()
    # a sharded and a rig context hold only a part of the map
    good = capi.scene(w.call_actors(), V)
    for configure in ("sm_shard_stream_configure", "sm_rig_configure"):
        part = _gpu(35)
        try:
            assert getattr(L, configure)(part._h, 0, 1) == 0
            for rc in both(part, good):
                assert rc == capi.SM_E_UNSUPPORTED, (configure, rc, L.sm_last_error())
        finally:
            part.close()
    assert (bgr == 7).all() and (sem == 7).all() and (rng == 7).all() and (ids == 7).all()
