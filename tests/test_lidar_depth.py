"""Lidar depth on the GPU (include/sm_c_api.h "lidar depth"): sparse_mm, index, depth_mm and the tally of the
kernels against the numpy restatement (lidar_depth_ref.py), bit for bit; the binding's helpers; the device path into the fusion."""
import ctypes as C
import functools

import numpy as np
import pytest

import lidar_depth_ref as lr
from backends import assert_models_equal

f32 = np.float32
NEW = ("sm_default_lidar_depth_params", "sm_set_lidar_depth", "sm_lidar_depth", "sm_lidar_depth_device", "sm_lidar_depth_stats")
KITTI = lr.STREET_CAM
SHAPES = [(97, 41), (20, 9), (131, 37)]
TALLY = ("points", "landed", "measured", "filled_small", "filled_top", "filled_large", "left_empty")
I4 = np.eye(4, dtype=f32)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _cam(w, h):
    """a camera of KITTI's field of view at another size"""
    if (w, h) == (KITTI["width"], KITTI["height"]):
        return dict(KITTI)
    f = KITTI["fx"] * w / KITTI["width"]
    return dict(width=w, height=h, fx=f, fy=f, cx=w / 2 - 0.5, cy=h * 0.46)


def _gpu(w, h, **over):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**_cam(w, h), **dict(dict(max_sqrt_vertices=64), **over)))


@functools.lru_cache(maxsize=None)
def _scan(w, h):
    """the analytic street scanned with about as many beams per pixel as 64 x 1100 have at KITTI size"""
    full = (w, h) == (KITTI["width"], KITTI["height"])
    return lr.street_scan() if full else lr.street_scan(rows=max(h // 5, 3), cols=max(w, 8))


@functools.lru_cache(maxsize=None)
def _random(w, h, seed=0):
    """20 W H points in the frustum, Z one of a few millimetre values, seen through a T with a rotation: many points per pixel and
    many ties of mm, so that the lowest index has to win.  (points, T)"""
    rng = np.random.default_rng(seed + w)
    cam, n = _cam(w, h), 20 * w * h
    Z = rng.choice(np.array([2.0, 2.004, 2.0041, 7.5, 30.0]), n)
    u, v = rng.uniform(-1.0, w, n), rng.uniform(-1.0, h, n)
    pc = np.stack([(u - cam["cx"]) * Z / cam["fx"], (v - cam["cy"]) * Z / cam["fy"], Z], axis=1)
    a = np.deg2rad(4.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.1, -0.08, -0.27])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    pl = (pc - t) @ R                                                  # R^T (pc - t), row-wise
    pts = np.concatenate([pl, rng.random((n, 1))], axis=1).astype(f32)
    return pts, T.astype(f32)


def _assert_same(m, pts, T, want=None, what="", **over):
    """one call on the GPU against the restatement: the three images and the tally"""
    cam = dict(width=m.W, height=m.H, fx=m.cfg.fx, fy=m.cfg.fy, cx=m.cfg.cx, cy=m.cfg.cy)
    want = lr.lidar_depth(pts, T, cam, **over) if want is None else want
    depth, sparse, index = m.lidar_depth(pts, T)
    for name, got in (("sparse_mm", sparse), ("index", index), ("depth_mm", depth)):
        assert got.dtype == want[name].dtype and got.shape == want[name].shape, (what, name)
        bad = np.argwhere(got != want[name])
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist())
    st = m.lidar_depth_stats()
    assert {k: st[k] for k in TALLY} == {k: want["stats"][k] for k in TALLY}, what
    assert st["launches"] == (4 if over.get("stages", 127) & lr.FILL_LARGE else 3) and st["device_ms"] > 0, what
    return want


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_lidar_depth_symbols():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.sm_api_version() == 4
    assert capi.LIDAR_DEPTH_MAX_POINTS == lr.MAX_POINTS == 1 << 24
    assert C.sizeof(capi.SmLidarDepthParams) == 20 and C.sizeof(capi.SmLidarDepthStats) == 112


def test_defaults():
    from surfelmapping_amd import capi
    cfg = capi.make_config(**_cam(97, 41))
    p = capi.lidar_depth_params(cfg)
    assert (p.min_z, p.max_z, p.stages, p.large, p.tol_256) == (f32(0.5), f32(65.0), 127, 31, 13)
    assert {k: getattr(p, k) for k in lr.DEFAULT} == {k: (f32(v) if isinstance(v, float) else v) for k, v in lr.DEFAULT.items()}
    q = capi.lidar_depth_params(cfg, large=15, stages=3)
    assert (q.large, q.stages, q.tol_256) == (15, 3, 13)
    with pytest.raises(KeyError):
        capi.lidar_depth_params(cfg, window=3)


def test_null_arguments_are_rejected_before_any_device_call():
    from surfelmapping_amd import capi
    L = capi.load()
    E = capi.SM_E_ARG
    cfg = capi.make_config(**_cam(97, 41))
    p, st = capi.lidar_depth_params(cfg), capi.SmLidarDepthStats()
    pts, out = np.zeros((4, 4), f32), np.zeros(16, np.uint16)
    assert L.sm_default_lidar_depth_params(None, C.byref(p)) == E and L.sm_default_lidar_depth_params(C.byref(cfg), None) == E
    assert L.sm_set_lidar_depth(None, C.byref(p)) == E and L.sm_set_lidar_depth(None, None) == E
    assert L.sm_lidar_depth(None, _vp(pts), 4, _fp(I4), _vp(out), None, None) == E
    assert L.sm_lidar_depth_device(None, _vp(pts), 4, _fp(I4), _vp(out), None, None) == E
    assert L.sm_lidar_depth_stats(None, C.byref(st)) == E


def test_read_velodyne_and_sweep_points(tmp_path):
    from surfelmapping_amd import capi
    pts = np.arange(28, dtype=f32).reshape(7, 4) / f32(3.0)
    pts.tofile(tmp_path / "000000.bin")
    got = capi.read_velodyne(str(tmp_path / "000000.bin"))
    assert got.dtype == f32 and np.array_equal(got, pts)
    (tmp_path / "bad.bin").write_bytes(b"\0" * 20)
    with pytest.raises(ValueError):
        capi.read_velodyne(str(tmp_path / "bad.bin"))
    sensor = capi.lidar_sensor(n_az=5, az0_deg=-10.0, az_step_deg=5.0, el_deg=[-4.0, 0.0, 3.0])
    d = capi.lidar_directions(sensor)
    rng = np.arange(15, dtype=f32).reshape(3, 5) * f32(0.7)
    rng[1, 2] = 0.0                                                    # (and beam (0, 0) has range 0 already)
    p = capi.sweep_points(rng, sensor)
    keep = rng.reshape(-1) > 0
    assert p.shape == (13, 4) and p.dtype == f32 and not p[:, 3].any()
    assert np.array_equal(p[:, :3], rng.reshape(-1)[keep, None] * d.reshape(-1, 3)[keep])
    assert p[6, 2] > 0 and abs(np.linalg.norm(p[6, :3]) - rng.reshape(-1)[keep][6]) < 1e-5
    with pytest.raises(ValueError):
        capi.sweep_points(rng[:2], sensor)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: against the restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_match_restatement(w, h):
    """97 x 41: partial tiles and partial waves; 20 x 9: narrower than the 31-window and the 9-pixel halo; 131 x 37: five tiles
    across"""
    m = _gpu(w, h)
    m.set_lidar_depth()
    want = _assert_same(m, _scan(w, h), lr.T_STREET, what="scan")
    assert want["stats"]["measured"] > w * h // 40 and (want["depth_mm"] > 0).mean() > 0.9
    pts, T = _random(w, h)
    want = _assert_same(m, pts, T, what="random")
    assert want["stats"]["landed"] > 15 * w * h and want["stats"]["measured"] == w * h
    # ties: pixels whose nearest mm several points share
    sparse, index = want["sparse_mm"], want["index"]
    proj = lr.project(pts[::-1], T, _cam(w, h), 0.5, 65.0)             # the same points in reverse order: another winner where mm ties
    tied = int((len(pts) - 1 - proj[1] != index).sum())
    assert np.array_equal(proj[0], sparse) and tied > w * h // 4, tied


@pytest.mark.gpu
def test_kitti_size_once():
    w, h = KITTI["width"], KITTI["height"]
    m = _gpu(w, h)
    m.set_lidar_depth()
    want = _assert_same(m, _scan(w, h), lr.T_STREET, what="kitti")
    assert want["stats"]["left_empty"] == 0 and want["stats"]["filled_large"] > 0 and want["stats"]["filled_top"] > 0


@pytest.mark.gpu
def test_point_counts_and_edge_case_points():
    w, h = 97, 41
    cam = _cam(w, h)
    m = _gpu(w, h)
    m.set_lidar_depth()
    index = lr.project(_scan(w, h), lr.T_STREET, cam, 0.5, 65.0)[1]
    scan = _scan(w, h)[np.sort(index[index >= 0])]                     # points that land
    for n in (0, 1, 63, 64, 65):
        want = _assert_same(m, scan[:n], lr.T_STREET, what=n)
        assert want["stats"]["points"] == n and (n == 0) == (not want["depth_mm"].any())
    fx, cx, fy, cy = (f32(cam[k]) for k in ("fx", "cx", "fy", "cy"))
    nan, inf = float("nan"), float("inf")
    z = f32(2.0)
    xl = (f32(-0.5) - cx) * z / fx                                     # projects to u = -0.5, or as near as fp32 comes
    xr = (f32(w - 0.5) - cx) * z / fx
    yt = (f32(-0.5) - cy) * z / fy
    edge = np.array([
        [nan, 0, 2, 0], [0, nan, 2, 0], [0, 0, nan, 0], [inf, 0, 2, 0], [0, -inf, 2, 0], [0, 0, inf, 0],
        [0, 0, -2, 0], [0.3, 0.1, -0.5, 0], [0, 0, 0, 0],              # behind the camera, and on its plane
        [0.2, 0.1, 0.5, 0], [0.5, 0.2, 65.0, 0],                       # Z exactly min_z and max_z
        [0.2, 0.1, np.nextafter(f32(0.5), f32(0)), 0], [0.5, 0.2, np.nextafter(f32(65.0), f32(100)), 0],
        [xl, 0, z, 0], [np.nextafter(xl, f32(-10)), 0.1, z, 0], [xr, 0, z, 0], [np.nextafter(xr, f32(-10)), 0.2, z, 0],
        [0, yt, z, 0], [0, np.nextafter(yt, f32(-10)), z, 0],
        [1e30, 1e30, 1.0, 0], [3e38, 0, 1.0, 0],                       # u overflows
    ], f32)
    want = _assert_same(m, edge, I4, what="edge")
    assert 4 <= want["stats"]["landed"] < len(edge) - 9
    # mm 0 and 65536 need a range the parameters allow: min_z below half a millimetre, max_z = 65.535 with Z rounding up
    wide = dict(min_z=1e-4, max_z=65.535)
    m.set_lidar_depth(**wide)
    mm = np.array([[0, 0, 0.0004, 0], [0, 0, 0.0006, 0], [5, 0, 65.535, 0], [5, 1, 65.5354, 0], [10, 2, 65.5346, 0]], f32)
    want = _assert_same(m, mm, I4, what="mm", **wide)
    got = sorted(want["sparse_mm"][want["sparse_mm"] > 0].tolist())
    assert got == [1, 65535, 65535] and want["stats"]["landed"] == 3
    # one measured column
    m.set_lidar_depth()
    col = np.array([[0.1, (v - float(cy)) * 6.0 / float(fy), 6.0 + 0.01 * v, 0] for v in range(12, h)], f32)
    want = _assert_same(m, col, I4, what="column")
    xs = np.nonzero(want["sparse_mm"].any(axis=0))[0]
    assert len(xs) == 1 and want["stats"]["filled_top"] > 0 and want["stats"]["left_empty"] > 0


@pytest.mark.gpu
def test_parameters():
    w, h = 97, 41
    m = _gpu(w, h)
    # every other pixel below row 8 measured, but for a hole of 44 x 24 that only a window of 31 closes
    cam = _cam(w, h)
    v, u = np.nonzero((np.add.outer(np.arange(h), np.arange(w)) % 2 == 0) & (np.arange(h) >= 8)[:, None])
    keep = ~((u >= 30) & (u < 74) & (v >= 14) & (v < 38))
    u, v = u[keep], v[keep]
    Z = 5.0 + 0.05 * v + 0.4 * (u % 7 == 0)
    scan = np.stack([(u - cam["cx"]) * Z / cam["fx"], (v - cam["cy"]) * Z / cam["fy"], Z, 0 * Z], axis=1).astype(f32)
    overs = [dict(large=3), dict(large=15), dict(large=31), dict(stages=0), dict(tol_256=0), dict(tol_256=255)]
    overs += [dict(stages=1 << b, large=9) for b in range(7)]
    overs += [dict(stages=127 & ~lr.EXTEND_TOP, large=5), dict(stages=lr.EXTEND_TOP | lr.FILL_LARGE | lr.MEDIAN, large=7)]
    seen = {}
    for over in overs:
        m.set_lidar_depth(**over)
        want = _assert_same(m, scan, I4, what=over, **over)
        seen[str(over)] = want["depth_mm"]
        if over.get("stages") == 0:
            assert np.array_equal(want["depth_mm"], want["sparse_mm"])
    # the parameters do change the answer
    assert not np.array_equal(seen[str(dict(large=3))], seen[str(dict(large=15))])
    assert not np.array_equal(seen[str(dict(large=15))], seen[str(dict(large=31))])
    assert not np.array_equal(seen[str(dict(tol_256=0))], seen[str(dict(tol_256=255))])


@pytest.mark.gpu
def test_repetition_and_outputs_left_out():
    from surfelmapping_amd import capi
    L = capi.load()
    w, h = 131, 37
    m = _gpu(w, h)
    m.set_lidar_depth()
    a, b = (_scan(w, h), lr.T_STREET), _random(w, h)
    want_a, want_b = lr.lidar_depth(*a, _cam(w, h)), lr.lidar_depth(*b, _cam(w, h))
    assert not np.array_equal(want_a["sparse_mm"], want_b["sparse_mm"])
    for name, (pts, T), want in (("A", a, want_a), ("B", b, want_b), ("A again", a, want_a), ("none", (a[0][:0], I4), None)):
        _assert_same(m, pts, T, want, name)
    _assert_same(m, *a, want_a, "A after none")
    depth, sparse, index = np.zeros((h, w), np.uint16), np.zeros((h, w), np.uint16), np.zeros((h, w), np.int32)
    pts, T = a[0], np.ascontiguousarray(a[1])
    assert L.sm_lidar_depth(m._h, _vp(pts), len(pts), _fp(T), _vp(depth), None, None) == capi.SM_OK and np.array_equal(depth, want_a["depth_mm"])
    assert L.sm_lidar_depth(m._h, _vp(pts), len(pts), _fp(T), None, _vp(sparse), None) == capi.SM_OK and np.array_equal(sparse, want_a["sparse_mm"])
    assert L.sm_lidar_depth(m._h, _vp(pts), len(pts), _fp(T), None, None, _vp(index)) == capi.SM_OK and np.array_equal(index, want_a["index"])
    assert L.sm_lidar_depth(m._h, _vp(pts), len(pts), _fp(T), None, None, None) == capi.SM_OK
    assert m.lidar_depth_stats()["left_empty"] == want_a["stats"]["left_empty"]
    _assert_same(m, *b, want_b, "B after the calls without outputs")


@pytest.mark.gpu
def test_every_step_as_a_launch_of_its_own_gives_the_same(monkeypatch):
    """the measuring aid of tools/lidar_depth_probe.py: SM_LIDAR_DEPTH_UNFUSED=1 at set_lidar_depth"""
    monkeypatch.setenv("SM_LIDAR_DEPTH_UNFUSED", "1")
    monkeypatch.setenv("SM_LIDAR_DEPTH_TIMING", "1")
    for w, h in ((97, 41), (20, 9)):
        m = _gpu(w, h)
        pts, T = _random(w, h)
        for over, launches in ((dict(), 12), (dict(large=5, tol_256=0), 12), (dict(stages=0), 3), (dict(stages=lr.CLOSE | lr.FILL_LARGE), 7),
                               (dict(stages=127 & ~lr.FILL_LARGE & ~lr.CLOSE), 8)):
            m.set_lidar_depth(**over)
            cam = _cam(w, h)
            for what, p, t in (("scan", _scan(w, h)[::2], lr.T_STREET), ("random", pts, T), ("scan again", _scan(w, h)[::2], lr.T_STREET)):
                want = lr.lidar_depth(p, t, cam, **over)
                depth, sparse, index = m.lidar_depth(p, t)
                assert np.array_equal(sparse, want["sparse_mm"]) and np.array_equal(index, want["index"]), (w, h, over, what)
                bad = np.argwhere(depth != want["depth_mm"])
                assert bad.size == 0, (w, h, over, what, len(bad), bad[:4].tolist())
                st = m.lidar_depth_stats()
                assert {k: st[k] for k in TALLY} == {k: want["stats"][k] for k in TALLY}, (w, h, over, what)
                assert st["launches"] == launches and sum(v >= 0 for v in st["launch_ms"]) == launches, (over, st)


CAM = dict(width=256, height=96, fx=200.0, fy=200.0, cx=127.7, cy=48.2)


@functools.lru_cache(maxsize=None)
def _frames():
    """three frames of the synthetic street, and each frame's depth image as a scan: the points of every 3rd pixel of every 2nd
    row, in a lidar frame that T_STREET maps to the camera's"""
    from surfelmapping_amd import synth
    seq = synth.make_sequence(CAM, [synth.pose_matrix(0.3, 0.0, 2.0 + 0.5 * k, 3.0) for k in range(3)], seed=0)
    out = []
    for rgb, depth, sem, pose in seq:
        v, u = np.nonzero(depth[::2, ::3])
        v, u = v * 2, u * 3
        Z = depth[v, u].astype(np.float64) / 1000.0
        pc = np.stack([(u - CAM["cx"]) * Z / CAM["fx"], (v - CAM["cy"]) * Z / CAM["fy"], Z], axis=1)
        pts = np.concatenate([pc - lr.T_STREET[:3, 3].astype(np.float64), np.zeros((len(Z), 1))], axis=1).astype(f32)
        out.append((rgb, pts, sem, pose, lr.lidar_depth(pts, lr.T_STREET, CAM)))
    return out


def _ctx(**over):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**CAM, **dict(dict(max_sqrt_vertices=440, stereo_border=20.0, preprocess=0), **over)))


@pytest.mark.gpu
def test_device_path_builds_the_same_model():
    by_lidar, by_file = _ctx(), _ctx()
    by_lidar.set_lidar_depth()
    for rgb, pts, sem, pose, ref in _frames():
        by_lidar.process_frame_lidar(rgb, pts, lr.T_STREET, sem, pose)
        by_file.process_frame(rgb, ref["depth_mm"], sem, pose)
    by_lidar.sync()
    a, b = by_lidar.download_model(), by_file.download_model()
    assert len(b) > 2000
    assert_models_equal(a, b, "lidar depth on the device vs the restatement's depth from the host")
    assert by_lidar.counts() == by_file.counts()
    # the device entry point with all three outputs
    rgb, pts, sem, pose, ref = _frames()[0]
    P = CAM["width"] * CAM["height"]
    d_pts, d_depth, d_sparse, d_index = (by_lidar.device_alloc(n) for n in (pts.nbytes, P * 2, P * 2, P * 4))
    by_lidar.device_upload(d_pts, pts)
    by_lidar.lidar_depth_device(d_pts, len(pts), lr.T_STREET, d_depth, d_sparse, d_index)
    shape = (CAM["height"], CAM["width"])
    assert np.array_equal(by_lidar.device_download(d_depth, P * 2, np.uint16).reshape(shape), ref["depth_mm"])
    assert np.array_equal(by_lidar.device_download(d_sparse, P * 2, np.uint16).reshape(shape), ref["sparse_mm"])
    assert np.array_equal(by_lidar.device_download(d_index, P * 4, np.int32).reshape(shape), ref["index"])
    assert by_lidar.lidar_depth_stats()["measured"] == ref["stats"]["measured"]


@pytest.mark.gpu
def test_back_to_back_device_calls_and_scans_of_changing_size():
    """device calls enqueued one after the other with no tally asked for in between: each writes its own outputs, and the tally is
    the last call's; process_frame_lidar with scans that grow and shrink (its staging buffer is replaced)"""
    from surfelmapping_amd import capi
    frames = _frames()
    m = _ctx()
    m.set_lidar_depth()
    P = CAM["width"] * CAM["height"]
    shape = (CAM["height"], CAM["width"])
    scans = [frames[0][1], frames[1][1][:700], frames[2][1][:0], frames[2][1]]
    refs = [lr.lidar_depth(p, lr.T_STREET, CAM) for p in scans]
    d_pts = [m.device_alloc(max(p.nbytes, 16)) for p in scans]
    d_out = [(m.device_alloc(P * 2), m.device_alloc(P * 2), m.device_alloc(P * 4)) for _ in scans]
    for d, p in zip(d_pts, scans):
        if len(p):
            m.device_upload(d, p)
    m.sync()
    for rounds in range(2):                                            # the second round over keys and parts the first one left
        for d, p, out in zip(d_pts, scans, d_out):
            m.lidar_depth_device(d, len(p), lr.T_STREET, *out)
    st = m.lidar_depth_stats()
    assert {k: st[k] for k in TALLY} == {k: refs[-1]["stats"][k] for k in TALLY}
    for k, (out, ref) in enumerate(zip(d_out, refs)):
        assert np.array_equal(m.device_download(out[0], P * 2, np.uint16).reshape(shape), ref["depth_mm"]), k
        assert np.array_equal(m.device_download(out[1], P * 2, np.uint16).reshape(shape), ref["sparse_mm"]), k
        assert np.array_equal(m.device_download(out[2], P * 4, np.int32).reshape(shape), ref["index"]), k
    assert not refs[2]["depth_mm"].any() and refs[1]["stats"]["measured"] < refs[0]["stats"]["measured"]
    # scans of 700, 3081, 0 and 3081 points through process_frame_lidar against the restatement's depth through process_frame
    by_lidar, by_file = _ctx(), _ctx()
    by_lidar.set_lidar_depth()
    for (rgb, _, sem, pose, _), k in zip(frames + frames[:1], (1, 0, 2, 3)):
        by_lidar.process_frame_lidar(rgb, scans[k], lr.T_STREET, sem, pose)
        by_file.process_frame(rgb, refs[k]["depth_mm"], sem, pose)
    assert by_lidar._ldepth_dev[4] >= len(scans[0])
    assert_models_equal(by_lidar.download_model(), by_file.download_model(), "scans of changing size")
    assert by_lidar.counts() == by_file.counts()
    # a set call that is rejected changes nothing: the stage stays as it was
    L = capi.load()
    m.set_lidar_depth(large=5)
    want = lr.lidar_depth(scans[1], lr.T_STREET, CAM, large=5)
    for over in (dict(large=4), dict(stages=128), dict(min_z=0.0)):
        assert L.sm_set_lidar_depth(m._h, C.byref(capi.lidar_depth_params(m.cfg, **over))) == capi.SM_E_ARG, over
        assert np.array_equal(m.lidar_depth(scans[1], lr.T_STREET)[0], want["depth_mm"]), over
    assert not np.array_equal(want["depth_mm"], refs[1]["depth_mm"])


@pytest.mark.gpu
def test_lidar_depth_leaves_the_model_alone():
    frames = _frames()
    m = _ctx()
    for rgb, pts, sem, pose, ref in frames[:2]:
        m.process_frame(rgb, ref["depth_mm"], sem, pose)
    counts, model, log = m.counts(), m.download_model(), m.read_frame_log()
    assert counts["count"] > 1000
    m.set_lidar_depth()
    rgb, pts, sem, pose, ref = frames[2]
    got = m.lidar_depth(pts, lr.T_STREET)
    m.lidar_depth_stats()
    assert np.array_equal(got[0], ref["depth_mm"])
    assert m.counts() == counts
    assert_models_equal(m.download_model(), model, "after lidar_depth")
    assert np.array_equal(m.read_frame_log(), log)
    m.set_lidar_depth(False)
    assert m.counts() == counts


@pytest.mark.gpu
def test_rejected_arguments_and_contexts():
    from surfelmapping_amd import capi
    L = capi.load()
    E, U = capi.SM_E_ARG, capi.SM_E_UNSUPPORTED
    w, h = 64, 32
    m = _gpu(w, h)
    pts = np.ascontiguousarray(_scan(97, 41)[:200])
    depth, index, st = np.zeros((h, w), np.uint16), np.zeros((h, w), np.int32), capi.SmLidarDepthStats()
    d_pts, d_out = m.device_alloc(pts.nbytes + 16), m.device_alloc(w * h * 4 + 4)
    m.device_upload(d_pts, pts)
    T = np.ascontiguousarray(lr.T_STREET)
    calls = {
        "sm_lidar_depth": lambda h_: L.sm_lidar_depth(h_, _vp(pts), len(pts), _fp(T), _vp(depth), None, _vp(index)),
        "sm_lidar_depth_device": lambda h_: L.sm_lidar_depth_device(h_, d_pts, len(pts), _fp(T), d_out, None, None),
    }
    stats = lambda h_: L.sm_lidar_depth_stats(h_, C.byref(st))
    for name, call in list(calls.items()) + [("sm_lidar_depth_stats", stats)]:       # no stage yet
        assert call(m._h) == E and b"sm_set_lidar_depth" in L.sm_last_error(), name
    nan, inf = float("nan"), float("inf")
    for over in (dict(min_z=0.0), dict(min_z=-1.0), dict(min_z=nan), dict(max_z=nan), dict(max_z=inf), dict(min_z=2.0, max_z=1.0), dict(max_z=65.536),
                 dict(max_z=70.0), dict(stages=-1), dict(stages=128), dict(large=1), dict(large=2), dict(large=4), dict(large=30), dict(large=33),
                 dict(large=-3), dict(tol_256=-1), dict(tol_256=256)):
        assert L.sm_set_lidar_depth(m._h, C.byref(capi.lidar_depth_params(m.cfg, **over))) == E, over
        assert calls["sm_lidar_depth"](m._h) == E, over                # a rejected set leaves the context without the stage
    for over in (dict(), dict(min_z=1e-4, max_z=65.535, stages=0, large=3, tol_256=0), dict(min_z=3.0, max_z=3.0, large=31, tol_256=255)):
        assert L.sm_set_lidar_depth(m._h, C.byref(capi.lidar_depth_params(m.cfg, **over))) == capi.SM_OK, over
    assert stats(m._h) == E and b"no call yet" in L.sm_last_error()                   # before the first call
    assert L.sm_lidar_depth(m._h, None, 5, _fp(T), _vp(depth), None, None) == E
    assert L.sm_lidar_depth(m._h, None, 0, _fp(T), _vp(depth), None, None) == capi.SM_OK and not depth.any()
    assert L.sm_lidar_depth(m._h, _vp(pts), (1 << 24) + 1, _fp(T), _vp(depth), None, None) == E
    assert L.sm_lidar_depth(m._h, _vp(pts), len(pts), None, _vp(depth), None, None) == E
    assert L.sm_lidar_depth_device(m._h, None, 5, _fp(T), d_out, None, None) == E
    assert L.sm_lidar_depth_device(m._h, d_pts, (1 << 24) + 1, _fp(T), d_out, None, None) == E
    assert L.sm_lidar_depth_device(m._h, d_pts + 4, 5, _fp(T), d_out, None, None) == E
    for bad in ((d_out + 1, None, None), (None, d_out + 1, None), (None, None, d_out + 2), (None, None, d_out + 1)):
        assert L.sm_lidar_depth_device(m._h, d_pts, len(pts), _fp(T), *bad) == E and b"misaligned" in L.sm_last_error(), bad
    for name, call in list(calls.items()) + [("sm_lidar_depth_stats", stats)]:
        assert call(m._h) == capi.SM_OK, name
    m.set_lidar_depth(False)                                           # after it has been switched off
    for name, call in list(calls.items()) + [("sm_lidar_depth_stats", stats)]:
        assert call(m._h) == E, name
    # between the conflict test and the cull
    rgb, fpts, sem, pose, ref = _frames()[0]
    g = _ctx()
    g.process_frame(rgb, ref["depth_mm"], sem, pose)
    g.set_lidar_depth()
    gp = capi.lidar_depth_params(g.cfg)
    gout = np.zeros((CAM["height"], CAM["width"]), np.uint16)
    # (the device entry point is only ever refused below, before it looks at its points; a device address all the same)
    gcalls = {
        "sm_set_lidar_depth": lambda h_: L.sm_set_lidar_depth(h_, C.byref(gp)),
        "sm_lidar_depth": lambda h_: L.sm_lidar_depth(h_, _vp(fpts), len(fpts), _fp(T), _vp(gout), None, None),
        "sm_lidar_depth_device": lambda h_: L.sm_lidar_depth_device(h_, d_pts, 0, _fp(T), None, None, None),
        "sm_lidar_depth_stats": stats,
    }
    g.stage_conflict(pose, 1.0, 30.0)
    for name, call in gcalls.items():
        assert call(g._h) == E and b"between sm_stage_conflict and sm_stage_cull" in L.sm_last_error(), name
    g.stage_cull()
    assert gcalls["sm_lidar_depth"](g._h) == capi.SM_OK and np.array_equal(gout, ref["depth_mm"])
    # a sharded context and a rig context: every entry point, whatever else it is given
    for kind in ("sharded", "rig"):
        s = _ctx(max_sqrt_vertices=64)
        s.shard_stream_configure(0, 2) if kind == "sharded" else s.rig_configure(0, 2)
        for name, call in gcalls.items():
            assert call(s._h) == U, (kind, name)
        assert L.sm_set_lidar_depth(s._h, None) == U and L.sm_set_lidar_depth(s._h, C.byref(capi.lidar_depth_params(s.cfg, large=4))) == U, kind
        assert L.sm_lidar_depth(s._h, None, 9, None, None, None, None) == U and L.sm_lidar_depth_stats(s._h, None) == U, kind


@pytest.mark.gpu
def test_round_trip_of_a_simulated_sweep():
    """fuse three frames, sweep the model with a small lidar at the last pose, and turn the sweep back into a depth image"""
    from surfelmapping_amd import capi
    m = _ctx()
    for rgb, pts, sem, pose, ref in _frames():
        m.process_frame(rgb, ref["depth_mm"], sem, pose)
    # the camera sees +-32.6 deg across and +-13.5 deg up and down: 129 columns and 28 rows over it
    sensor = capi.lidar_sensor(n_az=129, az0_deg=-32.0, az_step_deg=0.5, el_deg=np.linspace(-13.0, 13.0, 28))
    sweep = m.lidar_sweep(pose, sensor)
    pts = capi.sweep_points(sweep["range"], sensor)
    assert len(pts) > 1500
    m.set_lidar_depth()
    want = _assert_same(m, pts, I4, what="round trip")
    assert (want["depth_mm"] > 0).mean() > 0.5 and want["stats"]["measured"] > 1000
