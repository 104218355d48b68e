"""Closing loops unasked (sm_track_*_window, sm_close_loop_rgb, sm_old_in_view, sm_set_auto_loop; SurfelMap.track_window /
track_rgb_window / close_loop_rgb / old_in_view / set_auto_loop; DESIGN.md "4i. Closing loops unasked").  The census against the
numpy restatement of tests/loop_auto_ref.py, the two-sided window against tests/track_ref.py and tests/track_rgb_ref.py, the
colour measurement on the corridor where depth alone is degenerate, and the policy as the composition of the pieces, on the
scenes of tests/test_loop.py and tests/test_track_rgb.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import loop_auto_ref as lar
import retire_ref as rr
import test_loop as tl
import test_warp as tw
import track_ref as tr
import track_rgb_ref as trr
import warp_ref as wr
from backends import assert_models_equal
from test_loop import frames, old_map          # noqa: F401  (module-scoped fixtures: the scene and the old world)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
f32 = np.float32
IMIN, IMAX = lar.INT32_MIN, lar.INT32_MAX
NEW = ("sm_track_frame_window", "sm_track_debug_window", "sm_track_frame_rgb_window", "sm_track_rgb_debug_window", "sm_close_loop_rgb",
       "sm_old_in_view", "sm_default_auto_loop_params", "sm_set_auto_loop", "sm_auto_loop_stats")
_bits = tl._bits


def _same_track(a, b):
    """(pose, info) of two tracker calls, bit for bit (anchor_time, which only the windowed forms report, aside)"""
    keys = [k for k in a[1] if k != "anchor_time" and k in b[1]]
    return (np.array_equal(_bits(a[0]), _bits(b[0])) and all(np.array_equal(a[1][k], b[1][k]) for k in keys if k != "rmse")
            and f32(a[1]["rmse"]).view(np.uint32) == f32(b[1]["rmse"]).view(np.uint32) and len(keys) >= 6)


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_auto_loop_symbols():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.sm_api_version() == 4
    cfg = capi.make_config(1242, 375, 718.856, 718.856, 607.1928, 185.2157)
    p = capi.auto_loop_params(cfg)
    assert (p.every, p.rest, p.min_old) == (1, 10, 1000) and p.loop.min_age == cfg.time_delta
    lp = capi.loop_params(cfg)
    assert bytes(p.loop) == bytes(lp)
    q = capi.auto_loop_params(cfg, rest=3, max_trans=0.05)
    assert q.rest == 3 and q.loop.max_trans == f32(0.05) and q.every == 1


def test_arguments_are_rejected_before_any_device_call():
    from surfelmapping_amd import capi
    L = capi.load()
    img = np.zeros(48, np.uint16)
    pose = np.eye(4, dtype=f32).reshape(16)
    out = np.zeros(16, f32)
    n = C.c_uint32()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    E = capi.SM_E_ARG
    assert L.sm_track_frame_window(None, vp(img), vp(pose), None, 1, 5, vp(out), None, None) == E
    assert L.sm_track_debug_window(None, vp(img), vp(pose), 1, 5, None, None) == E
    assert L.sm_track_frame_rgb_window(None, vp(img), vp(img), vp(pose), None, None, 1, 5, vp(out), None, None, None) == E
    assert L.sm_track_rgb_debug_window(None, vp(img), vp(img), vp(pose), 0, 0, 1, 5, None, None) == E
    src = capi.map_source([])
    info = capi.SmLoopInfo()
    assert L.sm_close_loop_rgb(None, vp(img), vp(img), vp(pose), C.byref(src), None, None, None, vp(out), C.byref(info)) == E
    assert L.sm_old_in_view(None, vp(pose), 5, C.byref(n)) == E
    assert L.sm_default_auto_loop_params(None, None) == E
    cfg = capi.make_config(64, 48, 60.0, 60.0, 32.0, 24.0)
    assert L.sm_default_auto_loop_params(C.byref(cfg), None) == E
    assert L.sm_set_auto_loop(None, C.byref(capi.auto_loop_params(cfg)), None) == E
    assert L.sm_auto_loop_stats(None, C.byref(capi.SmAutoLoopStats())) == E


def _build_demo(tmp_path):
    exe = str(tmp_path / "auto_loop_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "auto_loop_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_auto_loop_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def _small_model():
    """one surfel per pixel of a 40 x 30 camera at depths 2..8 m (so the prediction keeps every one that passes the gates), a
    ring of them outside the image, some behind the camera and beyond far; times 0..11 and a NaN dealt out row by row"""
    cam = dict(width=40, height=30, fx=35.0, fy=35.0, cx=19.5, cy=14.5)
    vv, uu = np.mgrid[-3:33, -3:43]
    u, v = uu.reshape(-1).astype(np.float64), vv.reshape(-1).astype(np.float64)
    n = len(u)
    z = 2.0 + (np.arange(n) % 7).astype(np.float64)
    z[::17] = -3.0
    z[5::19] = 31.0
    m = np.zeros((n, 12), f32)
    m[:, 0] = (u + 0.25 - cam["cx"]) * z / cam["fx"]
    m[:, 1] = (v + 0.25 - cam["cy"]) * z / cam["fy"]
    m[:, 2] = z
    m[:, 3] = 5.0
    t = (np.arange(n) % 12).astype(f32)
    t[::23] = np.nan
    m[:, 7] = t
    m[:, 10] = -1.0
    m[:, 11] = 0.05
    return cam, m


def test_census_restatement_counts_what_the_prediction_is_offered():
    cam, m = _small_model()
    pose = np.eye(4, dtype=f32)
    for max_time in (-1, 0, 4, 11, 100):
        with np.errstate(invalid="ignore"):
            old = m[:, 7] <= f32(max_time)
        pred = tr.predict(m, pose, cam, live=old)
        kept = pred[pred >= 0]
        assert len(np.unique(kept)) == len(kept) == lar.census(m, pose, cam, max_time), max_time
    assert lar.census(m, pose, cam, -1) == 0 < lar.census(m, pose, cam, 4) < lar.census(m, pose, cam, 100) < 40 * 30
    # the window's two comparisons: false on a NaN, an open end is not compared
    t = np.array([3, 4, 5, np.nan, np.inf, -np.inf, 4.5], f32)
    assert list(lar.in_window(t, 3, 5)) == [False, True, True, False, False, False, True]
    assert list(lar.in_window(t, IMIN, 4)) == [True, True, False, False, False, True, False]
    assert list(lar.in_window(t, 4, IMAX)) == [False, False, True, False, True, False, True]
    assert lar.in_window(t, IMIN, IMAX).all()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the census
# ---------------------------------------------------------------------------------------------------------------------
CAM, OVER = rr.CAM, rr.OVER


def _gpu(cap=60, **over):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=cap, **over))


def _census_pose():
    a = math.radians(10.0)
    T = np.eye(4)
    T[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
    T[:3, 3] = (1.0, 0.2, -0.5)
    return T.astype(f32)


def _census_rows(n, max_time, pose):
    """hand-made rows around the camera `pose`: pixels up to 20 beyond the image on every side, depths from behind the camera to
    beyond far, rows on the image border and on the two depth bounds; the times are test_warp's edge cases around max_time"""
    rng = np.random.default_rng(11)
    W, H = CAM["width"], CAM["height"]
    u = rng.uniform(-20, W + 20, n)
    v = rng.uniform(-20, H + 20, n)
    z = rng.uniform(-5, 40, n)
    u[0:40] = np.repeat([-0.5, W - 0.5, -0.5 + 1e-4, W - 0.5 - 1e-4], 10)          # the border columns ...
    v[40:80] = np.repeat([-0.5, H - 0.5, -0.5 + 1e-4, H - 0.5 - 1e-4], 10)         # ... and rows, as floor(x + 0.5) sees them
    z[0:80] = rng.uniform(2, 25, 80)
    z[80:100] = np.repeat([1.0, 30.0, 1.0 + 1e-5, 30.0 - 1e-5], 5)                  # near and far themselves
    c = np.stack([(u - CAM["cx"]) * z / CAM["fx"], (v - CAM["cy"]) * z / CAM["fy"], z, np.ones(n)])
    m = tw._rows(n, tw._edge_times(max_time, 3), seed=5)
    m[:, 0:3] = (pose.astype(np.float64) @ c)[:3].T.astype(f32)
    return m


@pytest.mark.gpu
def test_census_matches_restatement():
    pose, max_time = _census_pose(), 40
    g = _gpu()
    model = _census_rows(2500, max_time, pose)
    g.upload_model(model)
    g.set_tick(60)
    c0 = g.counts()
    for mt in (max_time, max_time - 1, max_time + 2, -7, IMAX, IMIN):
        want = lar.census(model, pose, CAM, mt)
        got = g.old_in_view(pose, mt)
        print(f"2500 hand-made rows, max_time {mt}: {got} old in view (restatement {want})")
        assert got == want, mt
    with np.errstate(invalid="ignore"):
        assert 100 < lar.census(model, pose, CAM, max_time) < lar.census(model, pose, CAM, IMAX) < lar.gates(model, pose, CAM).sum()
    assert g.old_in_view(np.eye(4, dtype=f32), max_time) == lar.census(model, np.eye(4, dtype=f32), CAM, max_time)
    assert g.counts() == c0
    assert_models_equal(g.download_model(), model, "the census changes nothing")
    # one row, and none
    k = int(np.nonzero(lar.gates(model, pose, CAM) & (model[:, 7] == f32(max_time)))[0][0])
    for rows in (model[k:k + 1], model[:0]):
        h = _gpu()
        if len(rows):
            h.upload_model(rows)
        assert h.old_in_view(pose, IMAX) == lar.census(rows, pose, CAM, IMAX) == len(rows)
        assert h.old_in_view(pose, IMIN) == 0 and h.counts()["count"] == len(rows)


@pytest.mark.gpu
def test_census_skips_dead_slots():
    """after frames whose culls leave dead slots in place, the census is the restatement's on the live rows"""
    seq = rr.sequence(30)                          # (test_retire.py: dead slots are pending after 30 frames at this period)
    g = _gpu(440, compact_period=24)
    for fr in seq:
        g.process_frame(*fr)
    log = g.read_frame_log(1)
    pending = int(log["n_slots"][-1]) - int(log["n_before"][-1])
    print(f"{pending} dead slots pending at the census")
    assert pending > 0
    c0, log0 = g.counts(), g.read_frame_log(8)
    pose = seq[29][3]
    got = {mt: g.old_in_view(pose, mt) for mt in (20, 26, 29)}
    assert g.counts() == c0 and np.array_equal(g.read_frame_log(8), log0)
    model = g.download_model()
    for mt, n in got.items():
        want = lar.census(model, pose, CAM, mt)
        print(f"max_time {mt}: {n} old in view (restatement {want}) of {len(model)} live rows")
        assert n == want
    assert got[20] <= got[26] <= got[29] and got[29] > 1000


# ---------------------------------------------------------------------------------------------------------------------
# 2. the window
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_window_equalities(frames, old_map):     # noqa: F811
    cam, seq, poses = frames["cam"], frames["seq"], frames["poses"]
    model = old_map[1].copy()
    model[:, 7] = (np.arange(len(model)) % 10).astype(f32)
    m = tl._ctx(cam)
    m.process_frame(*seq[9])
    m.upload_model(model)
    m.set_tick(10)
    rgb, depth = seq[10][0], seq[10][1]
    pe = poses[10].copy()
    pe[:3, 3] += (0.03, -0.02, 0.05)
    pe = pe.astype(f32)
    times = model[:, 7]
    vm, nm = tr.vertex_normal(depth, cam)
    pyr0 = trr.pyramid(rgb, 1)[0]
    for lo, hi in ((2, 7), (4, IMAX)):
        live = lar.in_window(times, lo, hi)
        assert 0 < live.sum() < len(model)
        want = tr.predict(model, seq[9][3], cam, live=live)
        assert (want >= 0).mean() > 0.05
        pred, sys = m.track_debug_window(depth, pe, lo, hi)
        assert np.array_equal(pred, want), f"window ({lo}, {hi}]: {int((pred != want).sum())} pixels differ"
        terms = {1: tr.system_terms(vm, nm, want, model, pe, seq[9][3], cam)}
        assert sys[28] == len(terms[1]) and sys[28] > 1000
        tr.assert_system(sys, terms[1], f"window ({lo}, {hi}]")
        _, info = m.track_window(depth, lo, hi, guess=pe)
        assert info["anchor_time"] == float(times[want[want >= 0]].max()) <= min(hi, 9), info
        assert float(times[want[want >= 0]].min()) > lo
        # the colour form: the same prediction, and the level-0 systems of the restatement fed with it
        plane = trr.gather(want, model)
        terms[2] = trr.photo_terms_products(plane, depth, pyr0, pe, cam, level=0, stride=1)
        for w in (1, 2):
            pr, got = m.track_rgb_debug_window(rgb, depth, pe, lo, hi, level=0, which=w)
            assert np.array_equal(pr, want)
            wsys = tr.sum_terms(terms[w])
            print(f"window ({lo}, {hi}] which {w}: inliers {got[28]:.0f} (restatement {wsys[28]:.0f}), "
                  f"max |diff| / max |sys| {np.abs(got - wsys)[:28].max() / np.abs(wsys).max():.3g}")
            assert got[28] == len(terms[w]) and got[28] > 1000
            tr.assert_system(got, terms[w], f"window ({lo}, {hi}] which {w}")
        _, rinfo = m.track_rgb_window(rgb, depth, lo, hi, guess=pe)
        assert rinfo["anchor_time"] == info["anchor_time"]
    g = poses[10].astype(f32)
    # both ends open: the plain forms, bit for bit
    plain = m.track(depth, g, dist_thresh=0.5)
    assert plain[1]["status"] == "OK"
    assert _same_track(plain, m.track_window(depth, IMIN, IMAX, guess=g, dist_thresh=0.5))
    a, b = m.track_debug(depth, pe), m.track_debug_window(depth, pe, IMIN, IMAX)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    plain_rgb = m.track_rgb(rgb, depth, g, dist_thresh=0.5)
    assert plain_rgb[1]["status"] == "OK"
    assert _same_track(plain_rgb, m.track_rgb_window(rgb, depth, IMIN, IMAX, guess=g, dist_thresh=0.5))
    for w in (0, 1, 2):
        a, b = m.track_rgb_debug(rgb, depth, pe, level=1, which=w), m.track_rgb_debug_window(rgb, depth, pe, IMIN, IMAX, level=1, which=w)
        assert np.array_equal(a.view(np.uint64), b[1].view(np.uint64))
    # an open lower end: the old-map forms, bit for bit
    for mt in (5, IMAX):
        old = m.track_old(depth, mt, guess=g, dist_thresh=0.5)
        win = m.track_window(depth, IMIN, mt, guess=g, dist_thresh=0.5)
        assert _same_track(old, win) and old[1]["anchor_time"] == win[1]["anchor_time"]
        a, b = m.track_debug_old(depth, pe, mt), m.track_debug_window(depth, pe, IMIN, mt)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    # a window that holds nothing
    p2, i2 = m.track_window(depth, 9, IMAX, guess=g)
    assert i2["status"] == "NO_MODEL" and i2["anchor_time"] == -1.0 and np.array_equal(_bits(p2), _bits(g))
    assert_models_equal(m.download_model(), model, "tracking changes nothing")


@pytest.mark.gpu
def test_every_instantiation_of_the_splat_matches_the_restatement():
    """The prediction's splat is one kernel with a compile-time gate per end of the window.  Its four instantiations against the
    restatement on the census test's hand-made rows (2500 of them: a tail block and a partial wave), whose times lie around 40
    and hold NaNs: a NaN passes an open end and fails a closed one."""
    pose = np.eye(4, dtype=f32)
    model = _census_rows(2500, 40, np.eye(4))
    times = model[:, 7]
    frame = rr.sequence(1)[0]
    g = _gpu(200)
    g.process_frame(frame[0], frame[1], frame[2], pose)         # the prediction camera: the identity
    g.upload_model(model)                                       # slots = rows
    g.set_tick(60)
    occupied, nans = [], []
    for lo, hi in ((IMIN, IMAX), (IMIN, 40), (39, IMAX), (38, 40), (40, 40)):
        want = tr.predict(model, pose, CAM, live=lar.in_window(times, lo, hi))
        pred, _ = g.track_debug_window(frame[1], pose, lo, hi)
        occupied.append(int((want >= 0).sum()))
        nans.append(int(np.isnan(times[want[want >= 0]]).sum()))
        print(f"window ({lo}, {hi}]: {int((pred >= 0).sum())} pixels occupied (restatement {occupied[-1]}, {nans[-1]} by NaN-time slots), "
              f"{int((pred != want).sum())} differ")
        assert np.array_equal(pred, want), (lo, hi)
    assert np.all(pred == -1)                                   # (40, 40]: nothing
    # the scene tells the five apart, and NaN times are in the prediction exactly where no end is compared (the figures: the
    # restatement's, worked out without a GPU)
    assert occupied == [1034, 415, 694, 210, 0] and nans[0] == 64
    assert 0 == occupied[4] < occupied[3] < occupied[1] < occupied[2] < occupied[0]
    assert nans[0] > 0 and nans[1:] == [0, 0, 0, 0]
    assert_models_equal(g.download_model(), model, "tracking changes nothing")


# ---------------------------------------------------------------------------------------------------------------------
# 3. colour closes where depth cannot
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corridor():
    """test_track_rgb.py's corridor (walls and ground only) along kitti_trajectory(11), and the map of frames 0..9"""
    from surfelmapping_amd import synth
    cam = dict(synth.KITTI)
    poses = synth.kitti_trajectory(11)
    (seq,) = synth.make_sequences_parallel([(cam, poses, 0, 0.0, dict(seed=0, n_boxes=0))], workers=11)
    m = tl._ctx(cam)
    for fr in seq[:10]:
        m.process_frame(*fr)
    return dict(cam=cam, poses=poses, seq=seq), m.download_model()


@pytest.mark.gpu
def test_colour_closes_the_corridor_loop(corridor, tmp_path):
    fr, rows_f = corridor
    seq = fr["seq"]
    assert (rows_f[:, 7] <= 9).all()
    G = tl._drift()
    g, n_path = tl._returned(fr, rows_f, tmp_path, G)
    before, file_before = g.download_model(), rr.read_map(n_path)[0]
    snap, c0 = (open(n_path, "rb").read(), os.stat(n_path).st_mtime_ns), g.counts()
    believed = tl._moved(G, seq[10][3])
    pose, info = g.close_loop(seq[10][1], believed, paths=[n_path])
    assert info["status"] == "TRACK_FAILED" and info["track"]["status"] == "DEGENERATE", info
    assert np.array_equal(_bits(pose.T.reshape(16)), _bits(believed)) and (info["t_a"], info["t_b"]) == (-1, -1)
    assert_models_equal(g.download_model(), before, "depth alone: nothing changes")
    assert (open(n_path, "rb").read(), os.stat(n_path).st_mtime_ns) == snap and g.counts() == c0
    pose, info = g.close_loop_rgb(seq[10][0], seq[10][1], believed, paths=[n_path])
    assert info["status"] == "CLOSED" and info["track"]["status"] == "OK", info
    assert (info["t_a"], info["t_b"]) == (9, 405), info
    et, er = tr.pose_error(info["D"].astype(np.float64) @ G, np.eye(4))
    print(f"corridor loop, colour: D * G is {et * 100:.3f} cm and {er:.4f} deg from the identity")
    assert et < 0.01 and er < 0.05, f"D * G is {et * 100:.3f} cm and {er:.4f} deg from the identity"
    table = wr.loop_spread(info["D"].T.reshape(16), 9, 405)
    assert_models_equal(g.download_model(), wr.warp_rows(before, 10, table[1:]), "model after the loop")
    assert_models_equal(rr.read_map(n_path)[0], wr.warp_rows(file_before, 10, table[1:]), "file N after the loop")
    want_pose = (info["D"].astype(np.float64) @ believed.reshape(4, 4).T.astype(np.float64)).astype(f32)
    assert np.abs(pose - want_pose).max() < 1e-5
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".warp.tmp")]


# ---------------------------------------------------------------------------------------------------------------------
# 4. the policy is the composition
# ---------------------------------------------------------------------------------------------------------------------
def _sub(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    return d


@pytest.mark.gpu
def test_policy_is_the_composition(frames, old_map, tmp_path):     # noqa: F811
    cam, seq, poses = frames["cam"], frames["seq"], frames["poses"]
    G = tl._drift()
    A, n_a = tl._returned(frames, old_map[1], _sub(tmp_path, "a"), G)
    B, n_b = tl._returned(frames, old_map[1], _sub(tmp_path, "b"), G)
    before = A.download_model()
    assert_models_equal(B.download_model(), before, "two identical contexts")
    depth, believed = seq[10][1], tl._moved(G, seq[10][3])
    split = 406 - 1 - A.cfg.time_delta
    assert split == 205
    # by hand
    tracked = A.track_window(depth, split, IMAX, guess=believed, dist_thresh=0.5)
    assert tracked[1]["status"] == "OK" and tracked[1]["anchor_time"] == 405.0
    pose_a, info_a = A.close_loop(depth, tracked[0], paths=[n_a], dist_thresh=0.5)
    assert info_a["status"] == "CLOSED", info_a
    # by itself
    B.set_auto_loop(paths=[n_b])
    pose_b, info_b = B.track(depth, guess=believed, dist_thresh=0.5)
    st = B.auto_loop_stats()
    print(f"policy: {st['last_census']} old surfels in view, {st['last']['status']}")
    assert np.array_equal(_bits(pose_b), _bits(pose_a))
    assert all(np.array_equal(info_b[k], tracked[1][k]) for k in info_b), (info_b, tracked[1])
    assert_models_equal(B.download_model(), A.download_model(), "the policy's model")
    assert open(n_b, "rb").read() == open(n_a, "rb").read()
    assert (st["checked"], st["attempts"], st["closed"]) == (1, 1, 1), st
    assert (st["none"], st["rejected"], st["failed"], st["no_old_map"]) == (0, 0, 0, 0), st
    assert st["last_census"] == lar.census(before, tracked[0], cam, split) >= 1000
    assert st["last"]["status"] == "CLOSED" and (st["last"]["t_a"], st["last"]["t_b"]) == (9, 405)
    assert np.array_equal(_bits(st["last"]["D"]), _bits(info_a["D"]))
    et, er = tr.pose_error(pose_b, poses[10])
    print(f"corrected pose: {et * 100:.3f} cm and {er:.4f} deg from the truth")
    assert et < 0.02 and er < 0.1, (et, er)
    assert B.counts() == A.counts() and B.counts()["tick"] == 406
    # straight after: the rest period, so the young-window track and nothing else
    again = B.track(depth, guess=pose_b, dist_thresh=0.5)
    assert _same_track(again, A.track_window(depth, split, IMAX, guess=pose_a, dist_thresh=0.5))
    st2 = B.auto_loop_stats()
    assert (st2["checked"], st2["attempts"], st2["closed"]) == (1, 1, 1), st2


# ---------------------------------------------------------------------------------------------------------------------
# 5. the policy stays out of the way
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_policy_stays_out_of_the_way(frames, old_map, tmp_path):     # noqa: F811
    from surfelmapping_amd import capi
    cam, seq, poses = frames["cam"], frames["seq"], frames["poses"]
    G = tl._drift()
    g, n_path = tl._returned(frames, old_map[1], tmp_path, G)
    rgb, depth, believed = seq[10][0], seq[10][1], tl._moved(G, seq[10][3])
    before, snap = g.download_model(), open(n_path, "rb").read()
    plain = g.track(depth, guess=believed, dist_thresh=0.5)
    plain_rgb = g.track_rgb(rgb, depth, guess=believed, dist_thresh=0.5)
    young = g.track_window(depth, 205, IMAX, guess=believed, dist_thresh=0.5)
    young_rgb = g.track_rgb_window(rgb, depth, 205, IMAX, guess=believed, dist_thresh=0.5)
    assert young[1]["status"] == young_rgb[1]["status"] == "OK"
    n_old = g.old_in_view(young[0], 205)
    assert n_old == lar.census(before, young[0], cam, 205) >= 1000
    n_old_rgb = g.old_in_view(young_rgb[0], 205)                   # (the colour tracker's pose is its own: so is its census)
    assert n_old_rgb == lar.census(before, young_rgb[0], cam, 205) >= 1000
    # too few old surfels in view: a census and nothing else
    g.set_auto_loop(paths=[n_path], min_old=max(n_old, n_old_rgb) + 1)
    assert _same_track(g.track(depth, guess=believed, dist_thresh=0.5), young)
    st = g.auto_loop_stats()
    assert (st["checked"], st["attempts"], st["last_census"]) == (1, 0, n_old), st
    assert _same_track(g.track_rgb(rgb, depth, guess=believed, dist_thresh=0.5), young_rgb)
    st = g.auto_loop_stats()
    assert (st["checked"], st["attempts"], st["last_census"]) == (2, 0, n_old_rgb), st
    # off again: the plain trackers
    g.set_auto_loop()
    assert _same_track(g.track(depth, guess=believed, dist_thresh=0.5), plain)
    assert _same_track(g.track_rgb(rgb, depth, guess=believed, dist_thresh=0.5), plain_rgb)
    assert g.auto_loop_stats()["checked"] == 2
    assert_models_equal(g.download_model(), before, "nothing has changed")
    assert open(n_path, "rb").read() == snap
    # no window yet (tick - 1 - min_age < 0): the plain prediction, no census
    m = old_map[0]
    assert m.counts()["tick"] == 10
    p0 = m.track(seq[10][1], poses[10].astype(f32), dist_thresh=0.5)
    m.set_auto_loop(min_old=1)
    try:
        assert _same_track(m.track(seq[10][1], poses[10].astype(f32), dist_thresh=0.5), p0) and p0[1]["status"] == "OK"
        assert m.auto_loop_stats()["checked"] == 0
    finally:
        m.set_auto_loop()
    # parameters the setter rejects; a sharded context and a rig context hold only their own surfels
    L = capi.load()
    for bad in (dict(every=0), dict(rest=-1), dict(min_age=0), dict(max_trans=-1.0), dict(min_rot_deg=float("nan"))):
        assert L.sm_set_auto_loop(g._h, C.byref(capi.auto_loop_params(g.cfg, **bad)), None) == capi.SM_E_ARG, bad
    twice = capi.map_source([n_path, n_path])
    assert L.sm_set_auto_loop(g._h, C.byref(capi.auto_loop_params(g.cfg)), C.byref(twice)) == capi.SM_E_ARG
    assert g.auto_loop_stats()["checked"] == 2                     # (a rejected setting leaves the policy as it was: off)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    small = dict(width=160, height=64, fx=90.0, fy=90.0, cx=79.5, cy=31.5)
    img, d16 = np.zeros((64, 160, 3), np.uint8), np.zeros((64, 160), np.uint16)
    pose, out, n = np.eye(4, dtype=f32).reshape(16), np.zeros(16, f32), C.c_uint32()
    src, info = capi.map_source([]), capi.SmLoopInfo()
    for kind in ("sharded", "rig"):
        s = capi.SurfelMap(capi.make_config(**small, preprocess=0, max_sqrt_vertices=300))
        s.shard_stream_configure(0, 2) if kind == "sharded" else s.rig_configure(0, 2)
        U = capi.SM_E_UNSUPPORTED
        assert L.sm_set_auto_loop(s._h, C.byref(capi.auto_loop_params(s.cfg)), None) == U, kind
        assert L.sm_old_in_view(s._h, vp(pose), 5, C.byref(n)) == U, kind
        assert L.sm_close_loop_rgb(s._h, vp(img), vp(d16), vp(pose), C.byref(src), None, None, None, vp(out), C.byref(info)) == U, kind


# ---------------------------------------------------------------------------------------------------------------------
# 6. what an attempt moves: the caller's files and the retirement policy's, each once; `every`; a track that fails
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_attempt_lists_the_retirement_files_once(frames, old_map, tmp_path):     # noqa: F811
    cam, seq = frames["cam"], frames["seq"]
    G = tl._drift()
    g = tl._ctx(cam)
    g.set_tick(400)
    prefix = str(tmp_path / "R")
    g.set_auto_retire(3, prefix, min_age=1, min_distance=0.0)          # after the frames of ticks 401 and 404
    for fr in seq[4:10]:
        g.process_frame(fr[0], fr[1], fr[2], tl._moved(G, fr[3]))
    nf, retired = g.auto_retire_stats()
    files = [f"{prefix}_{i:06d}.bin" for i in range(nf)]
    assert nf >= 1 and retired > 1000 and all(os.path.exists(f) for f in files)
    f_path = str(tmp_path / "F.bin")
    tl.cr.write_map(f_path, old_map[1], 0, 9)
    assert g.recall([f_path], pose=tl._moved(G, seq[9][3]), mode="copy", radius=500.0) == len(old_map[1])
    before, files_before = g.download_model(), [rr.read_map(f)[0] for f in files]
    depth, believed = seq[10][1], tl._moved(G, seq[10][3])
    young = g.track_window(depth, 205, IMAX, guess=believed, dist_thresh=0.5)
    assert young[1]["status"] == "OK" and g.counts()["tick"] == 406
    # a tick that is no multiple of `every`: no census
    g.set_auto_loop(paths=[files[0]], every=4)
    assert _same_track(g.track(depth, guess=believed, dist_thresh=0.5), young)
    assert g.auto_loop_stats()["checked"] == 0
    # a track that fails: the guess comes back as without the policy, no census
    g.set_auto_loop(paths=[files[0]])                                  # (a file of the retirement policy's, listed by the caller too)
    lost = g.track(depth, guess=believed, dist_thresh=0.5, min_inliers=10 ** 8)
    assert lost[1]["status"] == "LOST" and np.array_equal(_bits(lost[0].T.reshape(16)), _bits(believed))
    assert g.auto_loop_stats()["checked"] == 0
    # the attempt: every retirement file moves, the one listed twice once
    pose, info = g.track(depth, guess=believed, dist_thresh=0.5)
    st = g.auto_loop_stats()
    assert (st["checked"], st["attempts"], st["closed"]) == (1, 1, 1) and st["last"]["status"] == "CLOSED", st
    assert (st["last"]["t_a"], st["last"]["t_b"]) == (9, 405)
    table = wr.loop_spread(st["last"]["D"].T.reshape(16), 9, 405)
    assert_models_equal(g.download_model(), wr.warp_rows(before, 10, table[1:]), "model after the loop")
    for f, rows in zip(files, files_before):
        now = rr.read_map(f)[0]
        assert_models_equal(now, wr.warp_rows(rows, 10, table[1:]), f)
        assert len(rows) > 0 and (_bits(now) != _bits(rows)).any(), f
    assert g.warp_stats()["files_listed"] == nf
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".warp.tmp")]
