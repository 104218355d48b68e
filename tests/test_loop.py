"""Closing loops (sm_track_frame_old / sm_track_debug_old / sm_close_loop, SurfelMap.track_old / track_debug_old / close_loop;
DESIGN.md "4h. Closing loops"): the windowed tracker against the numpy restatement of tests/track_ref.py, and a loop end to end
on the scene test_track.py tracks in -- a camera that comes back with a drifted pose finds its old surfels, measures the drift
and pulls the model and a map file straight, bit for bit as tests/warp_ref.py says."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import recall_ref as cr
import retire_ref as rr
import track_ref as tr
import warp_ref as wr
from backends import assert_models_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_loop_symbols():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ("sm_track_frame_old", "sm_track_debug_old", "sm_default_loop_params", "sm_close_loop"):
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert (capi.SM_LOOP_CLOSED, capi.SM_LOOP_NONE, capi.SM_LOOP_NO_OLD_MAP, capi.SM_LOOP_TRACK_FAILED, capi.SM_LOOP_REJECTED) == (0, 1, 2, 3, 4)
    cfg = capi.make_config(1242, 375, 718.856, 718.856, 607.1928, 185.2157)
    p = capi.loop_params(cfg)
    assert p.min_age == cfg.time_delta
    assert (p.min_trans, p.min_rot_deg, p.max_trans, p.max_rot_deg) == (f32(0.02), f32(0.05), f32(2.0), f32(10.0))
    assert capi.loop_params(cfg, max_trans=0.05).max_trans == f32(0.05)


def test_arguments_are_rejected_before_any_device_call():
    from surfelmapping_amd import capi
    L = capi.load()
    depth = np.zeros(16, np.uint16)
    pose = np.eye(4, dtype=f32).reshape(16)
    out = np.zeros(16, f32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sm_track_frame_old(None, vp(depth), vp(pose), None, 5, vp(out), None, None) == capi.SM_E_ARG
    assert L.sm_track_debug_old(None, vp(depth), vp(pose), 5, None, None) == capi.SM_E_ARG
    src = capi.map_source([])
    info = capi.SmLoopInfo()
    assert L.sm_close_loop(None, vp(depth), vp(pose), C.byref(src), None, None, vp(out), C.byref(info)) == capi.SM_E_ARG
    assert L.sm_default_loop_params(None, None) == capi.SM_E_ARG


# ---------------------------------------------------------------------------------------------------------------------
# the scene: test_track.py's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    """KITTI camera: kitti_trajectory(11) through Scene(n_boxes=40), clean depth"""
    from surfelmapping_amd import synth
    cam = dict(synth.KITTI)
    poses = synth.kitti_trajectory(11)
    (clean,) = synth.make_sequences_parallel([(cam, poses, 0, 0.0, dict(seed=0, n_boxes=40))], workers=11)
    return dict(cam=cam, poses=poses, seq=clean)


def _ctx(cam, **over):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**cam, preprocess=0, **over))


@pytest.fixture(scope="module")
def old_map(frames):
    """context 1: frames 0..9 at the true poses; its rows are the old world"""
    m = _ctx(frames["cam"])
    for fr in frames["seq"][:10]:
        m.process_frame(*fr)
    return m, m.download_model()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the windowed tracker
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_windowed_tracker_matches_restatement(frames, old_map):
    cam, seq, poses = frames["cam"], frames["seq"], frames["poses"]
    # the old world's rows with times 0..9 dealt out row by row (a fused model's surfels in view all carry the last tick), in a
    # context whose one processed frame -- a fresh context's first fuses nothing -- gives the prediction its pose
    model = old_map[1].copy()
    model[:, 7] = (np.arange(len(model)) % 10).astype(f32)
    m = _ctx(cam)
    m.process_frame(*seq[9])
    m.upload_model(model)
    m.set_tick(10)
    depth = seq[10][1]
    pe = poses[10].copy()
    pe[:3, 3] += (0.03, -0.02, 0.05)
    pe = pe.astype(f32)
    times = model[:, 7]
    for max_time in (5, 8):
        live = times <= f32(max_time)
        assert 0 < live.sum() < len(model)
        pred, sys = m.track_debug_old(depth, pe, max_time)
        want = tr.predict(model, seq[9][3], cam, live=live)
        assert (want >= 0).mean() > 0.05
        assert np.array_equal(pred, want), f"max_time {max_time}: {int((pred != want).sum())} pixels differ"
        vm, nm = tr.vertex_normal(depth, cam)
        terms = tr.system_terms(vm, nm, want, model, pe, seq[9][3], cam)
        assert sys[28] == len(terms) and sys[28] > 1000
        tr.assert_system(sys, terms, f"max_time {max_time}")
        # the newest surfel the prediction holds
        _, info = m.track_old(depth, max_time, guess=pe)
        assert info["anchor_time"] == float(times[want[want >= 0]].max()) <= max_time, info
    # no window: sm_track_frame itself, bit for bit
    g = poses[10].astype(f32)
    p0, i0 = m.track(depth, g, dist_thresh=0.5)
    p1, i1 = m.track_old(depth, 2 ** 31 - 1, guess=g, dist_thresh=0.5)
    assert i0["status"] == "OK"
    assert np.array_equal(_bits(p0), _bits(p1))
    assert all(np.array_equal(i0[k], i1[k]) for k in i0) and f32(i0["rmse"]).view(np.uint32) == f32(i1["rmse"]).view(np.uint32)
    everything = tr.predict(model, seq[9][3], cam)
    assert i1["anchor_time"] == float(times[everything[everything >= 0]].max()) == 9.0
    # ... and so is the debug form
    a, b = m.track_debug(depth, pe), m.track_debug_old(depth, pe, 2 ** 31 - 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    # a window below every surfel
    p2, i2 = m.track_old(depth, -1, guess=g)
    assert i2["status"] == "NO_MODEL" and i2["anchor_time"] == -1.0 and np.array_equal(_bits(p2), _bits(g))
    assert_models_equal(m.download_model(), model, "tracking changes nothing")


# ---------------------------------------------------------------------------------------------------------------------
# 8. a loop, end to end
# ---------------------------------------------------------------------------------------------------------------------
def _drift():
    """G: 0.15 m sideways and forward plus 0.2 degrees about the vertical through the world origin"""
    a = math.radians(0.2)
    G = np.eye(4)
    G[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
    G[:3, 3] = (0.12, 0.0, 0.09)
    return G


def _moved(G, pose16):
    """G * P as float32[16] column-major"""
    P = np.asarray(pose16, f32).reshape(4, 4).T.astype(np.float64)
    return (G @ P).astype(f32).T.reshape(16).copy()


def _returned(frames, rows_f, tmp_path, G, with_old=True):
    """context 2: comes back at tick 400 with every pose off by G, fuses frames 4..9, writes its rows to file N and (with_old)
    recalls the old world's file F.  Returns (context, path of N)."""
    cam, seq = frames["cam"], frames["seq"]
    g = _ctx(cam)
    g.set_tick(400)
    for fr in seq[4:10]:
        g.process_frame(fr[0], fr[1], fr[2], _moved(G, fr[3]))
    n_path = str(tmp_path / "N.bin")
    cr.write_map(n_path, g.download_model(), 400, 405)
    if with_old:
        f_path = str(tmp_path / "F.bin")
        cr.write_map(f_path, rows_f, 0, 9)
        assert g.recall([f_path], pose=_moved(G, seq[9][3]), mode="copy", radius=500.0) == len(rows_f)
    return g, n_path


@pytest.mark.gpu
def test_loop_end_to_end(frames, old_map, tmp_path):
    cam, seq, poses = frames["cam"], frames["seq"], frames["poses"]
    rows_f = old_map[1]
    G = _drift()
    cam_shift = tr.pose_error(G @ poses[10].astype(np.float64), poses[10])
    assert cam_shift[0] < 0.2 and cam_shift[1] < 0.3, cam_shift            # what test_track.py converges from
    g, n_path = _returned(frames, rows_f, tmp_path, G)
    assert g.counts()["tick"] == 406
    before, file_before = g.download_model(), rr.read_map(n_path)[0]
    believed = _moved(G, seq[10][3])
    pose, info = g.close_loop(seq[10][1], believed, paths=[n_path], dist_thresh=0.5)
    assert info["status"] == "CLOSED" and info["track"]["status"] == "OK", info
    assert (info["t_a"], info["t_b"]) == (9, 405), info
    et, er = tr.pose_error(info["D"].astype(np.float64) @ G, np.eye(4))
    print(f"loop measurement: D * G is {et * 100:.3f} cm and {er:.4f} deg from the identity")
    assert et < 0.01 and er < 0.05, f"D * G is {et * 100:.3f} cm and {er:.4f} deg from the identity"
    # model and file: the restatement with the table of the measured D, bit for bit; the old world has not moved
    table = wr.loop_spread(info["D"].T.reshape(16), 9, 405)
    from surfelmapping_amd import capi
    assert np.array_equal(_bits(table), _bits(capi.loop_spread(info["D"], 9, 405)))
    after = g.download_model()
    # (applied from t_a + 1 with the rows from 1 on: the same rows for everything newer than the anchor, none for the anchor tick)
    assert_models_equal(after, wr.warp_rows(before, 10, table[1:]), "model after the loop")
    assert_models_equal(rr.read_map(n_path)[0], wr.warp_rows(file_before, 10, table[1:]), "file N after the loop")
    old = before[:, 7] <= f32(9)
    assert old.sum() == len(rows_f) and np.array_equal(_bits(after[old]), _bits(before[old]))
    assert (_bits(after[~old]) != _bits(before[~old])).any()
    assert rr.read_map(n_path)[1:] == (400, 405)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".warp.tmp")]
    # the corrected pose is D * believed, and the next frame tracks in the straightened map
    want_pose = (info["D"].astype(np.float64) @ believed.reshape(4, 4).T.astype(np.float64)).astype(f32)
    assert np.abs(pose - want_pose).max() < 1e-5
    tracked, ti = g.process_frame_tracked(*seq[10][:3], guess=pose, dist_thresh=0.5)
    et, er = tr.pose_error(tracked, poses[10])
    print(f"frame 10 after the loop: {et * 100:.3f} cm and {er:.4f} deg from the truth")
    assert ti["status"] == "OK" and et < 0.02 and er < 0.1, (et, er, ti)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["no_old_map", "none", "rejected"])
def test_loops_that_do_not_close(frames, old_map, tmp_path, case):
    seq = frames["seq"]
    G = np.eye(4) if case == "none" else _drift()
    g, n_path = _returned(frames, old_map[1], tmp_path, G, with_old=case != "no_old_map")
    before, snap = g.download_model(), (open(n_path, "rb").read(), os.stat(n_path).st_mtime_ns)
    c0 = g.counts()
    believed = _moved(G, seq[10][3])
    over = dict(max_trans=0.05) if case == "rejected" else {}
    pose, info = g.close_loop(seq[10][1], believed, paths=[n_path], dist_thresh=0.5, **over)
    assert info["status"] == dict(no_old_map="NO_OLD_MAP", none="NONE", rejected="REJECTED")[case], info
    assert np.array_equal(_bits(pose.T.reshape(16)), _bits(believed))
    assert (info["t_a"], info["t_b"]) == (-1, -1)
    assert_models_equal(g.download_model(), before, case)
    assert (open(n_path, "rb").read(), os.stat(n_path).st_mtime_ns) == snap and g.counts() == c0
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".warp.tmp")]
