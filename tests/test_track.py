"""Camera tracking (sm_track_frame / sm_track_debug, SurfelMap.track / process_frame_tracked; DESIGN.md "4d. Tracking").
The reference has no tracker, so there is no oracle for the pose: the checks are the numpy restatement (tests/track_ref.py),
convergence and sequence accuracy on synthetic scenes with known poses, and invariance -- a map built from tracked poses is the
map (and the oracle's map) built from those poses given explicitly, and tracking itself changes nothing."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import track_ref as tr
from backends import assert_models_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_MM = 2.0          # the noisy sequence: depth noise sigma


def _kitti():
    from surfelmapping_amd import synth
    return dict(synth.KITTI)


@pytest.fixture(scope="module")
def frames():
    """KITTI camera: kitti_trajectory(40) through Scene(n_boxes=40) without and with depth noise, and 11 frames of the
    corridor Scene(n_boxes=0) (walls and ground only)"""
    from surfelmapping_amd import synth
    cam = _kitti()
    poses = synth.kitti_trajectory(40)
    boxes = dict(seed=0, n_boxes=40)
    clean, noisy, corridor = synth.make_sequences_parallel(
        [(cam, poses, 0, 0.0, boxes), (cam, poses, 0, NOISE_MM, boxes), (cam, poses[:11], 0, 0.0, dict(seed=0, n_boxes=0))],
        workers=12)
    return dict(cam=cam, poses=poses, clean=clean, noisy=noisy, corridor=corridor)


def _map(cam, seq, **over):
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, **over))
    for fr in seq:
        m.process_frame(*fr)
    return m


def _perturb(T, rng, dt=0.2, deg=0.3, vertical=True):
    """T moved by dt metres in a random direction (horizontal only unless `vertical`) and turned by deg degrees about a random
    axis through its centre"""
    d = rng.normal(size=3)
    if not vertical:
        d[1] = 0.0
    ax = rng.normal(size=3)
    G = np.asarray(T, np.float64).copy()
    G[:3, :3] = tr.se3_exp(np.r_[0.0, 0.0, 0.0, ax / np.linalg.norm(ax) * math.radians(deg)])[:3, :3] @ G[:3, :3]
    G[:3, 3] += d / np.linalg.norm(d) * dt
    return G.astype(np.float32)


def _rel_error(a0, a1, b0, b1):
    """error of the motion a0 -> a1 against b0 -> b1: (m, deg)"""
    ra = np.linalg.inv(np.asarray(a0, np.float64)) @ np.asarray(a1, np.float64)
    rb = np.linalg.inv(np.asarray(b0, np.float64)) @ np.asarray(b1, np.float64)
    return tr.pose_error(ra, rb)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_prediction_and_system_match_restatement(frames):
    cam, seq, poses = frames["cam"], frames["clean"], frames["poses"]
    m = _map(cam, seq[:10])
    depth = seq[10][1]
    pe = poses[10].copy()
    pe[:3, 3] += (0.03, -0.02, 0.05)
    pe = pe.astype(np.float32)
    pred0, sys0 = m.track_debug(depth, pe)             # before the forced compaction of the read-back below
    model = m.download_model()
    pred, sys = m.track_debug(depth, pe)
    assert np.array_equal(sys0.view(np.uint64), sys.view(np.uint64)), "the system depends on dead slots"
    want = tr.predict(model, seq[9][3], cam)
    assert (want >= 0).mean() > 0.3
    assert np.array_equal(pred, want), f"{int((pred != want).sum())} pixels differ"
    vm, nm = tr.vertex_normal(depth, cam)
    terms = tr.system_terms(vm, nm, want, model, pe, seq[9][3], cam)
    want_sys = tr.sum_terms(terms)
    assert sys[28] == want_sys[28] and sys[28] > 50000
    tr.assert_system(sys, terms, "frame 10 against frames 0..9")
    # one Gauss-Newton step of the restatement moves towards the truth
    T1, _ = tr.solve(want_sys, pe)
    assert tr.pose_error(T1, poses[10])[0] < tr.pose_error(pe, poses[10])[0]
    # bit-reproducible
    g = _perturb(poses[10], np.random.default_rng(5))
    p1, i1 = m.track(depth, g)
    p2, i2 = m.track(depth, g)
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32)) and i1["rmse"] == i2["rmse"] and i1["inliers"] == i2["inliers"]


# ---------------------------------------------------------------------------------------------------------------------
# 2. convergence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_converges_from_perturbed_guesses(frames):
    """guesses 0.2 m and 0.3 deg off the truth (moved in a random direction, turned about their centre) converge to < 1 cm and
    < 0.05 deg"""
    cam, seq, poses = frames["cam"], frames["clean"], frames["poses"]
    m = _map(cam, seq[:10])
    rng = np.random.default_rng(7)
    guesses = [_perturb(poses[10], rng) for _ in range(4)] + [_perturb(poses[10], rng, vertical=False) for _ in range(2)]
    for trial, g in enumerate(guesses):
        pose, info = m.track(seq[10][1], g, dist_thresh=0.5)
        et, er = tr.pose_error(pose, poses[10])
        assert info["status"] == "OK", (trial, info)
        assert np.array_equal(info["guess"], g)
        assert et < 0.01 and er < 0.05, (trial, et, er, info)


# ---------------------------------------------------------------------------------------------------------------------
# 3. sequences with the constant-velocity guess (4. invariance of the tracked map)
# ---------------------------------------------------------------------------------------------------------------------
def _track_sequence(cam, seq, given=2):
    """frames 0 and 1 with their poses (frame 0 is the reference frame: the model is still empty after it), every later one
    tracked from the constant-velocity guess and fused with the tracked pose; returns (map, poses 4x4, infos)"""
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    out, infos = [], []
    for k, (rgb, d, s, p16) in enumerate(seq):
        if k < given:
            m.process_frame(rgb, d, s, p16)
            out.append(p16.reshape(4, 4).T.copy())
        else:
            pose, info = m.process_frame_tracked(rgb, d, s)
            out.append(pose)
            infos.append(info)
    return m, out, infos


@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [False, True])
def test_sequence_tracks_with_constant_velocity(frames, noisy):
    """per-frame error = error of the tracked motion from the previous frame; drift = error of the last pose.  Without noise:
    < 2 cm / 0.1 deg per frame, drift < 10 cm.  With 2 mm depth noise: < 3 cm / 0.15 deg per frame, drift < 15 cm."""
    cam, poses = frames["cam"], frames["poses"]
    seq = frames["noisy" if noisy else "clean"]
    m, got, infos = _track_sequence(cam, seq)
    tmax, rmax, dmax = (0.03, 0.15, 0.15) if noisy else (0.02, 0.1, 0.10)
    bad = [(k + 2, i["status"], i["inliers"], i["iterations"]) for k, i in enumerate(infos) if i["status"] != "OK"]
    errs = [_rel_error(got[k - 1], got[k], poses[k - 1], poses[k]) for k in range(2, len(seq))]
    drift = tr.pose_error(got[-1], poses[-1])[0]
    worst = (max(e[0] for e in errs), max(e[1] for e in errs))
    assert not bad and worst[0] < tmax and worst[1] < rmax and drift < dmax, (bad, worst, drift, errs)


@pytest.mark.gpu
def test_tracked_map_equals_map_from_the_same_poses(frames, oracle_mod):
    cam, seq = frames["cam"], frames["clean"][:24]
    m, got, _ = _track_sequence(cam, seq)
    from surfelmapping_amd import capi
    b = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    o = oracle_mod.Oracle(oracle_mod.make_config(**cam, preprocess=0))
    for (rgb, d, s, _), pose in zip(seq, got):
        p16 = tr.colmajor(pose)
        b.process_frame(rgb, d, s, p16)
        o.process_frame(rgb, d, s, p16)
    am = m.download_model()
    assert_models_equal(am, b.download_model(), "tracked vs given poses")
    assert_models_equal(am, o.download_model(), "tracked vs oracle")
    assert m.counts() == b.counts()
    oc = o.counts()
    assert all(m.counts()[k] == oc[k] for k in oc), (m.counts(), oc)
    assert np.array_equal(m.read_frame_log(), b.read_frame_log())


@pytest.mark.gpu
@pytest.mark.parametrize("async_frames", [False, True])
def test_track_changes_nothing(async_frames):
    """tracking after every frame (also while asynchronous frames are in flight) leaves the model, the counters and the frame
    log exactly as the run without tracking"""
    from surfelmapping_amd import capi, synth
    cam = dict(width=320, height=120, fx=180.0, fy=180.0, cx=159.5, cy=59.5)
    seq = synth.make_sequence(cam, synth.kitti_trajectory(30), seed=4)

    def run(track):
        m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, stereo_border=20.0, max_sqrt_vertices=800))
        for k, fr in enumerate(seq):
            (m.process_frame_async if async_frames else m.process_frame)(*fr)
            if track and k + 1 < len(seq):
                m.track(seq[k + 1][1], min_inliers=10)
        m.sync()
        return m.download_model(), m.counts(), m.read_frame_log()

    a, b = run(False), run(True)
    assert_models_equal(b[0], a[0], f"async={async_frames}")
    assert a[1] == b[1]
    assert np.array_equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------------------------
# 5. failure is reported
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_failures_return_the_guess(frames):
    from surfelmapping_amd import capi
    cam, seq, poses = frames["cam"], frames["clean"], frames["poses"]
    g = _perturb(poses[10], np.random.default_rng(3))
    # fresh context: no model
    fresh = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    pose, info = fresh.track(seq[0][1], g)
    assert info["status"] == "NO_MODEL" and np.array_equal(pose, g)
    pose, info = fresh.track(seq[0][1])
    assert info["status"] == "NO_MODEL" and np.array_equal(pose, np.eye(4, dtype=np.float32))
    fresh.process_frame(*seq[0])                         # the reference frame: a pose, still no model
    pose, info = fresh.track(seq[1][1])
    assert info["status"] == "NO_MODEL" and np.array_equal(pose, seq[0][3].reshape(4, 4).T)
    # nothing in view
    m = _map(cam, seq[:10])
    away = poses[9].copy()
    away[:3, 3] += (0.0, 0.0, -500.0)
    pose, info = m.track(seq[10][1], away.astype(np.float32))
    assert info["status"] in ("LOST", "NO_MODEL") and np.array_equal(pose, away.astype(np.float32))
    # all-zero depth: no inlier
    pose, info = m.track(np.zeros_like(seq[10][1]), g)
    assert info["status"] == "LOST" and info["inliers"] == 0 and np.array_equal(pose, g), info
    # walls and ground only: translation along the corridor is free
    c = _map(cam, frames["corridor"][:10])
    gc = poses[10].astype(np.float32)
    pose, info = c.track(frames["corridor"][10][1], gc)
    assert info["status"] == "DEGENERATE" and np.array_equal(pose, gc), info
    # the constant-velocity guess is reported
    pose, info = c.track(frames["corridor"][10][1])
    assert info["status"] == "DEGENERATE" and np.abs(info["guess"][:3, 3] - np.array([0.0, 0.0, 8.0])).max() < 1e-3, info
    assert np.array_equal(pose, info["guess"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. arguments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_validation():
    from surfelmapping_amd import capi, synth
    L = capi.load()
    cam = dict(width=160, height=64, fx=90.0, fy=90.0, cx=79.5, cy=31.5)
    seq = synth.make_sequence(cam, synth.kitti_trajectory(3), seed=2)
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, stereo_border=10.0, max_sqrt_vertices=300))
    for fr in seq:
        m.process_frame(*fr)
    d = np.ascontiguousarray(seq[-1][1])
    out = np.zeros(16, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sm_track_frame(m._h, None, None, None, ptr(out), None) == capi.SM_E_ARG
    assert L.sm_track_frame(m._h, ptr(d), None, None, None, None) == capi.SM_E_ARG
    for bad in (dict(max_iters=0), dict(max_iters=101), dict(dist_thresh=0.0), dict(angle_thresh=0.0), dict(angle_thresh=181.0),
                dict(min_inliers=-1), dict(pixel_stride=0), dict(pixel_stride=65)):
        p = capi.track_params(**bad)
        assert L.sm_track_frame(m._h, ptr(d), None, C.byref(p), ptr(out), None) == capi.SM_E_ARG, bad
    assert L.sm_track_debug(m._h, ptr(d), None, None, None) == capi.SM_E_ARG
    pose, info = m.track(d, pixel_stride=2, min_inliers=10)
    assert info["status"] in capi.TRACK_STATUS.values() and info["iterations"] >= 1, info
    # between the conflict test and the cull
    m.stage_conflict(seq[-1][3], 1.0, 30.0)
    assert L.sm_track_frame(m._h, ptr(d), None, None, ptr(out), None) == capi.SM_E_ARG
    assert L.sm_track_debug(m._h, ptr(d), ptr(out), None, None) == capi.SM_E_ARG
    m.stage_cull()
    # a sharded context holds only its rank's surfels
    s = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=300))
    s.shard_stream_configure(0, 2)
    assert L.sm_track_frame(s._h, ptr(d), None, None, ptr(out), None) == capi.SM_E_UNSUPPORTED
    assert L.sm_track_debug(s._h, ptr(d), ptr(out), None, None) == capi.SM_E_UNSUPPORTED


def test_null_context_and_defaults_without_a_gpu():
    from surfelmapping_amd import capi
    L = capi.load()
    out = np.zeros(16, np.float32)
    assert L.sm_track_frame(None, None, None, None, out.ctypes.data_as(C.c_void_p), None) == capi.SM_E_ARG
    assert L.sm_track_debug(None, None, None, None, None) == capi.SM_E_ARG
    assert L.sm_default_track_params(None) == capi.SM_E_ARG
    p = capi.track_params()
    assert (p.max_iters, p.min_inliers, p.pixel_stride) == (15, 1000, 1)
    assert math.isclose(p.dist_thresh, 0.3, rel_tol=1e-7) and p.angle_thresh == 30.0


def test_restatement_pieces():
    """hand-checkable pieces of tests/track_ref.py: the rigid inverse, the metricise rule, the vertex of a fronto-parallel wall"""
    from surfelmapping_amd import synth
    T = synth.pose_matrix(1.0, -2.0, 3.0, 20.0)
    inv = tr.rigid_inv_d(tr.colmajor(T)).reshape(4, 4).T
    assert np.allclose(inv @ T, np.eye(4), atol=1e-6)
    cam = dict(width=8, height=4, fx=10.0, fy=10.0, cx=3.5, cy=1.5)
    mm = np.full((4, 8), 2000, np.uint16)
    mm[0, 0] = 999
    z = tr.metric_depth(mm, stereo_border=2.0)
    assert (z[:, :2] == 0).all() and z[1, 3] == np.float32(2.0) and z[0, 0] == 0
    vm, nm = tr.vertex_normal(mm, cam, stereo_border=0.0)
    ok = vm[:, 3] == 1
    assert ok.sum() == 8 * 4 - 3                       # (0, 0) has depth 999 (outside the clip): it and its two neighbours drop
    assert np.allclose(vm[ok, 2], 2.0) and np.allclose(np.abs(nm[ok, 2]), 1.0)
