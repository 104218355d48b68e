"""Camera tracking with the colour term (sm_track_frame_rgb / sm_track_rgb_debug, SurfelMap.track_rgb /
process_frame_tracked_rgb; DESIGN.md "4d. Tracking", "colour term").  The checks: the numpy restatement
(tests/track_rgb_ref.py) system by system, convergence on the corridor Scene(n_boxes=0) -- where depth alone is DEGENERATE --
and on the box scene, a corridor sequence from the constant-velocity guess, bit equality with sm_track_frame when the colour
term is switched off, and invariance: tracking changes nothing.

Bounds are those of tests/test_track.py (1 cm / 0.05 deg for one frame; 2 cm / 0.1 deg per frame and 10 cm drift for a
sequence, 3 cm / 0.15 deg / 15 cm with 2 mm depth noise).  A float64 prototype of the formulation measured 3.0 mm / 0.0047 deg
for one corridor frame, 7.9 mm / 0.0058 deg / 6.6 mm for the 30-frame corridor (7.2 mm / 0.0062 deg / 4.1 mm with noise) and
0.9 mm / 0.003 deg on the box scene; each GPU test prints what it measured before it asserts."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import track_ref as tr
import track_rgb_ref as rr
from backends import assert_models_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
NOISE_MM = 2.0
CORRIDOR = dict(seed=0, n_boxes=0)
BOUND = 1e-4            # SM_TRACK_DEGENERATE_BOUND


def _kitti():
    from surfelmapping_amd import synth
    return dict(synth.KITTI)


def _half_kitti():
    k = _kitti()
    return dict(width=k["width"] // 2, height=k["height"] // 2, fx=k["fx"] / 2, fy=k["fy"] / 2, cx=k["cx"] / 2, cy=k["cy"] / 2)


@pytest.fixture(scope="module")
def frames():
    """KITTI camera along kitti_trajectory: 11 frames of Scene(n_boxes=40), 30 of the corridor Scene(n_boxes=0) (walls and
    ground only) without and with depth noise"""
    from surfelmapping_amd import synth
    cam = _kitti()
    poses = synth.kitti_trajectory(30)
    boxes, corridor, noisy = synth.make_sequences_parallel(
        [(cam, poses[:11], 0, 0.0, dict(seed=0, n_boxes=40)), (cam, poses, 0, 0.0, CORRIDOR), (cam, poses, 0, NOISE_MM, CORRIDOR)],
        workers=12)
    return dict(cam=cam, poses=poses, boxes=boxes, corridor=corridor, noisy=noisy)


def _map(cam, seq, **over):
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, **over))
    for fr in seq:
        m.process_frame(*fr)
    return m


def _perturb(T, rng, dt=0.2, deg=0.3, vertical=True):
    """tests/test_track.py's: T moved by dt metres in a random direction and turned by deg degrees about a random axis"""
    d = rng.normal(size=3)
    if not vertical:
        d[1] = 0.0
    ax = rng.normal(size=3)
    G = np.asarray(T, np.float64).copy()
    G[:3, :3] = tr.se3_exp(np.r_[0.0, 0.0, 0.0, ax / np.linalg.norm(ax) * math.radians(deg)])[:3, :3] @ G[:3, :3]
    G[:3, 3] += d / np.linalg.norm(d) * dt
    return G.astype(np.float32)


def _along(T, dz, dx=0.05):
    """T moved dz metres along the corridor and dx sideways"""
    G = np.asarray(T, np.float64).copy()
    G[:3, 3] += (dx, 0.0, dz)
    return G.astype(np.float32)


def _rel_error(a0, a1, b0, b1):
    ra = np.linalg.inv(np.asarray(a0, np.float64)) @ np.asarray(a1, np.float64)
    rb = np.linalg.inv(np.asarray(b0, np.float64)) @ np.asarray(b1, np.float64)
    return tr.pose_error(ra, rb)


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_rgb_null_context_and_defaults_without_a_gpu():
    from surfelmapping_amd import capi
    L = capi.load()
    out = np.zeros(16, np.float32)
    img = np.zeros(16, np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sm_track_frame_rgb(None, ptr(img), ptr(img), None, None, None, ptr(out), None, None) == capi.SM_E_ARG
    assert L.sm_track_rgb_debug(None, ptr(img), ptr(img), ptr(out), 0, 0, None) == capi.SM_E_ARG
    assert L.sm_default_track_rgb_params(None) == capi.SM_E_ARG
    p = capi.track_rgb_params()
    assert p.levels == 3 and list(p.iters) == [10, 5, 4, 4, 4, 4]
    assert p.rgb_weight == np.float32(0.01) and p.rgb_max_residual == 0.25
    q = capi.track_rgb_params(levels=2, iters=[7, 3])
    assert q.levels == 2 and list(q.iters) == [7, 3, 4, 4, 4, 4]


def test_rgb_restatement_pieces():
    """hand-checkable pieces of tests/track_rgb_ref.py"""
    # luminance of a known colour word: sem 5, r 255, g 0, b 0 -> 0.299; white -> 1
    assert abs(float(rr.colour_luminance(np.uint32(5 << 24 | 255 << 16))) - 0.299) < 1e-7
    assert abs(float(rr.colour_luminance(np.uint32(0x00FFFFFF))) - 1.0) < 1e-6
    assert float(rr.colour_luminance(np.uint32(0x0A000000))) == 0.0
    # a 2x2 mean, odd sizes floor
    img = np.array([[1, 3, 9], [5, 7, 9], [9, 9, 9]], np.float32)
    h = rr.half(img)
    assert h.shape == (1, 1) and h[0, 0] == 4.0
    pyr = rr.pyramid(np.full((37, 70, 3), 255, np.uint8), 3)
    assert [p.shape for p in pyr] == [(37, 70), (18, 35), (9, 17)] and np.allclose(pyr[2], 1.0, atol=1e-6)
    # the bilinear value and derivative on a ramp I(x, y) = 2 x + 3 y
    yy, xx = np.mgrid[0:6, 0:8]
    ramp = (2 * xx + 3 * yy).astype(np.float32)
    u, v = np.array([1.25, 6.5, 6.99, 7.0, -0.1], np.float32), np.array([2.5, 0.0, 4.75, 1.0, 1.0], np.float32)
    val, du, dv, ok = rr.bilinear(ramp, u, v)
    assert list(ok) == [True, True, True, False, False]
    assert np.allclose(val[:3], 2 * u[:3] + 3 * v[:3], atol=1e-5) and np.allclose(du[:3], 2) and np.allclose(dv[:3], 3)


def _fd_scene():
    """a smooth image, a fronto-parallel wall of surfels at z = 5 with the colours a camera at the identity sees"""
    cam = dict(width=64, height=48, fx=60.0, fy=60.0, cx=32.0, cy=24.0)
    W, H = cam["width"], cam["height"]
    yy, xx = np.mgrid[0:H, 0:W]
    img = (0.5 + 0.2 * np.sin(xx / 7.0) * np.cos(yy / 5.0)).astype(np.float32)
    plane = np.zeros((H, W, 4), np.float32)
    z = 5.0
    plane[..., 0] = (xx + 0.5 - cam["cx"]) * z / cam["fx"]
    plane[..., 1] = (yy + 0.5 - cam["cy"]) * z / cam["fy"]
    plane[..., 2] = z
    plane[..., 3] = 0.5
    depth = np.full((H, W), 5000, np.uint16)
    return cam, img, plane, depth


def test_rgb_jacobian_matches_finite_difference():
    """the Jacobian row -[g_w, p x g_w] against a central difference of the residual under T <- exp(xi) T"""
    cam, img, plane, depth = _fd_scene()
    T = tr.se3_exp(np.r_[0.02, -0.01, 0.03, 0.004, -0.006, 0.003]) @ np.eye(4)
    kw = dict(level=0, stride=1, max_residual=10.0, stereo_border=0.0)
    J, r, ok = rr.photo_terms(plane, depth, img, T.astype(np.float32), cam, **kw)
    assert ok.sum() > 2000
    h = 1e-3
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = h
        _, rp, okp = rr.photo_terms(plane, depth, img, (tr.se3_exp(xi) @ T).astype(np.float32), cam, **kw)
        _, rm, okm = rr.photo_terms(plane, depth, img, (tr.se3_exp(-xi) @ T).astype(np.float32), cam, **kw)
        both = ok & okp & okm
        fd = (rp[both].astype(np.float64) - rm[both]) / (2 * h)
        # (the interpolant is piecewise bilinear: a sample that crosses a texel boundary sees the neighbouring cell's slope too)
        err = np.abs(fd - J[both, k])
        scale = np.abs(J[both, k]).max()
        assert np.median(err) < 0.02 * scale and np.mean(fd * J[both, k]) > 0, (k, np.median(err), scale)
    # level 1 of the pyramid: the same derivative in full-resolution pixels
    J1, r1, ok1 = rr.photo_terms(plane, depth, rr.half(img), T.astype(np.float32), cam, level=1, stride=2, max_residual=10.0,
                                 stereo_border=0.0)
    J0 = J.reshape(cam["height"], cam["width"], 6)[::2, ::2].reshape(-1, 6)
    ok0 = ok.reshape(cam["height"], cam["width"])[::2, ::2].reshape(-1)
    both = ok1 & ok0
    assert both.sum() > 500 and np.median(np.abs(J1[both] - J0[both])) < 0.1 * np.abs(J0[both]).max()


@pytest.fixture(scope="module")
def half_corridor(oracle_mod):
    """half-size KITTI camera: the oracle's map of corridor frames 0..9, frame 10"""
    from surfelmapping_amd import synth
    cam = _half_kitti()
    poses = synth.kitti_trajectory(11)
    (seq,) = synth.make_sequences_parallel([(cam, poses, 0, 0.0, CORRIDOR)], workers=11)
    o = oracle_mod.Oracle(oracle_mod.make_config(**cam, preprocess=0, stereo_border=40.0))
    for fr in seq[:10]:
        o.process_frame(*fr)
    return cam, poses, seq, o.download_model()


def test_restatement_tracks_the_corridor(half_corridor):
    """float64 prototype: 4.7 mm / 0.005 deg here; the joint system is well conditioned where the geometric one is not"""
    cam, poses, seq, model = half_corridor
    rgb, depth = seq[10][0], seq[10][1]
    for dz in (-0.2, 0.2):
        g = np.asarray(poses[10], np.float64).copy()
        g[2, 3] += dz
        T, info = rr.track(rgb, depth, model, seq[9][3], g, cam, stereo_border=40.0)
        et, er = tr.pose_error(T, poses[10])
        print(f"restatement, half-size corridor, guess {dz:+.1f} m: {et * 1e3:.2f} mm {er:.4f} deg, pivot ratio joint "
              f"{info['pivot_ratio']:.3g} icp {info['pivot_ratio_icp']:.3g}, {info['level_iterations']}")
        assert info["status"] == "OK", info
        assert et < 0.01 and er < 0.05, (dz, et, er, info)
        assert info["pivot_ratio"] > BOUND and not info["pivot_ratio_icp"] > BOUND, info


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rgb_systems_match_restatement(frames):
    cam, seq, poses = frames["cam"], frames["boxes"], frames["poses"]
    m = _map(cam, seq[:10])
    rgb, depth = seq[10][0], seq[10][1]
    pe = poses[10].copy()
    pe[:3, 3] += (0.03, -0.02, 0.05)
    pe = pe.astype(np.float32)
    model = m.download_model()                         # (compacts: slots = rows)
    pred = tr.predict(model, seq[9][3], cam)
    plane = rr.gather(pred, model)
    pyr = rr.pyramid(rgb, 3)
    for level in (0, 2):
        stride = 1 << level
        vm, nm = tr.vertex_normal(depth, cam, stride=stride)
        terms = {1: tr.system_terms(vm, nm, pred, model, pe, seq[9][3], cam),
                 2: rr.photo_terms_products(plane, depth, pyr[level], pe, cam, level=level, stride=stride)}
        want = {w: tr.sum_terms(terms[w]) for w in (1, 2)}
        got = {w: m.track_rgb_debug(rgb, depth, pe, level=level, which=w) for w in (0, 1, 2)}
        for w in (1, 2):
            print(f"level {level} which {w}: inliers {got[w][28]:.0f} (restatement {want[w][28]:.0f}), "
                  f"max |diff| / max |sys| {np.abs(got[w] - want[w])[:28].max() / np.abs(want[w]).max():.3g}")
            assert got[w][28] == want[w][28] and got[w][28] > 50000 / 4 ** level, (level, w, got[w][28], want[w][28])
            tr.assert_system(got[w], terms[w], f"level {level} which {w}")
        tr.assert_system(got[0], terms[1], f"level {level} joint", rgb_terms=terms[2], weight=0.01)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the corridor is tracked
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_corridor_is_tracked(frames):
    cam, seq, poses = frames["cam"], frames["corridor"], frames["poses"]
    m = _map(cam, seq[:10])
    rgb, depth = seq[10][0], seq[10][1]
    for dz in (-0.2, -0.1, 0.1, 0.2):
        g = _along(poses[10], dz)
        pose, info = m.track_rgb(rgb, depth, g)
        et, er = tr.pose_error(pose, poses[10])
        print(f"corridor, guess {dz:+.1f} m along z, 5 cm sideways: {info['status']} {et * 1e3:.2f} mm {er:.4f} deg, "
              f"levels {info['level_iterations'][:3]}, pivot ratio {info['pivot_ratio']:.3g}, rgb inliers {info['rgb_inliers']}")
        assert info["status"] == "OK", (dz, info)
        assert np.array_equal(info["guess"], g)
        assert et < 0.01 and er < 0.05, (dz, et, er, info)
        pose, info = m.track(depth, g)
        assert info["status"] == "DEGENERATE" and np.array_equal(pose, g), (dz, info)


# ---------------------------------------------------------------------------------------------------------------------
# 3. a corridor sequence from the constant-velocity guess
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [False, True])
def test_corridor_sequence_tracks_with_constant_velocity(frames, noisy):
    from surfelmapping_amd import capi
    cam, poses = frames["cam"], frames["poses"]
    seq = frames["noisy" if noisy else "corridor"]
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    got, infos = [], []
    for k, (rgb, d, s, p16) in enumerate(seq):
        if k < 2:
            m.process_frame(rgb, d, s, p16)
            got.append(p16.reshape(4, 4).T.copy())
        else:
            pose, info = m.process_frame_tracked_rgb(rgb, d, s)
            got.append(pose)
            infos.append(info)
    tmax, rmax, dmax = (0.03, 0.15, 0.15) if noisy else (0.02, 0.1, 0.10)
    bad = [(k + 2, i["status"], i["inliers"], i["level_iterations"]) for k, i in enumerate(infos) if i["status"] != "OK"]
    errs = [_rel_error(got[k - 1], got[k], poses[k - 1], poses[k]) for k in range(2, len(seq))]
    drift = tr.pose_error(got[-1], poses[-1])[0]
    worst = (max(e[0] for e in errs), max(e[1] for e in errs))
    print(f"corridor sequence, noise {NOISE_MM if noisy else 0} mm: worst frame-to-frame {worst[0] * 1e3:.2f} mm "
          f"{worst[1]:.4f} deg, drift {drift * 1e3:.2f} mm, failed {bad}")
    assert not bad and worst[0] < tmax and worst[1] < rmax and drift < dmax, (bad, worst, drift, errs)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the well-conditioned scene is not spoiled
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_box_scene_converges_from_perturbed_guesses(frames):
    cam, seq, poses = frames["cam"], frames["boxes"], frames["poses"]
    m = _map(cam, seq[:10])
    rng = np.random.default_rng(7)
    guesses = [_perturb(poses[10], rng) for _ in range(4)] + [_perturb(poses[10], rng, vertical=False) for _ in range(2)]
    for trial, g in enumerate(guesses):
        pose, info = m.track_rgb(seq[10][0], seq[10][1], g, dist_thresh=0.5)
        et, er = tr.pose_error(pose, poses[10])
        print(f"box scene, guess {trial}: {info['status']} {et * 1e3:.2f} mm {er:.4f} deg, levels {info['level_iterations'][:3]}")
        assert info["status"] == "OK", (trial, info)
        assert et < 0.01 and er < 0.05, (trial, et, er, info)


# ---------------------------------------------------------------------------------------------------------------------
# 5. equivalence with sm_track_frame, reproducibility
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_equals_track_without_the_colour_term(frames):
    cam, seq, poses = frames["cam"], frames["boxes"], frames["poses"]
    m = _map(cam, seq[:10])
    rgb, depth = seq[10][0], seq[10][1]
    keys = ("status", "iterations", "inliers", "rmse")
    for g in (_perturb(poses[10], np.random.default_rng(5)), None):
        p0, i0 = m.track(depth, g)
        p1, i1 = m.track_rgb(rgb, depth, g, rgb_weight=0.0, levels=1, iters=[15])
        assert np.array_equal(p0.view(np.uint32), p1.view(np.uint32)), (p0, p1)
        assert all(i0[k] == i1[k] for k in keys) and np.array_equal(i0["guess"], i1["guess"]), (i0, i1)
        assert i1["level_iterations"][0] == i1["iterations"]
    g = _perturb(poses[10], np.random.default_rng(6))
    pa, ia = m.track_rgb(rgb, depth, g)
    pb, ib = m.track_rgb(rgb, depth, g)
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    assert all(np.array_equal(ia[k], ib[k]) for k in ia), (ia, ib)
    assert ia["status"] == "OK" and ia["rgb_inliers"] > 10000 and sum(ia["level_iterations"]) == ia["iterations"]


# ---------------------------------------------------------------------------------------------------------------------
# 6. it changes nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("async_frames", [False, True])
def test_track_rgb_changes_nothing(async_frames):
    from surfelmapping_amd import capi, synth
    cam = dict(width=320, height=120, fx=180.0, fy=180.0, cx=159.5, cy=59.5)
    seq = synth.make_sequence(cam, synth.kitti_trajectory(30), seed=4)

    def run(track):
        m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, stereo_border=20.0, max_sqrt_vertices=800))
        for k, fr in enumerate(seq):
            (m.process_frame_async if async_frames else m.process_frame)(*fr)
            if track and k + 1 < len(seq):
                m.track_rgb(seq[k + 1][0], seq[k + 1][1], min_inliers=10)
        m.sync()
        return m.download_model(), m.counts(), m.read_frame_log()

    a, b = run(False), run(True)
    assert_models_equal(b[0], a[0], f"async={async_frames}")
    assert a[1] == b[1]
    assert np.array_equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------------------------
# 7. arguments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rgb_argument_validation():
    from surfelmapping_amd import capi, synth
    L = capi.load()
    cam = dict(width=160, height=64, fx=90.0, fy=90.0, cx=79.5, cy=31.5)
    seq = synth.make_sequence(cam, synth.kitti_trajectory(3), seed=2)
    over = dict(preprocess=0, stereo_border=10.0, max_sqrt_vertices=300)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rgb, d = np.ascontiguousarray(seq[-1][0]), np.ascontiguousarray(seq[-1][1])
    out = np.zeros(16, np.float32)
    g = seq[-1][3].copy()
    # a fresh context: no model, the guess comes back
    fresh = capi.SurfelMap(capi.make_config(**cam, **over))
    pose, info = fresh.track_rgb(rgb, d, g)
    assert info["status"] == "NO_MODEL" and np.array_equal(pose, g.reshape(4, 4).T) and info["rgb_inliers"] == 0
    m = capi.SurfelMap(capi.make_config(**cam, **over))
    for fr in seq:
        m.process_frame(*fr)

    def call(p=None, q=None, rgb_=rgb, d_=d, out_=out):
        return L.sm_track_frame_rgb(m._h, None if rgb_ is None else ptr(rgb_), None if d_ is None else ptr(d_), None,
                                    None if p is None else C.byref(p), None if q is None else C.byref(q),
                                    None if out_ is None else ptr(out_), None, None)

    assert call(rgb_=None) == capi.SM_E_ARG
    assert call(d_=None) == capi.SM_E_ARG
    assert call(out_=None) == capi.SM_E_ARG
    for bad in (dict(max_iters=0), dict(max_iters=101), dict(dist_thresh=0.0), dict(angle_thresh=0.0), dict(angle_thresh=181.0),
                dict(min_inliers=-1), dict(pixel_stride=0), dict(pixel_stride=65)):
        assert call(p=capi.track_params(**bad)) == capi.SM_E_ARG, bad
    for bad in (dict(levels=0), dict(levels=7), dict(iters=[10, 0, 4]), dict(levels=1, iters=[0]), dict(iters=[60, 30, 11]),
                dict(rgb_weight=-0.5), dict(rgb_weight=float("nan")), dict(rgb_weight=float("inf")), dict(rgb_max_residual=0.0),
                dict(rgb_max_residual=-1.0), dict(levels=5)):           # (64 >> 4 = 4 rows: below 8 x 8)
        assert call(q=capi.track_rgb_params(**bad)) == capi.SM_E_ARG, bad
    assert call(q=capi.track_rgb_params(levels=4, iters=[25, 25, 25, 25])) == capi.SM_OK      # 160 x 64 -> 20 x 8; sum = 100
    assert call(q=capi.track_rgb_params(levels=2, iters=[10, 5, 0])) == capi.SM_OK            # (an unused level's count is not read)
    assert L.sm_track_rgb_debug(m._h, None, ptr(d), ptr(out), 0, 0, None) == capi.SM_E_ARG
    assert L.sm_track_rgb_debug(m._h, ptr(rgb), ptr(d), None, 0, 0, None) == capi.SM_E_ARG
    assert L.sm_track_rgb_debug(m._h, ptr(rgb), ptr(d), ptr(g), 6, 0, None) == capi.SM_E_ARG
    assert L.sm_track_rgb_debug(m._h, ptr(rgb), ptr(d), ptr(g), 4, 0, None) == capi.SM_E_ARG
    assert L.sm_track_rgb_debug(m._h, ptr(rgb), ptr(d), ptr(g), 0, 3, None) == capi.SM_E_ARG
    pose, info = m.track_rgb(rgb, d, pixel_stride=2, min_inliers=10, levels=2)
    assert info["status"] in capi.TRACK_STATUS.values() and info["iterations"] >= 1, info
    # between the conflict test and the cull
    m.stage_conflict(seq[-1][3], 1.0, 30.0)
    assert call() == capi.SM_E_ARG
    assert L.sm_track_rgb_debug(m._h, ptr(rgb), ptr(d), ptr(g), 0, 0, None) == capi.SM_E_ARG
    m.stage_cull()
    # a sharded context holds only its rank's surfels
    s = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=300))
    s.shard_stream_configure(0, 2)
    assert L.sm_track_frame_rgb(s._h, ptr(rgb), ptr(d), None, None, None, ptr(out), None, None) == capi.SM_E_UNSUPPORTED
    assert L.sm_track_rgb_debug(s._h, ptr(rgb), ptr(d), ptr(g), 0, 0, None) == capi.SM_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
# 8. the facade
# ---------------------------------------------------------------------------------------------------------------------
def _build_demo(tmp_path):
    exe = str(tmp_path / "track_rgb_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "track_rgb_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_track_rgb_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_tracks_the_corridor_with_colour(tmp_path, frames):
    cam, seq, poses = frames["cam"], frames["corridor"][:11], frames["poses"]
    dump = tmp_path / "frames.bin"
    with open(dump, "wb") as f:
        f.write(np.array([cam["width"], cam["height"], len(seq)], np.uint32).tobytes())
        f.write(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32).tobytes())
        for rgb, d, s, p in seq:
            f.write(rgb.tobytes()); f.write(d.tobytes()); f.write(s.tobytes()); f.write(p.astype(np.float32).tobytes())
    exe = _build_demo(tmp_path)
    out = {}
    for colour in ("0", "1"):
        path = tmp_path / f"poses{colour}.bin"
        r = subprocess.run([exe, str(dump), "10", colour, str(path)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        out[colour] = (r.stdout, np.frombuffer(open(path, "rb").read(), np.float32).reshape(len(seq), 16))
    assert "frame 10: SM_TRACK_DEGENERATE" in out["0"][0], out["0"][0]
    assert "frame 10: SM_TRACK_OK" in out["1"][0], out["1"][0]
    et, er = tr.pose_error(out["1"][1][10].reshape(4, 4).T, poses[10])
    print(f"facade, corridor frame 10 from the constant-velocity guess: {et * 1e3:.2f} mm {er:.4f} deg")
    assert et < 0.01 and er < 0.05, (et, er, out["1"][0])
