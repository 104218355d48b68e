"""Pose search before the tracker (sm_score_poses_window, sm_search_pose, sm_close_loop_search, sm_set_auto_loop_search;
SurfelMap.score_poses / search_pose / close_loop(search=) / set_auto_loop(search=); DESIGN.md "4j. Pose search").  The score
against the tracker's own inlier count and against the numpy restatement of tests/search_ref.py, the search against the
restatement's candidate lists and ranking, and a loop closed from 1.4 m of drift, by hand and by the policy, on the street of
tests/retire_ref.py at its small camera."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import loop_auto_ref as lar
import recall_ref as cr
import retire_ref as rr
import search_ref as sr
import track_ref as tr
import warp_ref as wr
from backends import assert_models_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
IMIN, IMAX = lar.INT32_MIN, lar.INT32_MAX
CAM, OVER = rr.CAM, rr.OVER
BORDER = OVER["stereo_border"]
NEW = ("sm_default_search_params", "sm_score_poses_window", "sm_search_pose", "sm_close_loop_search", "sm_set_auto_loop_search")
# the search centre: the true pose right-multiplied by (x, z, yaw)
OFFSETS = ((0.9, -0.7, 2.0), (-1.6, 1.3, -2.5), (1.9, 1.9, 2.9))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _m4(p16):
    return np.asarray(p16, f32).reshape(4, 4).T


@pytest.fixture(scope="module")
def scene():
    """frames 0..11 of the street; the model of frames 0..9 on the CPU oracle (bit-equal to the GPU's: test_gpu_parity.py)"""
    import oracle_lib as ol
    seq = rr.sequence(12)
    cpu = ol.Oracle(ol.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=440))
    for fr in seq[:10]:
        cpu.process_frame(*fr)
    model = cpu.download_model()
    assert len(model) > 30000 and (model[:, 7] <= 9).all()
    return dict(seq=seq, model=model, truth=_m4(seq[10][3]), t_prev=np.asarray(seq[9][3], f32))


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_search_symbols():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.sm_api_version() == 4
    p = capi.search_params()
    assert (p.levels, p.refine, p.stride0, p.top_k, p.colour_thresh) == (2, 4, 8, 4, f32(0.1))
    assert (list(p.trans_half), list(p.trans_step)) == ([2.0, 0.0, 2.0], [0.25] * 3)
    assert (list(p.rot_half_deg), list(p.rot_step_deg)) == ([0.0, 3.0, 0.0], [0.5] * 3)
    q = capi.search_params(top_k=2, trans_half=(1.0, 0.5, 1.0))
    assert q.top_k == 2 and list(q.trans_half) == [1.0, 0.5, 1.0] and q.levels == 2
    for k, v in sr.DEFAULT.items():
        got = getattr(p, k)
        assert (list(got) == [f32(x) for x in v]) if isinstance(v, tuple) else (got == f32(v)), k


def test_arguments_are_rejected_before_any_device_call():
    from surfelmapping_amd import capi
    L = capi.load()
    img = np.zeros(48, np.uint16)
    pose = np.eye(4, dtype=f32).reshape(16)
    out, scores = np.zeros(16, f32), np.zeros(4, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    E = capi.SM_E_ARG
    assert L.sm_default_search_params(None) == E
    assert L.sm_score_poses_window(None, None, vp(img), vp(pose), 1, None, 1, 0.1, IMIN, IMAX, vp(scores)) == E
    assert L.sm_search_pose(None, None, vp(img), vp(pose), None, None, None, IMIN, IMAX, vp(out), None) == E
    src, info = capi.map_source([]), capi.SmLoopInfo()
    assert L.sm_close_loop_search(None, None, vp(img), vp(pose), C.byref(src), None, None, None, None, vp(out), C.byref(info)) == E
    assert L.sm_set_auto_loop_search(None, None) == E


def test_restatement_default_grid(scene):
    centre = tr.colmajor(scene["truth"])
    c = sr.level0(centre)
    assert c.shape == (3757, 16) and c.dtype == f32
    assert np.array_equal(_bits(c[3757 // 2]), _bits(centre))
    assert len(np.unique(c, axis=0)) == 3757
    # the nesting: translation z fastest, then x, then the yaw
    first = tr.pose_error(_m4(c[0]), scene["truth"])
    assert abs(first[0] - math.hypot(2.0, 2.0)) < 1e-5 and abs(first[1] - 3.0) < 1e-4
    step = np.linalg.inv(scene["truth"].astype(np.float64)) @ _m4(c[1]).astype(np.float64)
    np.testing.assert_allclose(step[:3, 3], (-2.0, 0.0, -1.75), atol=1e-5)
    nxt = sr.next_level(c[:2], 1)
    assert nxt.shape == (2 * 9 ** 3, 16) and np.array_equal(_bits(nxt[9 ** 3 // 2]), _bits(c[0]))
    assert list(sr.rank([5, 9, 9, 1, 7], 4, 80, 3)) == [1, 2, 4] and list(sr.rank([5, 9], 1, 10, 4)) == []


def test_restatement_search_finds_the_pose(scene):
    """guards the scenario: on the CPU oracle's model the two-level search, scored from stride 4 on as in the evidence the feature
    was planned on, ends (its best candidate) within 0.1 m and 0.3 degrees of the truth from each of the three offsets"""
    seq = scene["seq"]
    for off in OFFSETS:
        centre = sr.offset_pose(scene["truth"], *off)
        res = sr.search(seq[10][0], seq[10][1], scene["model"], scene["t_prev"], tr.colmajor(centre), CAM, sp=dict(sr.DEFAULT, stride0=4),
                        stereo_border=BORDER)
        assert res["status"] == "OK" and [len(l["cands"]) for l in res["levels"]] == [3757, 4 * 729]
        et, er = tr.pose_error(_m4(res["levels"][-1]["poses"][0]), scene["truth"])
        print(f"offset {off}: best scores {[int(l['scores'].max()) for l in res['levels']]}, ends {et:.3f} m and {er:.3f} deg from the truth")
        assert et < 0.1 and er < 0.3, (off, et, er)
        assert int(res["levels"][0]["scores"].max()) > 5 * int(np.median(res["levels"][0]["scores"]))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _gpu(**over):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=440, **over))


def _holding(scene, model):
    """a context whose one processed frame gives the prediction its pose (frame 9's) and whose model is `model`, row = slot"""
    m = _gpu()
    m.process_frame(*scene["seq"][9])
    m.upload_model(model)
    m.set_tick(10)
    return m


@pytest.fixture(scope="module")
def held(scene):
    return _holding(scene, scene["model"])


def _candidates(truth, n, seed):
    """the truth nudged, single-axis offsets of it, random poses around it (all six degrees of freedom) and, last when n > 8, one
    that puts every sample behind the prediction camera"""
    rng = np.random.default_rng(seed)
    T = truth.astype(np.float64)
    out = [truth.copy()]
    for a in range(6):
        D = np.eye(4)
        if a < 3:
            D[a, 3] = 0.2
        else:
            D[:3, :3] = tr.se3_exp([0, 0, 0] + [math.radians(3.0) if k == a - 3 else 0.0 for k in range(3)])[:3, :3]
        out.append((T @ D).astype(f32))
    while len(out) < n:
        xi = np.concatenate([rng.uniform(-0.6, 0.6, 3), rng.uniform(-0.05, 0.05, 3)])
        out.append((T @ tr.se3_exp(xi)).astype(f32))
    out = out[:n]
    if n > 8:
        back = np.eye(4)
        back[:3, :3] = sr.delta_rot(0.0, 180.0, 0.0)
        back[:3, 3] = (0.0, 0.0, -50.0)
        out[-1] = (T @ back).astype(f32)
    return np.stack([tr.colmajor(p) for p in out])


@pytest.mark.gpu
def test_score_is_the_trackers_inlier_count(scene):
    seq = scene["seq"]
    model = scene["model"].copy()
    model[:, 7] = (np.arange(len(model)) % 10).astype(f32)
    m = _holding(scene, model)
    depth = seq[10][1]
    cands = _candidates(scene["truth"], 64, 1)
    for lo, hi in ((IMIN, IMAX), (IMIN, 5)):
        got = m.score_poses(depth, cands, stride=1, min_time=lo, max_time=hi)
        want = np.array([m.track_debug_window(depth, c, lo, hi)[1][28] for c in cands])
        print(f"window ({lo}, {hi}]: scores {got[:8]} ... of 64; the tracker's inliers {want[:8].astype(int)}")
        assert np.array_equal(got.astype(np.float64), want), (lo, hi, np.nonzero(got != want)[0])
        assert got[0] > 1000 and got[-1] == 0 and len(np.unique(got)) > 20
    assert_models_equal(m.download_model(), model, "scoring changes nothing")


@pytest.mark.gpu
@pytest.mark.parametrize("stride,n,thresh", [(1, 65, 0.1), (1, 64, 0.0), (3, 63, 0.1), (3, 1, 0.0), (4, 1000, 0.1), (4, 64, 0.0)])
def test_score_matches_restatement(scene, held, stride, n, thresh):
    seq = scene["seq"]
    rgb, depth = seq[10][0], seq[10][1]
    cands = _candidates(scene["truth"], n, 100 + n)
    # the list at an odd offset inside a larger array
    big = np.full(16 * n + 7, np.nan, f32)
    big[3:3 + 16 * n] = cands.reshape(-1)
    got = held.score_poses(depth, big[3:3 + 16 * n].reshape(n, 16), rgb=rgb, stride=stride, colour_thresh=thresh)
    plane = sr.prediction(scene["model"], scene["t_prev"], CAM)
    smp = sr.samples(rgb, depth, CAM, stride, BORDER)
    want = sr.score(cands, smp, plane, scene["t_prev"], CAM, colour_thresh=thresh)
    print(f"stride {stride}, {n} candidates, colour_thresh {thresh}: {len(smp[0])} samples, scores up to {int(got.max())} (restatement {int(want.max())})")
    assert np.array_equal(got, want), np.nonzero(got != want)[0]
    assert got[0] > 0
    # without colour the gate is not made: never fewer
    plain = held.score_poses(depth, cands, stride=stride)
    assert np.array_equal(plain, sr.score(cands, smp, plane, scene["t_prev"], CAM)) and (plain >= got).all() and (plain > got).any()


@pytest.mark.gpu
def test_search_finds_the_pose(scene, held):
    seq, model, truth = scene["seq"], scene["model"], scene["truth"]
    rgb, depth = seq[10][0], seq[10][1]
    for off in OFFSETS:
        centre = sr.offset_pose(truth, *off)
        pose, info = held.search_pose(depth, centre, rgb=rgb)
        ref = sr.search(rgb, depth, model, scene["t_prev"], tr.colmajor(centre), CAM, stereo_border=BORDER)
        et, er = tr.pose_error(pose, truth)
        print(f"offset {off}: {info['status']}, rank {info['winner_rank']} wins with {info['track']['inliers']} inliers, {et * 100:.2f} cm and "
              f"{er:.3f} deg from the truth; best scores {info['best_score']}; score {info['score_ms']:.3f} ms of {info['total_ms']:.2f} ms")
        assert info["status"] == "OK" and info["track"]["status"] == "OK" and info["levels_run"] == 2, info
        assert et < 0.05 and er < 0.2, (off, et, er)
        assert ref["status"] == "OK"
        assert info["candidates"] == [len(l["cands"]) for l in ref["levels"]] == [3757, 2916]
        assert info["best_score"] == [int(l["scores"].max()) for l in ref["levels"]]
        kept = ref["levels"][-1]["poses"]
        assert 0 <= info["winner_rank"] < len(kept)
        assert np.array_equal(_bits(tr.colmajor(info["start"])), _bits(kept[info["winner_rank"]]))
        assert np.array_equal(_bits(info["track"]["guess"]), _bits(info["start"])) and info["anchor_time"] == 9.0
    # one level, one candidate: allowed to fail; what it reports is the restatement's all the same
    centre = sr.offset_pose(truth, *OFFSETS[0])
    one = dict(levels=1, top_k=1)
    pose, info = held.search_pose(depth, centre, rgb=rgb, search=one)
    ref = sr.search(rgb, depth, model, scene["t_prev"], tr.colmajor(centre), CAM, sp=dict(sr.DEFAULT, **one), stereo_border=BORDER)
    print(f"one level, top 1: {info['status']}, {tr.pose_error(pose, truth)}")
    assert info["levels_run"] == 1 and info["candidates"] == [3757] and info["best_score"] == [int(ref["levels"][0]["scores"].max())]
    if ref["status"] == "OK":
        assert np.array_equal(_bits(tr.colmajor(info["start"])), _bits(ref["levels"][0]["poses"][0]))
    if info["status"] != "OK":
        assert np.array_equal(_bits(pose), _bits(centre)) and info["winner_rank"] == -1
    # a window below every surfel
    pose, info = held.search_pose(depth, centre, rgb=rgb, max_time=-1)
    assert info["status"] == "NO_MODEL" and np.array_equal(_bits(pose), _bits(centre)) and info["winner_rank"] == -1
    # nothing reaches min_inliers
    pose, info = held.search_pose(depth, centre, rgb=rgb, min_inliers=10 ** 8)
    assert info["status"] == "LOST" and info["levels_run"] == 1 and np.array_equal(_bits(pose), _bits(centre))
    assert_models_equal(held.download_model(), model, "searching changes nothing")


@pytest.mark.gpu
def test_rejected_parameters_and_contexts(held, scene):
    from surfelmapping_amd import capi
    L = capi.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    depth = np.ascontiguousarray(scene["seq"][10][1], np.uint16)
    pose, out = tr.colmajor(scene["truth"]), np.zeros(16, f32)
    scores = np.zeros(2, np.uint32)
    two = np.concatenate([pose, pose])
    E, U = capi.SM_E_ARG, capi.SM_E_UNSUPPORTED
    score = lambda c, n, stride, thr: L.sm_score_poses_window(held._h, None, vp(depth), vp(c), n, None, stride, thr, IMIN, IMAX, vp(scores))
    assert score(two, 2, 4, 0.1) == capi.SM_OK and scores[0] == scores[1] > 0
    bad = two.copy()
    bad[20] = np.inf
    assert [score(two, 0, 4, 0.1), score(two, 2 ** 20 + 1, 4, 0.1), score(two, 2, 0, 0.1), score(two, 2, 4, -0.5), score(bad, 2, 4, 0.1),
            score(two, 2, 4, float("nan")), score(two, 2, CAM["height"] + 1, 0.1)] == [E] * 7
    assert L.sm_score_poses_window(held._h, None, vp(depth), vp(two), 2, None, 4, 0.1, IMIN, IMAX, None) == E
    for over in (dict(levels=0), dict(levels=5), dict(refine=0), dict(top_k=0), dict(top_k=17), dict(stride0=0), dict(colour_thresh=-1.0),
                 dict(trans_step=(0.25, float("nan"), 0.25)), dict(rot_half_deg=(0.0, -3.0, 0.0)),
                 dict(trans_half=(50.0, 50.0, 50.0), trans_step=(0.25, 0.25, 0.25)), dict(refine=60)):
        sp = capi.search_params(**over)
        assert L.sm_search_pose(held._h, None, vp(depth), vp(pose), None, None, C.byref(sp), IMIN, IMAX, vp(out), None) == E, over
        assert L.sm_set_auto_loop_search(held._h, C.byref(sp)) == E, over
    small = dict(width=160, height=64, fx=90.0, fy=90.0, cx=79.5, cy=31.5)
    d16 = np.zeros((64, 160), np.uint16)
    src, info = capi.map_source([]), capi.SmLoopInfo()
    for kind in ("sharded", "rig"):
        s = capi.SurfelMap(capi.make_config(**small, preprocess=0, max_sqrt_vertices=300))
        s.shard_stream_configure(0, 2) if kind == "sharded" else s.rig_configure(0, 2)
        assert L.sm_score_poses_window(s._h, None, vp(d16), vp(two), 2, None, 4, 0.1, IMIN, IMAX, vp(scores)) == U, kind
        assert L.sm_search_pose(s._h, None, vp(d16), vp(pose), None, None, None, IMIN, IMAX, vp(out), None) == U, kind
        assert L.sm_close_loop_search(s._h, None, vp(d16), vp(pose), C.byref(src), None, None, None, None, vp(out), C.byref(info)) == U, kind
        assert L.sm_set_auto_loop_search(s._h, None) == U, kind
    # an empty context: nothing to score against
    e = _gpu()
    assert (e.score_poses(depth, two.reshape(2, 16), stride=4) == 0).all()
    assert e.search_pose(depth, scene["truth"])[1]["status"] == "NO_MODEL"


# ---------------------------------------------------------------------------------------------------------------------
# a loop closed from 1.4 m away
# ---------------------------------------------------------------------------------------------------------------------
def _drift():
    """G: 1.2 m in the ground plane and 2 degrees about the vertical through the world origin -- frame 10's camera is 1.4 m and
    2 degrees from where it is believed to be.  Chosen on the CPU: the restatement's search around the believed pose keeps a
    candidate 0.05 m from the truth, and tests/track_rgb_ref.py's tracker started from the believed pose itself converges, on the
    self-similar street, 0.25 m from where it started and 1.5 m from the truth."""
    a = math.radians(2.0)
    G = np.eye(4)
    G[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
    G[:3, 3] = (0.85, 0.0, 0.85)
    return G


def _moved(G, pose16):
    """G * P as float32[16] column-major"""
    return (G @ _m4(pose16).astype(np.float64)).astype(f32).T.reshape(16).copy()


def _returned(scene, tmp_path, G):
    """a context that comes back at tick 400 with every pose off by G, fuses frames 4..9, writes its rows to file N and recalls
    the old world's file F.  Returns (context, path of N)."""
    seq, rows_f = scene["seq"], scene["model"]
    g = _gpu()
    g.set_tick(400)
    for fr in seq[4:10]:
        g.process_frame(fr[0], fr[1], fr[2], _moved(G, fr[3]))
    n_path = str(tmp_path / "N.bin")
    cr.write_map(n_path, g.download_model(), 400, 405)
    f_path = str(tmp_path / "F.bin")
    cr.write_map(f_path, rows_f, 0, 9)
    assert g.recall([f_path], pose=_moved(G, seq[9][3]), mode="copy", radius=500.0) == len(rows_f)
    return g, n_path


def _sub(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    return d


@pytest.mark.gpu
def test_loop_end_to_end_from_metres_of_drift(scene, tmp_path):
    seq, truth = scene["seq"], scene["truth"]
    rgb, depth = seq[10][0], seq[10][1]
    G = _drift()
    believed = _moved(G, seq[10][3])
    shift = tr.pose_error(_m4(believed), truth)
    assert 1.3 < shift[0] < 1.5 and 1.9 < shift[1] < 2.1, shift
    # without the search: no loop with a correct D
    a, n_a = _returned(scene, _sub(tmp_path, "a"), G)
    _, info = a.close_loop_rgb(rgb, depth, believed, paths=[n_a], max_trans=3.0)
    et, er = tr.pose_error(info["D"].astype(np.float64) @ G, np.eye(4))
    print(f"without the search: {info['status']}, D * G is {et:.3f} m and {er:.3f} deg from the identity")
    assert info["status"] != "CLOSED" or et > 0.3, (info, et)
    # with it
    g, n_path = _returned(scene, _sub(tmp_path, "g"), G)
    assert g.counts()["tick"] == 406
    before, file_before = g.download_model(), rr.read_map(n_path)[0]
    pose, info = g.close_loop_rgb(rgb, depth, believed, paths=[n_path], max_trans=3.0, search=True)
    assert info["status"] == "CLOSED" and info["track"]["status"] == "OK", info
    assert (info["t_a"], info["t_b"]) == (9, 405), info
    et, er = tr.pose_error(info["D"].astype(np.float64) @ G, np.eye(4))
    print(f"with the search: D * G is {et * 100:.3f} cm and {er:.4f} deg from the identity")
    assert et < 0.05 and er < 0.3, f"D * G is {et * 100:.3f} cm and {er:.4f} deg from the identity"
    table = wr.loop_spread(info["D"].T.reshape(16), 9, 405)
    after = g.download_model()
    assert_models_equal(after, wr.warp_rows(before, 10, table[1:]), "model after the loop")
    assert_models_equal(rr.read_map(n_path)[0], wr.warp_rows(file_before, 10, table[1:]), "file N after the loop")
    old = before[:, 7] <= f32(9)
    assert old.sum() == len(scene["model"]) and np.array_equal(_bits(after[old]), _bits(before[old]))
    assert (_bits(after[~old]) != _bits(before[~old])).any()
    assert not [f for f in os.listdir(tmp_path / "g") if f.endswith(".warp.tmp")]
    want_pose = (info["D"].astype(np.float64) @ _m4(believed).astype(np.float64)).astype(f32)
    assert np.abs(pose - want_pose).max() < 1e-5
    et, er = tr.pose_error(pose, truth)
    assert et < 0.05 and er < 0.3, (et, er)
    # the default bound of a loop is 2 m: this one, 1.4 m, passes it; one told to stay below 1 m is rejected
    r, n_r = _returned(scene, _sub(tmp_path, "r"), G)
    snap = r.download_model()
    pose, info = r.close_loop_rgb(rgb, depth, believed, paths=[n_r], max_trans=1.0, search=True)
    assert info["status"] == "REJECTED" and np.array_equal(_bits(pose.T.reshape(16)), _bits(believed))
    assert_models_equal(r.download_model(), snap, "a rejected loop moves nothing")


@pytest.mark.gpu
def test_auto_loop_with_the_search(scene, tmp_path):
    """the policy's attempt.  A loop is worth closing here from 0.5 m or 3 degrees on: started 1.4 m off, the tracker alone settles
    0.25 m from its guess (see _drift), which such a policy leaves alone; the search measures the 1.4 m."""
    seq, truth = scene["seq"], scene["truth"]
    rgb, depth = seq[10][0], seq[10][1]
    G = _drift()
    believed = _moved(G, seq[10][3])
    loop = dict(min_trans=0.5, min_rot_deg=3.0)
    ctx = {k: _returned(scene, _sub(tmp_path, k), G) for k in ("hand", "plain", "toggled", "search")}
    before = ctx["hand"][0].download_model()
    split = 406 - 1 - OVER["time_delta"]
    # today's policy, by hand: the young-window track, the census, one sm_close_loop_rgb
    h, n_h = ctx["hand"]
    tracked = h.track_rgb_window(rgb, depth, split, IMAX, guess=believed)
    assert tracked[1]["status"] == "OK" and tracked[1]["anchor_time"] == 405.0
    assert h.old_in_view(tracked[0], split) >= 1000
    pose_h, info_h = h.close_loop_rgb(rgb, depth, tracked[0], paths=[n_h], **loop)
    # by itself, the search never set / set and switched off again: bit for bit that
    outs = {}
    for k in ("plain", "toggled"):
        c, n_c = ctx[k]
        if k == "toggled":
            c.set_auto_loop(paths=[n_c], search=True, **loop)
        c.set_auto_loop(paths=[n_c], **loop)
        pose, info = c.track_rgb(rgb, depth, guess=believed)
        st = c.auto_loop_stats()
        print(f"{k}: {st['last_census']} old surfels in view, {st['last']['status']}")
        assert (st["checked"], st["attempts"], st["closed"]) == (1, 1, 0), st
        want = pose_h if info_h["status"] == "CLOSED" else tracked[0]
        assert np.array_equal(_bits(pose), _bits(want))
        assert all(np.array_equal(info[kk], tracked[1][kk]) for kk in info if kk != "rmse"), (info, tracked[1])
        assert st["last"]["status"] == info_h["status"] and np.array_equal(_bits(st["last"]["D"]), _bits(info_h["D"]))
        assert_models_equal(c.download_model(), h.download_model(), k)
        assert open(n_c, "rb").read() == open(n_h, "rb").read()
        outs[k] = (pose, st)
    assert outs["plain"][1] == {**outs["toggled"][1], "last": outs["plain"][1]["last"]}
    assert_models_equal(h.download_model(), before, "nothing was closed")
    # with the search
    s, n_s = ctx["search"]
    s.set_auto_loop(paths=[n_s], search=True, **loop)
    pose, info = s.track_rgb(rgb, depth, guess=believed)
    st = s.auto_loop_stats()
    et, er = tr.pose_error(pose, truth)
    print(f"search: {st['last']['status']}, corrected pose {et * 100:.3f} cm and {er:.4f} deg from the truth")
    assert (st["checked"], st["attempts"], st["closed"]) == (1, 1, 1), st
    assert st["last_census"] == outs["plain"][1]["last_census"]
    assert all(np.array_equal(info[kk], tracked[1][kk]) for kk in info if kk != "rmse")
    assert (st["last"]["t_a"], st["last"]["t_b"]) == (9, 405) and et < 0.05 and er < 0.3, (st, et, er)
    table = wr.loop_spread(st["last"]["D"].T.reshape(16), 9, 405)
    assert_models_equal(s.download_model(), wr.warp_rows(before, 10, table[1:]), "model after the policy's loop")
