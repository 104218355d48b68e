"""The map warped by surfel time (sm_warp_by_time / sm_loop_spread, SurfelMap.warp_by_time / capi.loop_spread; DESIGN.md "4h.
Closing loops").  The definition is the numpy restatement of tests/warp_ref.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import recall_ref as cr
import retire_ref as rr
import warp_ref as wr
from backends import assert_models_equal

CAM, OVER = cr.CAM, cr.OVER
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
IDENT12 = np.eye(3, 4, dtype=f32).reshape(1, 12)


def _gpu(cap=35, **over):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=cap, **over))


def _rows(n, times, seed=0):
    """n hand-made surfels with the given last-update times, distinct centres and unit normals"""
    rng = np.random.default_rng(100 + seed)
    m = np.zeros((n, 12), f32)
    m[:, 0:3] = rng.uniform(-20, 20, (n, 3))
    m[:, 3] = 5.0
    m[:, 4] = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) | np.uint32(0x03000000)).view(f32)
    m[:, 6] = np.arange(n) % 97
    m[:, 7] = np.resize(np.asarray(times, f32), n)
    v = rng.normal(size=(n, 3))
    m[:, 8:11] = v / np.linalg.norm(v, axis=1, keepdims=True)
    m[:, 11] = 0.05
    return m


def _edge_times(t0, n):
    """below t0, equal to it, the last row's, far beyond, NaN, infinite, negative, fractional"""
    return [t0 - 1, t0, t0 + n - 1, t0 + 1000, np.nan, np.inf, -np.inf, -7, t0 + 0.5, t0 + 1.75, t0 - 0.25, t0 + n - 1.5, t0 + 1, t0 + 2, 0]


def _snapshot(paths):
    return [(open(p, "rb").read(), os.stat(p).st_mtime_ns) for p in paths]


def _no_temporaries(d):
    assert not [f for f in os.listdir(d) if f.endswith(".warp.tmp")]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(autouse=True)
def _clean_env():
    os.environ.pop("SM_RECALL_NO_INDEX", None)
    yield
    os.environ.pop("SM_RECALL_NO_INDEX", None)


@pytest.fixture(scope="module")
def seq():
    return cr.sequence(9)


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_warp_symbols():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ("sm_warp_by_time", "sm_warp_stats", "sm_loop_spread"):
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.sm_api_version() == 4


def test_ctypes_mirror_has_the_header_layout(tmp_path):
    from surfelmapping_amd import capi
    mirrors = {"sm_warp_stats_t": capi.SmWarpStats}
    lines = []
    for cname, cls in mirrors.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sm_c_api.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    for cname, cls in mirrors.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_arguments_are_rejected_before_any_device_call():
    from surfelmapping_amd import capi
    L = capi.load()
    src = capi.map_source([], include_model=False)
    tab = IDENT12.copy()
    assert L.sm_warp_by_time(None, C.byref(src), 0, 1, tab.ctypes.data_as(C.c_void_p)) == capi.SM_E_ARG
    assert L.sm_warp_stats(None, None) == capi.SM_E_ARG
    D = np.eye(4, dtype=f32).reshape(16)
    out = np.zeros((4, 12), f32)
    assert L.sm_loop_spread(None, 0, 3, out.ctypes.data_as(C.c_void_p)) == capi.SM_E_ARG
    assert L.sm_loop_spread(D.ctypes.data_as(C.c_void_p), 0, 3, None) == capi.SM_E_ARG
    assert L.sm_loop_spread(D.ctypes.data_as(C.c_void_p), 3, 3, out.ctypes.data_as(C.c_void_p)) == capi.SM_E_ARG
    assert L.sm_loop_spread(D.ctypes.data_as(C.c_void_p), 4, 3, out.ctypes.data_as(C.c_void_p)) == capi.SM_E_ARG


def _D(axis, angle_deg, t):
    """a world->world correction, float32[16] column-major, made in double"""
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    ang = np.radians(angle_deg)
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    M[:3, 3] = t
    return M.T.reshape(16).astype(f32)


def _ulps(a, b):
    """distance in float32 steps, element by element"""
    def key(x):
        u = _bits(x).astype(np.int64)
        return np.where(u & 0x80000000, 0x80000000 - u, u)
    return np.abs(key(a) - key(b))


def test_loop_spread_against_the_restatement():
    from surfelmapping_amd import capi
    cases = [((0, 1, 0), 0.2, (0.15, 0.0, 0.02), 0, 7), ((1, 2, 3), 9.0, (1.5, -0.3, 0.8), 391, 409), ((0, 0, 1), 170.0, (0, 0, 0), -3, 2),
             ((1, 0, 0), 0.0, (0.5, 0.25, -1.0), 10, 11), ((3, -1, 2), 1e-4, (1e-3, 0, 0), 5, 300)]
    for axis, ang, t, ta, tb in cases:
        D = _D(axis, ang, t)
        got, want = capi.loop_spread(D, ta, tb), wr.loop_spread(D, ta, tb)
        assert got.shape == want.shape == (tb - ta + 1, 12)
        assert _ulps(got, want).max() <= 1, (axis, ang, int(_ulps(got, want).max()))
        assert np.array_equal(_bits(got[0]), _bits(IDENT12[0]))                                   # exactly the identity, +0 included
        last = np.array([[D[i + 4 * j] for j in range(4)] for i in range(3)], f32).reshape(12)
        assert _ulps(got[-1], last).max() <= 1
        # a 4x4 in numpy's indexing is the same correction
        assert np.array_equal(_bits(capi.loop_spread(D.reshape(4, 4).T, ta, tb)), _bits(got))
        # the ramp is monotone in the translation and rigid to float precision
        for row in got:
            R = row.reshape(3, 4)[:, :3].astype(np.float64)
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6
    # errors
    ok = _D((0, 1, 0), 1.0, (0, 0, 0))
    for bad in (np.where(np.arange(16) == 12, np.nan, ok), np.where(np.arange(16) == 0, np.inf, ok)):
        with pytest.raises(capi.SurfelMapError):
            capi.loop_spread(bad.astype(f32), 0, 4)
    skew = ok.copy()
    skew[0] += f32(0.01)
    with pytest.raises(capi.SurfelMapError):
        capi.loop_spread(skew, 0, 4)
    mirror = ok.copy()
    mirror[0:3] = -mirror[0:3]
    with pytest.raises(capi.SurfelMapError):
        capi.loop_spread(mirror, 0, 4)
    with pytest.raises(capi.SurfelMapError):
        capi.loop_spread(_D((0, 1, 0), 179.99, (0, 0, 0)), 0, 4)
    with pytest.raises(capi.SurfelMapError):
        capi.loop_spread(ok, 4, 4)
    assert capi.loop_spread(_D((0, 1, 0), 179.9, (0, 0, 0)), 0, 4).shape == (5, 12)


def test_restatement_self_checks():
    m = _rows(64, _edge_times(10, 5))
    assert np.array_equal(_bits(wr.warp_rows(m, 10, np.repeat(IDENT12, 5, axis=0))), _bits(m))
    sel, k = wr.select(np.array([np.nan, 9.999, 10.0, 11.75, 14.0, 1e9, np.inf, -np.inf, -7.0], f32), 10, 5)
    assert sel.tolist() == [False, False, True, True, True, True, True, False, False]
    assert k.tolist() == [0, 0, 0, 1, 4, 4, 4, 0, 0]
    assert wr.select(np.array([11.75], f32), 10, 1)[1].tolist() == [0]
    # a selected row moves in its centre and its normal only
    tab = wr.rigid_table(5, seed=1)
    out = wr.warp_rows(m, 10, tab)
    sel, _ = wr.select(m[:, 7], 10, 5)
    changed = (_bits(out) != _bits(m))
    assert not changed[~sel].any() and not changed[:, [3, 4, 5, 6, 7, 11]].any() and changed[sel][:, [0, 1, 2, 8, 9, 10]].all()
    # the stored-pose rule: identity keeps the pose, an unselected tick keeps it
    P = _D((0, 1, 0), 5.0, (1, 2, 3))
    assert np.array_equal(_bits(wr.warp_pose(P, 12, 10, np.repeat(IDENT12, 5, axis=0))), _bits(P))
    assert np.array_equal(_bits(wr.warp_pose(P, 9, 10, tab)), _bits(P))
    moved = wr.warp_pose(P, 12, 10, tab).reshape(4, 4).T.astype(np.float64)
    C4 = np.vstack([tab[2].reshape(3, 4), [0, 0, 0, 1]]).astype(np.float64)
    assert np.abs(moved - C4 @ P.reshape(4, 4).T.astype(np.float64)).max() < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# 1. the definition, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 1])
def test_definition_hand_made(tmp_path, n):
    t0 = 40
    m = _rows(301, _edge_times(t0, n), seed=n)
    tab = wr.rigid_table(n, seed=2)
    want = wr.warp_rows(m, t0, tab)
    sel, _ = wr.select(m[:, 7], t0, n)
    assert 0 < sel.sum() < 301 and (_bits(want) != _bits(m)).any()
    g = _gpu(35)
    g.upload_model(m)
    g.set_tick(60)
    c0, log0 = g.counts(), g.read_frame_log(4)
    path = str(tmp_path / "rows.bin")
    cr.write_map(path, m, 3, 9)
    g.warp_by_time([path], t0, tab)
    assert_models_equal(g.download_model(), want, "model")
    rows, a, b = rr.read_map(path)
    assert_models_equal(rows, want, "file")
    assert (a, b) == (3, 9)
    st = g.warp_stats()
    assert (st["files_listed"], st["files_read"], st["files_rewritten"], st["records_read"], st["chunks"]) == (1, 1, 1, 301, 1)
    assert st["records_moved"] == st["model_moved"] == int(sel.sum())
    assert g.counts() == c0 and np.array_equal(g.read_frame_log(4), log0)
    _no_temporaries(tmp_path)
    # the files alone: the model stays
    cr.write_map(path, m, 3, 9)
    g.warp_by_time([path], t0, tab, include_model=False)
    assert_models_equal(g.download_model(), want, "model left alone")
    assert_models_equal(rr.read_map(path)[0], want, "file again")
    assert g.warp_stats()["model_moved"] == 0
    # an empty source is a valid no-op
    g.warp_by_time([], t0, tab, include_model=False)
    assert g.warp_stats()["files_listed"] == 0


@pytest.mark.gpu
def test_definition_after_fused_frames(seq):
    """dead slots of the deferred compaction are no surfels: the result is defined on the downloaded rows, whatever the period"""
    tab = wr.rigid_table(3, seed=3, angle_deg=0.5, trans=0.1)
    t0 = 3                                                # ticks 3, 4 and 5: one table row each
    got = {}
    for cp in (24, 1):
        g = _gpu(440, compact_period=cp)
        for fr in seq[:6]:
            g.process_frame(*fr)
        log = g.read_frame_log(1)
        pending = int(log["n_slots"][-1]) - int(log["n_before"][-1])
        print(f"compact_period {cp}: {pending} dead slots pending at the warp")
        c0, log0 = g.counts(), g.read_frame_log(8)
        g.warp_by_time([], t0, tab)
        st = g.warp_stats()
        assert g.counts() == c0 and np.array_equal(g.read_frame_log(8), log0)
        got[cp] = (g.download_model(), st["model_moved"], g)
    h = _gpu(440)
    for fr in seq[:6]:
        h.process_frame(*fr)
    before = h.download_model()
    want = wr.warp_rows(before, t0, tab)
    sel, _ = wr.select(before[:, 7], t0, 3)
    assert 1000 < sel.sum() < len(before)
    for cp in (24, 1):
        assert_models_equal(got[cp][0], want, f"compact_period {cp}")
        assert got[cp][1] == int(sel.sum())


# ---------------------------------------------------------------------------------------------------------------------
# 2. the stored poses
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stored_poses_move_with_the_model(seq):
    g = _gpu(440)
    for fr in seq[:3]:
        g.process_frame(*fr)
    tick = g.counts()["tick"]
    assert tick == 3
    tab = wr.rigid_table(5, seed=4, angle_deg=0.05, trans=0.01)
    t0 = 0                                                # ticks 1 and 2 are selected, by different rows
    g.warp_by_time([], t0, tab)
    p1 = wr.warp_pose(seq[2][3], tick - 1, t0, tab)
    p2 = wr.warp_pose(seq[1][3], tick - 2, t0, tab)
    assert (_bits(p1) != _bits(seq[2][3])).any() and (_bits(p2) != _bits(seq[1][3])).any()
    want = wr.constant_velocity(p1, p2)
    _, info = g.track(seq[3][1])
    got = info["guess"].T.reshape(16)
    assert np.array_equal(_bits(got), _bits(want)), np.abs(got - want).max()
    # a warp that selects only the newer tick
    g.warp_by_time([], 2, tab)
    want = wr.constant_velocity(wr.warp_pose(p1, 2, 2, tab), p2)
    _, info = g.track(seq[3][1])
    assert np.array_equal(_bits(info["guess"].T.reshape(16)), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------
# 3. frames after a warp
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_frames_after_a_warp(seq):
    """a rigid whole-model warp G, then three more frames at G * P_k, against a fresh context that was handed the restated
    warped model: stale tile boxes or a forgotten flush of the held-back association would show (the recall sequence, 312 x 94)"""
    from surfelmapping_amd import synth
    G = np.eye(4)
    G[:3, :3] = wr.rigid_table(1, seed=5, angle_deg=25.0)[0].reshape(3, 4)[:, :3].astype(np.float64)
    G[:3, 3] = (40.0, -3.0, 25.0)
    G = G.astype(f32)
    tab = wr.table_of(G)
    moved_pose = [(G.astype(np.float64) @ np.asarray(fr[3], f32).reshape(4, 4).T.astype(np.float64)).astype(f32).T.reshape(16).copy() for fr in seq]
    a = _gpu(440)
    for fr in seq[:6]:
        a.process_frame(*fr)
    # (no download of `a` before the warp: it would compact, and the warp must meet the dead slots)
    a.warp_by_time([], -1000, tab)
    ref = _gpu(440)
    for fr in seq[:6]:
        ref.process_frame(*fr)
    before = ref.download_model()
    want = wr.warp_rows(before, -1000, tab)
    assert a.warp_stats()["model_moved"] == len(before)
    b = _gpu(440)
    b.process_frame(seq[5][0], seq[5][1], seq[5][2], moved_pose[5])      # a fresh context's first frame fuses nothing
    b.upload_model(want)
    b.set_tick(6)
    for k in (6, 7, 8):
        for g in (a, b):
            g.process_frame(seq[k][0], seq[k][1], seq[k][2], moved_pose[k])
        ca, cb = a.counts(), b.counts()
        assert ca == cb, (k, ca, cb)
    assert_models_equal(a.download_model(), b.download_model(), "three frames after the warp")
    assert len(a.download_model()) > len(before)


# ---------------------------------------------------------------------------------------------------------------------
# 4. chunking
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chunking(tmp_path):
    from surfelmapping_amd import synth
    n0, n1 = (1 << 20) + 70001, 4999
    big, small, live = synth.seeded_model(n0, 400, seed=5), synth.seeded_model(n1, 400, seed=6), synth.seeded_model(1001, 400, seed=7)
    old = synth.seeded_model(777, 150, seed=8)
    assert old[:, 7].max() < 200
    paths = [str(tmp_path / f) for f in ("big.bin", "small.bin", "old.bin")]
    cr.write_map(paths[0], big, 1, 2)
    cr.write_map(paths[1], small, 3, 4)
    cr.write_map(paths[2], old, 5, 6)
    t0, tab = 200, wr.rigid_table(150, seed=9, angle_deg=0.01, trans=0.01)
    sel = wr.select(big[:, 7], t0, 150)[0]
    assert n0 / 10 < sel.sum() < n0 and sel[: 1 << 20].any() and sel[1 << 20:].any() and (~sel)[1 << 20:].any()
    g = _gpu(40)
    g.upload_model(live)
    g.set_tick(400)
    g.warp_by_time(paths[:2], t0, tab)
    st = g.warp_stats()
    assert st["chunks"] == 3 and st["records_read"] == n0 + n1 and st["files_read"] == 2 and st["files_rewritten"] == 2
    assert st["records_moved"] == int(sel.sum() + wr.select(small[:, 7], t0, 150)[0].sum())
    assert_models_equal(g.download_model(), wr.warp_rows(live, t0, tab), "model")
    assert_models_equal(rr.read_map(paths[0])[0], wr.warp_rows(big, t0, tab), "big file")
    assert_models_equal(rr.read_map(paths[1])[0], wr.warp_rows(small, t0, tab), "small file")
    assert rr.read_map(paths[0])[1:] == (1, 2)
    _no_temporaries(tmp_path)
    # a file whose times are all below t0 keeps its bytes and its mtime
    was = _snapshot(paths[2:])
    g.warp_by_time(paths[1:], t0, tab, include_model=False)
    assert _snapshot(paths[2:]) == was and g.warp_stats()["files_rewritten"] == 1
    # only the second chunk of the big file holds selected rows: the temporary starts with the untouched chunk
    z = big.copy()
    z[: 1 << 20, 7] = f32(100.0)
    cr.write_map(paths[0], z, 1, 2)
    g.warp_by_time(paths[:1], t0, tab, include_model=False)
    assert g.warp_stats()["records_moved"] == int(sel[1 << 20:].sum())
    assert_models_equal(rr.read_map(paths[0])[0], wr.warp_rows(z, t0, tab), "second chunk alone moves")
    _no_temporaries(tmp_path)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the file index
# ---------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys, numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_warp as t
import warp_ref as wr, recall_ref as cr
g = t._gpu(64)
g.upload_model(t._rows(50, [5.0, 105.0, 205.0]))
paths = {paths!r}
tab = wr.rigid_table(4, seed=12)
out = []
def note():
    st = g.warp_stats()
    out.append((st["files_skipped"], st["files_read"], st["files_rewritten"]))
g.warp_by_time(paths, 1000, tab); note()          # nothing selected, everything learnt
g.warp_by_time(paths, 150, tab); note()           # two files end before t0
g.warp_by_time(paths, 150, tab); note()           # the rewritten file's entry is fresh: still only that one is read
far = np.eye(4, dtype=np.float32).T.reshape(16).copy(); far[12:15] = (0, 0, 50000.0)
g.recall(paths, pose=far, mode="count", radius=8.0)
out.append(g.recall_stats()["files_skipped"])      # the warped box is known: a recall from afar opens nothing
# a file the retirement policy writes is known without ever having been read
h = t._gpu(440)                                   # (set_tick makes the next frame a fusing one: room for its surfels)
rows = t._rows(40, [0.0]); rows[:, 2] += np.float32(1000.0)
h.upload_model(rows)
h.set_tick(49)
h.set_auto_retire(1, {prefix!r}, min_age=8, min_distance=15.0)
fr = cr.sequence(1)[0]
h.process_frame(*fr)
nf, ns = h.auto_retire_stats()
pf = [{prefix!r} + "_%06d.bin" % i for i in range(nf)]
h.warp_by_time(pf, 1000, tab, include_model=False)
st = h.warp_stats()
out.append((nf, ns, st["files_skipped"], st["files_read"]))
np.save({out!r}, g.download_model())
print("RESULT", out)
"""


def _index_files(d):
    paths = [str(d / f"i{i}.bin") for i in range(3)]
    for i, p in enumerate(paths):
        cr.write_map(p, _rows(300, 100.0 * i + np.arange(10), seed=20 + i), i, i)
    return paths


@pytest.mark.gpu
def test_file_index(tmp_path):
    res = {}
    for sw in ("0", "1"):
        d = tmp_path / ("b" + sw)
        d.mkdir()
        ps = _index_files(d)
        env = dict(os.environ, SM_RECALL_NO_INDEX=sw)
        out = str(d / "model.npy")
        code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), paths=ps, out=out, prefix=str(d / "ret"))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        txt = r.stdout
        line = [l for l in txt.splitlines() if l.startswith("RESULT")][0]
        res[sw] = (eval(line[7:]), np.load(out), [open(p, "rb").read() for p in ps])
    on, off = res["0"][0], res["1"][0]
    assert on[0] == (0, 3, 0) and on[1] == (2, 1, 1) and on[2] == (2, 1, 1) and on[3] == 3, on
    assert off[0] == (0, 3, 0) and off[1] == (0, 3, 1) and off[2] == (0, 3, 1) and off[3] == 0, off
    assert on[4][0] == 1 and on[4][1] == 40 and on[4][2:] == (1, 0), on
    assert off[4][:2] == on[4][:2] and off[4][2:] == (0, 1), off
    assert_models_equal(res["0"][1], res["1"][1], "model with and without the index")
    assert res["0"][2] == res["1"][2]
    # ... and they are the restatement's
    tab = wr.rigid_table(4, seed=12)
    for i, blob in enumerate(res["0"][2]):
        rows = _rows(300, 100.0 * i + np.arange(10), seed=20 + i)
        want = wr.warp_rows(wr.warp_rows(rows, 150, tab), 150, tab)
        assert blob[12:] == want.tobytes(), i


# ---------------------------------------------------------------------------------------------------------------------
# 6. durability and errors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_failures_change_nothing(tmp_path):
    from surfelmapping_amd import capi
    g = _gpu(35)
    with pytest.raises(capi.SurfelMapError):
        g.warp_stats()
    m = _rows(301, _edge_times(40, 5), seed=30)
    g.upload_model(m)
    g.set_tick(60)
    tab = wr.rigid_table(5, seed=31)
    paths = [str(tmp_path / f"f{i}.bin") for i in range(3)]
    for i, p in enumerate(paths):
        cr.write_map(p, _rows(280 + i, _edge_times(40, 5), seed=32 + i), i, i)
    snap = _snapshot(paths)

    def unchanged(what):
        assert _snapshot(paths) == snap, what
        assert_models_equal(g.download_model(), m, what)
        _no_temporaries(tmp_path)

    def refused(ps, t0=40, table=tab, rc=capi.SM_E_ARG, include_model=True):
        with pytest.raises(capi.SurfelMapError) as e:
            g.warp_by_time(ps, t0, table, include_model=include_model)
        assert e.value.rc == rc, e.value
    refused([paths[0], paths[1], paths[0]])
    unchanged("a path listed twice")
    short = str(tmp_path / "short.bin")
    open(short, "wb").write(snap[2][0][:-5])
    refused([paths[0], short])
    unchanged("a truncated file")
    refused([paths[0], str(tmp_path / "missing.bin")])
    unchanged("a missing file")
    bad = tab.copy()
    bad[3, 7] = np.nan
    refused(paths, table=bad)
    unchanged("a non-finite table entry")
    src = capi.map_source(paths)
    assert g._L.sm_warp_by_time(g._h, C.byref(src), 40, 0, tab.ctypes.data_as(C.c_void_p)) == capi.SM_E_ARG
    assert g._L.sm_warp_by_time(g._h, C.byref(src), 40, 5, None) == capi.SM_E_ARG
    assert g._L.sm_warp_by_time(g._h, None, 40, 5, tab.ctypes.data_as(C.c_void_p)) == capi.SM_E_ARG
    nul = capi.SmMapSource(None, 2, 1)
    assert g._L.sm_warp_by_time(g._h, C.byref(nul), 40, 5, tab.ctypes.data_as(C.c_void_p)) == capi.SM_E_ARG
    unchanged("bad arguments")
    os.remove(short)
    # a temporary that cannot be written, because something that is no file has its name: the temporaries before it are removed
    os.mkdir(paths[1] + ".warp.tmp")
    try:
        refused(paths)
    finally:
        os.rmdir(paths[1] + ".warp.tmp")
    unchanged("a temporary that could not be opened")
    # a directory that cannot be written
    if os.geteuid() != 0:
        os.chmod(tmp_path, 0o555)
        try:
            refused(paths)
        finally:
            os.chmod(tmp_path, 0o755)
        unchanged("a read-only directory")
    else:
        print("running as root: a read-only directory cannot be provoked")
    # the same call goes through once nothing is in the way
    g.warp_by_time(paths, 40, tab)
    assert_models_equal(g.download_model(), wr.warp_rows(m, 40, tab), "model")
    for i, p in enumerate(paths):
        assert_models_equal(rr.read_map(p)[0], wr.warp_rows(_rows(280 + i, _edge_times(40, 5), seed=32 + i), 40, tab), p)
    # a sharded context holds only its own surfels
    s = _gpu(35)
    assert s._L.sm_shard_stream_configure(s._h, 0, 1) == 0
    src = capi.map_source([])
    assert s._L.sm_warp_by_time(s._h, C.byref(src), 40, 5, tab.ctypes.data_as(C.c_void_p)) == capi.SM_E_UNSUPPORTED
