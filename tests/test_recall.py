"""Paging in (sm_recall / sm_set_auto_recall, SurfelMap.recall / set_auto_recall; DESIGN.md "4g. Paging in").  The definition is
the numpy predicate of tests/recall_ref.py; the CPU oracle has the equivalent without touching it: upload_model(concat(model,
recalled rows)), which changes neither its tick nor its images."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import recall_ref as cr
import retire_ref as rr
from backends import assert_models_equal

CAM, OVER = cr.CAM, cr.OVER
IDENT = np.eye(4, dtype=np.float32).T.reshape(16).copy()
IMG = (160, 60, 90.0, 90.0, 79.5, 29.5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _gpu(cap=440, **over):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=cap, **over))


def _pose(x=0.0, y=0.0, z=0.0):
    p = IDENT.copy()
    p[12:15] = (x, y, z)
    return p


def _rows(n, pos=(0.0, 0.0, 0.0), t=0.0):
    """n hand-made surfels: position `pos` (one, or one per row), row number in the creation time"""
    m = np.zeros((n, 12), f32)
    m[:, 0:3] = np.asarray(pos, f32)
    m[:, 3] = 5.0
    m[:, 4] = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) | np.uint32(0x03000000)).view(f32)
    m[:, 6] = np.arange(n) % 4096
    m[:, 7] = t
    m[:, 10] = -1.0
    m[:, 11] = 0.05
    return m


def _same_counts(g, o, what=""):
    cg, co = g.counts(), o.counts()
    assert all(cg[k] == co[k] for k in co), (what, cg, co)


def _snapshot(paths):
    return [(open(p, "rb").read(), os.stat(p).st_mtime_ns) for p in paths]


def _no_temporaries(d):
    assert not [f for f in os.listdir(d) if f.endswith(".recall.tmp")]


@pytest.fixture(autouse=True)
def _clean_env():
    os.environ.pop("SM_RECALL_NO_INDEX", None)
    yield
    os.environ.pop("SM_RECALL_NO_INDEX", None)


@pytest.fixture(scope="module")
def seq():
    return cr.sequence()


@pytest.fixture(scope="module")
def oracle_a(seq):
    return cr.oracle_run(seq, **cr.A)


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_recall_symbols():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ("sm_default_recall_params", "sm_recall", "sm_recall_stats", "sm_set_auto_recall", "sm_auto_recall_stats"):
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert (capi.SM_RECALL_MOVE, capi.SM_RECALL_COPY, capi.SM_RECALL_COUNT) == (0, 1, 2)
    cfg = capi.make_config(**CAM, **OVER)
    assert capi.recall_params(cfg).radius == f32(1.5) * f32(cfg.far_clip) == capi.retire_params(cfg).min_distance
    assert capi.recall_params(cfg, radius=3.0).radius == 3.0


def test_ctypes_mirrors_have_the_header_layout(tmp_path):
    from surfelmapping_amd import capi
    mirrors = {"sm_recall_params": capi.SmRecallParams, "sm_recall_stats_t": capi.SmRecallStats}
    lines = []
    for cname, cls in mirrors.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("modes %d %d %d\\n", SM_RECALL_MOVE, SM_RECALL_COPY, SM_RECALL_COUNT);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sm_c_api.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    out = subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines()
    got = dict(l.split(None, 1) for l in out)
    assert got["modes"] == "0 1 2"
    for cname, cls in mirrors.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_arguments_are_rejected_before_any_device_call():
    from surfelmapping_amd import capi
    L = capi.load()
    src = capi.map_source([], include_model=False)
    n = C.c_uint32()
    p = capi.SmRecallParams(5.0)
    assert L.sm_recall(None, C.byref(src), None, C.byref(p), capi.SM_RECALL_COUNT, C.byref(n)) == capi.SM_E_ARG
    assert L.sm_recall_stats(None, None) == capi.SM_E_ARG
    assert L.sm_set_auto_recall(None, C.byref(p)) == capi.SM_E_ARG
    assert L.sm_auto_recall_stats(None, None, None) == capi.SM_E_ARG
    assert L.sm_default_recall_params(None, C.byref(p)) == capi.SM_E_ARG


def test_box_test_never_skips_a_near_row():
    """the index's box test restated in numpy (recall_ref.box_out_of_reach) against the predicate: random boxes and centres, and
    rows exactly at d2 == r^2 and one ulp to either side with the box drawn tightly round them"""
    rng = np.random.default_rng(11)
    skipped = tested = 0
    for trial in range(400):
        scale = f32(10.0 ** rng.uniform(-2, 4))
        lo = (rng.uniform(-1, 1, 3) * scale).astype(f32)
        hi = lo + (rng.uniform(0, 1, 3) * scale * rng.choice([0.0, 0.01, 1.0])).astype(f32)
        rows = np.zeros((256, 12), f32)
        rows[:, 0:3] = (lo + (hi - lo) * rng.uniform(0, 1, (256, 3)).astype(f32)).clip(lo, hi)
        rows[:8, 0:3] = [[(hi if (c >> a) & 1 else lo)[a] for a in range(3)] for c in range(8)]      # the corners
        c = (lo + (hi - lo) * 0.5 + rng.normal(size=3) * scale * rng.choice([0.1, 1.0, 3.0])).astype(f32)
        pose = _pose(*c)
        for radius in (rng.uniform(0.01, 3.0) * scale, scale * 1e-3):
            out = bool(cr.box_out_of_reach(lo, hi, c, radius))
            tested += 1
            skipped += out
            assert not (out and cr.near(rows, pose, radius).any()), (trial, lo, hi, c, radius)
    assert 50 < skipped < tested - 50, (skipped, tested)         # both outcomes are exercised
    # a single row, the box is the row: the radius whose square is exactly d2, and its neighbours
    for trial in range(300):
        q = (rng.normal(size=3) * 30).astype(f32)
        c = (rng.normal(size=3) * 30).astype(f32)
        d = q - c
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        row = np.zeros((1, 12), f32)
        row[0, 0:3] = q
        r0 = np.sqrt(d2)
        for r in (np.nextafter(r0, f32(0)), r0, np.nextafter(r0, f32(np.inf)), np.nextafter(np.nextafter(r0, f32(0)), f32(0))):
            nr = bool(cr.near(row, _pose(*c), r)[0])
            assert nr == bool(d2 <= r * r)
            assert not (nr and cr.box_out_of_reach(q, q, c, r))
            # the point box is exact: it skips precisely the rows that are not near
            assert bool(cr.box_out_of_reach(q, q, c, r)) == (not nr)
    # d2 == r^2 exactly (every step is exact in fp32), and the floats next to that row
    c, r = np.array([1.5, -2.25, 7.0], f32), f32(3.0)
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            at = c.copy()
            at[ax] += f32(sgn) * r
            out = at[ax]
            while (out - c[ax]) * (out - c[ax]) <= r * r:              # the first float whose own dx*dx exceeds r^2
                out = np.nextafter(out, f32(sgn * np.inf))
            for x, want in ((at[ax], True), (out, False), (np.nextafter(out, c[ax]), True), (np.nextafter(at[ax], c[ax]), True)):
                q = at.copy()
                q[ax] = x
                row = np.zeros((1, 12), f32)
                row[0, 0:3] = q
                assert bool(cr.near(row, _pose(*c), r)[0]) == want
                assert bool(cr.box_out_of_reach(q, q, c, r)) == (not want)
                assert not (want and cr.box_out_of_reach(np.minimum(q, c + 9), np.maximum(q, c + 9), c, r))
    # an empty box (a file without a finite row) is always out of reach; a NaN row is never near
    assert cr.box_out_of_reach([np.inf] * 3, [-np.inf] * 3, [0, 0, 0], 1e9)
    bad = _rows(3)
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    assert not cr.near(bad, IDENT, 1e18).any()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the definition, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _drive(seq, n, tmp_path, name, cp, cap=440, **params):
    """the GPU over seq[:n] with the retirement policy of scenario A: (context, paths of its files)"""
    g = _gpu(cap, compact_period=cp)
    prefix = str(tmp_path / name)
    g.set_auto_retire(cr.EVERY, prefix, min_age=cr.MIN_AGE, min_distance=params.get("min_distance", cr.A["min_distance"]))
    for fr in seq[:n]:
        g.process_frame(*fr)
    nf, _ = g.auto_retire_stats()
    return g, [f"{prefix}_{i:06d}.bin" for i in range(nf)]


@pytest.mark.gpu
@pytest.mark.parametrize("cp", [1, 24])
@pytest.mark.parametrize("mode", ["move", "copy"])
def test_definition_bit_for_bit(seq, tmp_path, cp, mode):
    # the oracle retires in lockstep and does NOT recall: the files at tick 80 are those of the retirement policy alone
    # (capacity 900: the twenty frames after the recall run without a policy)
    ref = cr.oracle_run(seq, cr.A["min_distance"], 0.0, 900, recall=False, stop=79)
    o = ref["o"]
    g, paths = _drive(seq, 79, tmp_path, "d", cp, cap=900)
    # one more frame without the policy, so that the recall meets the model as a frame leaves it (dead slots pending)
    g.set_auto_retire(0, None)
    g.process_frame(*seq[79])
    o.process_frame(*seq[79])
    log = g.read_frame_log(1)
    pending = int(log["n_slots"][-1]) - int(log["n_before"][-1])
    print(f"compact_period {cp}: {pending} dead slots pending at the recall")
    if cp == 24:
        assert pending > 0
    assert g.counts()["tick"] == o.counts()["tick"] == 80 and len(paths) == len(ref["files"]) == 7
    files = [rr.read_map(p) for p in paths]
    for (rows, a, b), want in zip(files, ref["files"]):
        assert_models_equal(rows, want[0], "file before the recall")
    pose, radius = seq[79][3], 15.0
    nr = [cr.near(f[0], pose, radius) for f in files]
    R = np.concatenate([f[0][k] for f, k in zip(files, nr)])
    assert 1000 < len(R) < sum(len(f[0]) for f in files) - 1000
    before = _snapshot(paths)
    m = o.download_model()
    assert g.recall(paths, pose=pose, mode="count", radius=radius) == len(R)
    assert _snapshot(paths) == before
    assert g.recall(paths, pose=pose, mode=mode, radius=radius) == len(R)
    st = g.recall_stats()
    assert st["recalled"] == len(R) and st["files_listed"] == 7
    both = np.concatenate([m, R])
    assert_models_equal(g.download_model(), both, "model after the recall")
    o.upload_model(both)
    _same_counts(g, o, "after the recall")
    assert g.counts()["count"] == g.counts()["offset"] == len(both) and g.counts()["tick"] == 80
    _no_temporaries(tmp_path)
    if mode == "copy":
        assert _snapshot(paths) == before
        assert st["files_rewritten"] == 0
    else:
        assert st["files_rewritten"] == sum(bool(k.any()) for k in nr) > 0
        for p, f, k, was in zip(paths, files, nr, before):
            if k.any():
                rows, a, b = rr.read_map(p)
                assert_models_equal(rows, f[0][~k], p)
                assert (a, b) == (f[1], f[2])
            else:
                assert (open(p, "rb").read(), os.stat(p).st_mtime_ns) == was, p
    for k, fr in enumerate(seq[80:100]):
        g.process_frame(*fr)
        o.process_frame(*fr)
        _same_counts(g, o, f"frame {80 + k}")
    assert_models_equal(g.download_model(), o.download_model(), "20 frames later")


# ---------------------------------------------------------------------------------------------------------------------
# 2. COUNT and SM_E_CAPACITY leave no trace
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_count_and_capacity_leave_no_trace(seq, tmp_path):
    from surfelmapping_amd import capi
    a, paths = _drive(seq, 40, tmp_path, "a", 24)
    b, _ = _drive(seq, 40, tmp_path, "b", 24)
    a.set_auto_retire(0, None)
    b.set_auto_retire(0, None)
    # a file so large that the recall cannot fit (capacity 440^2 = 193 600)
    big = _rows(200000, (0.0, 0.0, 0.8 * 39))
    cr.write_map(tmp_path / "big.bin", big)
    paths = paths + [str(tmp_path / "big.bin")]
    before = _snapshot(paths)
    want = sum(int(cr.near(rr.read_map(p)[0], seq[39][3], 15.0).sum()) for p in paths)
    assert a.recall(paths, mode="count", radius=15.0) == want >= 200000          # (NULL pose: that of the last frame)
    for mode in ("move", "copy"):
        with pytest.raises(capi.SurfelMapError) as e:
            a.recall(paths, mode=mode, radius=15.0)
        assert e.value.rc == capi.SM_E_CAPACITY
        n = C.c_uint32()
        src = capi.map_source(paths, include_model=False)
        p = capi.SmRecallParams(15.0)
        rc = a._L.sm_recall(a._h, C.byref(src), None, C.byref(p), capi.RECALL_MODE[mode], C.byref(n))
        assert rc == capi.SM_E_CAPACITY and n.value == want
    assert _snapshot(paths) == before
    _no_temporaries(tmp_path)
    assert a.counts() == b.counts()
    assert np.array_equal(a.read_frame_log(), b.read_frame_log())
    for fr in seq[40:46]:
        a.process_frame(*fr)
        b.process_frame(*fr)
        assert a.counts() == b.counts()
    assert np.array_equal(a.read_frame_log(), b.read_frame_log())
    assert_models_equal(a.download_model(), b.download_model(), "after a COUNT and a refused recall")


# ---------------------------------------------------------------------------------------------------------------------
# 3. edges, hand-made
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_edges_hand_made(tmp_path):
    from surfelmapping_amd import capi
    c = np.array([1.5, -2.25, 7.0], f32)
    r = f32(3.0)
    # rows on the x axis from c: d2 == r^2 exactly, the next float above, NaN, +inf, and one well inside
    x_at = c[0] + r
    assert (x_at - c[0]) * (x_at - c[0]) == r * r
    x_up = x_at
    while (x_up - c[0]) * (x_up - c[0]) <= r * r:
        x_up = np.nextafter(x_up, f32(np.inf))
    pos = np.tile(c, (6, 1))
    pos[:, 0] = [x_at, x_up, np.nan, np.inf, c[0] + 1.0, -np.inf]
    f0 = _rows(6, pos)
    f2 = _rows(5, c + f32(0.5), t=2.0)            # every row comes back: the file is emptied
    f3 = _rows(4, c + f32(50.0), t=3.0)           # none does: untouched
    paths = [str(tmp_path / f"e{i}.bin") for i in range(4)]
    cr.write_map(paths[0], f0, 3, 9)
    cr.write_map(paths[1], np.zeros((0, 12), f32), 10, 11)         # an empty file
    cr.write_map(paths[2], f2, 12, 13)
    cr.write_map(paths[3], f3, 14, 15)
    live = _rows(7, c + f32(100.0), t=9.0)
    g = _gpu(64)
    g.upload_model(live)
    g.set_tick(20)
    pose = _pose(*c)
    want0 = cr.near(f0, pose, r)
    assert want0.tolist() == [True, False, False, False, True, False]
    before = _snapshot(paths)
    # the order of R is the order of the paths, then of the rows
    order = [paths[2], paths[0], paths[1], paths[3]]
    assert g.recall(order, pose=pose, mode="move", radius=float(r)) == 7
    assert_models_equal(g.download_model(), np.concatenate([live, f2, f0[want0]]), "file order and row order")
    assert g.counts()["count"] == g.counts()["offset"] == 14 and g.counts()["tick"] == 20
    rows, a, b = rr.read_map(paths[0])
    assert_models_equal(rows, f0[~want0], "NaN and inf rows stay")
    assert (a, b) == (3, 9)
    assert os.path.getsize(paths[2]) == 12 and rr.read_map(paths[2])[1:] == (12, 13)          # emptied: header alone
    assert (open(paths[1], "rb").read(), os.stat(paths[1]).st_mtime_ns) == before[1]
    assert (open(paths[3], "rb").read(), os.stat(paths[3]).st_mtime_ns) == before[3]
    assert g.recall_stats()["files_rewritten"] == 2
    _no_temporaries(tmp_path)
    # the emptied and the empty file still load in the streamed renderer
    view = _pose(*(c + f32([0, 0, -5])))
    bgr, sem = g.render_image_maps(paths, view[None], *IMG, include_model=True)
    assert bgr.shape == (1, IMG[1], IMG[0], 3)

    # a duplicate path: refused in MOVE (nothing changes), fine in COPY and COUNT
    m0 = g.download_model()
    snap = _snapshot(paths)
    with pytest.raises(capi.SurfelMapError):
        g.recall([paths[3], paths[0], paths[3]], pose=_pose(*(c + f32(50.0))), mode="move", radius=1.0)
    assert g.recall([paths[3], paths[3]], pose=_pose(*(c + f32(50.0))), mode="count", radius=1.0) == 8
    # a truncated file: refused, named, nothing changed -- although an earlier file of the list has near rows
    with open(paths[0], "r+b") as f:
        f.truncate(12 + 48 * 3 + 7)
    with pytest.raises(capi.SurfelMapError) as e:
        g.recall([paths[3], paths[0]], pose=_pose(*(c + f32(50.0))), mode="move", radius=1.0)
    assert "e0.bin" in str(e.value)
    cr.write_map(paths[0], f0[~want0], 3, 9)
    snap = _snapshot(paths)
    assert_models_equal(g.download_model(), m0, "after refused calls")
    # bad arguments
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf"))):
        with pytest.raises(capi.SurfelMapError):
            g.recall(paths, pose=pose, mode="count", **kw)
    bad = pose.copy()
    bad[13] = np.nan
    with pytest.raises(capi.SurfelMapError):
        g.recall(paths, pose=bad, mode="count", radius=1.0)
    n = C.c_uint32()
    src = capi.map_source(paths, include_model=False)
    assert g._L.sm_recall(g._h, C.byref(src), None, None, 3, C.byref(n)) == capi.SM_E_ARG              # unknown mode
    assert g._L.sm_recall(g._h, C.byref(src), None, None, capi.SM_RECALL_COUNT, None) == capi.SM_E_ARG
    src1 = capi.map_source(paths, include_model=True)
    assert g._L.sm_recall(g._h, C.byref(src1), None, None, capi.SM_RECALL_COUNT, C.byref(n)) == capi.SM_E_ARG
    nul = capi.SmMapSource(None, 2, 0)
    assert g._L.sm_recall(g._h, C.byref(nul), None, None, capi.SM_RECALL_COUNT, C.byref(n)) == capi.SM_E_ARG
    assert _snapshot(paths) == snap
    assert_models_equal(g.download_model(), m0, "after bad arguments")

    # a directory that cannot be written: SM_E_ARG, model and files unchanged
    if os.geteuid() != 0:
        os.chmod(tmp_path, 0o555)
        try:
            with pytest.raises(capi.SurfelMapError):
                g.recall([paths[3]], pose=_pose(*(c + f32(50.0))), mode="move", radius=1.0)
        finally:
            os.chmod(tmp_path, 0o755)
        assert _snapshot(paths) == snap
        assert_models_equal(g.download_model(), m0, "after a temporary that could not be written")
        _no_temporaries(tmp_path)
    else:
        print("running as root: a read-only directory cannot be provoked")


@pytest.mark.gpu
def test_stats_before_the_first_call():
    from surfelmapping_amd import capi
    g = _gpu(64)
    with pytest.raises(capi.SurfelMapError):
        g.recall_stats()
    assert g.auto_recall_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. chunking
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chunking(tmp_path):
    from surfelmapping_amd import synth
    n0, n1 = (1 << 20) + 70001, 4999
    assert n0 % 256 and n0 % 64 and n1 % 256 and n1 % 64
    big, small = synth.seeded_model(n0, 400, seed=5), synth.seeded_model(n1, 400, seed=6)
    paths = [str(tmp_path / "big.bin"), str(tmp_path / "small.bin")]
    cr.write_map(paths[0], big, 1, 2)
    cr.write_map(paths[1], small, 3, 4)
    pose = _pose(0.0, 1.0, 100.0)
    radius = 62.0
    k0, k1 = cr.near(big, pose, radius), cr.near(small, pose, radius)
    assert n0 / 10 < k0.sum() < n0 / 2 and k0[: 1 << 20].any() and k0[1 << 20:].any() and (~k0)[1 << 20:].any()
    live = synth.seeded_model(1001, 400, seed=7)
    g = _gpu(1100)
    g.upload_model(live)
    g.set_tick(400)
    want = int(k0.sum() + k1.sum())
    assert g.recall(paths, pose=pose, mode="move", radius=radius) == want
    st = g.recall_stats()
    assert st["chunks"] == 3 and st["records_read"] == n0 + n1 and st["files_read"] == 2 and st["files_rewritten"] == 2
    assert_models_equal(g.download_model(), np.concatenate([live, big[k0], small[k1]]), "model")
    assert_models_equal(rr.read_map(paths[0])[0], big[~k0], "big file")
    assert_models_equal(rr.read_map(paths[1])[0], small[~k1], "small file")
    assert rr.read_map(paths[0])[1:] == (1, 2)
    _no_temporaries(tmp_path)
    # a file whose first chunk loses nothing and whose second does: the temporary starts with the untouched chunk
    z = big.copy()
    z[: 1 << 20, 2] += f32(1000.0)
    cr.write_map(paths[0], z, 1, 2)
    kz = cr.near(z, pose, radius)
    assert not kz[: 1 << 20].any() and kz.any()
    g.upload_model(live)
    assert g.recall(paths[:1], pose=pose, mode="move", radius=radius) == int(kz.sum())
    assert_models_equal(rr.read_map(paths[0])[0], z[~kz], "second chunk alone loses rows")
    assert_models_equal(g.download_model(), np.concatenate([live, z[kz]]), "model")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the file index
# ---------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys, numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import test_recall as t
g = t._gpu(64)
g.upload_model(t._rows(3, (0, 0, 0)))
paths = {paths!r}
out = []
for z in (5.0, 500.0, 105.0, 5.0):
    out.append(g.recall(paths, pose=t._pose(0, 0, z), mode="move", radius=8.0))
    out.append(g.recall_stats()["files_skipped"])
np.save({out!r}, g.download_model())
print("RESULT", out)
"""


def _index_files(d):
    paths = [str(d / f"i{i}.bin") for i in range(3)]
    for i, p in enumerate(paths):
        cr.write_map(p, _rows(300, [(0.01 * k, 0.0, 100.0 * i + 0.02 * k) for k in range(300)], t=float(i)), i, i)
    return paths


@pytest.mark.gpu
def test_file_index(tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    paths = _index_files(tmp_path / "a")
    g = _gpu(64)
    g.upload_model(_rows(3, (0, 0, 0)))
    far = _pose(0, 0, 5000.0)
    assert g.recall(paths, pose=far, mode="count", radius=8.0) == 0
    st = g.recall_stats()
    assert (st["files_listed"], st["files_skipped"], st["files_read"]) == (3, 0, 3)          # nothing known yet: all read
    assert g.recall(paths, pose=far, mode="move", radius=8.0) == 0
    st = g.recall_stats()
    assert (st["files_listed"], st["files_skipped"], st["files_read"], st["records_read"]) == (3, 3, 0, 0)
    # near one file: that one is read, the others are not
    rows1 = rr.read_map(paths[1])[0]
    want = int(cr.near(rows1, _pose(0, 0, 103.0), 2.0).sum())
    assert 0 < want < 300
    assert g.recall(paths, pose=_pose(0, 0, 103.0), mode="move", radius=2.0) == want
    st = g.recall_stats()
    assert (st["files_skipped"], st["files_read"], st["files_rewritten"]) == (2, 1, 1)
    # the rewrite has updated the entry: still skipped from afar
    g.recall(paths, pose=far, mode="count", radius=8.0)
    assert g.recall_stats()["files_skipped"] == 3
    # a file rewritten behind the context's back, with rows where the old box was not: the entry is void
    moved = _rows(301, (0.0, 0.0, 5000.0))
    cr.write_map(paths[0], moved, 0, 0)
    assert g.recall(paths, pose=far, mode="copy", radius=8.0) == 301
    st = g.recall_stats()
    assert (st["files_skipped"], st["files_read"]) == (2, 1)
    # the A/B switch in fresh processes: the same model and files either way
    res = {}
    for sw in ("0", "1"):
        d = tmp_path / ("b" + sw)
        d.mkdir()
        ps = _index_files(d)
        env = dict(os.environ, SM_RECALL_NO_INDEX=sw)
        out = str(d / "model.npy")
        code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), paths=ps, out=out)
        txt = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True, text=True, timeout=300).stdout
        line = [l for l in txt.splitlines() if l.startswith("RESULT")][0]
        res[sw] = (eval(line[7:]), np.load(out), [open(p, "rb").read() for p in ps])
    on, off = res["0"], res["1"]
    assert on[0][0::2] == off[0][0::2] and sum(on[0][0::2]) > 0
    assert sum(on[0][1::2]) > 0 and sum(off[0][1::2]) == 0                       # the index skipped; the switch turned it off
    assert_models_equal(on[1], off[1], "model with and without the index")
    assert on[2] == off[2]


# ---------------------------------------------------------------------------------------------------------------------
# 6. the policy, scenario A
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_policy_scenario_a(seq, oracle_a, tmp_path):
    from surfelmapping_amd import capi
    ref = oracle_a
    assert ref["rounds"] == cr.A_ROUNDS and ref["first_fail"] is None
    assert (ref["peak"], len(ref["files"]), ref["rewrites"], len(ref["model"]), sum(len(f[0]) for f in ref["files"])) == \
        tuple(cr.A_RECORD[k] for k in ("peak", "files", "rewrites", "final", "in_files"))
    g = _gpu(cr.A["max_sqrt_vertices"])
    prefix = str(tmp_path / "p")
    g.set_auto_retire(cr.EVERY, prefix, min_age=cr.MIN_AGE, min_distance=cr.A["min_distance"])
    g.set_auto_recall(radius=cr.A["radius"])
    rounds, rewrites, last, last_files, read_rounds = [], 0, (0, 0, 0, 0), (0, 0), []
    for k, fr in enumerate(seq):
        g.process_frame(*fr)                      # (SM_E_CAPACITY would raise)
        cg, co = g.counts(), ref["frame_counts"][k]
        assert all(cg[x] == co[x] for x in co), (k, cg, co)
        if cg["tick"] % cr.EVERY == 0:
            (nf, ns), (nr, nrs) = g.auto_retire_stats(), g.auto_recall_stats()
            rounds.append((cg["tick"], ns - last[1], nrs - last[3]))
            last = (nf, ns, nr, nrs)
            st = g.recall_stats()
            rewrites += st["files_rewritten"]
            # the file this round wrote is never read (all its rows are far by construction), and its box is known at once:
            # while the drive goes out, the older files lie behind and out of reach as well
            assert st["files_listed"] == nf and st["files_read"] <= nf - (1 if ns > last_files[1] else 0), (k, st)
            assert st["files_read"] + st["files_skipped"] == nf
            read_rounds.append(st["files_read"])
            last_files = (nf, ns)
    assert rounds == cr.A_ROUNDS
    print("files read per round:", read_rounds)
    assert sum(read_rounds) < sum(range(1, 14)) - 13          # the index and the fresh file's exemption both spared reads
    assert rewrites == cr.A_RECORD["rewrites"]
    assert g.auto_recall_stats() == (13, sum(r[2] for r in cr.A_ROUNDS))
    assert g.auto_retire_stats()[0] == 13
    assert_models_equal(g.download_model(), ref["model"], "final model")
    for i, want in enumerate(ref["files"]):
        rows, a, b = rr.read_map(f"{prefix}_{i:06d}.bin")
        assert_models_equal(rows, want[0], f"file {i}")
        assert (a, b) == (want[1], want[2])
    _no_temporaries(tmp_path)


@pytest.mark.gpu
def test_policy_setters_check_each_other(tmp_path):
    from surfelmapping_amd import capi
    prefix = str(tmp_path / "s")
    for md in (15.0, 0.0):
        g = _gpu(64)
        g.set_auto_retire(10, prefix, min_age=8, min_distance=md)
        with pytest.raises(capi.SurfelMapError):
            g.set_auto_recall(radius=16.0)
        if md > 0:
            g.set_auto_recall(radius=15.0)       # the earlier setting was left alone and a valid radius is accepted
        g = _gpu(64)
        g.set_auto_recall(radius=16.0)
        with pytest.raises(capi.SurfelMapError):
            g.set_auto_retire(10, prefix, min_age=8, min_distance=md)
        g.set_auto_retire(10, prefix, min_age=8, min_distance=16.0)
        g.set_auto_recall()                      # off


# ---------------------------------------------------------------------------------------------------------------------
# 7. lossless, scenario B
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lossless_scenario_b(seq, tmp_path):
    """With min_distance = radius = 1.5 * far_clip, files + model after the out-and-back drive are the model of a run that
    never retired, as a multiset of rows.  This is a property of THIS scenario, not a theorem: slot 0's immunity to the
    conflict pass, the W*H conflict cap and depth ties between surfels all depend on the model's order and size,
    which retirement and recall change."""
    ref = cr.oracle_run(seq, **cr.B)
    assert ref["peak"] == cr.B_RECORD["peak"] and ref["first_fail"] is None
    g, plain = _gpu(cr.B["max_sqrt_vertices"]), _gpu(cr.B["max_sqrt_vertices"])
    prefix = str(tmp_path / "b")
    g.set_auto_retire(cr.EVERY, prefix, min_age=cr.MIN_AGE, min_distance=cr.B["min_distance"])
    g.set_auto_recall(radius=cr.B["radius"])
    for fr in seq:
        g.process_frame(*fr)
        plain.process_frame(*fr)
    nf = g.auto_retire_stats()[0]
    assert nf == len(ref["files"])
    files = [rr.read_map(f"{prefix}_{i:06d}.bin")[0] for i in range(nf)]
    model = g.download_model()
    assert_models_equal(model, ref["model"], "model against the oracle's lockstep run")
    for i, (rows, want) in enumerate(zip(files, ref["files"])):
        assert_models_equal(rows, want[0], f"file {i}")
    everything = np.concatenate(files + [model])
    assert len(everything) == cr.B_RECORD["total"]
    assert np.array_equal(cr.sorted_rows(everything), cr.sorted_rows(plain.download_model()))


# ---------------------------------------------------------------------------------------------------------------------
# 8. downstream equality; 9. the streamed renderers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_downstream_equality(tmp_path):
    from surfelmapping_amd import synth
    seq = rr.sequence(48)
    a, paths = _drive(seq, 45, tmp_path, "r", 1)
    assert len(paths) == 4
    k = 30
    pose = seq[k][3]
    R = np.concatenate([f[cr.near(f, pose, 15.0)] for f in (rr.read_map(p)[0] for p in paths)])
    assert len(R) > 10000
    b, c = _gpu(440), _gpu(440)
    before = _snapshot(paths)
    assert b.recall(paths, pose=pose, mode="copy", radius=15.0) == len(R)
    assert _snapshot(paths) == before
    c.upload_model(R)
    for g in (b, c):
        g.set_tick(k)
        g.process_frame(*seq[k])
    assert b.counts() == c.counts()
    pb, ib = b.track(seq[k + 1][1])
    pc, ic = c.track(seq[k + 1][1])
    print("track status after a recall:", ib["status"], ib["inliers"], ib["rmse"])
    assert np.array_equal(pb.view(np.uint32), pc.view(np.uint32))
    assert {x: ib[x] for x in ("status_code", "iterations", "inliers")} == {x: ic[x] for x in ("status_code", "iterations", "inliers")}
    assert np.float32(ib["rmse"]).view(np.uint32) == np.float32(ic["rmse"]).view(np.uint32)
    view = seq[k][3]
    for x, y in zip(b.render_image(view, *IMG), c.render_image(view, *IMG)):
        assert np.array_equal(x, y)
    import model_view_ref as ref
    P = ref.projection(160, 120, 105.0, 105.0, 80.0, 60.0, 0.1, 1000.0)
    mvp, inv = ref.view_mats(P, ref.look_at(0, -6, 0.8 * k - 10, 0, 0, 0.8 * k + 20, 0, -1, 0))
    for x, y in zip(b.render_model(mvp, inv, 160, 120, depth=True, ids=True), c.render_model(mvp, inv, 160, 120, depth=True, ids=True)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.gpu
def test_streamed_renderers_left_alone(tmp_path):
    seq = rr.sequence(45)
    a, paths = _drive(seq, 45, tmp_path, "v", 1)
    pose = seq[30][3]
    whole = np.concatenate([rr.read_map(p)[0] for p in paths] + [a.download_model()])
    views = np.stack([seq[5][3], seq[30][3], seq[44][3]])
    n = a.recall(paths, pose=pose, mode="move", radius=15.0)
    assert n > 10000
    files = [rr.read_map(p)[0] for p in paths]
    big = _gpu(900)
    big.upload_model(np.concatenate(files + [a.download_model()]))
    assert sum(len(f) for f in files) + a.counts()["count"] == len(whole)
    bgr, sem = a.render_image_maps(paths, views, *IMG, include_model=True)
    for i, v in enumerate(views):
        wb, ws = big.render_image(v, *IMG)
        assert np.array_equal(bgr[i], wb) and np.array_equal(sem[i], ws), i
    assert (sem != 0).any()
