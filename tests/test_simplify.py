"""Voxel-cell simplification (sm_simplify, sm_simplify_maps, sm_simplify_stats; SurfelMap.simplify / simplify_maps; DESIGN.md "4p.
Simplification").  CPU: the restatement (simplify_ref.py) against answers worked by hand and against its own invariances; the
library's symbols, defaults, header and the argument rules that need no device.  GPU: the HIP path against the restatement,
exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import recall_ref as cr
import retire_ref as rr
import simplify_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sm_default_simplify_params", "sm_simplify", "sm_simplify_maps", "sm_simplify_stats")
STAT_KEYS = ("records_in", "records_out", "cells_merged", "loose", "largest_cell")
W, H, F = 96, 64, 60.0
CAM = (W, H, F, F, W / 2 - 0.5, H / 2 - 0.5)
# The cell edge at which "the scene bites" (below) holds for the restatement alone, chosen on the CPU: the scene's pixels lie 25 cm
# apart at 10 m, and at 100 mm it merges 47 pairs and no cell of three (1858 -> 1811); at 250 mm 1858 -> 1275 with cells of up to six.
# The GPU runs add 10 (nothing merges), 100 (pairs only) and 2000 (a few cells take next to everything: the contention case).
BITE_MM = 250
VOXELS = (10, 100, BITE_MM, 2000)


def surfel(x, y, z, conf=1.0, sem=3, bgr=(10, 100, 200), t0=1.0, t1=1.0, n=(0, 0, -1), r=0.0078125):
    s = np.zeros(12, np.float32)
    s[0:3] = (x, y, z); s[3] = conf
    s[4:5].view(np.uint32)[0] = (sem << 24) | (bgr[2] << 16) | (bgr[1] << 8) | bgr[0]
    s[6], s[7] = t0, t1
    s[8:11] = n; s[11] = r
    return s


def same_rows(got, want, what):
    got, want = np.asarray(got, np.float32).reshape(-1, 12), np.asarray(want, np.float32).reshape(-1, 12)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist())


class Scene:
    """test_blend.py's kind of scene: four frames of the synthetic street fused by the oracle at 64 x 48, about 1.9 k surfels"""

    def __init__(self):
        import oracle_lib as ol
        from surfelmapping_amd import synth
        cam = dict(width=64, height=48, fx=40.0, fy=40.0, cx=31.5, cy=23.5)
        poses = synth.kitti_trajectory(4)
        o = ol.Oracle(ol.make_config(**cam, preprocess=0, stereo_border=0.0, max_sqrt_vertices=64))
        for frame in synth.make_sequence(cam, poses, seed=3):
            o.process_frame(*frame)
        self.rows = o.download_model().astype(np.float32)
        o.close()
        self.view = synth.pose_to_colmajor(poses[3])
        self._ref = {}

    def ref(self, voxel_mm, split):
        if (voxel_mm, split) not in self._ref:
            self._ref[voxel_mm, split] = sr.simplify(self.rows, voxel_mm=voxel_mm, split_normals=split)
        return self._ref[voxel_mm, split]


@pytest.fixture(scope="module")
def scene():
    return Scene()


# ---------------------------------------------------------------------------------------------------------------------
# answers worked by hand, all at voxel_mm = 100: V = (100 * 65536 + 500) / 1000 = 6554100 / 1000 = 6554
# ---------------------------------------------------------------------------------------------------------------------
def test_known_answer_two_records_in_one_cell():
    """A at x = 0.25 (X = 16384: cell 2 = 13108, off 3276), B at x = 0.28125 (X = 18432: cell 2, off 5324); y = 0 (cell 0, off 0);
    z = 1 (X = 65536: cell 9 = 58986, off 6550; cell 10 would begin at 65540).  conf 0.5 and 1.0: w = 8 and 16, SW = 24, half 12.
    x: SP = 8 * 3276 + 16 * 5324 = 111392, (111392 + 12) / 24 = 4641 (24 * 4641 = 111384), X = 13108 + 4641 = 17749, x = 17749 / 65536.
    z: every off 6550, mean 6550, X = 65536, z = 1.  Colours (b, g, r) = (10, 100, 200) and (250, 50, 0): b (80 + 4000 + 12) / 24 = 170,
    g (800 + 800 + 12) / 24 = 67, r (1600 + 12) / 24 = 67.  Normals (0, 0, -1): SN = (0, 0, -24 * 16384 = -393216), 19 bits, no shift,
    len 393216, n = (0, 0, -1).  Radii 2^-7 (RI 512) and 2^-8 (256): Rmax 512; the box is 5324 - 3276 = 2048 long, isqrt 2048,
    (2048 + 1) / 2 = 1024 > 512: radius 1024 / 65536 = 2^-6.  conf max 1; init_time min(3, 5) = 3; time max(7, 6) = 7; standby 0."""
    assert sr.cell_edge(100) == 6554 and sr.cell_edge(10) == 655 and sr.cell_edge(50) == 3277 and sr.cell_edge(10000) == 655360
    a = surfel(0.25, 0.0, 1.0, conf=0.5, t0=3.0, t1=7.0)
    b = surfel(0.28125, 0.0, 1.0, conf=1.0, bgr=(250, 50, 0), t0=5.0, t1=6.0, r=0.00390625)
    a[5] = b[5] = 9.0                                                       # (standby is not carried into a merged record)
    want = surfel(17749 / 65536, 0.0, 1.0, conf=1.0, bgr=(170, 67, 67), t0=3.0, t1=7.0, r=0.015625)
    for rows in ((a, b), (b, a)):
        out, st = sr.simplify(np.stack(rows), voxel_mm=100)
        same_rows(out, want[None], "pair")
        assert st == dict(records_in=2, records_out=1, cells_merged=1, loose=0, largest_cell=2)
    # the larger disc wins over the box: radius 0.0625 = 4096 > 1024
    b2 = b.copy(); b2[11] = 0.0625
    assert sr.simplify(np.stack([a, b2]), voxel_mm=100)[0][0, 11] == np.float32(0.0625)
    # float32(0.05) = 0.0500000007...: RI = floor(3276.80005) = 3276 > 1024, radius 3276 / 65536
    b3 = b.copy(); b3[11] = 0.05
    assert sr.simplify(np.stack([a, b3]), voxel_mm=100)[0][0, 11] == np.float32(3276 / 65536)


def test_known_answer_singles_classes_and_faces():
    a = surfel(0.25, 0.0, 1.0, conf=0.37, bgr=(1, 2, 3), t0=2.0, t1=9.0, n=(0.6, 0.0, -0.8), r=0.123)
    a[5] = 4.0
    out, st = sr.simplify(a[None], voxel_mm=100)
    same_rows(out, a[None], "a single record comes back verbatim")
    assert st == dict(records_in=1, records_out=1, cells_merged=0, loose=0, largest_cell=1)
    # the same cell with two classes
    b = surfel(0.25, 0.0, 1.0, sem=4)
    out, st = sr.simplify(np.stack([a, b]), voxel_mm=100)
    same_rows(out, np.stack([a, b]), "two classes")
    # opposite normals: two faces with split_normals; without, one cell whose normal sums cancel -- the normal of `first`
    up, down = surfel(0.25, 0.0, 1.0, n=(0, 0, 1)), surfel(0.26, 0.0, 1.0, n=(0, 0, -1))
    out, st = sr.simplify(np.stack([up, down]), voxel_mm=100, split_normals=1)
    same_rows(out, np.stack([up, down]), "two faces")
    out, st = sr.simplify(np.stack([up, down]), voxel_mm=100, split_normals=0)
    assert st["records_out"] == 1 and st["cells_merged"] == 1 and out[0, 8:11].tolist() == [0.0, 0.0, 1.0]
    out, _ = sr.simplify(np.stack([up, down]), ids=[1, 0], voxel_mm=100, split_normals=0)
    assert out[0, 8:11].tolist() == [0.0, 0.0, -1.0]
    # a tie of |n| goes to the lower axis: (0.5, -0.5, 0.5) faces +x, (-0.5, 0.5, 0.5) faces -x
    V = sr.cell_edge(100)
    assert sr.classify(surfel(0, 0, 0, n=(0.5, -0.5, 0.5)), V, 1, (0, 0, 0))[0][3] == 0
    assert sr.classify(surfel(0, 0, 0, n=(-0.5, 0.5, 0.5)), V, 1, (0, 0, 0))[0][3] == 1
    assert sr.classify(surfel(0, 0, 0, n=(0.1, -0.5, 0.5)), V, 1, (0, 0, 0))[0][3] == 3
    assert sr.classify(surfel(0, 0, 0, n=(0.1, -0.5, 0.6)), V, 1, (0, 0, 0))[0][3] == 4


def test_known_answer_negative_coordinates_floor():
    """x = -0.03125 (X = -2048: cell -1 = -6554, off 4506) and x = -0.0625 (X = -4096: cell -1, off 2458), conf 1 (w 16, SW 32):
    (16 * 6964 + 16) / 32 = 3482, X = -6554 + 3482 = -3072, x = -0.046875.  x = +0.03125 (X = 2048) is cell 0: truncation would
    have put all three into it.  With origin (-1, 0, 0) the three are X = 63488, 61440, 67584: cells 9, 9, 10 of 6554 again."""
    rows = np.stack([surfel(-0.03125, 0.0, 1.0), surfel(-0.0625, 0.0, 1.0), surfel(0.03125, 0.0, 1.0)])
    out, st = sr.simplify(rows, voxel_mm=100)
    assert st["records_out"] == 2 and st["largest_cell"] == 2
    assert out[0, 0] == np.float32(-0.046875) and out[1].tobytes() == rows[2].tobytes()
    assert sr.classify(rows[0], 6554, 1, (0, 0, 0))[0][:3] == (-1, 0, 9) and sr.classify(rows[0], 6554, 1, (0, 0, 0))[1] == [4506, 0, 6550]
    out, st = sr.simplify(rows, voxel_mm=100, origin=(-1.0, 0.0, 0.0))
    assert st["records_out"] == 2 and out[0, 0] == np.float32(-0.046875)


def loose_rows():
    """one of each kind, at voxel_mm = 10 (V = 655: cell 65536 begins at 655.0 m)"""
    nan, inf = np.float32("nan"), np.float32("inf")
    return np.stack([surfel(nan, 0, 1), surfel(0, inf, 1), surfel(0, 0, 1, conf=0.0), surfel(0, 0, 1, conf=-1.0), surfel(0, 0, 1, conf=nan),
                     surfel(0, 0, 1, t0=-1.0), surfel(0, 0, 1, t1=nan), surfel(0, 0, 1, r=-0.5), surfel(0, 0, 1, r=32768.0), surfel(0, 0, 1, r=inf),
                     surfel(0, 0, 1, n=(0, 0, 0)), surfel(0, 0, 1, n=(0, nan, 1)), surfel(3000.0, 0, 1), surfel(0, -3000.0, 1), surfel(0, 0, 2.0e7)])


def test_loose_records_come_back_verbatim_and_in_place():
    loose = loose_rows()
    for row in loose:
        assert sr.classify(row, sr.cell_edge(10), 1, (0, 0, 0)) is None, row.tolist()
    assert sr.classify(surfel(3000.0, 0, 1), sr.cell_edge(100), 1, (0, 0, 0)) is not None          # (regular at a coarser grid)
    assert sr.classify(surfel(3000.0, 0, 1), sr.cell_edge(10), 1, (2500.0, 0, 0)) is not None      # (... and about a nearer origin)
    a, b = surfel(0.25, 0.0, 1.0), surfel(0.251, 0.0, 1.0)
    rows = np.concatenate([loose[:5], a[None], loose[5:9], b[None], loose[9:]])
    out, st = sr.simplify(rows, voxel_mm=10)
    assert st == dict(records_in=17, records_out=16, cells_merged=1, loose=15, largest_cell=2)
    same_rows(np.delete(out, 5, axis=0), loose, "loose")
    assert out[5, 3] == 1.0 and 0.25 <= out[5, 0] <= 0.251


def test_restatement_is_a_function_of_ids_and_records(scene):
    rows = scene.rows
    want, st = scene.ref(BITE_MM, 1)
    perm = np.random.RandomState(7).permutation(len(rows))
    out, st2 = sr.simplify(rows[perm], ids=perm, voxel_mm=BITE_MM)
    same_rows(out, want, "permuted, ids kept")
    assert st2 == st
    for cuts in ((), (700,), (300, 301, 900, 900)):
        parts = np.split(rows, list(cuts))
        assert len(parts) in (1, 2, 5)
        out, st2 = sr.simplify_set(parts, voxel_mm=BITE_MM)
        same_rows(out, want, cuts)
    with pytest.raises(sr.Capacity):
        sr.simplify(rows, voxel_mm=BITE_MM, max_cells=8)


def test_the_scene_bites(scene):
    """at voxel_mm = BITE_MM = 250 the restatement merges the fused street: fewer records out than in, merged cells, a cell of three
    or more; at 10 it keeps nearly all, at 2000 it keeps few -- and without split_normals no more than with it"""
    n = len(scene.rows)
    assert 1500 < n < 2500
    out, st = scene.ref(BITE_MM, 1)
    print("scene", n, st)
    assert st["records_in"] == n and st["records_out"] == len(out) < n and st["cells_merged"] > 0 and st["largest_cell"] >= 3 and st["loose"] == 0
    assert scene.ref(10, 1)[1]["records_out"] > scene.ref(BITE_MM, 1)[1]["records_out"] > scene.ref(2000, 1)[1]["records_out"]
    assert scene.ref(2000, 1)[1]["largest_cell"] > 64                       # (more than a wave's worth in one cell)
    for mm in VOXELS:
        assert scene.ref(mm, 0)[1]["records_out"] <= scene.ref(mm, 1)[1]["records_out"]
    assert scene.ref(BITE_MM, 0)[1]["records_out"] < scene.ref(BITE_MM, 1)[1]["records_out"]


# ---------------------------------------------------------------------------------------------------------------------
# the library, without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_defaults_and_binding():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None and name in capi.SYMBOLS
    assert L.sm_api_version() == 4 and capi.API_VERSION == 4
    p = capi.default_simplify_params()
    got = dict(voxel_mm=p.voxel_mm, split_normals=p.split_normals, origin=tuple(p.origin), max_cells=p.max_cells)
    assert got == sr.DEFAULTS == dict(voxel_mm=50, split_normals=1, origin=(0.0, 0.0, 0.0), max_cells=1 << 26)
    q = capi.simplify_params(voxel_mm=20, origin=(1, 2, 3))
    assert q.voxel_mm == 20 and tuple(q.origin) == (1.0, 2.0, 3.0)
    with pytest.raises(KeyError):
        capi.simplify_params(voxel=1)
    for name in ("simplify", "simplify_maps", "simplify_stats"):
        assert callable(getattr(capi.SurfelMap, name))
    header = open(os.path.join(ROOT, "include", "sm_c_api.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
    assert "#define SM_API_VERSION 4 " in header and "typedef struct sm_simplify_params {" in header


def test_argument_rules_that_need_no_device():
    from surfelmapping_amd import capi
    L = capi.load()
    p, st = capi.default_simplify_params(), capi.SmSimplifyStats()
    src = capi.map_source([], True)
    assert L.sm_default_simplify_params(None) == capi.SM_E_ARG
    assert L.sm_simplify(None, C.byref(p)) == capi.SM_E_ARG
    assert L.sm_simplify_maps(None, C.byref(src), C.byref(p), b"out.bin") == capi.SM_E_ARG
    assert L.sm_simplify_stats(None, C.byref(st)) == capi.SM_E_ARG
    assert not os.path.exists("out.bin")


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _ctx(rows=None, cap=64):
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, preprocess=0, stereo_border=0.0, max_sqrt_vertices=cap))
    if rows is not None and len(rows):
        m.upload_model(rows)
    return m


def _no_tmp(folder):
    assert not [f for f in os.listdir(folder) if f.endswith(".tmp")], os.listdir(folder)


@pytest.mark.gpu
@pytest.mark.parametrize("voxel_mm", VOXELS)
@pytest.mark.parametrize("split", (0, 1))
def test_gpu_model_is_bit_exact(scene, split, voxel_mm):
    want, st = scene.ref(voxel_mm, split)
    m = _ctx(scene.rows)
    m.set_tick(9)
    got = m.simplify(voxel_mm=voxel_mm, split_normals=split)
    same_rows(m.download_model(), want, (voxel_mm, split))
    assert {k: got[k] for k in STAT_KEYS} == st, got
    assert got == m.simplify_stats() and got["launches"] == 4 and got["chunks"] == 2 and got["device_ms"] > 0.0
    c = m.counts()
    assert c["count"] == len(want) and c["tick"] == 9
    # what is alone in its cell stays: a second call changes nothing
    again = m.simplify(voxel_mm=voxel_mm, split_normals=split)
    if voxel_mm == 10:
        same_rows(m.download_model(), sr.simplify(want, voxel_mm=voxel_mm, split_normals=split)[0], "again")
        assert again["records_in"] == len(want)
    m.close()


@pytest.mark.gpu
def test_gpu_shuffled_rows(scene):
    """the device's work order is not the specification's order: the same rows in another order, and every id another"""
    perm = np.random.RandomState(5).permutation(len(scene.rows))
    rows = scene.rows[perm]
    for mm in (BITE_MM, 2000):
        want, st = sr.simplify(rows, voxel_mm=mm)
        m = _ctx(rows)
        got = m.simplify(voxel_mm=mm)
        same_rows(m.download_model(), want, mm)
        assert {k: got[k] for k in STAT_KEYS} == st
        m.close()


@pytest.mark.gpu
def test_gpu_map_sets(scene, tmp_path):
    """five files (one of a single row, one empty) plus a live remainder against the restatement and the one-file run, with and
    without the combine step; the view of the simplified model"""
    rows = scene.rows
    cuts = [300, 301, 900, 900, 1500]
    parts = np.split(rows, cuts)
    paths = [str(tmp_path / f"m{i}.bin") for i in range(5)]
    for i, (p, part) in enumerate(zip(paths, parts[:5])):
        cr.write_map(p, part, 10 + i, 20 + i)
    one = str(tmp_path / "one.bin")
    cr.write_map(one, rows, 3, 4)
    want, st = scene.ref(BITE_MM, 1)
    m = _ctx(parts[5])
    before = [open(p, "rb").read() for p in paths + [one]]
    try:
        for env in ("0", "1"):
            os.environ["SM_SIMPLIFY_NO_COMBINE"] = env
            out = str(tmp_path / f"out{env}.bin")
            got = m.simplify_maps(paths, out, include_model=True, voxel_mm=BITE_MM)
            r, a, b = rr.read_map(out)
            same_rows(r, want, ("five files", env))
            assert (a, b) == (10, 24) and {k: got[k] for k in STAT_KEYS} == st, got
            assert got["chunks"] == 2 * 5 and got["launches"] == 4 * 5          # (the empty file has no chunk; the model is one)
            got = m.simplify_maps([one], out, voxel_mm=BITE_MM)
            r, a, b = rr.read_map(out)
            same_rows(r, want, ("one file", env))
            assert (a, b) == (3, 4) and {k: got[k] for k in STAT_KEYS} == st
            m2 = _ctx(rows)
            m2.simplify(voxel_mm=BITE_MM)
            same_rows(m2.download_model(), want, ("model", env))
            m2.close()
    finally:
        os.environ.pop("SM_SIMPLIFY_NO_COMBINE", None)
    # without the live model: the files alone; the model alone
    got = m.simplify_maps(paths, str(tmp_path / "files.bin"), voxel_mm=BITE_MM)
    same_rows(rr.read_map(str(tmp_path / "files.bin"))[0], sr.simplify(rows[:1500], voxel_mm=BITE_MM)[0], "files alone")
    got = m.simplify_maps([], str(tmp_path / "live.bin"), include_model=True, voxel_mm=BITE_MM)
    same_rows(rr.read_map(str(tmp_path / "live.bin"))[0], sr.simplify(rows[1500:], voxel_mm=BITE_MM)[0], "model alone")
    got = m.simplify_maps([paths[3]], str(tmp_path / "none.bin"), voxel_mm=BITE_MM)
    assert len(rr.read_map(str(tmp_path / "none.bin"))[0]) == 0 and got["records_out"] == 0
    # sources and model are as they were; no temporary is left
    assert [open(p, "rb").read() for p in paths + [one]] == before
    same_rows(m.download_model(), parts[5], "the live model")
    _no_tmp(tmp_path)
    m.close()


@pytest.mark.gpu
def test_gpu_output_scratch_is_shared_with_change_detection(scene, tmp_path):
    """sm_simplify_maps, sm_compare_maps with an output, sm_simplify_maps again on one context: both write what they keep of a
    chunk through the same device buffers, which the second call -- its largest chunk has 958 records, the first call's 400 --
    has to grow.  Each result is its restatement's, and the third file is the first's, byte for byte"""
    import compare_ref as cf
    rows = scene.rows
    small = [rows[:300], rows[300:700]]
    query, ref = [rows[:900], rows[900:]], [rows[200:800], rows[800:1500]]
    assert max(len(p) for p in query) > max(len(p) for p in small)

    def write(name, parts):
        paths = [str(tmp_path / f"{name}{i}.bin") for i in range(len(parts))]
        for p, part in zip(paths, parts):
            cr.write_map(p, part, 1, 2)
        return paths
    sp, qp, rp = write("s", small), write("q", query), write("r", ref)
    want, st = sr.simplify_set(small, voxel_mm=BITE_MM)
    kw = dict(voxel_mm=BITE_MM, cover_shift=2, write_mask=0b0111)
    want_cmp = cf.compare_sets(query, ref, None, **kw)
    assert st["cells_merged"] > 0 and len(want) < 700 and 900 < len(want_cmp["written"]) and min(want_cmp["counts"][:3]) > 0
    m = _ctx()
    outs = [str(tmp_path / f"out{i}.bin") for i in range(3)]
    got = m.simplify_maps(sp, outs[0], voxel_mm=BITE_MM)
    same_rows(rr.read_map(outs[0])[0], want, "before")
    assert {k: got[k] for k in STAT_KEYS} == st
    lab, info = m.compare_maps(qp, rp, out_path=outs[1], **kw)
    assert np.array_equal(lab, want_cmp["labels"]) and info["counts_by_code"] == want_cmp["counts"]
    assert info["written"] == len(want_cmp["written"])
    same_rows(rr.read_map(outs[1])[0], want_cmp["written"], "change detection")
    got = m.simplify_maps(sp, outs[2], voxel_mm=BITE_MM)
    same_rows(rr.read_map(outs[2])[0], want, "after")
    assert {k: got[k] for k in STAT_KEYS} == st
    assert open(outs[0], "rb").read() == open(outs[2], "rb").read()
    _no_tmp(tmp_path)
    m.close()


@pytest.mark.gpu
def test_gpu_one_cell_across_files(tmp_path):
    """300 copies of one position with different colours and weights in three files, between records that are alone in their cells:
    more than a wave's worth, so the combine step, the atomics across waves and the rank across chunks all take part"""
    rs = np.random.RandomState(11)
    copies = np.stack([surfel(1.01, 0.52, 7.03, conf=float(rs.randint(1, 40)) / 16.0, bgr=tuple(int(v) for v in rs.randint(0, 256, 3)),
                              t0=float(rs.randint(0, 50)), t1=float(rs.randint(50, 99)), n=(0.0, -0.6, -0.8)) for _ in range(300)])
    alone = np.stack([surfel(0.3 * i, 1.0, 5.0) for i in range(9)])
    files = [np.concatenate([alone[3 * i:3 * i + 2], copies[100 * i:100 * i + 100], alone[3 * i + 2:3 * i + 3]]) for i in range(3)]
    paths = [str(tmp_path / f"c{i}.bin") for i in range(3)]
    for p, f in zip(paths, files):
        cr.write_map(p, f)
    want, st = sr.simplify_set(files, voxel_mm=50)
    assert st["records_out"] == 10 and st["largest_cell"] == 300 and st["cells_merged"] == 1
    m = _ctx()
    out = str(tmp_path / "out.bin")
    got = m.simplify_maps(paths, out, voxel_mm=50)
    same_rows(rr.read_map(out)[0], want, "300 copies")
    assert {k: got[k] for k in STAT_KEYS} == st
    m.upload_model(np.concatenate(files))
    m.simplify(voxel_mm=50)
    same_rows(m.download_model(), want, "300 copies, resident")
    m.close()


@pytest.mark.gpu
def test_gpu_loose_records(tmp_path):
    loose = loose_rows()
    a, b = surfel(0.25, 0.0, 1.0), surfel(0.251, 0.0, 1.0)
    rows = np.concatenate([loose[:5], a[None], loose[5:9], b[None], loose[9:]])
    rows[:, 5] = 0.0                                                        # (a model does not keep the standby word)
    want, st = sr.simplify(rows, voxel_mm=10)
    assert st["loose"] == 15 and st["records_out"] == 16
    m = _ctx(rows)
    got = m.simplify(voxel_mm=10)
    same_rows(m.download_model(), want, "loose, resident")
    assert {k: got[k] for k in STAT_KEYS} == st
    rows[:, 5] = 2.5                                                        # (a file does)
    want, st = sr.simplify(rows, voxel_mm=10)
    path, out = str(tmp_path / "l.bin"), str(tmp_path / "out.bin")
    cr.write_map(path, rows)
    got = m.simplify_maps([path], out, voxel_mm=10)
    r = rr.read_map(out)[0]
    same_rows(r, want, "loose, file")
    assert (r[:, 5] == 2.5).sum() == 15 and {k: got[k] for k in STAT_KEYS} == st
    m.close()


@pytest.mark.gpu
def test_gpu_capacity_and_refusals(scene, tmp_path):
    from surfelmapping_amd import capi
    m = _ctx(scene.rows)
    path, out = str(tmp_path / "a.bin"), str(tmp_path / "out.bin")
    cr.write_map(path, scene.rows[:500])
    fresh = _ctx()
    with pytest.raises(capi.SurfelMapError) as e:
        fresh.simplify_stats()
    assert e.value.rc == capi.SM_E_ARG
    assert fresh.simplify()["records_out"] == 0                              # (an empty model is a valid no-op)
    # max_cells: an error return, the model and the folder as before
    for call in (lambda: m.simplify(voxel_mm=BITE_MM, max_cells=8), lambda: m.simplify_maps([path], out, include_model=True, voxel_mm=BITE_MM, max_cells=8)):
        with pytest.raises(capi.SurfelMapError) as e:
            call()
        assert e.value.rc == capi.SM_E_CAPACITY and "max_cells" in str(e.value)
        same_rows(m.download_model(), scene.rows, "after SM_E_CAPACITY")
        assert m.counts()["count"] == len(scene.rows) and not os.path.exists(out)
        _no_tmp(tmp_path)
    for bad in (dict(voxel_mm=9), dict(voxel_mm=10001), dict(split_normals=2), dict(origin=(0, float("nan"), 0)), dict(max_cells=0)):
        for call in (lambda: m.simplify(**bad), lambda: m.simplify_maps([path], out, **bad)):
            with pytest.raises(capi.SurfelMapError) as e:
                call()
            assert e.value.rc == capi.SM_E_ARG and list(bad)[0].split("_")[0] in str(e.value)
    for call in (lambda: m.simplify_maps([path], path), lambda: m.simplify_maps([str(tmp_path / "nowhere.bin")], out)):
        with pytest.raises(capi.SurfelMapError) as e:
            call()
        assert e.value.rc == capi.SM_E_ARG
    assert rr.read_map(path)[0].tobytes() == scene.rows[:500].tobytes() and not os.path.exists(out)
    p = capi.default_simplify_params()
    src = capi.map_source([path], False)
    assert m._L.sm_simplify(m._h, None) == capi.SM_E_ARG
    assert m._L.sm_simplify_maps(m._h, None, C.byref(p), out.encode()) == capi.SM_E_ARG
    assert m._L.sm_simplify_maps(m._h, C.byref(src), C.byref(p), None) == capi.SM_E_ARG
    # between sm_stage_conflict and sm_stage_cull
    seq = rr.sequence(2)
    st = capi.SurfelMap(capi.make_config(**rr.CAM, **rr.OVER, preprocess=0, max_sqrt_vertices=200))
    for frame in seq:
        st.process_frame(*frame)
    st.stage_conflict(seq[1][3], 1.0, 30.0)
    for call in (lambda: st.simplify(), lambda: st.simplify_maps([path], out)):
        with pytest.raises(capi.SurfelMapError) as e:
            call()
        assert e.value.rc == capi.SM_E_ARG and "sm_stage_conflict" in str(e.value)
    st.stage_cull()
    n = st.counts()["count"]
    rows = st.download_model()
    got = st.simplify(voxel_mm=BITE_MM)                                      # (a model that frames have made, not an upload)
    assert got["records_in"] == n
    same_rows(st.download_model(), sr.simplify(rows, voxel_mm=BITE_MM)[0], "after frames")
    st.close()
    for configure in ("shard_stream_configure", "rig_configure"):
        part = _ctx()
        getattr(part, configure)(0, 1)
        for call in (lambda: part.simplify(), lambda: part.simplify_maps([path], out)):
            with pytest.raises(capi.SurfelMapError) as e:
                call()
            assert e.value.rc == capi.SM_E_UNSUPPORTED
        part.close()
    _no_tmp(tmp_path)
    fresh.close()
    m.close()


@pytest.mark.gpu
def test_gpu_view_of_the_simplified_model(scene):
    """render_image of the simplified model against a context that uploaded the restatement's rows"""
    want, _ = scene.ref(BITE_MM, 1)
    m, ref = _ctx(scene.rows), _ctx(want)
    full = m.render_image(scene.view, *CAM)
    m.simplify(voxel_mm=BITE_MM)
    got, exp = m.render_image(scene.view, *CAM), ref.render_image(scene.view, *CAM)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    drawn, before = int((got[1] != 0).sum()), int((full[1] != 0).sum())
    print("drawn pixels", drawn, "of", before, "before")
    assert before > 1000 and drawn > 0
    m.close(); ref.close()


@pytest.mark.gpu
def test_gpu_more_than_a_chunk(tmp_path):
    """2^20 + 450 records, so that the model goes through both passes in two pieces and a file in two chunks: surfels on a 1 m
    lattice, each alone in its 100 mm cell, and 150 exact copies of the first 150 laid across the boundary between the pieces.
    Every field of a copied pair is exact in the grid's units (integer coordinates, radius 0.5, one colour), so the merged record
    is its `first` bit for bit and the output is the input without the copies: the second piece's ranks go on from the first's."""
    n_a, n_b, n_dup = (1 << 20) - 100, 400, 150
    i = np.arange(n_a + n_b)
    rows = np.tile(surfel(0.0, 0.0, 5.0, r=0.5), (n_a + n_b, 1))
    rows[:, 0], rows[:, 1] = i % 1024, i // 1024
    rows[:, 6] = rows[:, 7] = (i % 50).astype(np.float32)
    rows = np.concatenate([rows[:n_a], rows[:n_dup], rows[n_a:]])
    want = np.concatenate([rows[:n_a], rows[n_a + n_dup:]])
    stats = dict(records_in=len(rows), records_out=len(want), cells_merged=n_dup, loose=0, largest_cell=2)
    small, st = sr.simplify(np.concatenate([rows[:200], rows[n_a:n_a + n_dup + 5]]), voxel_mm=100)      # (the construction, in the small)
    same_rows(small, np.concatenate([rows[:200], rows[n_a + n_dup:n_a + n_dup + 5]]), "the construction")
    m = _ctx(rows, cap=1040)
    path, out = str(tmp_path / "big.bin"), str(tmp_path / "out.bin")
    cr.write_map(path, rows)
    got = m.simplify_maps([path], out, voxel_mm=100)
    same_rows(rr.read_map(out)[0], want, "two chunks")
    assert {k: got[k] for k in STAT_KEYS} == stats and got["chunks"] == 4
    got = m.simplify(voxel_mm=100)
    same_rows(m.download_model(), want, "two pieces")
    assert {k: got[k] for k in STAT_KEYS} == stats and got["chunks"] == 4 and got["launches"] == 8
    m.close()
