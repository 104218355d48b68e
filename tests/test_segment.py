"""Segmentation of a map set into connected voxel components (sm_segment_maps, sm_segment_stats; SurfelMap.segment_maps; DESIGN.md
"4t. Segmentation").  CPU: the restatement (segment_ref.py) against answers worked by hand and against its own invariances; the
library's symbols, defaults, header and the argument rules that need no device.  GPU: labels, rows, info and the file of the HIP
path against the restatement, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import recall_ref as cr
import retire_ref as rr
import segment_ref as sg
import simplify_ref as sr
import test_simplify as ts
from test_simplify import surfel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sm_default_segment_params", "sm_segment_maps", "sm_segment_stats")
INFO_KEYS = ("records", "counts_by_kind", "cells", "components", "small_components", "largest")
NAN, INF = np.float32("nan"), np.float32("inf")
LOOSE, SMALL, SKIPPED = sg.LOOSE, sg.SMALL, sg.SKIPPED


@pytest.fixture(scope="module")
def scene():
    return ts.Scene()


def at(x, y, z, **kw):
    return surfel(x, y, z, **kw)


def in_cell(cx, cy, cz, **kw):
    """a record at the centre of a cell of a 1000 mm grid about the origin"""
    return surfel(cx + 0.5, cy + 0.5, cz + 0.5, **kw)


def example():
    return np.stack([at(.5, .5, .5), at(1.5, .5, .5), at(2.5, 1.5, .5), at(3.5, 2.5, 1.5), at(5.5, .5, .5)])


EXAMPLE_LABELS = {6: [0, 0, 1, 2, 3], 18: [0, 0, 0, 1, 2], 26: [0, 0, 0, 0, 1]}


def snake(n=3000):
    """The cells of a path that is one cell wide and never touches itself under connectivity 26: consecutive cells are neighbours,
    no others are.  Layers z = 0, 2, 4, ..: rows y = 0, 2, .., 38 run over x = 1..38, to and fro; a row is joined to the next by one
    cell diagonally off both ends, (39, y + 1) or (0, y + 1); a layer is joined to the next, which runs the same way backwards, by
    one cell (0, y_end, z + 1).  All within [0, 40)^3."""
    layer = []
    for r in range(20):
        xs = range(1, 39) if r % 2 == 0 else range(38, 0, -1)
        layer += [(x, 2 * r) for x in xs]
        if r < 19:
            layer.append((39 if r % 2 == 0 else 0, 2 * r + 1))
    cells, z = [], 0
    while len(cells) < n:
        run = layer if (z // 2) % 2 == 0 else layer[::-1]
        cells += [(x, y, z) for x, y in run]
        cells.append((0, run[-1][1], z + 1))
        z += 2
    cells = cells[:n]
    assert len(set(cells)) == n and max(max(c) for c in cells) < 40 and min(min(c) for c in cells) >= 0
    return cells


def snake_rows(cells):
    return np.stack([in_cell(*c, t0=float(i % 90)) for i, c in enumerate(cells)])


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_worked_example():
    """segment_ref's docstring: voxel_mm 1000, V = 65536, origin 0"""
    assert sg.cell_edge(1000) == 65536 and sg.cell_edge(200) == 13107 and sg.cell_edge(10) == 655
    rows = example()
    ok, cell, cls = sg.cells(rows, 1000)
    assert ok.all() and cell.tolist() == [[0, 0, 0], [1, 0, 0], [2, 1, 0], [3, 2, 1], [5, 0, 0]] and cls.tolist() == [3] * 5
    for conn, want in EXAMPLE_LABELS.items():
        got = sg.segment(rows, voxel_mm=1000, connectivity=conn)
        assert got["labels"].tolist() == want, conn
        assert got["info"] == dict(records=5, counts_by_kind=[5, 0, 0, 0], written=5, cells=5, components=max(want) + 1, small_components=0,
                                   largest=want.count(0))
        assert got["components"]["first"].tolist() == [want.index(i) for i in range(max(want) + 1)]
    got = sg.segment(rows, voxel_mm=1000, connectivity=26, min_records=2)
    assert got["labels"].tolist() == [0, 0, 0, 0, SMALL] and got["info"]["small_components"] == 1 and got["info"]["components"] == 1
    assert got["info"]["counts_by_kind"] == [4, 1, 0, 0] and got["info"]["largest"] == 4
    row = got["components"]
    assert len(row) == 1 and row.dtype.itemsize == 64
    assert (int(row["first"][0]), int(row["records"][0]), int(row["cells"][0]), int(row["cls"][0])) == (0, 4, 4, 3)
    assert row["cell_lo"][0].tolist() == [0, 0, 0] and row["cell_hi"][0].tolist() == [3, 2, 1]
    assert row["sum_cell"][0].tolist() == [4 * 65536 + 6, 4 * 65536 + 3, 4 * 65536 + 1]
    assert got["kept"].tobytes() == rows[:4].tobytes()
    assert sg.segment(rows, voxel_mm=1000, min_records=2, write_mask=2)["kept"].tobytes() == rows[4:].tobytes()


def test_diagonal_contact_pairs():
    """one pair per |d|_1, in every sign pattern of the forward and the backward half of the neighbourhood"""
    joined = {1: (6, 18, 26), 2: (18, 26), 3: (26,)}
    assert [len(sg.offsets(c)) for c in (6, 18, 26)] == [6, 18, 26]
    for d in sg.offsets(26):
        rows = np.stack([in_cell(10, 10, 10), in_cell(10 + d[0], 10 + d[1], 10 + d[2])])
        for conn in (6, 18, 26):
            for pair in (rows, rows[::-1]):
                got = sg.segment(pair, voxel_mm=1000, connectivity=conn)
                want = 1 if conn in joined[sum(abs(v) for v in d)] else 2
                assert got["info"]["components"] == want, (d, conn)
    two_apart = np.stack([in_cell(0, 0, 0), in_cell(2, 0, 0)])
    assert sg.segment(two_apart, voxel_mm=1000)["info"]["components"] == 2


def test_classes():
    rows = np.stack([in_cell(0, 0, 0, sem=3), in_cell(1, 0, 0, sem=7), in_cell(1, 1, 0, sem=7), in_cell(0, 1, 0, sem=200)])
    got = sg.segment(rows, voxel_mm=1000, by_class=1)
    assert got["labels"].tolist() == [0, 1, 1, 2] and got["components"]["cls"].tolist() == [3, 7, 200]
    got = sg.segment(rows, voxel_mm=1000, by_class=0)
    assert got["labels"].tolist() == [0, 0, 0, 0] and got["components"]["cls"].tolist() == [-1] and got["components"]["cells"].tolist() == [4]
    # two classes in one cell: two nodes with by_class, one without
    both = np.stack([in_cell(0, 0, 0, sem=3), in_cell(0, 0, 0, sem=7)])
    assert sg.segment(both, voxel_mm=1000)["info"]["cells"] == 2 and sg.segment(both, voxel_mm=1000, by_class=0)["info"]["cells"] == 1
    # class_mask: a class that does not take part is SKIPPED, whatever by_class is, and does not connect its neighbours
    line = np.stack([in_cell(0, 0, 0, sem=3), in_cell(1, 0, 0, sem=7), in_cell(2, 0, 0, sem=3), in_cell(3, 0, 0, sem=200)])
    mask = sg.class_mask(set(range(256)) - {7})
    assert mask[0] == 0xFFFFFF7F and mask[1:] == (0xFFFFFFFF,) * 7
    for by_class in (0, 1):
        got = sg.segment(line, voxel_mm=1000, by_class=by_class, class_mask=mask, write_mask=4)
        assert got["labels"].tolist() == ([0, SKIPPED, 1, 1] if by_class == 0 else [0, SKIPPED, 1, 2])
        assert got["info"]["counts_by_kind"] == [3, 0, 1, 0] and got["kept"].tobytes() == line[1:2].tobytes()
    assert sg.segment(line, voxel_mm=1000, class_mask=sg.class_mask({200}))["labels"].tolist() == [SKIPPED, SKIPPED, SKIPPED, 0]


def test_negative_coordinates_and_minus_zero():
    V = sg.cell_edge(100)                                                     # 6554
    cx = lambda x, o=0.0: int(sg.cells(at(x, 0, 0)[None], 100, (o, 0, 0))[1][0, 0])    # noqa: E731
    assert cx(-0.03125) == -1 and cx(0.03125) == 0                            # X = -2048 floors to cell -1: no truncation
    assert cx(-0.0) == 0 and cx(0.0) == 0
    assert cx(-0.03125, -1.0) == 9 and cx(0.03125, -1.0) == 10                # X = 63488, 67584 about origin -1
    x = np.float32(3 * V / 65536.0)
    assert cx(x) == 3 and cx(np.nextafter(x, np.float32(0))) == 2
    x = np.float32(-3 * V / 65536.0)
    assert cx(x) == -3 and cx(np.nextafter(x, np.float32(-1))) == -4
    # -0.0 and +0.03 share cell 0; -0.03125 is its neighbour -1; -0.25 (cell -3) is two cells off
    rows = np.stack([at(-0.0, 0, 0), at(0.03, 0, 0), at(-0.03125, 0, 0), at(-0.25, 0, 0)])
    got = sg.segment(rows, voxel_mm=100)
    assert got["labels"].tolist() == [0, 0, 0, 1] and got["components"]["cell_lo"][:, 0].tolist() == [-1, -3]
    assert got["components"]["sum_cell"][0].tolist() == [3 * 65536 - 1, 3 * 65536, 3 * 65536]


def grid_edge_rows():
    """voxel_mm 10 (V = 655): per axis a record in cell 65535 (654.995 m) and one in cell -65536 (-655.0 m).  The second lies where
    a key made of cell 65535 + 1 without the range test would point: the carry out of an axis' 17 bits adds one to the next field
    up, so it sits in cell 1 of that axis (0.015 m: X = 983 = 655 + 328)."""
    rows = []
    for k in range(3):
        hi, lo = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        hi[k], lo[k] = 654.995, -655.0
        if k:
            lo[k - 1] = 0.015
        rows += [at(*hi), at(*lo)]
    return np.stack(rows)


def test_grid_edge_does_not_wrap_or_carry():
    rows = grid_edge_rows()
    ok, cell, _ = sg.cells(rows, 10)
    assert ok.all() and cell.tolist() == [[65535, 0, 0], [-65536, 0, 0], [0, 65535, 0], [1, -65536, 0], [0, 0, 65535], [0, 1, -65536]]
    for conn in (6, 18, 26):
        got = sg.segment(rows, voxel_mm=10, connectivity=conn)
        assert got["labels"].tolist() == [0, 1, 2, 3, 4, 5], conn
    # the first cell outside the range is loose
    out = np.stack([at(655.0, 0, 0), at(np.nextafter(np.float32(-655.0), -INF), 0, 0), at(654.995, 0, 0)])
    assert sg.segment(out, voxel_mm=10)["labels"].tolist() == [LOOSE, LOOSE, 0]
    assert sg.segment(out, voxel_mm=100)["info"]["counts_by_kind"] == [3, 0, 0, 0]       # (regular on a coarser grid)


def test_loose_records_and_the_simplifications_test():
    loose = ts.loose_rows()
    got = sg.segment(loose, voxel_mm=10, write_mask=8)
    assert got["labels"].tolist() == [LOOSE] * len(loose) and got["info"]["cells"] == 0 and got["info"]["largest"] == 0
    assert got["kept"].tobytes() == loose.tobytes()
    # LOOSE comes before SKIPPED
    assert sg.segment(loose, voxel_mm=10, class_mask=(0,) * 8)["info"]["counts_by_kind"] == [0, 0, 0, len(loose)]
    # the regular-record test and the cells are the simplification's, row by row
    rs = np.random.RandomState(4)
    rows = np.stack([at(*(rs.rand(3) * 60.0 - 30.0), sem=int(rs.randint(0, 256))) for _ in range(200)] + list(loose))
    for mm, origin in ((10, (0, 0, 0)), (200, (0, 0, 0)), (200, (1.5, -2.0, 0.25))):
        ok, cell, cls = sg.cells(rows, mm, origin)
        for i, row in enumerate(rows):
            want = sr.classify(row, sr.cell_edge(mm), 0, origin)
            assert (want is not None) == bool(ok[i]), (mm, i)
            if want is not None:
                assert want[0] == (cell[i, 0], cell[i, 1], cell[i, 2], 0, cls[i]), (mm, i)


def same(got, want, what):
    assert np.array_equal(got["labels"], want["labels"]), (what, np.flatnonzero(got["labels"] != want["labels"])[:8])
    assert got["components"].tobytes() == want["components"].tobytes(), what
    assert got["info"] == want["info"], (what, got["info"], want["info"])
    assert got["kept"].tobytes() == want["kept"].tobytes(), what


def test_restatement_is_a_function_of_ids_and_records(scene):
    rows = scene.rows
    kw = dict(voxel_mm=200, min_records=3, write_mask=3)
    want = sg.segment(rows, **kw)
    assert want["info"]["components"] > 20 and want["info"]["small_components"] > 0
    perm = np.random.RandomState(7).permutation(len(rows))
    got = sg.segment(rows[perm], ids=perm, **kw)
    got["labels"] = got["labels"][np.argsort(perm)]                           # (per id)
    same(got, want, "permuted, ids kept")
    for cuts in ((), (700,), (300, 301, 900, 900)):
        parts = np.split(rows, list(cuts))
        assert len(parts) in (1, 2, 5)
        same(sg.segment_set(parts, **kw), want, cuts)
    # other ids: the numbers follow `first`
    moved = sg.segment(rows, ids=perm, **kw)
    table = moved["components"]
    assert (np.diff(table["first"].astype(np.int64)) > 0).all() and sorted(table["records"].tolist()) == sorted(want["components"]["records"].tolist())
    for i in (0, 1, len(table) - 1):
        assert perm[moved["labels"] == i].min() == table["first"][i] and (moved["labels"] == i).sum() == table["records"][i]
    assert not np.array_equal(moved["labels"], want["labels"])
    with pytest.raises(sg.Capacity):
        sg.segment(rows, voxel_mm=200, max_cells=8)


def test_snake_is_one_path():
    cells = snake()
    rows = snake_rows(cells)
    got = sg.segment(rows, voxel_mm=1000)
    assert got["info"]["components"] == 1 and got["components"]["records"][0] == got["components"]["cells"][0] == 3000
    assert got["components"]["cell_hi"][0].max() < 40
    # it never touches itself: without any one cell it falls into exactly two pieces, which are the cells before and after it
    for cut in (1, 38, 39, 40, 778, 779, 780, 1500, 2998):
        got = sg.segment(np.delete(rows, cut, axis=0), voxel_mm=1000)
        assert got["components"]["records"].tolist() == [cut, 2999 - cut], cut


# ---------------------------------------------------------------------------------------------------------------------
# the library, without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_defaults_and_binding():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None and name in capi.SYMBOLS
    p = capi.default_segment_params()
    got = dict(voxel_mm=p.voxel_mm, connectivity=p.connectivity, by_class=p.by_class, class_mask=tuple(p.class_mask), min_records=p.min_records,
               write_mask=p.write_mask, max_cells=p.max_cells, origin=tuple(p.origin))
    assert got == sg.DEFAULTS == dict(voxel_mm=200, connectivity=26, by_class=1, class_mask=(0xFFFFFFFF,) * 8, min_records=1, write_mask=1,
                                      max_cells=1 << 24, origin=(0.0, 0.0, 0.0))
    q = capi.segment_params(voxel_mm=20, origin=(1, 2, 3), classes=(7, 200))
    assert q.voxel_mm == 20 and tuple(q.origin) == (1.0, 2.0, 3.0) and tuple(q.class_mask) == sg.class_mask((7, 200))
    with pytest.raises(KeyError):
        capi.segment_params(cell=1)
    for name in ("segment_maps", "segment_stats"):
        assert callable(getattr(capi.SurfelMap, name))
    assert (capi.SM_SEGMENT_LOOSE, capi.SM_SEGMENT_SMALL, capi.SM_SEGMENT_SKIPPED) == (LOOSE, SMALL, SKIPPED)
    assert capi.SEGMENT_COMPONENT == sg.COMPONENT
    header = open(os.path.join(ROOT, "include", "sm_c_api.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
    assert "#define SM_API_VERSION 4 " in header and L.sm_api_version() == 4
    for line in ("#define SM_SEGMENT_LOOSE   0xFFFFFFFEu", "#define SM_SEGMENT_SMALL   0xFFFFFFFDu", "#define SM_SEGMENT_SKIPPED 0xFFFFFFFCu",
                 "typedef struct sm_segment_params {", "typedef struct sm_segment_component {", "typedef struct sm_segment_info {",
                 "typedef struct sm_segment_stats_t {"):
        assert line in header, line
    # the box and the centroid in metres: the worked example's one row
    row = sg.segment(example(), voxel_mm=1000, min_records=2)["components"]
    lo, hi, mean = capi.segment_boxes(row, voxel_mm=1000)
    assert lo.tolist() == [[0.0, 0.0, 0.0]] and hi.tolist() == [[4.0, 3.0, 2.0]] and mean.tolist() == [[2.0, 1.25, 0.75]]


def test_argument_rules_that_need_no_device():
    from surfelmapping_amd import capi
    L = capi.load()
    p, st, info = capi.default_segment_params(), capi.SmSegmentStats(), capi.SmSegmentInfo()
    src = capi.map_source([], True)
    assert L.sm_default_segment_params(None) == capi.SM_E_ARG
    assert L.sm_segment_maps(None, C.byref(src), C.byref(p), None, None, 0, b"segmented.bin", C.byref(info)) == capi.SM_E_ARG
    assert L.sm_segment_stats(None, C.byref(st)) == capi.SM_E_ARG
    assert not os.path.exists("segmented.bin")


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
_ctx, _no_tmp = ts._ctx, ts._no_tmp


def check(got, want, what, out_path=None, frame=(0, 0)):
    """labels, rows, info and the file against the restatement, bit for bit"""
    assert got["labels"].dtype == np.uint32 and np.array_equal(got["labels"], want["labels"]), (what, np.flatnonzero(got["labels"] != want["labels"])[:8])
    assert got["components"].tobytes() == want["components"].tobytes(), (what, got["components"][:4], want["components"][:4])
    assert {k: got["info"][k] for k in INFO_KEYS} == {k: want["info"][k] for k in INFO_KEYS}, (what, got["info"], want["info"])
    if out_path is None:
        assert got["info"]["written"] == 0
    else:
        assert got["info"]["written"] == want["info"]["written"] == len(want["kept"])
        assert open(out_path, "rb").read() == sg.file_bytes(want["kept"], *frame), what


def run(m, paths, parts, what, include_model=False, out_path=None, frame=(0, 0), want=None, **kw):
    """segment_maps of `paths` against the restatement of `parts`; -> (what the call returned, the restatement)"""
    got = m.segment_maps(paths, include_model=include_model, out_path=None if out_path is None else str(out_path), **kw)
    want = sg.segment_set(parts, **kw) if want is None else want
    check(got, want, what, out_path, frame)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("conn", (6, 18, 26))
def test_gpu_worked_example(tmp_path, conn):
    rows = example()
    path = str(tmp_path / "e.bin")
    cr.write_map(path, rows)
    m = _ctx()
    got, _ = run(m, [path], [rows], conn, voxel_mm=1000, connectivity=conn)
    assert got["labels"].tolist() == EXAMPLE_LABELS[conn]
    if conn == 26:
        got, _ = run(m, [path], [rows], "min_records 2", voxel_mm=1000, min_records=2)
        assert got["labels"].tolist() == [0, 0, 0, 0, SMALL] and len(got["components"]) == 1
        assert got["components"]["sum_cell"][0].tolist() == [4 * 65536 + 6, 4 * 65536 + 3, 4 * 65536 + 1]
        st = m.segment_stats()
        assert st["readings"] == 2 and st["chunks"] == 2 and st["launches"] >= 8
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("conn", (6, 26))
@pytest.mark.parametrize("by_class", (0, 1))
@pytest.mark.parametrize("voxel_mm", (50, 200))
def test_gpu_scene_as_one_file(scene, tmp_path, voxel_mm, by_class, conn):
    path = str(tmp_path / "scene.bin")
    cr.write_map(path, scene.rows, 3, 4)
    m = _ctx()
    got, want = run(m, [path], [scene.rows], (voxel_mm, by_class, conn), voxel_mm=voxel_mm, by_class=by_class, connectivity=conn)
    # (a trivial scene would pass without exercising anything; the bounds: test_the_scene_has_components)
    assert want["info"]["components"] > 20 and want["info"]["largest"] > SCENE_LARGEST_ABOVE[voxel_mm], want["info"]
    m.close()


# The scene's surfels lie about 25 cm apart at 10 m (test_simplify.py): at 200 mm its cells touch -- 492 to 645 components over the
# four cases, the largest of 841 or 902 records -- and at 50 mm next to none do: 1 687 (connectivity 26) or 1 781 (6) components, none
# of more than 3 records.  So "one of more than 100 records" can hold at 200 mm only; at 50 mm the case pins many tiny components.
SCENE_LARGEST_ABOVE = {50: 2, 200: 100}


def test_the_scene_has_components(scene):
    """what the GPU test above asserts of the restatement, on the CPU as well: every case has more than 20 components, and at 200 mm
    one of more than 100 records (at 50 mm the largest has 3: see SCENE_LARGEST_ABOVE)"""
    for voxel_mm in (50, 200):
        for by_class in (0, 1):
            for conn in (6, 26):
                info = sg.segment(scene.rows, voxel_mm=voxel_mm, by_class=by_class, connectivity=conn)["info"]
                print(voxel_mm, by_class, conn, info)
                assert info["components"] > 20 and info["largest"] > SCENE_LARGEST_ABOVE[voxel_mm], (voxel_mm, by_class, conn, info)


@pytest.mark.gpu
def test_gpu_snake(tmp_path):
    """3 000 cells in a row, rows shuffled and spread over five files (one of a single row, one empty) and the live model: long
    parent chains, unions in every order, chunk boundaries; 3 000 nodes in 8 192 slots, so probes collide"""
    cells = snake()
    rows = snake_rows(cells)
    perm = np.random.RandomState(12).permutation(len(rows))
    m = None
    for name, keep in (("whole", np.ones(len(rows), bool)), ("cut", np.arange(len(rows)) != 1500)):
        shuffled = rows[perm][keep[perm]]
        parts = np.split(shuffled, [700, 701, 1600, 1600, 2400])
        paths = [str(tmp_path / f"{name}{i}.bin") for i in range(5)]
        for p, part in zip(paths, parts[:5]):
            cr.write_map(p, part)
        if m is not None:
            m.close()
        m = _ctx(parts[5])
        got, want = run(m, paths, parts, name, include_model=True, voxel_mm=1000)
        if name == "whole":
            assert got["info"]["components"] == 1 and got["components"]["records"].tolist() == [3000] and got["components"]["cells"].tolist() == [3000]
        else:
            assert got["info"]["components"] == 2 and sorted(got["components"]["records"].tolist()) == [1499, 1500]
            first = got["components"]["first"].tolist()
            assert first[0] == 0 and first[1] > 0 and got["labels"][0] == 0 and got["labels"][first[1]] == 1
        assert m.segment_stats()["chunks"] == 2 * 5
        ts.same_rows(m.download_model(), parts[5], "the live model")
    m.close()


def slab_rows():
    rs = np.random.RandomState(21)
    x, y, z = np.meshgrid(np.arange(100), np.arange(100), np.arange(7), indexing="ij")
    cells = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    specks = np.stack([200 + 3 * np.arange(300), np.zeros(300, np.int64), 3 * (np.arange(300) % 5)], axis=1)
    cells = np.concatenate([cells, specks])[rs.permutation(70300)]
    rows = np.tile(in_cell(0, 0, 0), (len(cells), 1))
    rows[:, 0:3] = cells.astype(np.float32) + np.float32(0.5)
    rows[:, 6] = np.arange(len(rows)) % 97
    return rows


@pytest.mark.gpu
def test_gpu_slab_and_specks_with_and_without_the_combination(tmp_path):
    """70 000 records fill 100 x 100 x 7 cells: one root that every slot adds to; 300 single records alone in their cells are specks"""
    rows = slab_rows()
    path, out = str(tmp_path / "slab.bin"), tmp_path / "kept.bin"
    cr.write_map(path, rows, 5, 6)
    kw = dict(voxel_mm=1000, min_records=2)
    want = sg.segment(rows, **kw)
    assert want["info"]["counts_by_kind"] == [70000, 300, 0, 0] and want["info"]["components"] == 1 and want["info"]["small_components"] == 300
    m = _ctx()
    got, _ = run(m, [path], [rows], "combined", out_path=out, frame=(5, 6), want=want, **kw)
    assert len(got["components"]) == 1 and got["components"]["records"][0] == got["components"]["cells"][0] == 70000
    assert got["info"]["counts_by_kind"] == [70000, 300, 0, 0] and got["info"]["small_components"] == 300 and got["info"]["written"] == 70000
    os.environ["SM_SEGMENT_NO_COMBINE"] = "1"
    try:
        alone, _ = run(m, [path], [rows], "not combined", out_path=tmp_path / "kept2.bin", frame=(5, 6), want=want, **kw)
    finally:
        os.environ.pop("SM_SEGMENT_NO_COMBINE", None)
    assert np.array_equal(alone["labels"], got["labels"]) and alone["components"].tobytes() == got["components"].tobytes() and alone["info"] == got["info"]
    assert open(tmp_path / "kept2.bin", "rb").read() == open(out, "rb").read()
    _no_tmp(tmp_path)
    m.close()


@pytest.mark.gpu
def test_gpu_cap_below_the_components(scene, tmp_path):
    from surfelmapping_amd import capi
    path = str(tmp_path / "scene.bin")
    cr.write_map(path, scene.rows)
    want = sg.segment(scene.rows, voxel_mm=200)
    assert want["info"]["components"] > 3
    m = _ctx()
    got = m.segment_maps([path], max_components=2, voxel_mm=200)
    assert got["info"]["components"] == want["info"]["components"] and np.array_equal(got["labels"], want["labels"])
    assert got["components"].tobytes() == want["components"][:2].tobytes()
    # the third row of the caller's buffer is not touched
    buf = np.full(3 * 64, 0xA5, np.uint8)
    p, info, src = capi.segment_params(voxel_mm=200), capi.SmSegmentInfo(), capi.map_source([path], False)
    assert m._L.sm_segment_maps(m._h, C.byref(src), C.byref(p), None, buf.ctypes.data_as(C.c_void_p), 2, None, C.byref(info)) == capi.SM_OK
    assert buf[:128].tobytes() == want["components"][:2].tobytes() and (buf[128:] == 0xA5).all() and info.components == want["info"]["components"]
    # no rows at all
    assert m._L.sm_segment_maps(m._h, C.byref(src), C.byref(p), None, None, 0, None, C.byref(info)) == capi.SM_OK
    assert info.components == want["info"]["components"] and info.largest == want["info"]["largest"]
    got = m.segment_maps([path], max_components=0, labels=False, voxel_mm=200)
    assert got["labels"] is None and len(got["components"]) == 0 and got["info"]["components"] == want["info"]["components"]
    m.close()


@pytest.mark.gpu
def test_gpu_out_path(scene, tmp_path):
    """every kind in one set: numbered and small components, a class that is skipped, loose records; two files with frame ranges"""
    loose = ts.loose_rows()
    rows = np.concatenate([scene.rows[:500], loose[:7], scene.rows[500:], loose[7:]])
    classes = sorted(set((np.ascontiguousarray(scene.rows[:, 4]).view(np.uint32) >> 24).tolist()))
    assert len(classes) >= 2
    kw = dict(voxel_mm=100, min_records=4, classes=set(range(256)) - {classes[0]})
    ref_kw = dict(voxel_mm=100, min_records=4, class_mask=sg.class_mask(set(range(256)) - {classes[0]}))
    parts = [rows[:900], rows[900:]]
    paths = [str(tmp_path / "a.bin"), str(tmp_path / "b.bin")]
    cr.write_map(paths[0], parts[0], 7, 12)
    cr.write_map(paths[1], parts[1], 3, 9)
    before = [open(p, "rb").read() for p in paths]
    m = _ctx()
    for mask in (1, 2, 8, 15, 4):
        want = sg.segment_set(parts, write_mask=mask, **ref_kw)
        assert all(c > 0 for c in want["info"]["counts_by_kind"]), want["info"]
        out = tmp_path / f"w{mask}.bin"
        got = m.segment_maps(paths, out_path=str(out), write_mask=mask, **kw)
        check(got, want, mask, out, frame=(3, 12))
        assert rr.read_map(str(out))[1:] == (3, 12)
        assert got["info"]["written"] == sum(c for k, c in enumerate(want["info"]["counts_by_kind"]) if mask >> k & 1)
    # nothing qualifies: a valid empty file
    out = tmp_path / "empty.bin"
    got = m.segment_maps(paths, out_path=str(out), write_mask=2, voxel_mm=100)
    assert got["info"]["written"] == 0 and got["info"]["small_components"] == 0 and open(out, "rb").read() == sg.file_bytes(np.zeros((0, 12)), 3, 12)
    # the output can be read as a set again: the records of numbered components alone have no small component
    again = m.segment_maps([str(tmp_path / "w1.bin")], **kw)
    assert again["info"]["small_components"] == 0 and again["info"]["counts_by_kind"][1:] == [0, 0, 0]
    _no_tmp(tmp_path)
    assert [open(p, "rb").read() for p in paths] == before
    m.close()


@pytest.mark.gpu
def test_gpu_capacity_writes_nothing(scene, tmp_path):
    from surfelmapping_amd import capi
    path = str(tmp_path / "a.bin")
    cr.write_map(path, scene.rows)
    want = sg.segment(scene.rows, voxel_mm=100)
    m = _ctx(scene.rows[:300])
    labels, buf = np.full(len(scene.rows), 0xA5A5A5A5, np.uint32), np.full(4 * 64, 0xA5, np.uint8)
    info, src = capi.SmSegmentInfo(), capi.map_source([path], False)
    info.components = 12345
    p = capi.segment_params(voxel_mm=100, max_cells=want["info"]["cells"] - 1)
    rc = m._L.sm_segment_maps(m._h, C.byref(src), C.byref(p), labels.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), 4,
                              str(tmp_path / "out.bin").encode(), C.byref(info))
    assert rc == capi.SM_E_CAPACITY and "max_cells" in m._L.sm_last_error().decode()
    assert (labels == 0xA5A5A5A5).all() and (buf == 0xA5).all() and info.components == 12345
    assert os.listdir(tmp_path) == ["a.bin"]
    p.max_cells = want["info"]["cells"]                                       # exactly enough
    assert m._L.sm_segment_maps(m._h, C.byref(src), C.byref(p), labels.ctypes.data_as(C.c_void_p), None, 0, None, C.byref(info)) == capi.SM_OK
    assert np.array_equal(labels, want["labels"]) and info.cells == want["info"]["cells"]
    ts.same_rows(m.download_model(), scene.rows[:300], "the live model")
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 257))
def test_gpu_one_record_and_one_lane_in_a_second_block(tmp_path, n):
    rs = np.random.RandomState(n)
    rows = np.stack([surfel(*(rs.rand(3) * 4.0 - 2.0), t0=float(i)) for i in range(n)])
    path = str(tmp_path / "s.bin")
    cr.write_map(path, rows)
    m = _ctx(rows)
    run(m, [path], [rows], n, out_path=tmp_path / "o.bin", voxel_mm=200)
    run(m, [], [rows], (n, "model"), include_model=True, voxel_mm=200, by_class=0)
    run(m, [path], [rows, rows], (n, "both"), include_model=True, out_path=tmp_path / "b.bin", voxel_mm=200, min_records=2, write_mask=3)
    m.close()


@pytest.mark.gpu
def test_gpu_grid_edge_classes_and_loose_records(tmp_path):
    """the hand-made cases of the CPU tests on the device: no wrap and no carry at the grid's edge, negative cells, classes, loose kinds"""
    m = _ctx()
    edge = np.concatenate([grid_edge_rows(), np.stack([at(655.0, 0, 0), at(-0.0, 0, 0), at(-0.004, 0, 0)]), ts.loose_rows()])
    path = str(tmp_path / "edge.bin")
    cr.write_map(path, edge)
    for conn in (6, 18, 26):
        got, _ = run(m, [path], [edge], ("edge", conn), voxel_mm=10, connectivity=conn, out_path=tmp_path / "o.bin", write_mask=9)
        assert got["labels"][:9].tolist() == [0, 1, 2, 3, 4, 5, LOOSE, 6, 6]
    line = np.stack([in_cell(0, 0, 0, sem=3), in_cell(1, 0, 0, sem=7), in_cell(2, 0, 0, sem=3), in_cell(3, 0, 0, sem=200), in_cell(-1, -1, -1, sem=3)])
    cr.write_map(path, line)
    for by_class in (0, 1):
        run(m, [path], [line], ("classes", by_class), voxel_mm=1000, by_class=by_class)
        run(m, [path], [line], ("skipped", by_class), voxel_mm=1000, by_class=by_class, class_mask=sg.class_mask(set(range(256)) - {7}))
    pairs = np.stack([in_cell(10 * i + (d[0] if j else 0), d[1] if j else 0, d[2] if j else 0) for i, d in enumerate(sg.offsets(26)) for j in (0, 1)])
    cr.write_map(path, pairs)
    for conn in (6, 18, 26):
        got, _ = run(m, [path], [pairs], ("pairs", conn), voxel_mm=1000, connectivity=conn)
        assert got["info"]["components"] == 52 - conn
    m.close()


@pytest.mark.gpu
def test_gpu_refusals(scene, tmp_path):
    from surfelmapping_amd import capi
    m = _ctx(scene.rows[:200])
    path = str(tmp_path / "a.bin")
    cr.write_map(path, scene.rows[:600])
    fresh = _ctx()
    with pytest.raises(capi.SurfelMapError) as e:
        fresh.segment_stats()
    assert e.value.rc == capi.SM_E_ARG
    got = fresh.segment_maps([], include_model=True, out_path=str(tmp_path / "none.bin"))        # (an empty set: an empty file)
    assert got["info"]["records"] == 0 and len(got["labels"]) == 0 and open(tmp_path / "none.bin", "rb").read() == sg.file_bytes(np.zeros((0, 12)))
    os.remove(tmp_path / "none.bin")
    for bad in (dict(voxel_mm=9), dict(voxel_mm=10001), dict(connectivity=8), dict(connectivity=0), dict(by_class=2), dict(min_records=0),
                dict(max_cells=0), dict(origin=(0, float("nan"), 0))):
        with pytest.raises(capi.SurfelMapError) as e:
            m.segment_maps([path], **bad)
        assert e.value.rc == capi.SM_E_ARG and list(bad)[0] in str(e.value), (bad, str(e.value))
    for mask in (0, 16):
        with pytest.raises(capi.SurfelMapError) as e:
            m.segment_maps([path], out_path=str(tmp_path / "o.bin"), write_mask=mask)
        assert e.value.rc == capi.SM_E_ARG and "write_mask" in str(e.value)
        m.segment_maps([path], write_mask=mask)                               # (read only with out_path)
    with pytest.raises(capi.SurfelMapError) as e:
        m.segment_maps([path], out_path=path)
    assert e.value.rc == capi.SM_E_ARG and "a.bin" in str(e.value)
    with pytest.raises(capi.SurfelMapError) as e:
        m.segment_maps([str(tmp_path / "nowhere.bin")])
    assert e.value.rc == capi.SM_E_ARG
    short = str(tmp_path / "short.bin")
    with open(short, "wb") as f:
        f.write(open(path, "rb").read()[:-7])
    with pytest.raises(capi.SurfelMapError) as e:                            # (the file checks of the map-set calls)
        m.segment_maps([path, short], out_path=str(tmp_path / "o.bin"))
    assert e.value.rc == capi.SM_E_ARG and "short.bin" in str(e.value)
    p, info, src = capi.default_segment_params(), capi.SmSegmentInfo(), capi.map_source([path], False)
    buf = np.zeros(64, np.uint8)
    assert m._L.sm_segment_maps(m._h, None, C.byref(p), None, None, 0, None, C.byref(info)) == capi.SM_E_ARG
    assert m._L.sm_segment_maps(m._h, C.byref(src), None, None, None, 0, None, C.byref(info)) == capi.SM_E_ARG
    assert m._L.sm_segment_maps(m._h, C.byref(src), C.byref(p), None, None, 0, None, None) == capi.SM_E_ARG
    assert m._L.sm_segment_maps(m._h, C.byref(src), C.byref(p), None, None, 1, None, C.byref(info)) == capi.SM_E_ARG
    assert m._L.sm_segment_maps(m._h, C.byref(src), C.byref(p), None, buf.ctypes.data_as(C.c_void_p), 1, None, C.byref(info)) == capi.SM_OK
    assert m._L.sm_segment_stats(m._h, None) == capi.SM_E_ARG
    # between sm_stage_conflict and sm_stage_cull
    seq = rr.sequence(2)
    st = capi.SurfelMap(capi.make_config(**rr.CAM, **rr.OVER, preprocess=0, max_sqrt_vertices=200))
    for frame in seq:
        st.process_frame(*frame)
    st.stage_conflict(seq[1][3], 1.0, 30.0)
    with pytest.raises(capi.SurfelMapError) as e:
        st.segment_maps([path], include_model=True)
    assert e.value.rc == capi.SM_E_ARG and "sm_stage_conflict" in str(e.value)
    st.stage_cull()
    rows = st.download_model()
    run(st, [path], [scene.rows[:600], rows], "after frames", include_model=True)        # (a model that frames have made)
    st.close()
    for configure in ("shard_stream_configure", "rig_configure"):
        part = _ctx()
        getattr(part, configure)(0, 1)
        with pytest.raises(capi.SurfelMapError) as e:
            part.segment_maps([path])
        assert e.value.rc == capi.SM_E_UNSUPPORTED
        part.close()
    assert sorted(os.listdir(tmp_path)) == ["a.bin", "short.bin"]
    ts.same_rows(m.download_model(), scene.rows[:200], "the live model")
    fresh.close()
    m.close()
