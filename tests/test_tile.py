"""Spatial tiling of a map set (sm_tile_maps, sm_tile_stats; SurfelMap.tile_maps; DESIGN.md "4s. Spatial tiling").  CPU: the
restatement (tile_ref.py) against answers worked by hand and against its own invariances; the library's symbols, defaults, header
and the argument rules that need no device.  GPU: every file the HIP path writes against the restatement, byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import recall_ref as cr
import retire_ref as rr
import test_simplify as ts
import tile_ref as tr
from test_simplify import surfel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sm_default_tile_params", "sm_tile_maps", "sm_tile_stats")
STAT_KEYS = ("records_in", "placed", "loose", "tiles", "largest_tile", "files_written")
NAN, INF = np.float32("nan"), np.float32("inf")


@pytest.fixture(scope="module")
def scene():
    return ts.Scene()


def at(x, y, z, **kw):
    return surfel(x, y, z, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, by hand
# ---------------------------------------------------------------------------------------------------------------------
def test_worked_example():
    """tile_ref's docstring: cell_mm 1000, V = 65536, origin 0"""
    assert tr.cell_edge(1000) == 65536 and tr.cell_edge(100) == 6554 and tr.cell_edge(200) == 13107 and tr.cell_edge(10) == 655
    names = "FAGBCDE"
    rows = np.stack([at(-0.5, .5, .5), at(.5, .5, .5), at(-0.0, .5, .5), at(1.5, .5, .5), at(.5, 1.5, .5), at(.5, .5, 1.5), at(2.5, .5, .5)])
    M, placed = tr.keys(rows, 1000)
    assert placed.all()
    assert [hex(int(m)) for m in M] == ["0x6249249249249", "0x7000000000000", "0x7000000000000", "0x7000000000001", "0x7000000000002",
                                       "0x7000000000004", "0x7000000000008"]
    # given in the order E D C B G A F: A and G tie on M and go by id
    back = rows[::-1]
    files, st = tr.tile(back, cell_mm=1000, tile_shift=17)
    assert len(files) == 1 and st["tiles"] == 1
    order = "".join(names[[r.tobytes() for r in rows].index(f.tobytes())] for f in files[0])
    assert order == "FGABCDE"                                                # (in `back` G has id 4 and A id 5)
    files, st = tr.tile(rows, cell_mm=1000, tile_shift=17)
    assert "".join(names[[r.tobytes() for r in rows].index(f.tobytes())] for f in files[0]) == "FAGBCDE"
    # tile_shift 1: F | A G B C D | E
    files, st = tr.tile(rows, cell_mm=1000, tile_shift=1, max_file_records=5)
    assert st["tiles"] == 3 and st["largest_tile"] == 5 and [len(f) for f in files] == [1, 5, 1]
    files, st = tr.tile(rows, cell_mm=1000, tile_shift=1, max_file_records=6)
    assert [len(f) for f in files] == [6, 1]
    assert (M >> np.uint64(3)).tolist() == [0xC49249249249, 0xE00000000000, 0xE00000000000, 0xE00000000000, 0xE00000000000, 0xE00000000000,
                                            0xE00000000001]


def test_single_bits_sort_by_3i_plus_k():
    """the 51 records that differ from the base (cell -65536 on every axis: u = 0, M = 0) in bit i of axis k have M = 1 << (3 i + k)"""
    V = tr.cell_edge(1000)
    assert V == 65536
    rows, want = [], []
    for i in range(17):
        for k in range(3):
            p = [-65536.0 + 0.5] * 3
            p[k] = float(-65536 + (1 << i)) + 0.5
            rows.append(at(*p))
            want.append(1 << (3 * i + k))
    rows = np.stack(rows)
    M, placed = tr.keys(rows, 1000)
    assert placed.all() and [int(m) for m in M] == want and want == sorted(want)
    perm = np.random.RandomState(1).permutation(51)
    files, _ = tr.tile(rows[perm], cell_mm=1000, tile_shift=17)
    assert files[0].tobytes() == rows.tobytes()


def test_negative_coordinates_origin_and_minus_zero():
    V = tr.cell_edge(100)                                                     # 6554
    u = lambda x, o=0.0: int(tr.keys(at(x, 0, 0)[None], 100, (o, 0, 0))[0][0]) & 0x1249249249249    # noqa: E731  (the x bits)
    spread = lambda c: sum(((c + 65536) >> i & 1) << (3 * i) for i in range(17))                    # noqa: E731
    assert u(-0.03125) == spread(-1) and u(0.03125) == spread(0)             # X = -2048 floors to cell -1: no truncation
    assert u(-0.0) == spread(0) and u(0.0) == spread(0)
    assert u(-0.03125, -1.0) == spread(9) and u(0.03125, -1.0) == spread(10)  # X = 63488, 67584 about origin -1
    # exactly on a cell face: X a multiple of V belongs to the cell that begins there
    x = np.float32(3 * V / 65536.0)
    assert int(np.floor(np.float64(x) * 65536.0)) == 3 * V
    assert u(x) == spread(3) and u(np.nextafter(x, np.float32(0))) == spread(2)
    x = np.float32(-3 * V / 65536.0)
    assert u(x) == spread(-3) and u(np.nextafter(x, np.float32(-1))) == spread(-4)


def test_grid_edge_and_loose_records():
    """cell_mm 10: V = 655; cell 65535 is [655 * 65535, 655 * 65536) / 65536 m = [654.99.., 655.0) m"""
    last, first_out = np.float32(654.995), np.float32(655.0)
    M, ok = tr.keys(at(last, 0, 0)[None], 10)
    assert ok[0] and int(M[0]) & 0x1249249249249 == 0x1249249249249          # u[0] = 131071: all 17 bits
    assert not tr.keys(at(first_out, 0, 0)[None], 10)[1][0]
    assert tr.keys(at(-655.0, 0, 0)[None], 10)[1][0] and not tr.keys(at(np.nextafter(np.float32(-655.0), -INF), 0, 0)[None], 10)[1][0]
    assert tr.keys(at(first_out, 0, 0)[None], 100)[1][0]                      # (placed on a coarser grid)
    assert not tr.keys(at(first_out, 0, 0)[None], 10, (-0.5, 0, 0))[1][0] and tr.keys(at(first_out, 0, 0)[None], 10, (0.5, 0, 0))[1][0]
    loose = loose_rows()
    assert not tr.keys(loose, 10000)[1][:5].any() and not tr.keys(loose, 10)[1].any()
    assert tr.keys(at(300000.0, 0, 0)[None], 10000)[1][0]                     # 300 km at 10 m cells: cell 30000
    placed = np.stack([at(0, 0, 1, conf=0.0), at(0, 0, 1, conf=-1.0), at(0, 0, 1, n=(0, NAN, 1)), at(0, 0, 1, r=-0.5), at(0, 0, 1, n=(0, 0, 0)),
                       at(0, 0, 1, t1=NAN)])
    assert tr.keys(placed, 10)[1].all()
    rows = np.concatenate([loose[:3], placed[:2], loose[3:], placed[2:]])
    files, st = tr.tile(rows, cell_mm=10)
    assert st["placed"] == 6 and st["loose"] == len(loose) and len(files) == 2
    assert files[0].tobytes() == placed.tobytes() and files[1].tobytes() == loose.tobytes()


def loose_rows():
    """one of each kind at cell_mm = 10: NaN, +-inf, |p - origin| >= 2^24, the first cell outside the grid"""
    return np.stack([at(NAN, 0, 1), at(0, INF, 1), at(0, 0, -INF), at(2.0e7, 0, 1), at(0, -16777216.0, 1), at(655.0, 0, 1), at(0, 0, -3000.0)])


def test_file_plan():
    assert tr.plan_files([3, 4, 2, 9, 1, 1], 10) == [9, 10, 1]                # 3 + 4 + 2 | 9 + 1 | 1
    assert tr.plan_files([3, 4, 3, 1], 10) == [10, 1]                        # (a file may be exactly full)
    assert tr.plan_files([25], 10) == [10, 10, 5]                            # 2.5 * max_file_records: three files
    assert tr.plan_files([4, 25, 4], 10) == [4, 10, 10, 5, 4]                # (a large tile is written alone)
    assert tr.plan_files([], 10) == []
    assert tr.plan_batches([3, 4, 2, 9, 1, 1], 10) == [9, 10, 1]
    with pytest.raises(tr.Capacity):
        tr.plan_batches([3, 11], 10)
    rows = np.stack([at(0.5 + (i % 3), 0.5, 0.5) for i in range(30)] + [at(NAN, 0, 0)])
    files, st = tr.tile(rows, cell_mm=1000, tile_shift=0, max_file_records=4)
    assert [len(f) for f in files] == [4, 4, 2, 4, 4, 2, 4, 4, 2, 1] and st["tiles"] == 3 and st["largest_tile"] == 10
    assert np.isnan(files[-1][0, 0])                                          # the loose file comes last
    files, st = tr.tile(np.zeros((0, 12), np.float32))
    assert files == [] and st["files_written"] == 0
    with pytest.raises(tr.Capacity):
        tr.tile(rows, cell_mm=1000, tile_shift=0, max_tiles=2)
    st = dict(batches=[9, 9, 2], file_records=[5, 4, 5, 4, 2])
    assert not tr.spans_a_batch_boundary(st)
    assert tr.spans_a_batch_boundary(dict(batches=[9, 9, 2], file_records=[5, 6, 7, 2]))


def same_files(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.asarray(g, np.float32).tobytes() == np.asarray(w, np.float32).tobytes(), (what, i)


def test_restatement_is_a_function_of_ids_and_records_and_idempotent(scene):
    rows = scene.rows
    kw = dict(cell_mm=100, tile_shift=3, max_file_records=256)
    want, st = tr.tile(rows, **kw)
    assert st["tiles"] > 20 and len(want) > 4 and st["loose"] == 0
    perm = np.random.RandomState(7).permutation(len(rows))
    same_files(tr.tile(rows[perm], ids=perm, **kw)[0], want, "permuted, ids kept")
    for cuts in ((), (700,), (300, 301, 900, 900)):
        parts = np.split(rows, list(cuts))
        assert len(parts) in (1, 2, 5)
        same_files(tr.tile_set(parts, **kw)[0], want, cuts)
    same_files(tr.tile(rows, capacity=256, **kw)[0], want, "capacity")
    again, st2 = tr.tile_set(want, **kw)
    same_files(again, want, "idempotent")
    # ties keep id order whatever the order of the rows
    copies = np.stack([at(1.0, 2.0, 3.0, t0=float(i)) for i in range(40)])
    files, _ = tr.tile(copies[::-1], ids=np.arange(40)[::-1], cell_mm=100)
    assert files[0].tobytes() == copies.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the library, without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_defaults_and_binding():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None and name in capi.SYMBOLS
    p = capi.default_tile_params()
    got = dict(cell_mm=p.cell_mm, tile_shift=p.tile_shift, origin=tuple(p.origin), max_file_records=p.max_file_records, max_tiles=p.max_tiles)
    assert got == tr.DEFAULTS == dict(cell_mm=200, tile_shift=7, origin=(0.0, 0.0, 0.0), max_file_records=1 << 20, max_tiles=1 << 20)
    q = capi.tile_params(cell_mm=20, origin=(1, 2, 3))
    assert q.cell_mm == 20 and tuple(q.origin) == (1.0, 2.0, 3.0)
    with pytest.raises(KeyError):
        capi.tile_params(cell=1)
    for name in ("tile_maps", "tile_stats"):
        assert callable(getattr(capi.SurfelMap, name))
    header = open(os.path.join(ROOT, "include", "sm_c_api.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
    assert "typedef struct sm_tile_params {" in header and "typedef struct sm_tile_stats_t {" in header


def test_argument_rules_that_need_no_device():
    from surfelmapping_amd import capi
    L = capi.load()
    p, st = capi.default_tile_params(), capi.SmTileStats()
    src = capi.map_source([], True)
    assert L.sm_default_tile_params(None) == capi.SM_E_ARG
    assert L.sm_tile_maps(None, C.byref(src), C.byref(p), b"tiled") == capi.SM_E_ARG
    assert L.sm_tile_stats(None, C.byref(st)) == capi.SM_E_ARG
    assert not os.path.exists("tiled_000000.bin")


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
_ctx, _no_tmp = ts._ctx, ts._no_tmp


def check_files(paths, want, frame, what):
    """every file byte for byte: header (count, the frame range) and records"""
    assert len(paths) == len(want), (what, len(paths), len(want))
    for i, (p, w) in enumerate(zip(paths, want)):
        assert os.path.basename(p).endswith("_%06d.bin" % i)
        assert open(p, "rb").read() == tr.file_bytes(w, *frame), (what, i)


def check_stats(got, st, what):
    assert {k: got[k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}, (what, got, st)
    batches = len(st["batches"])
    assert got["readings"] == ((1 + max(batches, 1 if st["loose"] else 0)) if st["records_in"] else 0), (what, got, st)


def run(m, paths, prefix, what, parts, frame=(0, 0), include_model=False, **kw):
    """tile_maps of `paths` against the restatement of `parts`; -> (the files written, the tally)"""
    files = m.tile_maps(paths, str(prefix), include_model=include_model, **{k: v for k, v in kw.items() if k != "capacity"})
    got = m.tile_stats()
    want, st = tr.tile_set(parts, **kw)
    check_files(files, want, frame, what)
    check_stats(got, st, what)
    return files, got, st


@pytest.mark.gpu
@pytest.mark.parametrize("cell_mm", (100, 1000))
@pytest.mark.parametrize("tile_shift", (0, 2, 17))
def test_gpu_scene_as_one_file(scene, tmp_path, tile_shift, cell_mm):
    path = str(tmp_path / "scene.bin")
    cr.write_map(path, scene.rows, 3, 4)
    m = _ctx()
    files, got, st = run(m, [path], tmp_path / "t", (cell_mm, tile_shift), [scene.rows], frame=(3, 4), cell_mm=cell_mm, tile_shift=tile_shift,
                         max_file_records=256)
    assert got["tiles"] == (1 if tile_shift == 17 else st["tiles"]) and len(files) >= 7 and got["sort_passes"] >= 2
    assert got["readings"] == 2 and got["chunks"] == 2 and got["device_ms"] > 0.0 and got["launches"] > 0
    assert rr.read_map(path)[0].tobytes() == scene.rows.tobytes()
    _no_tmp(tmp_path)
    m.close()


@pytest.mark.gpu
def test_gpu_rows_shuffled_and_idempotent(scene, tmp_path):
    """the same rows in another order, and every id another; then the output tiled again reproduces itself"""
    rows = scene.rows[np.random.RandomState(5).permutation(len(scene.rows))]
    path = str(tmp_path / "shuffled.bin")
    cr.write_map(path, rows, 1, 2)
    m = _ctx()
    kw = dict(cell_mm=100, tile_shift=3, max_file_records=256)
    files, got, st = run(m, [path], tmp_path / "t", "shuffled", [rows], frame=(1, 2), **kw)
    again = m.tile_maps(files, str(tmp_path / "u"), **kw)
    assert len(again) == len(files) and [open(p, "rb").read() for p in again] == [open(p, "rb").read() for p in files]
    _no_tmp(tmp_path)
    m.close()


@pytest.mark.gpu
def test_gpu_five_files_and_the_model(scene, tmp_path):
    """five files (one of a single row, one empty) plus a live remainder against the restatement and against the one-file run"""
    rows = scene.rows
    parts = np.split(rows, [300, 301, 900, 900, 1500])
    paths = [str(tmp_path / f"m{i}.bin") for i in range(5)]
    for i, (p, part) in enumerate(zip(paths, parts[:5])):
        cr.write_map(p, part, 10 + i, 20 + i)
    one = str(tmp_path / "one.bin")
    cr.write_map(one, rows, 10, 24)
    m = _ctx(parts[5])
    before = [open(p, "rb").read() for p in paths + [one]]
    kw = dict(cell_mm=100, tile_shift=3, max_file_records=256)
    files, got, st = run(m, paths, tmp_path / "five", "five files", parts, frame=(10, 24), include_model=True, **kw)
    assert got["chunks"] == 2 * 5                                            # (the empty file has no chunk; the model is one)
    single, _, _ = run(m, [one], tmp_path / "one", "one file", [rows], frame=(10, 24), **kw)
    assert [open(p, "rb").read() for p in single] == [open(p, "rb").read() for p in files]
    # the files alone; the model alone (no file: the frame range is 0, 0)
    run(m, paths, tmp_path / "files", "files alone", parts[:5], frame=(10, 24), **kw)
    run(m, [], tmp_path / "live", "model alone", parts[5:], include_model=True, **kw)
    assert m.tile_maps([paths[3]], str(tmp_path / "none")) == [] and m.tile_stats()["records_in"] == 0
    assert [open(p, "rb").read() for p in paths + [one]] == before
    ts.same_rows(m.download_model(), parts[5], "the live model")
    _no_tmp(tmp_path)
    m.close()


@pytest.mark.gpu
def test_gpu_result_does_not_depend_on_the_sort_capacity(scene, tmp_path):
    """SM_TILE_SORT_RECORDS=256 with max_file_records=256 against the default capacity: the same bytes from more readings.  With the
    two limits equal, files and batches are cut by one rule and no file can span a batch boundary; at a capacity of 384 the plans
    differ, and the restatement confirms that a file then holds records of two batches."""
    path = str(tmp_path / "scene.bin")
    cr.write_map(path, scene.rows)
    kw = dict(cell_mm=100, tile_shift=2, max_file_records=256)
    m = _ctx()
    base, got0, st0 = run(m, [path], tmp_path / "d", "default capacity", [scene.rows], **kw)
    assert st0["largest_tile"] <= 256 and got0["readings"] == 2
    want = [open(p, "rb").read() for p in base]
    try:
        for cap in (256, 384):
            os.environ["SM_TILE_SORT_RECORDS"] = str(cap)
            files, got, st = run(m, [path], tmp_path / f"c{cap}", cap, [scene.rows], capacity=cap, **kw)
            assert [open(p, "rb").read() for p in files] == want
            assert got["readings"] == 1 + len(st["batches"]) > 2
            assert tr.spans_a_batch_boundary(st) == (cap == 384)
    finally:
        os.environ.pop("SM_TILE_SORT_RECORDS", None)
    _no_tmp(tmp_path)
    m.close()


@pytest.mark.gpu
def test_gpu_equal_keys_keep_id_order(tmp_path):
    """300 copies of one position across three files, between records that are alone in their cells: the copies come out in id
    order (they differ in colour and times), and a set of nothing but copies needs no sort pass"""
    rs = np.random.RandomState(11)
    copies = np.stack([surfel(1.01, 0.52, 7.03, conf=float(rs.randint(1, 40)) / 16.0, bgr=tuple(int(v) for v in rs.randint(0, 256, 3)),
                              t0=float(i), t1=float(rs.randint(50, 99))) for i in range(300)])
    alone = np.stack([surfel(0.3 * i, 1.0, 5.0) for i in range(9)])
    parts = [np.concatenate([alone[3 * i:3 * i + 2], copies[100 * i:100 * i + 100], alone[3 * i + 2:3 * i + 3]]) for i in range(3)]
    paths = [str(tmp_path / f"c{i}.bin") for i in range(3)]
    for p, f in zip(paths, parts):
        cr.write_map(p, f)
    m = _ctx()
    files, got, st = run(m, paths, tmp_path / "t", "300 copies", parts, cell_mm=50, tile_shift=17)
    out = rr.read_map(files[0])[0]
    mine = out[out[:, 0] == np.float32(1.01)]
    assert len(mine) == 300 and mine[:, 6].tolist() == [float(i) for i in range(300)]
    only = [str(tmp_path / f"o{i}.bin") for i in range(3)]
    for i, p in enumerate(only):
        cr.write_map(p, copies[100 * i:100 * i + 100])
    files, got, st = run(m, only, tmp_path / "o", "copies only", [copies], cell_mm=50, tile_shift=0)
    assert got["sort_passes"] == 0 and got["tiles"] == 1 and rr.read_map(files[0])[0].tobytes() == copies.tobytes()
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 257))
def test_gpu_one_record_and_one_lane_in_a_second_block(tmp_path, n):
    rs = np.random.RandomState(n)
    rows = np.stack([surfel(*(rs.rand(3) * 40.0 - 20.0), t0=float(i)) for i in range(n)])
    path = str(tmp_path / "s.bin")
    cr.write_map(path, rows)
    m = _ctx()
    run(m, [path], tmp_path / "t", n, [rows], cell_mm=200, tile_shift=4, max_file_records=256)
    m.close()


@pytest.mark.gpu
def test_gpu_scan_over_more_than_one_of_its_tiles(tmp_path):
    """140 000 records in one batch: a sort pass has ceil(140000 / 8192) = 18 blocks, so its (digit, block) scan runs over 18 * 256 =
    4608 entries, more than the 4096 one step of the scan covers; the last block is partly filled (736 of 8192).  Random centres in
    a 200 m cube at 200 mm cells, so every digit varies."""
    n = 140000
    rs = np.random.RandomState(3)
    rows = np.tile(surfel(0.0, 0.0, 0.0), (n, 1))
    rows[:, 0:3] = (rs.rand(n, 3) * 200.0 - 100.0).astype(np.float32)
    rows[:, 6] = np.arange(n) % 97
    rows[1000:1200, 0:3] = rows[5, 0:3]                                       # (ties across blocks)
    path = str(tmp_path / "s.bin")
    cr.write_map(path, rows)
    m = _ctx()
    files, got, st = run(m, [path], tmp_path / "t", "140000", [rows], cell_mm=200, tile_shift=17, max_file_records=65536)
    assert got["sort_passes"] >= 4 and len(files) == 3 and got["readings"] == 2
    m.close()


@pytest.mark.gpu
def test_gpu_passes_with_one_digit_in_all_keys_are_skipped(tmp_path):
    """cell_mm 10 (V = 655).  (a) x = 0.001 and x = 327.501 (X = 21463105 = 655 * 32768 + 65: cell 32768 = bit 15 of u[0] = bit 45 of
    M), everything else equal: the keys differ in the sixth digit alone.  (b) cells 0..3 on every axis: bits 0..5 of M, the lowest
    digit alone.  One pass each; (c) both together vary two digits: two passes."""
    assert int(tr.keys(at(327.501, 0.001, 0.001)[None], 10)[0][0]) ^ int(tr.keys(at(0.001, 0.001, 0.001)[None], 10)[0][0]) == 1 << 45
    rs = np.random.RandomState(2)
    far = np.stack([at(327.501 if rs.rand() < 0.5 else 0.001, 0.001, 0.001, t0=float(i)) for i in range(600)])
    low = np.stack([at(*(rs.randint(0, 4, 3) * 0.01 + 0.001), t0=float(i)) for i in range(600)])
    assert len(np.unique(tr.keys(low, 10)[0])) == 64 and int(tr.keys(low, 10)[0].max() ^ tr.keys(low, 10)[0].min()) < 256
    m = _ctx()
    for name, rows, passes in (("far", far, 1), ("low", low, 1), ("both", np.concatenate([far, low]), 2)):
        path = str(tmp_path / f"{name}.bin")
        cr.write_map(path, rows)
        files, got, st = run(m, [path], tmp_path / name, name, [rows], cell_mm=10, tile_shift=17)
        assert got["sort_passes"] == passes, (name, got)
    m.close()


@pytest.mark.gpu
def test_gpu_loose_records(tmp_path):
    """one loose record of each kind and placed records that the simplification would call irregular, in a file and in the model;
    then a set of loose records alone"""
    loose = loose_rows()
    placed = np.stack([at(0.3, 0, 1, conf=0.0), at(0.1, 0, 1, n=(0, NAN, 1)), at(0.2, 0, 1, r=-0.5), at(-0.2, 0.1, 1)])
    rows = np.concatenate([loose[:3], placed[:2], loose[3:], placed[2:]])
    rows[:, 5] = 0.0                                                          # (a model does not keep the standby word)
    path = str(tmp_path / "l.bin")
    cr.write_map(path, rows)
    m = _ctx(rows)
    files, got, st = run(m, [path], tmp_path / "f", "loose, file", [rows], cell_mm=10)
    assert got["loose"] == len(loose) and got["placed"] == 4 and len(files) == 2
    run(m, [], tmp_path / "m", "loose, model", [rows], include_model=True, cell_mm=10)
    run(m, [path], tmp_path / "b", "loose, both", [rows, rows], include_model=True, cell_mm=10)
    cr.write_map(path, loose)
    files, got, st = run(m, [path], tmp_path / "o", "loose alone", [loose], cell_mm=10)
    assert len(files) == 1 and got["tiles"] == 0 and got["readings"] == 2
    _no_tmp(tmp_path)
    m.close()


@pytest.mark.gpu
def test_gpu_capacity_errors_write_nothing(scene, tmp_path):
    from surfelmapping_amd import capi
    path = str(tmp_path / "a.bin")
    cr.write_map(path, scene.rows)
    m = _ctx()
    with pytest.raises(capi.SurfelMapError) as e:
        m.tile_maps([path], str(tmp_path / "t"), cell_mm=100, tile_shift=0, max_tiles=2)
    assert e.value.rc == capi.SM_E_CAPACITY and "max_tiles" in str(e.value)
    os.environ["SM_TILE_SORT_RECORDS"] = "256"
    try:
        with pytest.raises(capi.SurfelMapError) as e:
            m.tile_maps([path], str(tmp_path / "t"), cell_mm=100, tile_shift=17, max_file_records=256)
        assert e.value.rc == capi.SM_E_CAPACITY and "tile_shift" in str(e.value)
        with pytest.raises(capi.SurfelMapError) as e:                        # max_file_records above the sort capacity
            m.tile_maps([path], str(tmp_path / "t"), cell_mm=100, tile_shift=0, max_file_records=257)
        assert e.value.rc == capi.SM_E_ARG and "max_file_records" in str(e.value)
    finally:
        os.environ.pop("SM_TILE_SORT_RECORDS", None)
    assert os.listdir(tmp_path) == ["a.bin"]
    m.close()


@pytest.mark.gpu
def test_gpu_refusals(scene, tmp_path):
    from surfelmapping_amd import capi
    m = _ctx(scene.rows[:200])
    path, prefix = str(tmp_path / "a_000001.bin"), str(tmp_path / "t")
    cr.write_map(path, scene.rows[:600])
    fresh = _ctx()
    with pytest.raises(capi.SurfelMapError) as e:
        fresh.tile_stats()
    assert e.value.rc == capi.SM_E_ARG
    assert fresh.tile_maps([], prefix, include_model=True) == [] and fresh.tile_stats()["files_written"] == 0     # (an empty set: no file)
    for bad in (dict(cell_mm=9), dict(cell_mm=10001), dict(tile_shift=-1), dict(tile_shift=18), dict(origin=(0, float("nan"), 0)),
                dict(max_file_records=255), dict(max_file_records=(1 << 22) + 1), dict(max_tiles=0)):
        with pytest.raises(capi.SurfelMapError) as e:
            m.tile_maps([path], prefix, **bad)
        assert e.value.rc == capi.SM_E_ARG and list(bad)[0] in str(e.value), (bad, str(e.value))
    # an output name that is a source: the second file of the plan (256-record files of 600 + 200 records) would be a_000001.bin
    with pytest.raises(capi.SurfelMapError) as e:
        m.tile_maps([path], str(tmp_path / "a"), include_model=True, cell_mm=100, tile_shift=2, max_file_records=256)
    assert e.value.rc == capi.SM_E_ARG and "a_000001.bin" in str(e.value)
    with pytest.raises(capi.SurfelMapError) as e:
        m.tile_maps([str(tmp_path / "nowhere.bin")], prefix)
    assert e.value.rc == capi.SM_E_ARG
    short = str(tmp_path / "short.bin")
    with open(short, "wb") as f:
        f.write(open(path, "rb").read()[:-7])
    with pytest.raises(capi.SurfelMapError) as e:                            # (the file checks of the map-set calls)
        m.tile_maps([path, short], prefix)
    assert e.value.rc == capi.SM_E_ARG and "short.bin" in str(e.value)
    p = capi.default_tile_params()
    src = capi.map_source([path], False)
    assert m._L.sm_tile_maps(m._h, None, C.byref(p), prefix.encode()) == capi.SM_E_ARG
    assert m._L.sm_tile_maps(m._h, C.byref(src), None, prefix.encode()) == capi.SM_E_ARG
    assert m._L.sm_tile_maps(m._h, C.byref(src), C.byref(p), None) == capi.SM_E_ARG
    assert m._L.sm_tile_stats(m._h, None) == capi.SM_E_ARG
    # between sm_stage_conflict and sm_stage_cull
    seq = rr.sequence(2)
    st = capi.SurfelMap(capi.make_config(**rr.CAM, **rr.OVER, preprocess=0, max_sqrt_vertices=200))
    for frame in seq:
        st.process_frame(*frame)
    st.stage_conflict(seq[1][3], 1.0, 30.0)
    with pytest.raises(capi.SurfelMapError) as e:
        st.tile_maps([path], prefix, include_model=True)
    assert e.value.rc == capi.SM_E_ARG and "sm_stage_conflict" in str(e.value)
    st.stage_cull()
    rows = st.download_model()
    run(st, [path], tmp_path / "frames", "after frames", [scene.rows[:600], rows], include_model=True)   # (a model that frames have made)
    st.close()
    for f in os.listdir(tmp_path):
        if f.startswith("frames_"):
            os.remove(tmp_path / f)
    for configure in ("shard_stream_configure", "rig_configure"):
        part = _ctx()
        getattr(part, configure)(0, 1)
        with pytest.raises(capi.SurfelMapError) as e:
            part.tile_maps([path], prefix)
        assert e.value.rc == capi.SM_E_UNSUPPORTED
        part.close()
    assert sorted(os.listdir(tmp_path)) == ["a_000001.bin", "short.bin"]
    ts.same_rows(m.download_model(), scene.rows[:200], "the live model")
    fresh.close()
    m.close()


@pytest.mark.gpu
def test_gpu_more_than_a_chunk(tmp_path):
    """2^20 + 450 records in one file, so that every reading takes the file in two chunks and the ranks of the second go on from the
    first's: surfels on a 1 m lattice 1024 wide, 1 m cells, tiles of 128 m (8 by 8, and 3 that the last 300 records begin), and 150 exact positions of the first
    150 laid across the chunk boundary (they differ from the originals in their times, so their id order shows)."""
    n_a, n_b, n_dup = (1 << 20) - 100, 400, 150
    i = np.arange(n_a + n_b)
    rows = np.tile(surfel(0.0, 0.0, 5.0, r=0.5), (n_a + n_b, 1))
    rows[:, 0], rows[:, 1] = i % 1024 + 0.5, i // 1024 + 0.5
    rows[:, 6] = rows[:, 7] = (i % 50).astype(np.float32)
    dup = rows[:n_dup].copy()
    dup[:, 6] = 77.0
    rows = np.concatenate([rows[:n_a], dup, rows[n_a:]])
    assert len(rows) == (1 << 20) + 450
    path = str(tmp_path / "big.bin")
    cr.write_map(path, rows)
    m = _ctx()
    files, got, st = run(m, [path], tmp_path / "t", "two chunks", [rows], cell_mm=1000, tile_shift=7, max_file_records=1 << 18)
    assert got["chunks"] == 4 and got["tiles"] == 64 + 3 and got["largest_tile"] == 128 * 128 + 128 and len(files) >= 4
    first = rr.read_map(files[0])[0]
    assert first[0].tobytes() == rows[0].tobytes() and first[1].tobytes() == dup[0].tobytes()
    m.close()


@pytest.mark.gpu
def test_gpu_downstream_calls_profit(scene, tmp_path):
    """The scene at three offsets 60 m apart, rows shuffled, against the same set tiled into 256-record files: a COUNT recall finds
    the same records and skips files by their boxes; the streamed renderer draws the same depth and skips more (block, view) pairs."""
    parts = []
    for k in range(3):
        r = scene.rows.copy()
        r[:, 0] += np.float32(60.0 * k)
        parts.append(r)
    rows = np.concatenate(parts)
    rows = rows[np.random.RandomState(9).permutation(len(rows))]
    shuffled = str(tmp_path / "shuffled.bin")
    cr.write_map(shuffled, rows)
    m = _ctx()
    tiled, got, st = run(m, [shuffled], tmp_path / "t", "three scenes", [rows], cell_mm=200, tile_shift=5, max_file_records=256)
    assert len(tiled) > 12
    pose = np.array(scene.view, np.float32).reshape(16).copy()
    n_shuffled = m.recall([shuffled], pose=pose, mode="count", radius=20.0)
    n_tiled = m.recall(tiled, pose=pose, mode="count", radius=20.0)
    assert n_tiled == n_shuffled == int(cr.near(rows, pose, 20.0).sum()) > 0
    assert m.recall_stats()["files_skipped"] > 0
    views = []
    for k in range(3):
        v = pose.copy()
        v[12] += np.float32(60.0 * k)
        views.append(v)
    views = np.stack(views)
    d_shuffled = m.render_image_maps([shuffled], views, *ts.CAM, include_model=False, depth=True)[2]
    skipped_shuffled = m.render_maps_stats()["pairs_skipped"]
    d_tiled = m.render_image_maps(tiled, views, *ts.CAM, include_model=False, depth=True)[2]
    skipped_tiled = m.render_maps_stats()["pairs_skipped"]
    print("pairs skipped: shuffled", skipped_shuffled, "tiled", skipped_tiled, "of", m.render_maps_stats()["pairs_tested"])
    assert (d_shuffled != 0).sum() > 1000 and np.array_equal(d_tiled, d_shuffled)
    assert skipped_tiled > skipped_shuffled
    m.close()
