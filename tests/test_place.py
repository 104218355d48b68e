"""Place recognition (sm_fern_*, sm_search_pose_at, sm_close_loop_at; SurfelMap.set_ferns / fern_encode / fern_add / fern_match /
fern_keyframes / fern_save / fern_load, search_pose(pred=), close_loop(place=); DESIGN.md "4l. Place recognition").  The table,
the code, the match, the keyframe file and the keyframe-pose rule of the warp against the numpy restatement of tests/place_ref.py,
bit for bit; the prediction drawn elsewhere against tests/search_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loop_auto_ref as lar
import place_ref as pr
import retire_ref as rr
import search_ref as sr
import track_ref as tr
import warp_ref as wr
from backends import assert_models_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfelmapping_amd", "csrc")
f32 = np.float32
IMIN, IMAX = lar.INT32_MIN, lar.INT32_MAX
CAM, OVER = rr.CAM, rr.OVER
BORDER = OVER["stereo_border"]
NEW = ("sm_default_fern_params", "sm_fern_table", "sm_set_ferns", "sm_fern_encode", "sm_fern_encode_device", "sm_fern_add", "sm_fern_count",
       "sm_fern_download", "sm_fern_save", "sm_fern_load", "sm_fern_match", "sm_search_pose_at", "sm_close_loop_at",
       "sm_default_auto_place_params", "sm_set_auto_place", "sm_auto_place_stats")
# (seed, width, height, cell, n_ferns): the default; remainders on both axes; one cell column (gw == 1)
TABLES = ((1, 312, 94, 8, 512), (7, 45, 37, 4, 32), (2 ** 63 + 11, 40, 100, 32, 2048))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _m4(p16):
    return np.asarray(p16, f32).reshape(4, 4).T


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------------------------------
# CPU only
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_place_symbols():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert L.sm_api_version() == 4
    cfg = capi.SmConfig()
    L.sm_default_config(C.byref(cfg), 312, 94, 180.0, 180.0, 155.5, 46.5)
    p = capi.fern_params(cfg)
    assert (p.n_ferns, p.cell, p.seed, p.depth_lo_mm, p.depth_hi_mm) == (512, 8, 1, 1000, 30000)
    assert {k: getattr(p, k) for k in pr.DEFAULT} == pr.DEFAULT
    q = capi.fern_params(cfg, n_ferns=64, seed=2 ** 63 + 5)
    assert (q.n_ferns, q.seed, q.cell) == (64, 2 ** 63 + 5, 8)
    a = capi.auto_place_params(cfg)
    assert (a.every, a.rest, a.add_above, a.match_below, a.min_jump) == (1, 10, f32(0.2), f32(0.3), 2.0)
    lp, sp = capi.loop_params(cfg), capi.search_params()
    assert (a.loop.max_trans, a.loop.max_rot_deg, a.loop.min_age, a.loop.min_trans, a.loop.min_rot_deg) == (50.0, 45.0, lp.min_age, lp.min_trans, lp.min_rot_deg)
    assert bytes(a.search) == bytes(sp)


def test_ctypes_mirrors_have_the_header_layout(tmp_path):
    from surfelmapping_amd import capi
    mirrors = {"sm_fern_params": capi.SmFernParams, "sm_fern": capi.SmFern, "sm_auto_place_params": capi.SmAutoPlaceParams,
               "sm_auto_place_stats_t": capi.SmAutoPlaceStats}
    lines = []
    for cname, cls in mirrors.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("version %d %u\\n", SM_API_VERSION, SM_FERN_MAX_KEYFRAMES);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sm_c_api.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(src)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    assert got["version"] == f"4 {capi.FERN_MAX_KEYFRAMES}"
    for cname, cls in mirrors.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert capi.FERN_DTYPE.itemsize == C.sizeof(capi.SmFern) == pr.FERN_DTYPE.itemsize == 12


def test_arguments_are_rejected_before_any_device_call():
    from surfelmapping_amd import capi
    L = capi.load()
    E = capi.SM_E_ARG
    cfg = capi.SmConfig()
    L.sm_default_config(C.byref(cfg), 312, 94, 180.0, 180.0, 155.5, 46.5)
    p = capi.fern_params(cfg)
    out = np.zeros(2048, capi.FERN_DTYPE)
    img, code, pose = np.zeros(48, np.uint16), np.zeros(64, np.uint32), np.eye(4, dtype=f32).reshape(16)
    assert L.sm_default_fern_params(None, C.byref(p)) == E and L.sm_default_fern_params(C.byref(cfg), None) == E
    assert L.sm_fern_table(None, 312, 94, _vp(out)) == E and L.sm_fern_table(C.byref(p), 312, 94, None) == E
    assert L.sm_fern_table(C.byref(p), 312, 94, _vp(out)) == capi.SM_OK
    for over in (dict(n_ferns=0), dict(n_ferns=16), dict(n_ferns=48), dict(n_ferns=2080), dict(cell=0), dict(cell=12), dict(cell=64),
                 dict(depth_lo_mm=30000), dict(depth_lo_mm=40000), dict(depth_hi_mm=65536), dict(depth_lo_mm=-1)):
        assert L.sm_fern_table(C.byref(capi.fern_params(cfg, **over)), 312, 94, _vp(out)) == E, over
    assert L.sm_fern_table(C.byref(p), 7, 94, _vp(out)) == E and L.sm_fern_table(C.byref(p), 312, 7, _vp(out)) == E
    k, d, n = C.c_int32(), C.c_uint32(), C.c_uint32()
    assert L.sm_set_ferns(None, C.byref(p)) == E
    assert L.sm_fern_encode(None, None, _vp(img), _vp(code)) == E and L.sm_fern_encode_device(None, None, _vp(img), _vp(code)) == E
    assert L.sm_fern_add(None, _vp(code), _vp(pose), 0, None) == E and L.sm_fern_count(None, C.byref(n)) == E
    assert L.sm_fern_download(None, None, None, None) == E
    assert L.sm_fern_save(None, b"x") == E and L.sm_fern_load(None, b"x") == E
    assert L.sm_fern_match(None, _vp(code), IMIN, IMAX, C.byref(k), C.byref(d), None) == E
    o16 = np.zeros(16, f32)
    assert L.sm_search_pose_at(None, None, _vp(img), _vp(pose), _vp(pose), None, None, None, IMIN, IMAX, _vp(o16), None) == E
    src, info = capi.map_source([]), capi.SmLoopInfo()
    assert L.sm_close_loop_at(None, None, _vp(img), _vp(pose), _vp(pose), C.byref(src), None, None, None, None, _vp(o16), C.byref(info)) == E
    ap = capi.auto_place_params(cfg)
    assert L.sm_default_auto_place_params(None, C.byref(ap)) == E and L.sm_default_auto_place_params(C.byref(cfg), None) == E
    assert L.sm_set_auto_place(None, C.byref(ap)) == E and L.sm_set_auto_place(None, None) == E
    assert L.sm_auto_place_stats(None, C.byref(capi.SmAutoPlaceStats())) == E


@pytest.mark.parametrize("seed,w,h,cell,n", TABLES)
def test_table_matches_restatement(seed, w, h, cell, n):
    from surfelmapping_amd import capi
    L = capi.load()
    cfg = capi.SmConfig()
    L.sm_default_config(C.byref(cfg), w, h, 180.0, 180.0, 155.5, 46.5)
    over = dict(n_ferns=n, cell=cell, seed=seed, depth_lo_mm=700, depth_hi_mm=65535)
    got = capi.fern_table(capi.fern_params(cfg, **over), w, h)
    want = pr.table(pr.params(**over), w, h)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert got["x"].max() == w // cell - 1 and got["y"].max() <= h // cell - 1
    assert got["td"].min() >= 700 and got["td"].max() < 65535 and max(got[c].max() for c in ("tr", "tg", "tb")) <= 254
    assert len(np.unique(got)) > n // 2


# the stand-alone program over sm_fernfile.h, plain and with the sanitizers
@pytest.fixture(scope="module")
def fernfile(tmp_path_factory):
    d = tmp_path_factory.mktemp("fernfile")
    flags = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC]
    src = os.path.join(ROOT, "tests", "cpp", "fernfile_check.cpp")
    plain, san = str(d / "fernfile_check"), str(d / "fernfile_check_san")
    subprocess.check_call(flags + ["-o", plain, src])
    subprocess.check_call(flags + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    return plain, san


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return r.stdout.splitlines()


def _database(p, n, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 2 ** 32, (n, p["n_ferns"] // 8), dtype=np.uint64).astype(np.uint32)
    poses = rng.normal(size=(n, 16)).astype(f32)
    times = rng.integers(-50, 5000, n).astype(np.int32)
    return codes, poses, times


def _bad_files(d, p, w, h):
    """name -> (path, parses): one good file, and the ways a keyframe file can be wrong"""
    codes, poses, times = _database(p, 5, 3)
    good = pr.file_bytes(p, w, h, codes, poses, times)
    files = {"good": good, "empty_database": pr.file_bytes(p, w, h, codes[:0], poses[:0], times[:0]), "no_bytes": b"", "half_header": good[:20],
             "header_only": good[:48], "truncated_record": good[:-1], "one_record_short": good[:-(68 + p["n_ferns"] // 2)], "over_long": good + b"\0",
             "count_too_large": pr.file_bytes(p, w, h, codes, poses, times, count=2 ** 31), "count_past_max": pr.file_bytes(p, w, h, codes, poses, times, count=2 ** 20 + 1),
             "bad_magic": b"XXXX" + good[4:], "bad_version": good[:4] + b"\2\0\0\0" + good[8:],
             "bad_n_ferns": pr.file_bytes(dict(p, n_ferns=48), w, h, np.zeros((5, 6), np.uint32), poses, times),
             "bad_cell": good[:12] + b"\5\0\0\0" + good[16:], "negative_n": good[:8] + b"\xe0\xff\xff\xff" + good[12:]}
    out = {}
    for name, b in files.items():
        path = str(d / (name + ".fern"))
        with open(path, "wb") as f:
            f.write(b)
        out[name] = (path, name in ("good", "empty_database"))
    return out, (codes, poses, times)


def test_table_and_file_parser_stand_alone_and_sanitized(fernfile, tmp_path):
    for exe in fernfile:
        for seed, w, h, cell, n in TABLES:
            lines = _run(exe, "table", n, cell, seed, 700, 65535, w, h)
            want = pr.table(pr.params(n_ferns=n, cell=cell, seed=seed, depth_lo_mm=700, depth_hi_mm=65535), w, h)
            assert [tuple(int(v) for v in l.split()) for l in lines] == [tuple(int(v) for v in r) for r in want]
        p = pr.params(n_ferns=64)
        files, (codes, poses, times) = _bad_files(tmp_path, p, 312, 94)
        names = sorted(files)
        lines = _run(exe, "parse", *[files[k][0] for k in names])
        assert len(lines) == len(names)
        for name, line in zip(names, lines):
            assert line.startswith("ok " if files[name][1] else "err "), (name, line)
        assert lines[names.index("good")] == f"ok 5 {int(times.sum())} {int(np.bitwise_xor.reduce(codes.reshape(-1)))}"
        assert _run(exe, "parse", str(tmp_path / "missing.fern"))[0].startswith("err ")
        # the writer gives the reader's bytes back, through a temporary that is gone afterwards
        copy = str(tmp_path / "copy.fern")
        assert _run(exe, "copy", files["good"][0], copy) == ["ok 5"]
        assert open(copy, "rb").read() == open(files["good"][0], "rb").read() and not os.path.exists(copy + ".tmp")


def test_restatement_of_code_and_match():
    """what the bit-for-bit comparisons stand on: the restated code against a plain per-fern loop, the match against a plain scan"""
    rng = np.random.default_rng(5)
    p = pr.params(n_ferns=32, cell=4)
    rgb = rng.integers(0, 256, (37, 45, 3), dtype=np.uint8)
    depth = np.where(rng.random((37, 45)) < 0.3, 0, rng.integers(1, 65536, (37, 45))).astype(np.uint16)
    tab = pr.table(p, 45, 37)
    nib = pr.nibbles(rgb, depth, p)
    for f, t in enumerate(tab):
        blk = (slice(int(t["y"]) * 4, int(t["y"]) * 4 + 4), slice(int(t["x"]) * 4, int(t["x"]) * 4 + 4))
        d = [int(v) for v in depth[blk].reshape(-1) if v]
        D = sum(d) // len(d) if d else 0
        m = [int(rgb[blk][..., c].astype(np.int64).sum()) // 16 for c in range(3)]
        assert nib[f] == (m[0] > t["tr"]) | ((m[1] > t["tg"]) << 1) | ((m[2] > t["tb"]) << 2) | ((D > t["td"]) << 3), f
    code = pr.encode(rgb, depth, p)
    assert code.shape == (4,) and np.array_equal(pr.unpack(code), nib) and (pr.encode(None, depth, p) & np.uint32(0x77777777) == 0).all()
    codes = rng.integers(0, 2 ** 32, (9, 4), dtype=np.uint64).astype(np.uint32)
    codes[6] = codes[2] = code
    times = np.arange(9, dtype=np.int32) * 10
    k, d, every = pr.match(code, codes, times, IMIN, IMAX)
    assert (k, d) == (2, 0) and every[6] == 0 and every[0] == sum(int(a) != int(b) for a, b in zip(pr.unpack(codes[0]), nib))
    assert pr.match(code, codes, times, 20, IMAX)[:2] == (6, 0) and pr.match(code, codes, times, 80, IMAX)[:2] == (-1, 0xFFFFFFFF)
    assert pr.match(code, codes, times, 19, 20)[:2] == (2, 0)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the code
# ---------------------------------------------------------------------------------------------------------------------
def _gpu(w=CAM["width"], h=CAM["height"], **over):
    from surfelmapping_amd import capi
    cam = CAM if (w, h) == (CAM["width"], CAM["height"]) else dict(width=w, height=h, fx=90.0, fy=90.0, cx=w / 2 - 0.5, cy=h / 2 - 0.5)
    return capi.SurfelMap(capi.make_config(**cam, **OVER, preprocess=0, **dict(dict(max_sqrt_vertices=440), **over)))


def _images(w, h, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    depth = np.where(rng.random((h, w)) < 0.3, 0, rng.integers(1, 65536, (h, w))).astype(np.uint16)
    return rgb, depth


# the issue's four shapes, and two whose rows are aligned to 2 bytes and to 1: the lanes' narrower loads at cell 16 and 32
ENCODE = ((312, 94, 8, 512), (45, 37, 4, 32), (64, 64, 32, 2048), (40, 24, 16, 512), (50, 33, 16, 64), (67, 35, 32, 96))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,cell,n", ENCODE)
def test_encode_matches_restatement(w, h, cell, n):
    over = dict(n_ferns=n, cell=cell, seed=w * 1000 + cell)
    p = pr.params(**over)
    m = _gpu(w, h, max_sqrt_vertices=64)
    m.set_ferns(**over)
    rgb, depth = _images(w, h, n + w)
    tab = pr.table(p, w, h)
    # a cell with every depth zero, and one with a single sample left
    other = [f for f in range(n) if (tab["x"][f], tab["y"][f]) != (tab["x"][0], tab["y"][0])]
    for f in [0] + other[:1]:
        y, x = int(tab["y"][f]) * cell, int(tab["x"][f]) * cell
        depth[y:y + cell, x:x + cell] = 0
        if f:
            depth[y + cell - 1, x + cell - 1] = 40000
    got = m.fern_encode(depth, rgb)
    want = pr.encode(rgb, depth, p, tab)
    assert got.dtype == np.uint32 and got.shape == want.shape == (n // 8,)
    assert np.array_equal(got, want), np.nonzero(got != want)[0]
    assert (pr.unpack(got)[0] & 8) == 0
    # without colour
    plain = m.fern_encode(depth)
    assert np.array_equal(plain, pr.encode(None, depth, p, tab)) and (plain & np.uint32(0x77777777) == 0).all() and plain.any()
    # images resident on the device: the same code
    d_rgb, d_depth = m.device_alloc(rgb.nbytes), m.device_alloc(depth.nbytes)
    m.device_upload(d_rgb, rgb)
    m.device_upload(d_depth, depth)
    assert np.array_equal(m.fern_encode_device(d_depth, d_rgb), want) and np.array_equal(m.fern_encode_device(d_depth), plain)
    m.device_free(d_rgb)
    m.device_free(d_depth)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,cell,n", [(312, 94, 8, 512), (45, 37, 4, 32), (64, 64, 32, 2048), (40, 24, 16, 512)])
def test_encode_at_the_thresholds(w, h, cell, n):
    """a cell painted constant at exactly t gives bit 0, at t + 1 bit 1, in each channel and in depth"""
    over = dict(n_ferns=n, cell=cell, seed=3)
    p = pr.params(**over)
    m = _gpu(w, h, max_sqrt_vertices=64)
    m.set_ferns(**over)
    tab = pr.table(p, w, h)
    # three ferns whose cells no other of the three shares
    picked, cells = [], set()
    for f in list(range(n))[::-1]:
        if (tab["x"][f], tab["y"][f]) not in cells and len(picked) < 3:
            picked.append(f)
            cells.add((tab["x"][f], tab["y"][f]))
    assert len(picked) == 3 or (w // cell) * (h // cell) < 3
    for plus in (0, 1):
        rgb, depth = _images(w, h, 9)
        for f in picked:
            y, x = int(tab["y"][f]) * cell, int(tab["x"][f]) * cell
            rgb[y:y + cell, x:x + cell] = (int(tab["tr"][f]) + plus, int(tab["tg"][f]) + plus, int(tab["tb"][f]) + plus)
            depth[y:y + cell, x:x + cell] = int(tab["td"][f]) + plus
        got = m.fern_encode(depth, rgb)
        assert np.array_equal(got, pr.encode(rgb, depth, p, tab))
        assert all(pr.unpack(got)[f] == (15 if plus else 0) for f in picked), (plus, [pr.unpack(got)[f] for f in picked])


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the database and the match
# ---------------------------------------------------------------------------------------------------------------------
def _loaded(tmp_path, p, n, seed, w=64, h=32):
    """a context whose database came from a file the restatement wrote, and that database"""
    codes, poses, times = _database(p, n, seed)
    path = str(tmp_path / f"db_{n}_{p['n_ferns']}.fern")
    with open(path, "wb") as f:
        f.write(pr.file_bytes(p, w, h, codes, poses, times))
    m = _gpu(w, h, max_sqrt_vertices=64)
    m.set_ferns(**p)
    m.fern_load(path)
    return m, codes, poses, times


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf,n", [(1, 512), (63, 512), (64, 512), (65, 512), (1000, 512), (70001, 512), (257, 32), (257, 2048), (300, 96)])
def test_match_matches_restatement(tmp_path, n_kf, n):
    p = pr.params(n_ferns=n, depth_lo_mm=500, depth_hi_mm=20000)
    m, codes, poses, times = _loaded(tmp_path, p, n_kf, n_kf + n)
    assert m.fern_count() == n_kf
    rng = np.random.default_rng(n_kf)
    # a query near keyframe n_kf // 2: a tenth of its ferns changed
    query = pr.unpack(codes[n_kf // 2]).copy()
    flip = rng.choice(n, n // 10, replace=False)
    query[flip] ^= rng.integers(1, 16, len(flip)).astype(np.uint32)
    query = pr.pack(query)
    k, d, every = m.fern_match(query, dis_all=True)
    wk, wd, wevery = pr.match(query, codes, times, IMIN, IMAX)
    assert np.array_equal(every, wevery), np.nonzero(every != wevery)[0][:8]
    assert (k, d) == (wk, wd) == (n_kf // 2, n // 10)
    assert m.fern_match(query) == (wk, wd)
    # windows: one that excludes the global best, a one-sided one, an empty one
    t_best = int(times[wk])
    for lo, hi in ((t_best, IMAX), (IMIN, t_best - 1), (IMIN, t_best), (t_best - 1, t_best), (4999, IMAX), (100, 100), (IMAX, IMAX)):
        got, want = m.fern_match(query, lo, hi), pr.match(query, codes, times, lo, hi)[:2]
        assert got == want, (lo, hi, got, want)
    assert m.fern_match(query, 4999, IMAX) == (-1, 0xFFFFFFFF)
    kf = m.fern_keyframes()
    assert np.array_equal(kf["codes"], codes) and np.array_equal(_bits(kf["poses"]), _bits(poses)) and np.array_equal(kf["times"], times)


@pytest.mark.gpu
def test_match_ties_and_growth(tmp_path):
    """planted duplicates of the query: the lower index wins; adding after a match grows the database across a capacity doubling
    and the codes survive it"""
    p = pr.params()
    m, codes, poses, times = _loaded(tmp_path, p, 1000, 77)
    query = codes[900].copy()
    codes, poses, times = list(codes), list(poses), list(times)
    for k in (1000, 1001):                                  # two more copies of keyframe 900, by hand
        assert m.fern_add(query, poses[900], 6000 + k) == k
        codes.append(query), poses.append(poses[900]), times.append(6000 + k)
    assert m.fern_match(query) == (900, 0) and m.fern_match(query, 5999, IMAX) == (1000, 0) and m.fern_match(query, 7000, IMAX) == (1001, 0)
    rng = np.random.default_rng(1)
    for k in range(1002, 1100):                             # past the first capacity (1024)
        c = rng.integers(0, 2 ** 32, 64, dtype=np.uint64).astype(np.uint32)
        pose = rng.normal(size=16).astype(f32)
        assert m.fern_add(c, pose, k) == k
        codes.append(c), poses.append(pose), times.append(k)
    assert m.fern_count() == 1100
    kf = m.fern_keyframes()
    assert np.array_equal(kf["codes"], np.stack(codes)) and np.array_equal(_bits(kf["poses"]), _bits(np.stack(poses)))
    assert np.array_equal(kf["times"], np.array(times, np.int32))
    probe = codes[1090]
    k, d, every = m.fern_match(probe, dis_all=True)
    assert (k, d) == (1090, 0) and np.array_equal(every, pr.dis_all(probe, np.stack(codes)))
    # reset empties the database and keeps the table; NULL frees both
    m.reset()
    assert m.fern_count() == 0 and m.fern_match(probe) == (-1, 0xFFFFFFFF)
    assert m.fern_add(probe, poses[0], 3) == 0 and m.fern_match(probe) == (0, 0)
    m.set_ferns(False)
    with pytest.raises(Exception):
        m.fern_count()


@pytest.mark.gpu
def test_save_and_load(tmp_path):
    from surfelmapping_amd import capi
    p = pr.params(n_ferns=96, cell=16)
    m, codes, poses, times = _loaded(tmp_path, p, 37, 5)
    path = str(tmp_path / "saved.fern")
    m.fern_save(path)
    assert open(path, "rb").read() == pr.file_bytes(p, 64, 32, codes, poses, times) and not os.path.exists(path + ".tmp")
    other = _gpu(64, 32, max_sqrt_vertices=64)
    other.set_ferns(**p)
    other.fern_add(codes[0], poses[0], 1)                    # replaced by the load
    other.fern_load(path)
    kf = other.fern_keyframes()
    assert np.array_equal(kf["codes"], codes) and np.array_equal(_bits(kf["poses"]), _bits(poses)) and np.array_equal(kf["times"], times)
    q = codes[20].copy()
    q[1] ^= np.uint32(0x10)                                   # one fern of keyframe 20 changed
    assert other.fern_match(q, dis_all=True)[:2] == m.fern_match(q, dis_all=True)[:2] == (20, 1)
    # files that must not load: each leaves the database as it was
    files, _ = _bad_files(tmp_path, p, 64, 32)
    files["other_seed"] = (str(tmp_path / "other_seed.fern"), False)
    files["other_size"] = (str(tmp_path / "other_size.fern"), False)
    open(files["other_seed"][0], "wb").write(pr.file_bytes(dict(p, seed=2), 64, 32, codes, poses, times))
    open(files["other_size"][0], "wb").write(pr.file_bytes(p, 64, 48, codes, poses, times))
    files["missing"] = (str(tmp_path / "missing.fern"), False)
    for name, (fp, ok) in sorted(files.items()):
        rc = other._L.sm_fern_load(other._h, os.fsencode(fp))
        if ok:
            assert rc == capi.SM_OK, name
            other.fern_load(path)
        else:
            assert rc == capi.SM_E_ARG and os.path.basename(fp).encode() in other._L.sm_last_error(), (name, rc)
            assert other.fern_count() == 37 and np.array_equal(other.fern_keyframes()["codes"], codes), name
    assert other._L.sm_fern_save(other._h, os.fsencode(str(tmp_path / "no_such_dir" / "x.fern"))) == capi.SM_E_ARG


@pytest.mark.gpu
def test_rejected_arguments_and_contexts():
    from surfelmapping_amd import capi
    L = capi.load()
    E, U = capi.SM_E_ARG, capi.SM_E_UNSUPPORTED
    m = _gpu(64, 32, max_sqrt_vertices=64)
    p = capi.fern_params(m.cfg)
    code, pose, img = np.zeros(64, np.uint32), np.eye(4, dtype=f32).reshape(16), np.zeros((32, 64), np.uint16)
    k, d, n = C.c_int32(), C.c_uint32(), C.c_uint32()
    # no ferns yet
    assert L.sm_fern_encode(m._h, None, _vp(img), _vp(code)) == E and L.sm_fern_count(m._h, C.byref(n)) == E
    assert L.sm_fern_match(m._h, _vp(code), IMIN, IMAX, C.byref(k), C.byref(d), None) == E
    assert L.sm_set_ferns(m._h, C.byref(capi.fern_params(m.cfg, cell=12))) == E and L.sm_set_ferns(m._h, C.byref(capi.fern_params(m.cfg, n_ferns=40))) == E
    big = capi.fern_params(m.cfg, cell=32)
    tiny = _gpu(40, 24, max_sqrt_vertices=64)
    assert L.sm_set_ferns(tiny._h, C.byref(big)) == E                 # gh == 0
    assert L.sm_set_ferns(m._h, C.byref(p)) == capi.SM_OK
    assert L.sm_fern_encode(m._h, None, None, _vp(code)) == E and L.sm_fern_encode(m._h, None, _vp(img), None) == E
    assert L.sm_fern_add(m._h, None, _vp(pose), 0, None) == E and L.sm_fern_add(m._h, _vp(code), None, 0, None) == E
    bad = pose.copy()
    bad[13] = np.nan
    assert L.sm_fern_add(m._h, _vp(code), _vp(bad), 0, None) == E and L.sm_fern_count(m._h, None) == E
    assert L.sm_fern_match(m._h, None, IMIN, IMAX, C.byref(k), C.byref(d), None) == E
    assert L.sm_fern_match(m._h, _vp(code), IMIN, IMAX, None, C.byref(d), None) == E
    assert L.sm_fern_save(m._h, None) == E and L.sm_fern_load(m._h, None) == E
    assert L.sm_fern_match(m._h, _vp(code), IMIN, IMAX, C.byref(k), C.byref(d), None) == capi.SM_OK and (k.value, d.value) == (-1, 0xFFFFFFFF)
    # the policy's rules
    stats = capi.SmAutoPlaceStats()
    nf = _gpu(64, 32, max_sqrt_vertices=64)
    assert L.sm_set_auto_place(nf._h, C.byref(capi.auto_place_params(nf.cfg))) == E                 # no ferns
    assert L.sm_set_auto_place(nf._h, None) == capi.SM_OK and L.sm_auto_place_stats(nf._h, None) == E
    nan = float("nan")
    for over in (dict(every=0), dict(every=-3), dict(rest=-1), dict(add_above=-0.1), dict(add_above=1.5), dict(add_above=nan), dict(match_below=-0.1),
                 dict(match_below=1.01), dict(match_below=nan), dict(min_jump=-1.0), dict(min_jump=nan), dict(min_jump=float("inf")), dict(min_age=0),
                 dict(max_trans=-1.0), dict(max_rot_deg=nan), dict(search=dict(levels=0)), dict(search=dict(top_k=17)),
                 dict(search=dict(colour_thresh=-1.0))):
        assert L.sm_set_auto_place(m._h, C.byref(capi.auto_place_params(m.cfg, **over))) == E, over
    assert L.sm_auto_place_stats(m._h, C.byref(stats)) == capi.SM_OK and stats.encoded == 0
    for over in (dict(), dict(every=7, rest=0, add_above=0.0, match_below=1.0, min_jump=0.0)):
        assert L.sm_set_auto_place(m._h, C.byref(capi.auto_place_params(m.cfg, **over))) == capi.SM_OK, over
    assert L.sm_auto_place_stats(m._h, C.byref(stats)) == capi.SM_OK and (stats.last_k, stats.last_dis) == (-1, 0xFFFFFFFF)
    # setting the ferns again switches the policy off: a tracked frame encodes nothing
    assert L.sm_set_ferns(m._h, C.byref(p)) == capi.SM_OK
    # between the conflict test and the cull: every entry point that takes a context
    g = _gpu()
    seq = rr.sequence(2)
    g.process_frame(*seq[0])
    g.set_ferns()
    gp = capi.fern_params(g.cfg)
    gimg, o16 = np.ascontiguousarray(seq[1][1]), np.zeros(16, f32)
    gpose = np.asarray(seq[1][3], f32)
    src, info = capi.map_source([]), capi.SmLoopInfo()
    calls = {
        "sm_set_ferns": lambda h: L.sm_set_ferns(h, C.byref(gp)),
        "sm_fern_encode": lambda h: L.sm_fern_encode(h, None, _vp(gimg), _vp(code)),
        "sm_fern_encode_device": lambda h: L.sm_fern_encode_device(h, None, _vp(gimg), _vp(code)),
        "sm_fern_add": lambda h: L.sm_fern_add(h, _vp(code), _vp(gpose), 0, None),
        "sm_fern_count": lambda h: L.sm_fern_count(h, C.byref(n)),
        "sm_fern_download": lambda h: L.sm_fern_download(h, None, None, None),
        "sm_fern_save": lambda h: L.sm_fern_save(h, b"/nonexistent/x.fern"),
        "sm_fern_load": lambda h: L.sm_fern_load(h, b"/nonexistent/x.fern"),
        "sm_fern_match": lambda h: L.sm_fern_match(h, _vp(code), IMIN, IMAX, C.byref(k), C.byref(d), None),
        "sm_search_pose_at": lambda h: L.sm_search_pose_at(h, None, _vp(gimg), _vp(gpose), _vp(gpose), None, None, None, IMIN, IMAX, _vp(o16), None),
        "sm_close_loop_at": lambda h: L.sm_close_loop_at(h, None, _vp(gimg), _vp(gpose), _vp(gpose), C.byref(src), None, None, None, None, _vp(o16), C.byref(info)),
    }
    g.stage_conflict(seq[1][3], 1.0, 30.0)
    for name, call in calls.items():
        assert call(g._h) == E and b"between sm_stage_conflict and sm_stage_cull" in L.sm_last_error(), name
    g.stage_cull()
    assert calls["sm_fern_count"](g._h) == capi.SM_OK and calls["sm_fern_match"](g._h) == capi.SM_OK
    # a sharded context and a rig context hold only their own surfels: every entry point, whatever else it is given
    bad_pose = gpose.copy()
    bad_pose[12] = np.nan
    for kind in ("sharded", "rig"):
        s = _gpu()
        s.shard_stream_configure(0, 2) if kind == "sharded" else s.rig_configure(0, 2)
        for name, call in calls.items():
            assert call(s._h) == U, (kind, name)
        assert L.sm_set_auto_place(s._h, C.byref(capi.auto_place_params(s.cfg))) == U and L.sm_set_auto_place(s._h, None) == U, kind
        assert L.sm_auto_place_stats(s._h, C.byref(stats)) == U, kind
        assert L.sm_search_pose_at(s._h, None, _vp(gimg), _vp(bad_pose), _vp(gpose), None, None, None, IMIN, IMAX, _vp(o16), None) == U, kind
        assert L.sm_close_loop_at(s._h, None, _vp(gimg), _vp(gpose), _vp(bad_pose), C.byref(src), None, None, None, None, _vp(o16), C.byref(info)) == U, kind


# ---------------------------------------------------------------------------------------------------------------------
# GPU: keyframe poses move with the map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_keyframe_poses_move_with_the_map():
    seq = rr.sequence(4)
    m = _gpu()
    for fr in seq:
        m.process_frame(*fr)
    p = pr.params(n_ferns=32)
    m.set_ferns(**p)
    rng = np.random.default_rng(2)
    times = np.array([-3, 0, 1, 2, 3, 4, 5, 9, 2 ** 24 + 1, IMAX], np.int32)
    poses = np.stack([tr.colmajor(sr.offset_pose(np.eye(4), *rng.uniform(-2, 2, 3))) for _ in times])
    for P, t in zip(poses, times):
        m.fern_add(np.zeros(4, np.uint32), P, int(t))
    corr = wr.rigid_table(4, seed=3)
    model = m.download_model()
    m.warp_by_time([], 2, corr)
    got = m.fern_keyframes()
    want = pr.warp_poses(poses, times, 2, corr)
    assert np.array_equal(_bits(got["poses"]), _bits(want)) and np.array_equal(got["times"], times)
    old = times < 2
    assert old.sum() == 3 and np.array_equal(_bits(got["poses"][old]), _bits(poses[old])) and (_bits(got["poses"][~old]) != _bits(poses[~old])).any(axis=1).all()
    assert_models_equal(m.download_model(), wr.warp_rows(model, 2, corr), "the model moved as without ferns")


# ---------------------------------------------------------------------------------------------------------------------
# GPU: a prediction somewhere else
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """test_search.py's: frames 0..11 of the street; the model of frames 0..9 on the CPU oracle"""
    import oracle_lib as ol
    seq = rr.sequence(12)
    cpu = ol.Oracle(ol.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=440))
    for fr in seq[:10]:
        cpu.process_frame(*fr)
    return dict(seq=seq, model=cpu.download_model(), truth=_m4(seq[10][3]), t_prev=np.asarray(seq[9][3], f32))


def _holding(scene, frame=9):
    m = _gpu()
    m.process_frame(*scene["seq"][frame])
    m.upload_model(scene["model"])
    m.set_tick(10)
    return m


@pytest.mark.gpu
def test_prediction_at_t_prev_is_the_plain_search(scene):
    seq, truth = scene["seq"], scene["truth"]
    rgb, depth = seq[10][0], seq[10][1]
    m = _holding(scene)
    centre = sr.offset_pose(truth, 0.9, -0.7, 2.0)
    for kw in (dict(rgb=rgb), dict(), dict(rgb=rgb, max_time=5)):
        a_pose, a = m.search_pose(depth, centre, **kw)
        b_pose, b = m.search_pose(depth, centre, pred=scene["t_prev"], **kw)
        assert (a["status"] == "OK" or "max_time" in kw) and np.array_equal(_bits(a_pose), _bits(b_pose)), (a["status"], sorted(kw))
        for key in a:
            if key in ("score_ms", "total_ms"):
                continue
            if key == "track":
                assert all(np.array_equal(a[key][k], b[key][k]) for k in a[key]), (kw, a[key], b[key])
            else:
                assert np.array_equal(a[key], b[key]), (kw, key)
    # the trackers' guess and history are untouched: the next constant-velocity track is what it was
    fresh = _holding(scene)
    assert np.array_equal(_bits(m.track(depth)[0]), _bits(fresh.track(depth)[0]))


@pytest.mark.gpu
def test_prediction_elsewhere_matches_restatement(scene):
    """the context's last frame is frame 1, 6.4 m behind frame 9, whose pose the prediction is drawn at: the candidate counts, the
    level scores and the ranking are the restatement's with t_prev16 = pred"""
    seq, truth, model = scene["seq"], scene["truth"], scene["model"]
    rgb, depth = seq[10][0], seq[10][1]
    m = _holding(scene, frame=1)
    pred = scene["t_prev"]
    far = tr.pose_error(_m4(pred), _m4(seq[1][3]))[0]
    assert far > 6.0
    centre = sr.offset_pose(truth, -1.6, 1.3, -2.5)
    pose, info = m.search_pose(depth, centre, rgb=rgb, pred=pred)
    ref = sr.search(rgb, depth, model, pred, tr.colmajor(centre), CAM, stereo_border=BORDER)
    et, er = tr.pose_error(pose, truth)
    print(f"prediction {far:.2f} m from T_prev: {info['status']}, best scores {info['best_score']}, {et * 100:.2f} cm and {er:.3f} deg from the truth")
    assert info["status"] == "OK" and ref["status"] == "OK" and et < 0.05 and er < 0.2
    assert info["candidates"] == [len(l["cands"]) for l in ref["levels"]] == [3757, 2916]
    assert info["best_score"] == [int(l["scores"].max()) for l in ref["levels"]]
    kept = ref["levels"][-1]["poses"]
    assert np.array_equal(_bits(tr.colmajor(info["start"])), _bits(kept[info["winner_rank"]]))
    # from T_prev itself (frame 1's pose) the same centre sees another prediction and scores otherwise
    plain = m.search_pose(depth, centre, rgb=rgb)[1]
    ref2 = sr.search(rgb, depth, model, np.asarray(seq[1][3], f32), tr.colmajor(centre), CAM, stereo_border=BORDER)
    assert plain["best_score"] == [int(l["scores"].max()) for l in ref2["levels"][:plain["levels_run"]]] and plain["best_score"] != info["best_score"]
    assert_models_equal(m.download_model(), model, "searching changes nothing")


# ---------------------------------------------------------------------------------------------------------------------
# the drive: out, away, back with 18 m and 5 degrees of drift
# ---------------------------------------------------------------------------------------------------------------------
LOOP = dict(max_trans=50.0, max_rot_deg=45.0)                # the bounds the policy judges a correction against
# The search at the place: scored from stride 4 on, as in tests/test_search.py's guard, and with a colour gate of 0.03 -- the drive's
# texture is exact (a function of the world point), and between flat ground and flat walls only the gate tells two places 0.1 m
# apart along the street: the default 0.1 is 0.3 m of this texture.
SEARCH = dict(colour_thresh=0.03, stride0=4)


def _col(m44):
    return tr.colmajor(np.asarray(m44, np.float64).astype(f32))


@pytest.fixture(scope="module")
def drive():
    """the frames, every frame's restated code, and the tick of the first revisit frame"""
    frames = pr.drive()
    p = pr.params()
    tab = pr.table(p, CAM["width"], CAM["height"])
    codes = np.stack([pr.encode(f["rgb"], f["depth"], p, tab) for f in frames])
    first = [k for k, f in enumerate(frames) if f["leg"] == "revisit"][0]
    return dict(frames=frames, codes=codes, first=first, split=first - 1 - OVER["time_delta"])


@pytest.fixture(scope="module")
def drive_oracle(drive):
    """the CPU oracle's model of the drive up to the first revisit frame, every frame fused at its believed pose"""
    import oracle_lib as ol
    cpu = ol.Oracle(ol.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=pr.CAPACITY))
    for f in drive["frames"][:drive["first"]]:
        cpu.process_frame(f["rgb"], f["depth"], f["sem"], _col(f["believed"]))
    assert cpu.counts()["tick"] == drive["first"]
    return cpu.download_model()


def test_drive_is_what_the_issue_asks(drive):
    frames, first = drive["frames"], drive["first"]
    legs = [f["leg"] for f in frames]
    assert legs.count("out") == 30 and legs[:30] == ["out"] * 30 and legs.count("revisit") == 5 and first == 88
    for f in frames[:50]:
        assert np.array_equal(f["true"], f["believed"])
    drift = tr.pose_error(frames[first]["believed"].astype(f32), frames[first]["true"].astype(f32))
    step = max(tr.pose_error((np.linalg.inv(a["true"]) @ a["believed"]).astype(f32), (np.linalg.inv(b["true"]) @ b["believed"]).astype(f32))[0]
               for a, b in zip(frames[49:first], frames[50:first + 1]))
    print(f"drift at the first revisit frame {drift[0]:.2f} m and {drift[1]:.2f} deg, at most {step:.2f} m of it per frame")
    # (a twentieth of the drift per frame: 0.92 m of shift and 0.25 degrees about a vertical up to 56 m away, 0.25 m more)
    assert drift[0] >= 6.0 and drift[1] >= 4.0 and step < 1.25
    for f, k, in zip(frames[first:], pr.REVISIT_OF):
        et, er = tr.pose_error(f["true"].astype(f32), frames[k]["true"].astype(f32))
        assert et <= 0.4 + 1e-6 and er <= 1.5 + 1e-4, (k, et, er)


def test_guard_ferns_recognise_the_revisit(drive):
    """on the restatement: every revisit frame's best old keyframe is within one keyframe of the nearest true one, at most
    match_below * n ferns away, and every keyframe farther than 2.4 m along the road is at least 32 ferns worse; on the way back
    nothing matches"""
    frames, codes, first = drive["frames"], drive["codes"], drive["first"]
    z = np.array([f["true"][2, 3] for f in frames])
    for r, want in enumerate(pr.REVISIT_OF):
        T = first + r
        split = T - 1 - OVER["time_delta"]
        k, d, every = pr.match(codes[T], codes[:T], np.arange(T), IMIN, split)
        far = [i for i in range(split + 1) if abs(z[i] - z[T]) > 2.4]
        print(f"revisit frame {r}: keyframe {k} (the nearest true one {want}) at {d} ferns; the best farther than 2.4 m at {int(every[far].min())}")
        assert abs(k - want) <= 1 and d <= 0.3 * 512 and int(every[far].min()) - d >= 32, (r, k, d)
    for T in range(first):
        split = T - 1 - OVER["time_delta"]
        if split >= 0:
            assert pr.match(codes[T], codes[:T], np.arange(T), IMIN, split)[1] > 0.3 * 512, T


def test_guard_search_finds_the_place_not_the_believed_pose(drive, drive_oracle):
    """on the oracle's model: the search at the matched keyframe's pose with the prediction drawn there ends -- its best candidate --
    within 0.1 m and 0.3 degrees of the truth, for a revisit frame of either offset; the same search centred at the believed pose
    with the prediction at T_prev does not: it finds nothing to start from.  (Extra: the restated colour tracker, started from the
    best candidate as sm_search_pose starts it, ends within a few centimetres.)"""
    import track_rgb_ref as trr
    frames, codes, first = drive["frames"], drive["codes"], drive["first"]
    sp = dict(sr.DEFAULT, **SEARCH)
    for r in (0, 1):
        T = first + r
        split = T - 1 - OVER["time_delta"]
        f = frames[T]
        truth = f["true"].astype(f32)
        k = pr.match(codes[T], codes[:T], np.arange(T), IMIN, split)[0]
        place = _col(frames[k]["believed"])
        res = sr.search(f["rgb"], f["depth"], drive_oracle, place, place, CAM, sp=sp, max_time=split, stereo_border=BORDER)
        assert res["status"] == "OK"
        start = _m4(res["levels"][-1]["poses"][0])
        et, er = tr.pose_error(start, truth)
        print(f"revisit frame {r} at keyframe {k}: best scores {[int(l['scores'].max()) for l in res['levels']]}, the best candidate {et * 100:.1f} cm "
              f"and {er:.3f} deg from the truth")
        assert et < 0.1 and er < 0.3, (r, et, er)
        if r == 0:
            old = drive_oracle[drive_oracle[:, 7] <= f32(split)]
            pose, info = trr.track(f["rgb"], f["depth"], old, place, start, CAM, stereo_border=BORDER)
            et, er = tr.pose_error(pose.astype(f32), truth)
            print(f"  tracked from it: {info['status']}, {et * 100:.2f} cm and {er:.3f} deg from the truth")
            assert info["status"] == "OK" and et < 0.1 and er < 0.3, (et, er)
    f, split = frames[first], drive["split"]
    believed, t_prev = _col(f["believed"]), _col(frames[first - 1]["believed"])
    res = sr.search(f["rgb"], f["depth"], drive_oracle, t_prev, believed, CAM, sp=sp, max_time=split, stereo_border=BORDER)
    print(f"at the believed pose: {res['status']}, best scores {[int(l['scores'].max()) for l in res['levels']]}")
    if res["status"] == "OK":
        for p in res["levels"][-1]["poses"]:
            et, er = tr.pose_error(_m4(p), f["true"].astype(f32))
            assert et > 0.1 or er > 0.3, (et, er)


def _big():
    return _gpu(max_sqrt_vertices=pr.CAPACITY)


@pytest.mark.gpu
def test_loop_by_hand_from_the_recognised_place(drive):
    frames, codes, first, split = drive["frames"], drive["codes"], drive["first"], drive["split"]
    m = _big()
    m.set_ferns()
    for T, f in enumerate(frames[:first]):
        b = _col(f["believed"])
        m.process_frame(f["rgb"], f["depth"], f["sem"], b)
        code = m.fern_encode(f["depth"], f["rgb"])
        assert np.array_equal(code, codes[T]), T
        assert m.fern_add(code, b, T) == T
    assert m.counts()["tick"] == first
    f = frames[first]
    truth, believed = f["true"].astype(f32), _col(f["believed"])
    before = m.download_model()
    # from the believed pose, with the pose search and bounds wide enough for this drift: no loop -- what the feature is for
    pose, info = m.close_loop_rgb(f["rgb"], f["depth"], believed, search=SEARCH, **LOOP)
    print(f"from the believed pose: {info['status']} (track {info['track']['status']})")
    assert info["status"] != "CLOSED" and np.array_equal(_bits(tr.colmajor(pose)), _bits(believed))
    assert_models_equal(m.download_model(), before, "nothing was closed")
    # the ferns name the place
    code = m.fern_encode(f["depth"], f["rgb"])
    k, d = m.fern_match(code, IMIN, split)
    assert (k, d) == pr.match(codes[first], codes[:first], np.arange(first), IMIN, split)[:2] and abs(k - pr.REVISIT_OF[0]) <= 1
    place = m.fern_keyframes()["poses"][k]
    assert np.array_equal(_bits(place), _bits(_col(frames[k]["believed"])))
    # ... and from there the loop closes
    pose, info = m.close_loop_rgb(f["rgb"], f["depth"], believed, place=place, search=SEARCH, **LOOP)
    et, er = tr.pose_error(pose, truth)
    print(f"from keyframe {k} at {d} ferns: {info['status']}, t_a {info['t_a']}, t_b {info['t_b']}, the corrected pose {et * 100:.2f} cm and "
          f"{er:.3f} deg from the truth")
    assert info["status"] == "CLOSED" and info["track"]["status"] == "OK" and info["t_b"] == first - 1, info
    assert et < 0.1 and er < 0.3, (et, er)
    after = m.download_model()
    old = before[:, 7] <= f32(info["t_a"])
    assert len(after) == len(before) and old.sum() > 30000 and np.array_equal(_bits(after[old]), _bits(before[old]))
    table = wr.loop_spread(info["D"].T.reshape(16), info["t_a"], info["t_b"])
    assert_models_equal(after, wr.warp_rows(before, info["t_a"] + 1, table[1:]), "the model after the loop")
    # the keyframes moved with the map
    kf = m.fern_keyframes()
    want = pr.warp_poses(np.stack([_col(g["believed"]) for g in frames[:first]]), np.arange(first), info["t_a"] + 1, table[1:])
    assert np.array_equal(_bits(kf["poses"]), _bits(want))


def _policy_run(drive, place, ferns):
    """the drive through the trackers: every frame tracked from its believed pose (so that the policy sees it) and fused at it, the
    revisit frames fused where the tracker call says.  Returns (context, poses returned, statuses)."""
    frames, first = drive["frames"], drive["first"]
    m = _big()
    if ferns:
        m.set_ferns()
    if place:
        m.set_auto_place(**place)
    poses, status = [], []
    for T, f in enumerate(frames):
        pose, info = m.track_rgb(f["rgb"], f["depth"], guess=_col(f["believed"]))
        poses.append(pose)
        status.append(info["status"])
        m.process_frame(f["rgb"], f["depth"], f["sem"], _col(f["believed"]) if T < first else tr.colmajor(pose))
    return m, poses, status


@pytest.mark.gpu
def test_policy_closes_the_loop_once(drive):
    frames, codes, first, split = drive["frames"], drive["codes"], drive["first"], drive["split"]
    m, poses, status = _policy_run(drive, dict(search=SEARCH), True)
    st = m.auto_place_stats()
    et, er = tr.pose_error(poses[first], frames[first]["true"].astype(f32))
    print(f"policy: {st['attempts']} attempts, {st['closed']} closed, {st['added']} keyframes of {st['encoded']} frames, {st['matched']} matched; "
          f"frame {first}: {status[first]}, returned {et * 100:.2f} cm and {er:.3f} deg from the truth; last {st['last']['status']}")
    assert status[first] == "OK"
    assert (st["attempts"], st["closed"], st["none"], st["rejected"], st["failed"], st["no_old_map"]) == (1, 1, 0, 0, 0, 0), st
    assert st["last"]["status"] == "CLOSED" and st["last"]["t_b"] == first - 1 and et < 0.1 and er < 0.3
    # the keyframes up to the closure are the restatement's
    ok = [s == "OK" for s in status]
    kept = pr.keyframe_policy(codes[:first], ok[:first])
    kf = m.fern_keyframes()
    assert list(kf["times"][:len(kept)]) == kept and np.array_equal(kf["codes"][:len(kept)], codes[kept])
    late = pr.keyframe_policy(codes, ok)
    assert st["added"] == len(late) == len(kf["times"]) and list(kf["times"]) == late
    assert st["encoded"] == sum(ok)
    # the policy off -- never set, or the ferns set and the policy set and switched off again -- is today's run, bit for bit
    a, poses_a, status_a = _policy_run(drive, None, False)
    b = _big()
    b.set_ferns()
    b.set_auto_place(search=SEARCH)
    b.set_auto_place(False)
    poses_b = []
    for T, f in enumerate(frames):
        pose, info = b.track_rgb(f["rgb"], f["depth"], guess=_col(f["believed"]))
        poses_b.append(pose)
        b.process_frame(f["rgb"], f["depth"], f["sem"], _col(f["believed"]) if T < first else tr.colmajor(pose))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(poses_a, poses_b))
    assert_models_equal(a.download_model(), b.download_model(), "policy off")
    assert b.fern_count() == 0 and b.auto_place_stats()["encoded"] == 0
    # ... and with it on, every frame before the closure returned what it returns without it
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(poses[:first], poses_a[:first]))
    assert status[:first] == status_a[:first]


@pytest.mark.gpu
@pytest.mark.parametrize("every,rest,want", [(1, 0, [88, 89, 90, 91, 92]), (1, 2, [88, 90, 92]), (2, 0, [88, 90, 92]), (3, 0, [90]), (2, 3, [88, 92]),
                                             (1, 10, [88]), (1000, 0, [])])
def test_policy_every_and_rest(drive, every, rest, want):
    """the gating: with bounds that reject this loop nothing is ever corrected, every revisit frame matches an old keyframe 18 m from
    where the camera believes it is, and attempts are made on the ticks that are multiples of `every` and not within `rest` of the
    attempt before"""
    first = drive["first"]
    assert first == 88
    m, poses, status = _policy_run(drive, dict(every=every, rest=rest, max_trans=1.0, search=SEARCH), True)
    st = m.auto_place_stats()
    print(f"every {every}, rest {rest}: {st['attempts']} attempts, {st['rejected']} rejected, {st['failed']} failed, {st['matched']} matched")
    assert status[first:] == ["OK"] * 5 and st["matched"] == 5
    # the restatement of step 4 on the ticks of the five revisit frames
    ticks, rest_until = [], 0
    for T in range(first, first + 5):
        if T % every == 0 and T >= rest_until:
            ticks.append(T)
            rest_until = T + rest
    assert ticks == want and st["attempts"] == len(want) and st["closed"] == 0
    assert st["rejected"] + st["failed"] + st["none"] + st["no_old_map"] == len(want) and st["rejected"] >= min(1, len(want))
    assert all(np.array_equal(_bits(poses[T]), _bits(_policy_off(drive)[T])) for T in range(first + 5))


_OFF = {}


def _policy_off(drive):
    """the poses of the run without the policy, made once"""
    if "poses" not in _OFF:
        _OFF["poses"] = _policy_run(drive, None, False)[1]
    return _OFF["poses"]
