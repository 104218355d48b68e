"""Hole filling of novel views (sm_fill_image*, sm_render_image_ex, sm_render_image_maps_ex; SurfelMap.fill_image, render_image /
render_image_maps with fill / depth; DESIGN.md "4n. Hole filling").  CPU: the integer restatement (fill_ref.py) against its own
scalar loop, against answers derived by hand and against the properties the rules promise; the library's symbols, defaults and
header; the 16-bit PNG writer against the reader's decoder, plain and under the address and undefined-behaviour sanitizers.  GPU:
the HIP path against the restatement, exactly, on all three planes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fill_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("bgr", "sem", "depth_mm")


def random_images(rng, n, h, w, share, layers=(5120, 5380, 5381, 20000, 0)):
    """n images with `share` of their pixels valid; depths from few layers, so that ties and the exact tolerance boundary (5120
    against 5380 / 5381 at the default tolerance) occur, valid pixels without depth (0) among them; invalid pixels are zeros"""
    valid = rng.random((n, h, w)) < share
    sem = np.where(valid, rng.integers(1, 20, (n, h, w)), 0).astype(np.uint8)
    bgr = np.where(valid[..., None], rng.integers(0, 256, (n, h, w, 3)), 0).astype(np.uint8)
    depth = np.where(valid, rng.choice(np.array(layers), (n, h, w)), 0).astype(np.uint16)
    return bgr, sem, depth


def same(got, want, what):
    for g, w_, name in zip(got, want, PLANES):
        if w_ is None:
            assert g is None, (what, name)
            continue
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, name)
        bad = np.argwhere(g != w_)
        assert len(bad) == 0, (what, name, len(bad), bad[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, without a GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [0, 8])
@pytest.mark.parametrize("tol", [0, 255])
@pytest.mark.parametrize("through", [0, 8])
def test_restatement_equals_the_scalar_loop_at_the_ends_of_every_range(levels, tol, through):
    rng = np.random.default_rng(levels * 100 + tol + through)
    for far in (0, 1):
        for cover in (0, 256):
            p = dict(levels=levels, depth_tol_256=tol, through_count=through, prefer_far=far, min_cover_256=cover)
            bgr, sem, depth = random_images(rng, 1, 10, 24, 0.4)
            a, b = fr.fill(bgr[0], sem[0], depth[0], p), fr.fill_scalar(bgr[0], sem[0], depth[0], p)
            same(a[:3], b[:3], p)
            assert a[3] == b[3], p


def test_restatement_equals_the_scalar_loop_in_between():
    rng = np.random.default_rng(7)
    for p in (dict(), dict(levels=2, through_count=1), dict(levels=5, through_count=3, min_cover_256=1), dict(levels=3, prefer_far=0, depth_tol_256=40)):
        for share in (0.1, 0.6):
            bgr, sem, depth = random_images(rng, 2, 10, 24, share)
            a, b = fr.fill(bgr, sem, depth, p), fr.fill_scalar(bgr, sem, depth, p)
            same(a[:3], b[:3], p)
            assert a[3] == b[3], p
    bgr, sem, _ = random_images(rng, 1, 10, 24, 0.5)
    a, b = fr.fill(bgr[0], sem[0], None), fr.fill_scalar(bgr[0], sem[0], None)          # no depth plane: one layer
    same(a[:3], b[:3], "no depth")
    assert a[2] is None and a[3] == b[3]


def _grey(rows, depth, labels):
    """images from nested lists: a colour per pixel (None = empty) on all three channels, one depth / label per pixel or for all"""
    c = np.array([[0 if v is None else v for v in r] for r in rows], np.uint8)
    valid = np.array([[v is not None for v in r] for r in rows])
    d = np.where(valid, np.broadcast_to(np.array(depth), c.shape), 0).astype(np.uint16)
    s = np.where(valid, np.broadcast_to(np.array(labels), c.shape), 0).astype(np.uint8)
    return np.repeat(c[..., None], 3, -1), s, d


def test_known_answer_2x2():
    """Three valid pixels at 10000 mm, (1, 1) empty, levels 1, see-through off.  Pull: the one cell of level 1 has zmin 10000, all
    three children near, n = 3: c = ((10+20+40+1)/3, (20+30+50+1)/3, (30+40+60+1)/3) = (71/3, 101/3, 131/3) = (23, 33, 43);
    z = (30000+1)/3 = 10000; label of the first child at zmin: 5; cnt 3 of area 4: 768 >= 256, may fill.  Push: (1, 1) has X = Y = 0,
    Xn = Yn = 1 outside level 1: one tap of weight 9: c = (9*23+4)/9 = 23, (9*33+4)/9 = 33, (9*43+4)/9 = 43; z = 10000; label 5."""
    bgr = np.zeros((2, 2, 3), np.uint8); sem = np.zeros((2, 2), np.uint8); d = np.zeros((2, 2), np.uint16)
    bgr[0, 0], bgr[0, 1], bgr[1, 0] = (10, 20, 30), (20, 30, 40), (40, 50, 60)
    sem[0, 0], sem[0, 1], sem[1, 0] = 5, 6, 7
    d[sem > 0] = 10000
    for f in (fr.fill, fr.fill_scalar):
        ob, os_, od, t = f(bgr, sem, d, dict(levels=1, through_count=0))
        assert tuple(ob[1, 1]) == (23, 33, 43) and os_[1, 1] == 5 and od[1, 1] == 10000
        assert np.array_equal(ob[sem > 0], bgr[sem > 0]) and t == dict(valid=3, seen_through=0, filled=1, left_empty=0)


def test_known_answer_row_of_four():
    """10, -, -, 250 at 1000 mm, labels 2, -, -, 3, levels 1.  Level 1: cell 0 = (10, label 2, cnt 1 of area 2: 256 >= 128), cell 1 =
    (250, label 3).  Pixel 1: X = 0, odd so Xn = 1; the row has no Yn.  Taps (10, weight 9) and (250, weight 3), one layer:
    (90 + 750 + 6) / 12 = 846 / 12 = 70; the greatest weight is tap 0's: label 2.  Pixel 2: X = 1, even so Xn = 0:
    (2250 + 30 + 6) / 12 = 2286 / 12 = 190; label 3.  With all depths 0 every z is 65536: one layer again, the same colours, and
    (9*65536 + 3*65536 + 6) / 12 = 65536 comes out as depth 0 -- at levels 8 too: each higher level is one valid cell, nothing more
    is invalid when its push comes."""
    bgr, sem, d = _grey([[10, None, None, 250]], 1000, [[2, 0, 0, 3]])
    for f in (fr.fill, fr.fill_scalar):
        ob, os_, od, _ = f(bgr, sem, d, dict(levels=1, through_count=0))
        assert ob[0, :, 0].tolist() == [10, 70, 190, 250] and os_[0].tolist() == [2, 2, 3, 3] and od[0].tolist() == [1000] * 4
        ob, os_, od, _ = f(bgr, sem, np.zeros_like(d), dict(levels=8, through_count=0))
        assert ob[0, :, 1].tolist() == [10, 70, 190, 250] and os_[0].tolist() == [2, 2, 3, 3] and od[0].tolist() == [0] * 4


def test_known_answer_two_layers():
    """[[200, 200, 100, 100], [200, -, -, 100]], depths 5000 | 20000, labels 8 | 4, levels 1.  Level 1: cell 0 = (200, 5000, label 8,
    cnt 3), cell 1 = (100, 20000, label 4, cnt 3).  Hole (1, 1): taps cell 0 (9) and cell 1 (3), Yn = 1 outside.  20000 and 5000 are
    two layers (5000 * 269 < 20000 * 256).  prefer_far: the group is cell 1 alone: 100 / 4 / 20000; otherwise cell 0 alone:
    200 / 8 / 5000.  Hole (2, 1) mirrors it: taps cell 1 (9) and cell 0 (3), the same groups."""
    bgr, sem, d = _grey([[200, 200, 100, 100], [200, None, None, 100]], [[5000, 5000, 20000, 20000]] * 2, [[8, 8, 4, 4]] * 2)
    for f in (fr.fill, fr.fill_scalar):
        for far, want in ((1, (100, 4, 20000)), (0, (200, 8, 5000))):
            ob, os_, od, _ = f(bgr, sem, d, dict(levels=1, through_count=0, prefer_far=far))
            for x in (1, 2):
                assert (ob[1, x, 0], os_[1, x], od[1, x]) == want, (far, x)


def test_known_answer_see_through_3x3():
    """A ring of eight pixels at 5120 mm.  Tolerance 13: a neighbour is nearer iff 5120 * 269 = 1377280 < z * 256.  z = 5381:
    1377536, nearer, eight times >= 6: the centre is removed, then refilled at levels 1 from the ring: colour 50, depth 5120.
    z = 5380: 1377280, not less: kept.  A far pixel in a corner has three neighbours only: it survives through_count 4 (and falls
    at 3)."""
    ring = [[50, 50, 50], [50, 90, 50], [50, 50, 50]]
    for f in (fr.fill, fr.fill_scalar):
        for zc, gone in ((5381, True), (5380, False)):
            bgr, sem, d = _grey(ring, [[5120, 5120, 5120], [5120, zc, 5120], [5120, 5120, 5120]], 3)
            ob, os_, od, t = f(bgr, sem, d, dict(levels=1, through_count=6))
            assert t["seen_through"] == int(gone)
            assert (ob[1, 1, 0], od[1, 1]) == ((50, 5120) if gone else (90, zc)) and os_[1, 1] == 3
        bgr, sem, d = _grey(ring, [[9000, 5120, 5120], [5120, 5120, 5120], [5120, 5120, 5120]], 3)
        assert f(bgr, sem, d, dict(levels=0, through_count=4))[3]["seen_through"] == 0
        assert f(bgr, sem, d, dict(levels=0, through_count=3))[3]["seen_through"] == 1


def test_known_answer_single_pixel():
    """One valid pixel at (3, 2) of 7 x 5, defaults (min_cover_256 64).  Level 1: cell (1, 1) covers x 2..3, y 2..3: cnt 1 of 4,
    256 >= 256: may fill.  Level 2: cell (0, 0) covers x 0..3, y 0..3: cnt 1 of 16, 256 < 1024: may not, and no higher cell may
    either, so nothing above level 1 pushes.  Level 0 takes cell (1, 1) as its first tap for x 2..3, as Xn for x = 1 (X = 0, odd)
    and x = 4 (X = 2, even), and likewise in y: the block x 1..4, y 1..4, for any levels >= 1.  min_cover_256 128: 256 < 512, nothing
    fills.  min_cover_256 1 at levels 3: every cell above the pixel may fill, level 3 is one cell, and everything is filled."""
    bgr = np.zeros((5, 7, 3), np.uint8); sem = np.zeros((5, 7), np.uint8); d = np.zeros((5, 7), np.uint16)
    bgr[2, 3], sem[2, 3], d[2, 3] = (9, 8, 7), 4, 3000
    block = np.zeros((5, 7), bool); block[1:5, 1:5] = True
    for f in (fr.fill, fr.fill_scalar):
        for levels in (1, 2, 3, 8):
            _, os_, _, _ = f(bgr, sem, d, dict(levels=levels))
            assert np.array_equal(os_ == 4, block), levels
        assert f(bgr, sem, d, dict(levels=3, min_cover_256=128))[3]["filled"] == 0
        ob, os_, od, t = f(bgr, sem, d, dict(levels=3, min_cover_256=1))
        assert t["left_empty"] == 0 and np.all(os_ == 4) and np.all(od == 3000) and np.all(ob == (9, 8, 7))


def two_layer_scene(seed=3, w=96, h=64):
    """a wall at 20 m (label 4), a pole at 5 m (label 8) in front of it, random holes in both, and a strip of holes three pixels
    wide beside the pole: (bgr, sem, depth_mm, strip mask)"""
    rng = np.random.default_rng(seed)
    sem = np.full((h, w), 4, np.uint8); d = np.full((h, w), 20000, np.uint16)
    bgr = np.full((h, w, 3), (90, 100, 110), np.uint8)
    sem[:, 40:52], d[:, 40:52], bgr[:, 40:52] = 8, 5000, (200, 30, 30)
    hole = rng.random((h, w)) < 0.2
    strip = np.zeros((h, w), bool); strip[:, 52:55] = True
    hole |= strip
    hole[:, 48:52] = False; hole[:, 55:58] = False               # both sides of the strip are observed
    sem[hole] = 0; d[hole] = 0; bgr[hole] = 0
    return bgr, sem, d, strip


def test_properties_on_a_two_layer_scene():
    bgr, sem, d, strip = two_layer_scene()
    valid = sem > 0
    prev = None
    for levels in (0, 1, 2, 3, 5, 8):
        ob, os_, od, t = fr.fill(bgr, sem, d, dict(levels=levels, through_count=0))
        assert np.array_equal(ob[valid], bgr[valid]) and np.array_equal(os_[valid], sem[valid]) and np.array_equal(od[valid], d[valid])
        if levels == 0:
            assert np.array_equal(ob, bgr) and np.array_equal(os_, sem) and np.array_equal(od, d)
        filled = os_ > 0
        assert prev is None or not np.any(prev & ~filled), levels
        prev = filled
    for far, label, z in ((1, 4, 20000), (0, 8, 5000)):
        _, os_, od, _ = fr.fill(bgr, sem, d, dict(levels=3, through_count=0, prefer_far=far))
        assert np.all(os_[strip] == label) and np.all(od[strip] == z), far


def test_depth_rule_known_answers():
    """zmm = (d24 * 200000 + 8388607) // 16777215, 0 beyond 65535.  By hand: 41 * 200000 + 8388607 = 16588607 < 16777215 -> 0 and
    42 * 200000 + 8388607 = 16788607 -> 1 (a millimetre is 83.9 quanta, half of one 41.9); 65536 * 16777215 = 1099511562240, and
    5497515 * 200000 + 8388607 = 1099511388607 lies below it (65535) while 5497516 * 200000 + 8388607 = 1099511588607 does not (0);
    the greatest d24 that is drawn, 16777214, is 200 m."""
    d24 = np.array([0, 41, 42, 5497515, 5497516, 16777214])
    assert fr.depth_of_d24(d24).tolist() == [0, 0, 1, 65535, 0, 0]
    assert fr.depth_of_d24(d24).dtype == np.uint16


# ---------------------------------------------------------------------------------------------------------------------
# the library, without a GPU
# ---------------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("sm_default_fill_params", "sm_fill_image", "sm_fill_image_device", "sm_render_image_ex", "sm_render_image_maps_ex", "sm_fill_stats")


def test_library_exports_defaults_and_binding():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None and name in capi.SYMBOLS
    assert L.sm_api_version() == 4 and capi.API_VERSION == 4
    p = capi.fill_params()
    assert (p.levels, p.depth_tol_256, p.through_count, p.prefer_far, p.min_cover_256) == (3, 13, 6, 1, 64)
    assert {k: getattr(p, k) for k in fr.DEFAULTS} == fr.DEFAULTS
    assert capi.fill_params(levels=5).levels == 5
    with pytest.raises(KeyError):
        capi.fill_params(level=5)
    assert L.sm_default_fill_params(None) == capi.SM_E_ARG
    for name in ("fill_image", "fill_image_device", "fill_stats", "render_image", "render_image_maps"):
        assert callable(getattr(capi.SurfelMap, name))
    header = open(os.path.join(ROOT, "include", "sm_c_api.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
    assert "#define SM_API_VERSION 4 " in header and "typedef struct sm_fill_params {" in header


@pytest.mark.parametrize("sanitize", [False, True])
def test_png16_round_trip_host_only(tmp_path, sanitize):
    """tests/cpp/png16_check.cpp, a program of its own that is never loaded into Python: plain, then under ASan + UBSan with both
    runtimes linked into the program itself, so that it starts in whatever environment the suite runs in"""
    exe = str(tmp_path / "png16_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "png16_check.cpp"), "-lz"])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr)


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(64, 48, 100.0, 100.0, 32.0, 24.0, preprocess=0, max_sqrt_vertices=64))
    yield m
    m.close()


def check(m, bgr, sem, depth, p, what):
    want = fr.fill(bgr, sem, depth, p)
    got = m.fill_image(bgr, sem, depth, fill=p)
    same(got if depth is not None else got + (None,), want[:3], (what, p))
    st = m.fill_stats()
    assert {k: st[k] for k in want[3]} == want[3], (what, p, st)
    assert 1 <= st["launches"] <= p.get("levels", 3) + 2 and st["device_ms"] >= 0.0
    return st


SHAPES = [(131, 37), (33, 65), (64, 32), (2, 2), (1, 1), (1, 9), (9, 1)]      # w x h


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
def test_gpu_shapes_and_levels(ctx, w, h):
    """partial tiles both ways and an odd size at every level (131 x 37), one more pixel than a tile, whole tiles, and images
    smaller than 2^levels"""
    rng = np.random.default_rng(w * 1000 + h)
    for levels in (0, 1, 3, 5, 6, 8):
        bgr, sem, depth = random_images(rng, 1, h, w, 0.5)
        st = check(ctx, bgr[0], sem[0], depth[0], dict(levels=levels, through_count=2), (w, h))
        assert st["launches"] == max(levels, 1) + 1 + (levels > 5)      # the pull, levels 6..8, one push per level (levels 0: the image's)


@pytest.mark.gpu
def test_gpu_batches_and_scratch_regrowth(ctx):
    rng = np.random.default_rng(11)
    for (w, h, n) in ((131, 37, 3), (9, 1, 1), (131, 37, 3), (64, 32, 5)):
        bgr, sem, depth = random_images(rng, n, h, w, 0.3)
        check(ctx, bgr, sem, depth, dict(levels=6, through_count=1), (w, h, n))
        check(ctx, bgr, sem, depth, dict(levels=2), (w, h, n))


@pytest.mark.gpu
def test_gpu_content(ctx):
    rng = np.random.default_rng(12)
    w, h = 131, 37
    for share in (0.05, 0.5, 0.95, 0.0, 1.0):
        bgr, sem, depth = random_images(rng, 2, h, w, share)
        for p in (dict(), dict(levels=5, through_count=3, min_cover_256=8)):
            check(ctx, bgr, sem, depth, p, share)
        check(ctx, bgr, sem, None, dict(levels=4), (share, "no depth"))
    bgr, sem, depth, _ = two_layer_scene()
    check(ctx, bgr, sem, depth, dict(), "two layers")
    # the inputs are left alone, and an invalid pixel that carries rubbish comes out as zeros
    bgr, sem, depth = random_images(rng, 1, h, w, 0.5)
    bgr[sem == 0] = 77; depth[sem == 0] = 1234
    keep = bgr.copy(), sem.copy(), depth.copy()
    check(ctx, bgr, sem, depth, dict(levels=0, through_count=0), "rubbish")
    assert all(np.array_equal(a, b) for a, b in zip(keep, (bgr, sem, depth)))


@pytest.mark.gpu
@pytest.mark.parametrize("tol", [0, 255])
@pytest.mark.parametrize("far", [0, 1])
def test_gpu_parameter_corners(ctx, tol, far):
    rng = np.random.default_rng(13 + tol + far)
    bgr, sem, depth = random_images(rng, 1, 65, 33, 0.4, layers=(5120, 5380, 5381, 20000, 0, 10240, 65535))
    for through in (0, 1, 8):
        for cover in (0, 1, 256):
            check(ctx, bgr[0], sem[0], depth[0], dict(levels=3, depth_tol_256=tol, through_count=through, prefer_far=far, min_cover_256=cover), "corner")


@pytest.mark.gpu
def test_gpu_arguments(ctx):
    from surfelmapping_amd import capi
    L = ctx._L
    bgr, sem, depth = random_images(np.random.default_rng(1), 1, 4, 4, 0.5)
    for bad in (dict(levels=9), dict(levels=-1), dict(depth_tol_256=256), dict(through_count=9), dict(prefer_far=2), dict(min_cover_256=257)):
        with pytest.raises(capi.SurfelMapError) as e:
            ctx.fill_image(bgr, sem, depth, fill=bad)
        assert e.value.rc == capi.SM_E_ARG and list(bad)[0] in str(e.value)
        with pytest.raises(capi.SurfelMapError) as e:
            ctx.render_image(IDENT, 8, 8, 10.0, 10.0, 4.0, 4.0, fill=bad)
        assert e.value.rc == capi.SM_E_ARG and list(bad)[0] in str(e.value)
    p = capi.fill_params()
    assert L.sm_fill_image(ctx._h, C.byref(p), 0, 4, 1, capi._ptr(bgr), capi._ptr(sem), None) == capi.SM_E_ARG
    assert L.sm_fill_image(ctx._h, C.byref(p), 4, 4, 1, None, capi._ptr(sem), None) == capi.SM_E_ARG
    assert L.sm_fill_image(ctx._h, None, 4, 4, 1, capi._ptr(bgr), capi._ptr(sem), None) == capi.SM_E_ARG
    assert L.sm_fill_image(ctx._h, C.byref(p), 1 << 15, 1 << 14, 1, capi._ptr(bgr), capi._ptr(sem), None) == capi.SM_E_ARG


@pytest.mark.gpu
def test_gpu_device_call_equals_the_host_call(ctx):
    rng = np.random.default_rng(14)
    w, h, n = 131, 37, 2
    bgr, sem, depth = random_images(rng, n, h, w, 0.4)
    p = dict(levels=6, through_count=2)
    want = ctx.fill_image(bgr, sem, depth, fill=p)
    bufs = [ctx.device_alloc(a.nbytes) for a in (bgr, sem, depth)]
    for b, a in zip(bufs, (bgr, sem, depth)):
        ctx.device_upload(b, a)
    ctx.fill_image_device(bufs[0], bufs[1], bufs[2], w, h, n, fill=p)
    got = [ctx.device_download(b, a.nbytes, a.dtype).reshape(a.shape) for b, a in zip(bufs, (bgr, sem, depth))]
    same(got, want, "device")
    assert {k: v for k, v in ctx.fill_stats().items() if k != "device_ms"} == dict(fr.fill(bgr, sem, depth, p)[3], launches=8)
    for b in bufs:
        ctx.device_free(b)


# ---- the render path: a 200 x 160 view of an uploaded model, as tests/test_render.py builds them
RW, RH, RF = 200, 160, 150.0
RCX, RCY = RW / 2 - 0.5, RH / 2 - 0.5
IDENT = np.eye(4, dtype=np.float32).T.reshape(16).copy()


def surfel(x, y, z, r, n=(0, 0, 1), sem=3, rgb=(10, 20, 30)):
    s = np.zeros(12, np.float32)
    s[0:3] = (x, y, z); s[3] = 0.9
    s[4] = np.array([(sem << 24) | (rgb[0] << 16) | (rgb[1] << 8) | rgb[2]], np.uint32).view(np.float32)[0]
    s[6] = s[7] = 1.0
    s[8:11] = n; s[11] = r
    return s


def scene_rows():
    """a wall of discs with gaps at 10 m, a column of discs at 4 m in front of it, one disc at 70 m beside them"""
    rows = []
    for j in range(-6, 7):
        for i in range(-7, 8):
            if i < 5:                                         # (the right of the view stays open for the far disc)
                rows.append(surfel(0.8 * i, 0.8 * j, 10.0, 0.42, sem=4, rgb=(90 + 5 * i, 100 + 3 * j, 110)))
    for j in range(-8, 9):
        rows.append(surfel(-0.4, 0.25 * j, 4.0, 0.3, sem=8, rgb=(200, 30, 30 + j)))
    rows.append(surfel(31.0, 0.0, 70.0, 4.0, sem=11, rgb=(5, 250, 5)))
    return np.stack(rows)


def _model(rows, cap=64):
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(RW, RH, RF, RF, RCX, RCY, preprocess=0, stereo_border=0.0, max_sqrt_vertices=cap))
    m.upload_model(rows)
    return m


@pytest.mark.gpu
def test_gpu_render_path_depth_and_fill():
    m = _model(scene_rows())
    view = (IDENT, RW, RH, RF, RF, RCX, RCY)
    b0, s0 = m.render_image(*view)
    b1, s1, d1 = m.render_image(*view, depth=True)
    assert np.array_equal(b0, b1) and np.array_equal(s0, s1)
    # a fronto-parallel far-mode disc at 10 m: d24 = 0.05 * 16777215 to within a few quanta of 0.012 mm, so 10000 on every pixel
    assert (s1 == 5).sum() > 2000 and np.all(d1[s1 == 5] == 10000)
    assert (s1 == 9).sum() > 300 and (s1 == 12).sum() > 50
    # the rule itself, on keys known from the geometry: all three kinds of disc face the camera, so every pixel of one carries its
    # vertices' window z up to the rounding of the float interpolation -- two quanta of d24 either way cover it, and the rule
    # maps all five candidates to one value: 10000, 4000 exactly, and 0 for the disc beyond 65.535 m, which is drawn all the same
    for label, z_m, mm in ((5, 10.0, 10000), (9, 4.0, 4000), (12, 70.0, 0)):
        f = np.float32
        zw = f(0.5) * (f(2.0) * f(z_m) / f(200.0) - f(1.0)) + f(0.5)                  # render_surfel: zn, then the window z
        d24 = int(np.floor(float(zw) * 16777215.0 + 0.5)) + np.arange(-2, 3)
        assert abs(int(d24[2]) - z_m / 200.0 * 16777215) < 2 and np.all(fr.depth_of_d24(d24) == mm), (label, d24)
        assert np.all(d1[s1 == label] == mm), (label, np.unique(d1[s1 == label]))
    assert (s1 == 0).sum() > 2000 and np.all(d1[s1 == 0] == 0) and np.all((d1 > 0) <= (s1 > 0))
    for p in (dict(), dict(levels=5, prefer_far=0), dict(levels=2, through_count=3)):
        want = fr.fill(b1, s1, d1, p)
        got = m.render_image(*view, fill=p, depth=True)
        same(got, want[:3], p)
        st = m.fill_stats()
        assert {k: st[k] for k in want[3]} == want[3]
        assert 0 < st["left_empty"] < (s1 == 0).sum() and st["filled"] > 0
        b2, s2 = m.render_image(*view, fill=p)                            # without the depth plane: the same two planes
        assert np.array_equal(b2, got[0]) and np.array_equal(s2, got[1])
    m.close()


def write_map(path, rows):
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 12)
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([0, 0], np.int32).tobytes())
        f.write(rows.tobytes())
    return str(path)


def scene_views():
    from surfelmapping_amd import synth
    return np.stack([synth.pose_to_colmajor(p) for p in (synth.pose_matrix(0, 0, 0), synth.pose_matrix(0.6, 0.2, -1.5, 4.0), synth.pose_matrix(-1.0, 0, 1.0, -6.0))])


@pytest.mark.gpu
def test_gpu_map_sets(tmp_path):
    rows = scene_rows()
    n0, n1 = 60, 150
    paths = [write_map(tmp_path / "a.bin", rows[:n0]), write_map(tmp_path / "b.bin", rows[n0:n1])]
    views = scene_views()
    big, m = _model(rows), _model(rows[n1:])
    cam = (RW, RH, RF, RF, RCX, RCY)
    p = dict(levels=4)
    want = [np.stack(x) for x in zip(*[big.render_image(v, *cam, fill=p, depth=True) for v in views])]
    plain = [np.stack(x) for x in zip(*[big.render_image(v, *cam, depth=True) for v in views])]
    keys = ("SM_RENDER_MAPS_KEY_MB", "SM_RENDER_MAPS_NO_CULL")
    try:
        for env in ({}, {"SM_RENDER_MAPS_KEY_MB": "1"}, {"SM_RENDER_MAPS_NO_CULL": "1"}):
            for k in keys:
                os.environ.pop(k, None)
            os.environ.update(env)
            got = m.render_image_maps(paths, views, *cam, fill=p, depth=True)
            same(got, want, env)
            st, passes = m.fill_stats(), m.render_maps_stats()["passes"]
            assert passes == (2 if "SM_RENDER_MAPS_KEY_MB" in env else 1), passes
            assert st["launches"] == (p["levels"] + 1) * passes        # per pass of all its views: the pull and one push per level
            assert passes > 1 or st["launches"] <= p["levels"] + 2
            assert st == dict(st, **fr.fill(*plain, p)[3])
            same(m.render_image_maps(paths, views, *cam, depth=True), plain, (env, "no fill"))
            b, s = m.render_image_maps(paths, views, *cam)
            assert np.array_equal(b, plain[0]) and np.array_equal(s, plain[1])
    finally:
        for k in keys:
            os.environ.pop(k, None)
    assert (want[1] > 0).sum() > (plain[1] > 0).sum()
    big.close(); m.close()
