"""Blended novel views (sm_render_image_blend, sm_render_image_maps_blend, sm_blend_stats; SurfelMap.render_image /
render_image_maps with blend; DESIGN.md "4o. Blended views").  CPU: the numpy restatement (blend_ref.py) against the oracle's
render for its fragments, against answers derived by hand for its sums; the library's symbols, defaults, header and the argument
rules that need no device.  GPU: the HIP path against the restatement, exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import blend_ref as br
import fill_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, F = 96, 64, 60.0
CX, CY = W / 2 - 0.5, H / 2 - 0.5
CAM = (W, H, F, F, CX, CY)
IDENT = np.eye(4, dtype=np.float32).T.reshape(16).copy()
FALLOFFS, TOLS = (0, 1, 2), (0, 13, 255)
ENTRY_POINTS = ("sm_default_blend_params", "sm_render_image_blend", "sm_render_image_maps_blend", "sm_blend_stats")


def surfel(x, y, z, r, n=(0, 0, -1), sem=3, bgr=(10, 20, 30)):
    s = np.zeros(12, np.float32)
    s[0:3] = (x, y, z); s[3] = 0.9
    s[4] = np.array([(sem << 24) | (bgr[2] << 16) | (bgr[1] << 8) | bgr[0]], np.uint32).view(np.float32)[0]
    s[6] = s[7] = 1.0
    s[8:11] = n; s[11] = r
    return s


def t_inv_of(view16):
    import oracle_lib as ol
    return ol.invert4(view16)


# ---------------------------------------------------------------------------------------------------------------------
# the scene of the exact comparisons: a fused street and one large disc laid on its ground
# ---------------------------------------------------------------------------------------------------------------------
class Scene:
    """Four frames of the synthetic street fused by the oracle at 64 x 48 (about 1.9 k surfels whose discs overlap everywhere),
    and one disc of radius 3 m laid on the ground.  Views: the last fused pose; half a metre to its side; and straight down from
    3 m above the big disc, where every disc is nearer than 5 m (the oriented branch) and the big one covers more than the image."""

    def __init__(self):
        import oracle_lib as ol
        from surfelmapping_amd import synth
        cam = dict(width=64, height=48, fx=40.0, fy=40.0, cx=31.5, cy=23.5)
        poses = synth.kitti_trajectory(4)
        self.over = dict(preprocess=0, stereo_border=0.0, max_sqrt_vertices=64)
        self.cam = cam
        o = ol.Oracle(ol.make_config(**cam, **self.over))
        for frame in synth.make_sequence(cam, poses, seed=3):
            o.process_frame(*frame)
        fused = o.download_model()
        o.close()
        big = surfel(0.3, 1.65, 6.2, 3.0, n=(0, -1, 0), sem=0, bgr=(90, 180, 40))
        self.rows = np.concatenate([fused, big[None]]).astype(np.float32)
        down = np.eye(4)
        down[:3, 0], down[:3, 1], down[:3, 2], down[:3, 3] = (1, 0, 0), (0, 0, -1), (0, 1, 0), (0, 1.65 - 3.0, 6.0)
        mats = [poses[3], synth.pose_matrix(0.5, 0.0, 2.4), down,
                synth.pose_matrix(-0.5, 0.0, 1.0, 10.0), synth.pose_matrix(0.0, -0.5, 3.0, -15.0)]
        self.all_views = np.stack([synth.pose_to_colmajor(m) for m in mats])
        self.views = self.all_views[:3]
        self.t_inv = [t_inv_of(v) for v in self.all_views]
        self.frags = [br.fragments(self.rows, t, *CAM) for t in self.t_inv]
        self._ref = {}

    def ref(self, view, tol=13, falloff=2):
        key = (view, tol, falloff)
        if key not in self._ref:
            self._ref[key] = br.blend(self.frags[view], self.rows, W, H, dict(depth_tol_256=tol, falloff=falloff))
        return self._ref[key]


@pytest.fixture(scope="module")
def scene():
    return Scene()


def test_restatement_draws_what_the_oracle_draws(scene):
    """the fragments decide the key map, and the key map the plain view: nearest colour and label equal the oracle's render -- for a
    view from 3 m behind the first pose, whose discs are all beyond 5 m (the screen-aligned branch), for the view from above, whose
    discs are all nearer (the oriented branch), and for the others, which have both"""
    import oracle_lib as ol
    from surfelmapping_amd import synth
    o = ol.Oracle(ol.make_config(**scene.cam, **scene.over))
    o.upload_model(scene.rows)
    back = synth.pose_to_colmajor(synth.pose_matrix(0.0, 0.0, -3.0))
    cases = [(back, t_inv_of(back), None, "far")] + [(scene.all_views[v], scene.t_inv[v], scene.frags[v], "near" if v == 2 else "both")
                                                      for v in range(len(scene.all_views))]
    for view, t_inv, frags, kind in cases:
        frags = br.fragments(scene.rows, t_inv, *CAM) if frags is None else frags
        m = np.asarray(t_inv, np.float32)
        z = ((m[2] * scene.rows[:, 0] + m[6] * scene.rows[:, 1]) + m[10] * scene.rows[:, 2]) + m[14]
        seen = np.unique(frags["k"])
        assert len(seen) > 100
        assert kind == "both" or (np.all(z[seen] <= 5.0) if kind == "near" else np.all(z[seen] > 5.0)), kind
        bgr, sem = o.render_image(view, *CAM)
        r = br.blend(frags, scene.rows, W, H)
        assert (sem != 0).sum() > 1000 and np.array_equal(r["nearest"], bgr) and np.array_equal(r["sem"], sem), kind
    o.close()


def test_the_scene_bites(scene):
    """blending is no no-op on any of the three views: with the defaults at least a quarter of the drawn pixels have two or more
    contributors and some colour changes; the big disc's pixel box is larger than 64 x 64 and crosses the image border in view 2"""
    for v in range(3):
        r = scene.ref(v)
        drawn = r["sem"] != 0
        multi = (r["contributors"] >= 2) & drawn
        assert drawn.sum() > 2000 and multi.sum() * 4 >= drawn.sum() and r["stats"]["changed"] > 0, (v, r["stats"])
        assert r["stats"]["contributions"] == r["contributors"].sum() > r["stats"]["drawn"]
    ok, X, Y, _ = br._vertices(scene.rows[-1:], scene.t_inv[2], *CAM)
    xs, ys = np.array([x[0] for x in X]) / 256.0, np.array([y[0] for y in Y]) / 256.0
    assert ok[0] and xs.min() < 0 and xs.max() > W and ys.min() < 0 and ys.max() > H and min(W, H) >= 64
    assert (scene.frags[2]["k"] == len(scene.rows) - 1).sum() > 3000      # a radius of 40 pixels, less what the border cuts


# ---------------------------------------------------------------------------------------------------------------------
# answers derived by hand
# ---------------------------------------------------------------------------------------------------------------------
A_BGR, B_BGR = (10, 100, 200), (250, 50, 0)
PX, PY = 57, 31


def pair(z2=10.0):
    """Two discs facing the camera of the identity view, radius 5 m.  At 10 m a metre is 6 pixels: A's centre falls on the centre of
    pixel (47, 31), B's -- 4 m to the right -- on that of (71, 31), both have a radius of 30 pixels.  Beyond 5 m the quad is the
    square with corners at r * 1.41421356 along the image axes and texture corners (+-1, +-1), so q = (dx^2 + dy^2) / r^2 in pixels.
    At pixel (57, 31): qA = 100 / 900 = 0.1111, 256 qA = 28.44, i = 28; qB = 196 / 900 = 0.2178, 256 qB = 55.75, i = 55.  (The
    24.8 vertices move a corner by at most 1 / 512 pixel of 42: 256 q moves by less than 0.03.)"""
    return np.stack([surfel(0, 0, 10.0, 5.0, bgr=A_BGR), surfel(4.0, 0, z2, 5.0, bgr=B_BGR)])


def at_pixel(rows, **params):
    r = br.render(rows, t_inv_of(IDENT), *CAM, params)
    return tuple(int(c) for c in r["bgr"][PY, PX]), int(r["contributors"][PY, PX])


def test_known_answer_two_discs_at_equal_depth():
    """falloff 0: wt 256, 256; SW 512: B (2560 + 64000 + 256) / 512 = 130.5 -> 130, G (25600 + 12800 + 256) / 512 = 75.5 -> 75,
    R (51200 + 0 + 256) / 512 = 100.5 -> 100.
    falloff 1: wt 256 - 28 = 228 and 256 - 55 = 201; SW 429, half 214: B (2280 + 50250 + 214) / 429 = 52744 / 429 = 122 (429 * 123 =
    52767), G (22800 + 10050 + 214) / 429 = 33064 / 429 = 77 (429 * 77 = 33033), R (45600 + 214) / 429 = 45814 / 429 = 106 (429 * 107
    = 45903).
    falloff 2: wt (228^2 + 255) >> 8 = 52239 >> 8 = 204 and (201^2 + 255) >> 8 = 40656 >> 8 = 158; SW 362, half 181:
    B (2040 + 39500 + 181) / 362 = 41721 / 362 = 115 (362 * 116 = 41992), G (20400 + 7900 + 181) / 362 = 28481 / 362 = 78 (362 * 79 =
    28598), R (40800 + 181) / 362 = 40981 / 362 = 113 (362 * 114 = 41268)."""
    assert br.weight(np.float32([100 / 900, 196 / 900, 0.0, 1.0]), 1).tolist() == [228, 201, 256, 1]
    assert br.weight(np.float32([100 / 900, 196 / 900, 0.0, 1.0]), 2).tolist() == [204, 158, 256, 1]
    for falloff, want in ((0, (130, 75, 100)), (1, (122, 77, 106)), (2, (115, 78, 113))):
        assert at_pixel(pair(), falloff=falloff) == (want, 2), falloff


def test_known_answer_the_band():
    """A at 10 m has d24 = round(0.05 * 16777215) = 838861 and is the front of pixel (57, 31); a metre is 83886 quanta.  B
    contributes iff d24 * 256 <= 838861 * (256 + tol): at tol 0 only at the same depth; at tol 13 up to 838861 * 269 / 256 = 881459,
    10.50782 m; at tol 255 up to 838861 * 511 / 256 = 1674445, 19.96094 m.  B is placed 0.1 mm to 0.2 mm (8 to 17 quanta) either
    side; at 20 m its radius is still 15 pixels around (59.5, 31.5).  falloff 0: inside the band the mean of the test above,
    outside A's own colour."""
    for tol, inside, outside in ((0, 10.0, 10.0001), (13, 10.5077, 10.5079), (255, 19.9608, 19.9611)):
        assert at_pixel(pair(inside), depth_tol_256=tol, falloff=0) == ((130, 75, 100), 2), tol
        assert at_pixel(pair(outside), depth_tol_256=tol, falloff=0) == (A_BGR, 1), tol


def test_known_answer_single_disc():
    """one contributor: (wt * c + wt / 2) / wt = c for every weight in 1..256"""
    for falloff in FALLOFFS:
        r = br.render(pair()[:1], t_inv_of(IDENT), *CAM, dict(falloff=falloff))
        drawn = r["sem"] != 0
        assert 2700 < drawn.sum() < 2900                                   # pi * 30^2 = 2827
        assert np.all(r["bgr"][drawn] == A_BGR) and np.all(r["bgr"][~drawn] == 0) and np.all(r["contributors"][drawn] == 1)
        assert r["stats"] == dict(drawn=int(drawn.sum()), contributions=int(drawn.sum()), changed=0)
    for wt in (1, 2, 3, 255, 256):
        assert br.normalise([wt] * 256, [wt * c for c in range(256)]).tolist() == list(range(256))


def test_normalisation_beyond_32_bits():
    """66000 fragments of weight 256 and colour 255: SW = 16896000, SC = 4308480000 > 2^32; (SC + SW / 2) / SW = 255.  2^31 - 1
    of them: SW = 549755813632 < 2^40, SC = 140187732476160 < 2^47.  And 2^32 * 100 + 2^31 over 2^32: (2^32 * 100 + 2^32) / 2^32 =
    101, one less below the half."""
    assert br.normalise([66000 * 256], [66000 * 256 * 255]).tolist() == [255] and 66000 * 256 * 255 > 2 ** 32
    n = 2 ** 31 - 1
    assert br.normalise([n * 256], [n * 256 * 255]).tolist() == [255] and n * 256 * 255 < 2 ** 47
    assert br.normalise([2 ** 32] * 2, [2 ** 32 * 100 + 2 ** 31, 2 ** 32 * 100 + 2 ** 31 - 1]).tolist() == [101, 100]
    assert br.normalise([0], [0]).tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------------
# the library, without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_defaults_and_binding():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert getattr(L, name) is not None and name in capi.SYMBOLS
    assert L.sm_api_version() == 4 and capi.API_VERSION == 4
    p = capi.blend_params()
    assert {k: getattr(p, k) for k in br.DEFAULTS} == br.DEFAULTS == dict(depth_tol_256=13, falloff=2)
    assert capi.blend_params(falloff=0).falloff == 0
    with pytest.raises(KeyError):
        capi.blend_params(fallof=1)
    for name in ("blend_stats", "render_image", "render_image_maps"):
        assert callable(getattr(capi.SurfelMap, name))
    header = open(os.path.join(ROOT, "include", "sm_c_api.h")).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header
    assert "#define SM_API_VERSION 4 " in header and "typedef struct sm_blend_params {" in header


def test_argument_rules_that_need_no_device():
    from surfelmapping_amd import capi
    L = capi.load()
    p, st = capi.blend_params(), capi.SmBlendStats()
    buf = np.zeros(64 * 3, np.uint8)
    ptr = capi._ptr(buf)
    src = capi.map_source([], True)
    assert L.sm_default_blend_params(None) == capi.SM_E_ARG
    assert L.sm_blend_stats(None, C.byref(st)) == capi.SM_E_ARG
    assert L.sm_render_image_blend(None, capi._ptr(IDENT), 4, 4, 1.0, 1.0, 2.0, 2.0, C.byref(p), None, ptr, ptr, None) == capi.SM_E_ARG
    assert L.sm_render_image_blend(None, capi._ptr(IDENT), 4, 4, 1.0, 1.0, 2.0, 2.0, None, None, ptr, ptr, None) == capi.SM_E_ARG
    assert L.sm_render_image_maps_blend(None, C.byref(src), capi._ptr(IDENT), 1, 4, 4, 1.0, 1.0, 2.0, 2.0, C.byref(p), None, ptr, ptr,
                                        None) == capi.SM_E_ARG
    for bad in (dict(depth_tol_256=-1), dict(depth_tol_256=256), dict(falloff=-1), dict(falloff=3)):
        q = capi.blend_params(**bad)
        assert L.sm_render_image_maps_blend(None, C.byref(src), capi._ptr(IDENT), 1, 4, 4, 1.0, 1.0, 2.0, 2.0, C.byref(q), None, ptr, ptr,
                                            None) == capi.SM_E_ARG
        assert list(bad)[0] in L.sm_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _ctx(rows=None, cap=64, w=W, h=H, f=F):
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(w, h, f, f, w / 2 - 0.5, h / 2 - 0.5, preprocess=0, stereo_border=0.0, max_sqrt_vertices=cap))
    if rows is not None:
        m.upload_model(rows)
    return m


@pytest.fixture(scope="module")
def model(scene):
    m = _ctx(scene.rows)
    yield m
    m.close()


def same_image(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist())


STAT_KEYS = ("drawn", "contributions", "changed")


@pytest.mark.gpu
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("falloff", FALLOFFS)
def test_gpu_bgr_is_bit_exact(scene, model, falloff, tol):
    p = dict(depth_tol_256=tol, falloff=falloff)
    for v in range(3):
        r = scene.ref(v, tol, falloff)
        drawn = r["sem"] != 0
        if tol == 13 and falloff == 2:                                      # (the test bites: see test_the_scene_bites)
            assert ((r["contributors"] >= 2) & drawn).sum() * 4 >= drawn.sum() and r["stats"]["changed"] > 0
        bgr, sem, depth = model.render_image(scene.views[v], *CAM, blend=p, depth=True)
        st = model.blend_stats()
        same_image(bgr, r["bgr"], (v, p))
        assert {k: st[k] for k in STAT_KEYS} == r["stats"], (v, p, st)
        assert st["launches"] == 2 and st["device_ms"] > 0.0
        plain = model.render_image(scene.views[v], *CAM, depth=True)
        same_image(sem, plain[1], (v, "sem")); same_image(depth, plain[2], (v, "depth"))
        same_image(sem, r["sem"], (v, "sem ref")); same_image(plain[0], r["nearest"], (v, "nearest"))
        b2, s2 = model.render_image(scene.views[v], *CAM, blend=p)          # without the depth plane: the same two planes
        assert np.array_equal(b2, bgr) and np.array_equal(s2, sem)


@pytest.mark.gpu
def test_gpu_unblended_outputs(scene, model):
    from surfelmapping_amd import capi
    L = model._L
    v = scene.views[1]
    fp = capi.fill_params(levels=2)
    for fill in (None, fp):
        want = model.render_image(v, *CAM, fill=fill, depth=True)
        got = np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint16)
        rc = L.sm_render_image_blend(model._h, capi._ptr(v), *CAM, None, C.byref(fp) if fill is not None else None,
                                     *(capi._ptr(a) for a in got))
        assert rc == capi.SM_OK
        for g, w_ in zip(got, want):
            same_image(g, w_, "blend NULL")
    # discs that do not overlap: every drawn pixel has one contributor and keeps its colour
    rows = np.stack([surfel(1.5 * i, 1.2 * j, 12.0, 0.5, sem=6 + i, bgr=(100 + 20 * i, 90 + 30 * j, 7)) for i in range(-3, 4) for j in range(-2, 3)])
    m = _ctx(rows)
    plain = m.render_image(IDENT, *CAM)
    for falloff in FALLOFFS:
        got = m.render_image(IDENT, *CAM, blend=dict(falloff=falloff, depth_tol_256=255))
        same_image(got[0], plain[0], falloff); same_image(got[1], plain[1], falloff)
        st = m.blend_stats()
        assert st["changed"] == 0 and st["contributions"] == st["drawn"] == (plain[1] != 0).sum() > 200
    m.close()


@pytest.mark.gpu
def test_gpu_accumulator_width():
    """66000 discs of colour 255 and radius 0.4 pixel centred on the centre of pixel (3, 3) of an 8 x 8 view: q = 0 there, so
    wt = 256 for every falloff, SW = 16896000 and every colour sum is 4308480000 > 2^32"""
    n = 66000
    rows = np.tile(surfel(0.0, 0.0, 10.0, 0.5, bgr=(255, 255, 255)), (n, 1))
    m = _ctx(rows, cap=257)
    for falloff in FALLOFFS:
        bgr, sem = m.render_image(IDENT, 8, 8, 8.0, 8.0, 3.5, 3.5, blend=dict(falloff=falloff, depth_tol_256=0))
        want = np.zeros((8, 8, 3), np.uint8)
        want[3, 3] = 255
        same_image(bgr, want, falloff)
        assert (sem != 0).sum() == 1 and sem[3, 3] == 4
        st = m.blend_stats()
        assert {k: st[k] for k in STAT_KEYS} == dict(drawn=1, contributions=n, changed=0)
    m.close()


@pytest.mark.gpu
def test_gpu_determinism_and_the_model_is_left_alone(scene, model):
    before, counts = model.download_model(), model.counts()
    a = model.render_image(scene.views[2], *CAM, blend=True, depth=True)
    sa = model.blend_stats()
    b = model.render_image(scene.views[2], *CAM, blend=True, depth=True)
    sb = model.blend_stats()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert {k: sa[k] for k in STAT_KEYS + ("launches",)} == {k: sb[k] for k in STAT_KEYS + ("launches",)}
    assert np.array_equal(model.download_model().view(np.uint32), before.view(np.uint32)) and model.counts() == counts
    assert np.array_equal(before.view(np.uint32), scene.rows.view(np.uint32))
    # a smaller view after a larger one, and the larger again: the scratch is reused
    small = model.render_image(scene.views[0], 33, 21, 20.0, 20.0, 16.0, 10.0, blend=True)
    r = br.render(scene.rows, scene.t_inv[0], 33, 21, 20.0, 20.0, 16.0, 10.0)
    same_image(small[0], r["bgr"], "33 x 21")
    assert model.render_image(scene.views[2], *CAM, blend=True)[0].tobytes() == a[0].tobytes()


def write_map(path, rows):
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 12)
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([0, 0], np.int32).tobytes())
        f.write(rows.tobytes())
    return str(path)


@pytest.mark.gpu
def test_gpu_map_sets(scene, model, tmp_path):
    """files plus the live model against the context that holds their concatenation; five views, so that a key budget of 1 MiB --
    6144 pixels * (8 + 2 + 32) bytes a view -- makes two batches"""
    rows = scene.rows
    n0, n1 = 600, 1400
    paths = [write_map(tmp_path / "a.bin", rows[:n0]), write_map(tmp_path / "b.bin", rows[n0:n1])]
    views = scene.all_views
    V = len(views)
    m = _ctx(rows[n1:])
    p = dict(depth_tol_256=13, falloff=2)
    want = [np.stack(x) for x in zip(*[model.render_image(v, *CAM, blend=p, depth=True) for v in views])]
    total = {k: sum(scene.ref(v)["stats"][k] for v in range(V)) for k in STAT_KEYS}
    for v in range(V):
        same_image(want[0][v], scene.ref(v)["bgr"], ("resident", v))
    plain = [np.stack(x) for x in zip(*[model.render_image(v, *CAM, depth=True) for v in views])]
    assert not np.array_equal(want[0], plain[0])
    keys = ("SM_RENDER_MAPS_KEY_MB", "SM_RENDER_MAPS_NO_CULL")
    try:
        for env in ({}, {"SM_RENDER_MAPS_KEY_MB": "1"}, {"SM_RENDER_MAPS_NO_CULL": "1"}):
            for k in keys:
                os.environ.pop(k, None)
            os.environ.update(env)
            got = m.render_image_maps(paths, views, *CAM, blend=p, depth=True)
            for g, w_, name in zip(got, want, ("bgr", "sem", "depth_mm")):
                same_image(g, w_, (env, name))
            ms, st = m.render_maps_stats(), m.blend_stats()
            assert ms["passes"] == (2 if "SM_RENDER_MAPS_KEY_MB" in env else 1), ms
            assert ms["surfels_read"] == 2 * n1 * ms["passes"] and ms["chunks"] == 2 * 2 * ms["passes"]
            assert {k: st[k] for k in STAT_KEYS} == total and st["launches"] > 0
            b, s = m.render_image_maps(paths, views, *CAM, blend=p)
            assert np.array_equal(b, want[0]) and np.array_equal(s, want[1])
            # without the live model: the files alone
            only = _ctx(rows[:n1]) if not env else None
            if only is not None:
                w2 = [np.stack(x) for x in zip(*[only.render_image(v, *CAM, blend=p) for v in views])]
                g2 = m.render_image_maps(paths, views, *CAM, blend=p, include_model=False)
                same_image(g2[0], w2[0], "files alone"); same_image(g2[1], w2[1], "files alone sem")
                only.close()
            # blend None through the map-set entry point is the _ex call
            g3 = m.render_image_maps(paths, views, *CAM, depth=True)
            for g, w_ in zip(g3, plain):
                same_image(g, w_, (env, "plain"))
            assert m.render_maps_stats()["surfels_read"] == n1 * m.render_maps_stats()["passes"]
    finally:
        for k in keys:
            os.environ.pop(k, None)
    m.close()


@pytest.mark.gpu
def test_gpu_with_fill(scene, model, tmp_path):
    for p, fp in ((dict(), dict()), (dict(falloff=1, depth_tol_256=40), dict(levels=5, prefer_far=0))):
        for v in (0, 2):
            unfilled = model.render_image(scene.views[v], *CAM, blend=p, depth=True)
            want = fr.fill(*unfilled, fp)
            got = model.render_image(scene.views[v], *CAM, blend=p, fill=fp, depth=True)
            for g, w_, name in zip(got, want[:3], ("bgr", "sem", "depth_mm")):
                same_image(g, w_, (v, name))
            st = model.fill_stats()
            assert {k: st[k] for k in want[3]} == want[3]
    # ... and over a map set
    paths = [write_map(tmp_path / "a.bin", scene.rows[:900])]
    m = _ctx(scene.rows[900:])
    fp = dict(levels=3)
    unfilled = m.render_image_maps(paths, scene.views, *CAM, blend=True, depth=True)
    got = m.render_image_maps(paths, scene.views, *CAM, blend=True, fill=fp, depth=True)
    want = fr.fill(*unfilled, fp)
    for g, w_, name in zip(got, want[:3], ("bgr", "sem", "depth_mm")):
        same_image(g, w_, ("maps", name))
    assert (want[1][0] != 0).sum() > (unfilled[1][0] != 0).sum()
    m.close()


@pytest.mark.gpu
def test_gpu_refusals(scene, model, tmp_path):
    import retire_ref as rr
    from surfelmapping_amd import capi
    L = model._L
    path = write_map(tmp_path / "a.bin", scene.rows[:50])
    fresh = _ctx()
    with pytest.raises(capi.SurfelMapError) as e:
        fresh.blend_stats()
    assert e.value.rc == capi.SM_E_ARG
    for bad in (dict(depth_tol_256=-1), dict(depth_tol_256=256), dict(falloff=-1), dict(falloff=3)):
        for call in (lambda: model.render_image(IDENT, *CAM, blend=bad), lambda: model.render_image_maps([path], [IDENT], *CAM, blend=bad)):
            with pytest.raises(capi.SurfelMapError) as e:
                call()
            assert e.value.rc == capi.SM_E_ARG and list(bad)[0] in str(e.value)
    with pytest.raises(capi.SurfelMapError) as e:
        model.render_image(IDENT, *CAM, blend=True, fill=dict(levels=9))
    assert e.value.rc == capi.SM_E_ARG and "levels" in str(e.value)
    p = capi.blend_params()
    bgr, sem = np.full((H, W, 3), 0xA5, np.uint8), np.full((H, W), 0x5A, np.uint8)
    args = lambda view=IDENT, w=W, h=H, b=bgr, s=sem: (capi._ptr(view) if view is not None else None, w, h, F, F, CX, CY, C.byref(p), None,
                                                        capi._ptr(b) if b is not None else None, capi._ptr(s) if s is not None else None, None)
    for a in (args(view=None), args(w=0), args(h=-1), args(b=None), args(s=None), args(w=1 << 15, h=1 << 14)):
        assert L.sm_render_image_blend(model._h, *a) == capi.SM_E_ARG
    src = capi.map_source([str(tmp_path / "nowhere.bin")], True)
    rc = L.sm_render_image_maps_blend(model._h, C.byref(src), capi._ptr(IDENT), 1, W, H, F, F, CX, CY, C.byref(p), None, capi._ptr(bgr),
                                      capi._ptr(sem), None)
    assert rc == capi.SM_E_ARG and "nowhere.bin" in L.sm_last_error().decode()
    assert (bgr == 0xA5).all() and (sem == 0x5A).all()
    # between sm_stage_conflict and sm_stage_cull
    seq = rr.sequence(2)
    st = capi.SurfelMap(capi.make_config(**rr.CAM, **rr.OVER, preprocess=0, max_sqrt_vertices=200))
    for frame in seq:
        st.process_frame(*frame)
    st.stage_conflict(seq[1][3], 1.0, 30.0)
    for call in (lambda: st.render_image(IDENT, *CAM, blend=True), lambda: st.render_image_maps([path], [IDENT], *CAM, blend=True)):
        with pytest.raises(capi.SurfelMapError) as e:
            call()
        assert e.value.rc == capi.SM_E_ARG and "sm_stage_conflict" in str(e.value)
    st.stage_cull()
    st.render_image(IDENT, *CAM, blend=True)
    st.close()
    # a sharded and a rig context
    for configure in ("shard_stream_configure", "rig_configure"):
        part = _ctx()
        getattr(part, configure)(0, 1)
        for call in (lambda: part.render_image(IDENT, *CAM, blend=True), lambda: part.render_image_maps([path], [IDENT], *CAM, blend=True)):
            with pytest.raises(capi.SurfelMapError) as e:
                call()
            assert e.value.rc == capi.SM_E_UNSUPPORTED
        part.close()
    fresh.close()
