"""Known-answer tests K1..K16, K18 and K19 for the CPU oracle and the HIP product (K17 is the raw feedback
cloud's, K20 and K22 are open).

The reference ships no tests or golden vectors for the fusion path ("parity unpinned"),
so the oracle is pinned by answers derived by hand from the cited shader lines
(paths under /root/reference/src/Shaders unless noted).
"""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib as ol
from backends import BACKENDS, make

IDENT = np.eye(4, dtype=np.float32).T.reshape(16).copy()


class _Cfg:
    def __init__(self, W, H):
        self.width, self.height = W, H
        self.fx = self.fy = 100.0
        self.cx, self.cy = W / 2 - 0.5, H / 2 - 0.5


def cfg_small(W=160, H=96, border=0.0, **kw):
    return ol.make_config(W, H, 100.0, 100.0, W / 2 - 0.5, H / 2 - 0.5,
                          stereo_border=border, preprocess=0, **kw)


def mk(backend, W=160, H=96, border=0.0, **kw):
    """(cfg-like, instance) for either backend; same defaults as cfg_small."""
    inst = make(backend, W, H, 100.0, 100.0, W / 2 - 0.5, H / 2 - 0.5,
                stereo_border=border, preprocess=0, **kw)
    return _Cfg(W, H), inst


def surfel(x, y, z, conf=0.9, sem=0, rgb=(10, 20, 30), t0=1.0, t1=1.0, n=(0, 0, 1), r=0.05):
    s = np.zeros(12, np.float32)
    s[0:3] = (x, y, z)
    s[3] = conf
    bits = np.uint32((sem << 24) | (rgb[0] << 16) | (rgb[1] << 8) | rgb[2])
    s[4] = np.array([bits], np.uint32).view(np.float32)[0]
    s[6], s[7] = t0, t1
    s[8:11] = n
    s[11] = r
    return s


def plane_frame(cfg, z_mm, sem_val=0):
    W, H = cfg.width, cfg.height
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = 200, 100, 50
    depth = np.full((H, W), z_mm, np.uint16)
    sem = np.full((H, W), sem_val, np.uint8)
    return rgb, depth, sem


def bits(f):
    return int(np.array([f], np.float32).view(np.uint32)[0])


# ---------------------------------------------------------------- K1 color.glsl:19-37
def test_k1_encode_color():
    L = ol.lib()
    assert bits(L.smo_encode_color(1.0, 0.0, 0.0, 5)) == 0x05FF0000
    assert bits(L.smo_encode_color(0.0, 1.0, 0.0, 0)) == 0x0000FF00
    assert bits(L.smo_encode_color(10 / 255.0, 20 / 255.0, 30 / 255.0, 18)) == 0x120A141E
    # every u8 survives the b/255.f -> round(c*255) round trip
    for b in range(256):
        f = float(np.float32(b) / np.float32(255.0))
        assert bits(L.smo_encode_color(f, f, f, 0)) == (b << 16 | b << 8 | b)


# ---------------------------------------------------------------- K2 geometry.glsl:12-24, surfels.glsl:19-32
@pytest.mark.parametrize("backend", BACKENDS)
def test_k2_plane_normal_radius(backend):
    cfg, o = mk(backend)
    rgb, depth, sem = plane_frame(cfg, 4000)
    o.process_frame(rgb, depth, sem, IDENT)     # reference frame only
    o.process_frame(rgb, depth, sem, IDENT)     # all new
    m = o.download_model()
    assert m.shape[0] > 0
    np.testing.assert_array_equal(m[:, 8:11], np.tile(np.float32([0, 0, 1]), (m.shape[0], 1)))
    z = np.float32(4.0)
    inv_f = np.float32(1.0 / 100.0)
    mean_focal = (np.float32(1.0) / inv_f + np.float32(1.0) / inv_f) / np.float32(2.0)
    radius = (z / mean_focal) * np.float32(1.41421356237)
    np.testing.assert_array_equal(m[:, 11], np.full(m.shape[0], radius, np.float32))
    assert abs(float(radius) - 4.0 * math.sqrt(2) / 100.0) < 1e-6
    np.testing.assert_array_equal(m[:, 3], np.float32(0.9))
    np.testing.assert_array_equal(m[:, 5], 0.0)
    np.testing.assert_array_equal(m[:, 2], z)
    # getRadius: cap at 2x when the normal is nearly perpendicular to the ray
    L = ol.lib()
    r0 = L.smo_get_radius(4.0, 1.0, 0.01, 0.01)
    assert L.smo_get_radius(4.0, 0.1, 0.01, 0.01) == pytest.approx(2 * r0, rel=1e-6)
    assert L.smo_get_radius(4.0, 0.0, 0.01, 0.01) == pytest.approx(2 * r0, rel=1e-6)
    assert L.smo_get_radius(4.0, float("nan"), 0.01, 0.01) == pytest.approx(2 * r0, rel=1e-6)


# ---------------------------------------------------------------- K3/K4 data.vert:33-52,87-88 ; src/GlobalModel.cpp:67-74
@pytest.mark.parametrize("backend", BACKENDS)
def test_k3_k4_checkerboard_neighbours_order(backend):
    cfg, o = mk(backend, W=32, H=24)
    rgb, depth, sem = plane_frame(cfg, 5000)
    depth[10, 7] = 0          # hole at (i=7, j=10)
    o.process_frame(rgb, depth, sem, IDENT)
    o.process_frame(rgb, depth, sem, IDENT)
    m = o.download_model()
    # recover pixel of each new surfel from its position (identity pose, z = 5)
    i = np.rint(m[:, 0] / m[:, 2] * cfg.fx + cfg.cx - 0.5).astype(int)
    j = np.rint(m[:, 1] / m[:, 2] * cfg.fy + cfg.cy - 0.5).astype(int)
    assert np.all((i + j) % 2 == 1)
    emitted = set(zip(i.tolist(), j.tolist()))
    for bad in [(7, 10), (6, 10), (8, 10), (7, 9), (7, 11)]:
        assert bad not in emitted
    expect = [(a, b) for a in range(32) for b in range(24)
              if (a + b) % 2 == 1 and (a, b) not in [(7, 10), (6, 10), (8, 10), (7, 9), (7, 11)]]
    assert list(zip(i.tolist(), j.tolist())) == expect      # x-outer / y-inner (K4)
    c = o.counts()
    assert c["count"] == len(expect) == c["unstable_count"] == c["data_count"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_k3_stereo_border_after_metricise(backend):
    cfg, o = mk(backend, W=160, H=48, border=80.0)
    rgb, depth, sem = plane_frame(cfg, 5000)
    o.process_frame(rgb, depth, sem, IDENT)
    dm = o.download_depth(0)
    assert np.all(dm[:, :80] == 0) and np.all(dm[:, 80:] == np.float32(5.0))
    o.process_frame(rgb, depth, sem, IDENT)
    m = o.download_model()
    i = np.rint(m[:, 0] / m[:, 2] * cfg.fx + cfg.cx - 0.5).astype(int)
    assert i.min() == 81      # column 80 has a zero left neighbour


def test_metricise_range():
    cfg = cfg_small(W=8, H=1)
    raw = np.array([[0, 1000, 1001, 29998, 29999, 30000, 65535, 5000]], np.uint16)
    out = ol.metricise(cfg, raw)
    exp = np.float32([0, 0, 1001, 29998, 0, 0, 0, 5000]) / np.float32(1000.0)
    np.testing.assert_array_equal(out[0], exp)


# ---------------------------------------------------------------- K5 index_map.vert:59, GL_LESS gui/GUI.cpp:32
@pytest.mark.parametrize("backend", BACKENDS)
def test_k5_zbuffer_nearest_and_tie(backend):
    cfg, o = mk(backend)
    model = np.stack([
        surfel(0, 0, 9.0),              # id 0 (dummy, elsewhere in depth)
        surfel(0.5, 0.25, 6.0),         # id 1
        surfel(0.5 * 4 / 6, 0.25 * 4 / 6, 4.0),   # id 2 same pixel, nearer
        surfel(-0.5, 0.25, 5.0),        # id 3
        surfel(-0.5, 0.25, 5.0),        # id 4 identical -> lower id wins
    ])
    o.upload_model(model)
    o.stage_predict_indices(IDENT, 2, 30.0, 200)
    idx, vc, ct, nr = o.download_index_map()
    idx = idx.reshape(cfg.height, cfg.width)
    def pix(s):
        return (int(math.floor(s[1] / s[2] * cfg.fy + cfg.cy)), int(math.floor(s[0] / s[2] * cfg.fx + cfg.cx)))
    assert pix(model[1]) == pix(model[2])
    assert idx[pix(model[2])] == 2
    assert idx[pix(model[3])] == 3
    assert (idx > 0).sum() == 2           # id 0's pixel reads as "no surfel" (A5)
    p = pix(model[2])[0] * cfg.width + pix(model[2])[1]
    np.testing.assert_array_equal(vc[p], np.float32([model[2][0], model[2][1], 4.0, 0.9]))
    np.testing.assert_array_equal(nr[p], np.float32([0, 0, 1, 0.05]))
    # far plane: z >= far is not drawn
    o.upload_model(np.stack([surfel(0, 0, 9), surfel(0, 0, 30.0), surfel(0.3, 0, 29.99)]))
    o.stage_predict_indices(IDENT, 2, 30.0, 200)
    idx = o.download_index_map()[0]
    assert set(np.unique(idx).tolist()) == {0, 2}


# ---------------------------------------------------------------- K6 data.vert:142, conflict.geom:15
@pytest.mark.parametrize("backend", BACKENDS)
def test_k6_surfel_zero_never_fuses_never_conflicts(backend):
    cfg, o = mk(backend)
    rgb, depth, sem = plane_frame(cfg, 4000)
    o.process_frame(rgb, depth, sem, IDENT)
    o.process_frame(rgb, depth, sem, IDENT)
    n1 = o.counts()["count"]
    first = o.download_model()[0].copy()
    # same frame again: everything fuses except surfel 0, whose pixel spawns a duplicate
    o.process_frame(rgb, depth, sem, IDENT)
    c = o.counts()
    assert c["fused_count"] == n1 - 1 and c["unstable_count"] == 1 and c["count"] == n1 + 1
    m = o.download_model()
    np.testing.assert_array_equal(m[0], first)           # untouched: conf 0.9, time 1
    # farther depth: every in-view surfel conflicts except id 0
    rgb2, depth2, sem2 = plane_frame(cfg, 4001)
    o.process_frame(rgb2, depth2, sem2, IDENT)
    c2 = o.counts()
    assert c2["conflict_count"] == n1          # ids 1..n1 (the duplicate included), not id 0
    m2 = o.download_model()
    np.testing.assert_array_equal(m2[0], first)


# ---------------------------------------------------------------- K7 data.vert:151,177-194
@pytest.mark.parametrize("backend", BACKENDS)
def test_k7_static_plane_fuses(backend):
    cfg, o = mk(backend)
    rgb, depth, sem = plane_frame(cfg, 4000, sem_val=7)
    o.process_frame(rgb, depth, sem, IDENT)
    o.process_frame(rgb, depth, sem, IDENT)
    a = o.download_model()
    rgb_b = rgb.copy()
    rgb_b[..., 0] = 17
    o.process_frame(rgb_b, depth, sem, IDENT)
    b = o.download_model()
    n = a.shape[0]
    np.testing.assert_array_equal(b[1:n, 3], np.float32(0.9) + np.float32(0.9))
    np.testing.assert_array_equal(b[1:n, 6], 1.0)        # initTime kept
    np.testing.assert_array_equal(b[1:n, 7], 2.0)        # time updated
    np.testing.assert_array_equal(b[1:n, 11], a[1:n, 11])
    np.testing.assert_array_equal(b[1:n, 8:11], a[1:n, 8:11])
    assert bits(b[1, 4]) == (7 << 24 | 17 << 16 | 100 << 8 | 50)   # colour := new colour
    np.testing.assert_allclose(b[1:n, 0:3], a[1:n, 0:3], rtol=0, atol=1e-6)
    assert o.counts()["conflict_count"] == 0


# ---------------------------------------------------------------- K8 conflict.vert:64-73, back_map.geom:17
@pytest.mark.parametrize("backend", BACKENDS)
def test_k8_farther_depth_culls(backend):
    cfg, o = mk(backend)
    rgb, depth, sem = plane_frame(cfg, 4000)
    o.process_frame(rgb, depth, sem, IDENT)
    o.process_frame(rgb, depth, sem, IDENT)
    n1 = o.counts()["count"]
    rgb2, depth2, sem2 = plane_frame(cfg, 4001)
    o.process_frame(rgb2, depth2, sem2, IDENT)
    c = o.counts()
    assert c["conflict_count"] == n1 - 1
    assert c["offset"] == 1                      # only surfel 0 survives the cull
    assert c["unstable_count"] == n1 and c["count"] == n1 + 1
    # closer depth never conflicts
    _, o2 = mk(backend)
    o2.process_frame(rgb, depth, sem, IDENT)
    o2.process_frame(rgb, depth, sem, IDENT)
    rgb3, depth3, sem3 = plane_frame(cfg, 3999)
    o2.process_frame(rgb3, depth3, sem3, IDENT)
    assert o2.counts()["conflict_count"] == 0 and o2.counts()["offset"] == n1


# ---------------------------------------------------------------- K9/K10 conflict.vert:51-59
@pytest.mark.parametrize("backend", BACKENDS)
def test_k9_k10_zero_depth_and_sky(backend):
    cfg, o = mk(backend)
    model = np.stack([surfel(0, 0, 9.0), surfel(0.2, 0.1, 5.0, conf=0.9), surfel(-0.2, 0.1, 5.0, conf=1.8)])
    dm = np.zeros((cfg.height, cfg.width), np.float32)
    sem = np.zeros((cfg.height, cfg.width), np.uint8)
    o.upload_model(model)
    o.set_frame(depth_metric=dm, sem=sem)
    o.stage_process_conflict(IDENT, 1.0, 30.0, 0.0, 0)
    assert o.counts()["conflict_count"] == 2           # zero depth => far+20 => conflict
    o.stage_update_conflict(); o.stage_back_mapping()
    m = o.download_model()
    assert m.shape[0] == 2 and m[1, 3] == np.float32(1.8) - np.float32(1.0)
    # clean mode: zero depth is NOT far
    o.upload_model(model)
    o.stage_process_conflict(IDENT, 1.0, 15.0, 0.1, 1)
    assert o.counts()["conflict_count"] == 0
    # sky pixel => conflict in either mode, whatever the depth
    sem[:] = 10
    dm[:] = 2.0
    o.set_frame(depth_metric=dm, sem=sem)
    o.stage_process_conflict(IDENT, 1.0, 15.0, 0.1, 1)
    assert o.counts()["conflict_count"] == 2
    # range gate: surfel at z >= max is not tested
    o.stage_process_conflict(IDENT, 1.0, 5.0, 0.0, 0)
    assert o.counts()["conflict_count"] == 0


# ---------------------------------------------------------------- K11 index_map.vert:45
@pytest.mark.parametrize("backend", BACKENDS)
def test_k11_time_window(backend):
    cfg, o = mk(backend)
    model = np.stack([surfel(0, 0, 9.0), surfel(0.2, 0.1, 5.0, t0=1, t1=1), surfel(-0.2, 0.1, 5.0, t0=1, t1=100)])
    o.upload_model(model)
    o.stage_predict_indices(IDENT, 250, 30.0, 200)
    idx = o.download_index_map()[0]
    assert set(np.unique(idx).tolist()) == {0, 2}       # 250-1 > 200 -> id 1 absent
    o.stage_predict_indices(IDENT, 201, 30.0, 200)      # 201-1 == 200 -> not > -> present
    assert set(np.unique(o.download_index_map()[0]).tolist()) == {0, 1, 2}
    o.stage_predict_indices(IDENT, 202, 30.0, 200)      # 202-1 == 201 > 200 -> absent: the edge is bracketed on both sides
    assert set(np.unique(o.download_index_map()[0]).tolist()) == {0, 2}
    dm = np.zeros((cfg.height, cfg.width), np.float32)
    o.set_frame(depth_metric=dm, sem=np.zeros_like(dm, dtype=np.uint8))
    o.stage_process_conflict(IDENT, 1.0, 30.0, 0.0, 0)
    assert o.counts()["conflict_count"] == 2            # conflict pass has no time test


# ---------------------------------------------------------------- K12 src/SurfelMapping.cpp:142-154
@pytest.mark.parametrize("backend", BACKENDS)
def test_k12_first_call_reference_only(backend):
    cfg, o = mk(backend)
    o.process_frame(*plane_frame(cfg, 4000), IDENT)
    c = o.counts()
    assert c["count"] == 0 and c["tick"] == 1


# ---------------------------------------------------------------- K13 data.vert:54-57,158
def test_k13_acos_domain():
    L = ol.lib()
    assert math.isnan(L.smo_acosf(np.float32(1.0000001)))
    assert math.isnan(L.smo_acosf(-1.5))
    assert math.isnan(L.smo_acosf(float("nan")))
    assert L.smo_acosf(1.0) == 0.0
    xs = np.linspace(-1, 1, 4001, dtype=np.float32)
    got = np.array([L.smo_acosf(float(x)) for x in xs], np.float64)
    np.testing.assert_allclose(got, np.arccos(xs.astype(np.float64)), atol=5e-7)


def test_expf_accuracy():
    L = ol.lib()
    xs = np.linspace(-5, 1, 2001, dtype=np.float32)
    got = np.array([L.smo_expf(float(x)) for x in xs], np.float64)
    np.testing.assert_allclose(got, np.exp(xs.astype(np.float64)), rtol=3e-7)
    assert L.smo_expf(0.0) == 1.0


def test_invert4_rigid():
    a = math.radians(20)
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    m[:3, 3] = (1, -2, 3)
    inv = ol.invert4(m.T.astype(np.float32).reshape(16)).reshape(4, 4).T
    np.testing.assert_allclose(inv, np.linalg.inv(m), atol=1e-6)
    np.testing.assert_array_equal(ol.invert4(IDENT), IDENT)


# ---------------------------------------------------------------- frame invariants
@pytest.mark.parametrize("backend", BACKENDS)
def test_frame_invariants_moving_camera(backend):
    from surfelmapping_amd import synth
    cam = dict(width=320, height=120, fx=180.0, fy=180.0, cx=159.5, cy=59.5)
    seq = synth.make_sequence(cam, synth.kitti_trajectory(6), seed=3)
    o = make(backend, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"],
             preprocess=0, stereo_border=20.0)
    prev = 0
    for k, fr in enumerate(seq):
        o.process_frame(*fr)
        c = o.counts()
        assert c["tick"] == k + 1
        if k == 0:
            continue
        assert c["count"] == c["offset"] + c["unstable_count"]
        assert c["data_count"] == c["fused_count"] + c["unstable_count"]
        assert c["conflict_count"] <= max(prev - 1, 0)
        m = o.download_model()
        assert np.all(m[:, 5] == 0) and np.all(m[:, 3] > 0)
        assert np.all(m[:, 6] <= m[:, 7]) and np.all(m[:, 7] <= k)
        nn = np.linalg.norm(m[:, 8:11].astype(np.float64), axis=1)
        np.testing.assert_allclose(nn, 1.0, atol=1e-6)
        prev = c["count"]
    assert prev > 0


# ---------------------------------------------------------------- pre-processing known answers (oracle)
def test_filter_depth_support_rule():
    """depth_filter.frag:16-80: keep iff >= 7 of the 8 neighbours agree (class and |dz| < thr)."""
    cfg = cfg_small(W=8, H=8)
    d = np.full((8, 8), 5.0, np.float32)
    sem = np.zeros((8, 8), np.uint8)
    out = ol.filter_depth(cfg, d, sem, 0.15)
    assert np.all(out[1:-1, 1:-1] == 5.0) and np.all(out[0, :] == 0) and np.all(out[:, 0] == 0)   # borders: < 7 in-image
    d2 = d.copy(); d2[3, 3] = 5.2                     # outlier: kills itself, neighbours keep 7 of 8
    out = ol.filter_depth(cfg, d2, sem, 0.15)
    assert out[3, 3] == 0 and out[3, 4] == 5.0
    d3 = d.copy(); d3[3, 3] = 5.2; d3[3, 5] = 5.2     # (3,4) now has 2 disagreeing neighbours
    out = ol.filter_depth(cfg, d3, sem, 0.15)
    assert out[3, 4] == 0
    sem2 = sem.copy(); sem2[4, 4] = 11                 # person class is dropped
    assert ol.filter_depth(cfg, d, sem2, 0.15)[4, 4] == 0


def test_smooth_depth_constant_plane_and_weights():
    """depth_smooth.frag:17-82: a constant plane stays constant; a step within one class is averaged
    with weights exp(-(dx^2+dy^2) * 0.5/30^2) (the sigPix quirk, src/SurfelMapping.cpp:309)."""
    cfg = cfg_small(W=40, H=40)
    d = np.full((40, 40), 7.0, np.float32)
    sem = np.zeros((40, 40), np.uint8)
    out = ol.smooth_depth(cfg, d, sem)
    np.testing.assert_allclose(out, 7.0, rtol=2e-6)
    d[:, 20:] = 8.0
    out = ol.smooth_depth(cfg, d, sem)
    ix = np.arange(-6, 7)
    w = np.exp(-(ix[None, :] ** 2 + ix[:, None] ** 2) * (0.5 / 900.0))
    vals = np.where((20 + ix)[None, :] >= 20, 8.0, 7.0) * np.ones((13, 1))
    want = (w * vals).sum() / w.sum()
    assert abs(out[20, 20] - want) < 1e-5
    sem[:, 20:] = 2                                    # different classes do not mix
    out = ol.smooth_depth(cfg, d, sem)
    np.testing.assert_allclose(out[20, 19], 7.0, rtol=2e-6)
    np.testing.assert_allclose(out[20, 20], 8.0, rtol=2e-6)


def test_remove_movings_rule():
    """depth_movings.frag:30-82: class 13..18 pixels whose reprojected depth disagrees with LAST by > 0.5 m -> 0."""
    cfg = cfg_small(W=32, H=24)
    d = np.full((24, 32), 6.0, np.float32)
    last = np.full((24, 32), 6.0, np.float32)
    sem = np.zeros((24, 32), np.uint8); sem[8:16, 8:16] = 13
    out = ol.remove_movings(cfg, d, sem, last, IDENT)
    assert np.array_equal(out, d)
    last2 = last.copy(); last2[8:16, 8:16] = 7.0
    out = ol.remove_movings(cfg, d, sem, last2, IDENT)
    assert np.all(out[8:16, 8:16] == 0) and out[0, 0] == 6.0
    sem[:] = 0                                         # static classes are never removed
    assert np.array_equal(ol.remove_movings(cfg, d, sem, last2, IDENT), d)


# ---------------------------------------------------------------- K14/K15 data.vert:177-208 (both fuse branches, by hand)
def _f32(x):
    return np.float32(x)


@pytest.mark.parametrize("backend", BACKENDS)
def test_k14_k15_fuse_branches_hand_derived(backend):
    """Two surfels sit exactly on the rays of two checkerboard pixels of a fronto-parallel plane (identity pose, same
    depth => |z_o*lambda - z*lambda| = 0 <= fuseThresh 0, normals equal => acos(1) = 0 < 0.5): both associate.
    K14 data.vert:177-194 (radii_n < 1.5 r_o): confidence-weighted average of position and normal, colour := the NEW
      colour through the sic average ((c_n*color_n + c_o*color_n)/w, :183), conf = c_n + c_o, radius = min, initTime
      kept, time = tick.
    K15 data.vert:195-208 (radii_n >= 1.5 r_o): geometry, colour and radius of the OLD surfel are kept, conf += 0.9,
      time = tick.
    Expected values are worked out below in float32 from the shader lines, not taken from either implementation."""
    cfg, o = mk(backend)                       # 160 x 96, fx = fy = 100, cx = 79.5, cy = 47.5
    z = _f32(4.0)
    inv_f = _f32(1.0 / 100.0)                  # cam.z = 1/fx as float (src/GlobalModel.cpp:273-276)

    def ray_point(i, j):                       # getVertex geometry.glsl:5-9 at pixel centre (i+0.5, j+0.5)
        return np.array([(_f32(i + 0.5) - _f32(cfg.cx)) * z * inv_f, (_f32(j + 0.5) - _f32(cfg.cy)) * z * inv_f, z], np.float32)

    pa, pb = ray_point(100, 51), ray_point(40, 21)       # (i + j) odd: candidate pixels
    r_n = (z / ((_f32(1.0) / inv_f + _f32(1.0) / inv_f) / _f32(2.0))) * _f32(1.41421356237)     # surfels.glsl:19-32, n_z = 1
    c_o_a, c_o_b = _f32(1.8), _f32(2.7)
    r_a, r_b = _f32(0.05), _f32(0.03)
    assert r_n < _f32(1.5) * r_a and not (r_n < _f32(1.5) * r_b)
    model = np.stack([
        surfel(0.0, 0.0, 9.0),                                                        # id 0: never associates (A5)
        surfel(*pa, conf=c_o_a, sem=7, rgb=(10, 20, 30), t0=2.0, t1=3.0, r=r_a),      # K14
        surfel(*pb, conf=c_o_b, sem=7, rgb=(10, 20, 30), t0=2.0, t1=3.0, r=r_b),      # K15
    ])
    o.upload_model(model)
    o.set_tick(5)
    rgb, depth, sem = plane_frame(cfg, 4000, sem_val=7)                               # colour (200, 100, 50)
    o.process_frame(rgb, depth, sem, IDENT)
    c = o.counts()
    assert c["fused_count"] == 2 and c["conflict_count"] == 0 and c["offset"] == 3
    m = o.download_model()
    c_n = _f32(0.9)
    # ---- K14
    w = c_n + c_o_a
    exp_pos = ((c_n * pa) + (c_o_a * pa)) / w                                         # :179, identity pose
    np.testing.assert_array_equal(m[1, 0:3], exp_pos)
    assert m[1, 3] == w
    col = [_f32(v) / _f32(255.0) for v in (200, 100, 50)]
    avg = [((c_n * cn) + (c_o_a * cn)) / w for cn in col]                             # :183 multiplies color_n twice
    enc = [int(np.floor(np.float64(a * _f32(255.0)) + 0.5)) for a in avg]             # color.glsl:21-24 round()
    assert enc == [200, 100, 50]                                                      # i.e. the new colour survives the average
    assert bits(m[1, 4]) == (7 << 24 | 200 << 16 | 100 << 8 | 50)
    assert m[1, 5] == 0.0 and m[1, 6] == 2.0 and m[1, 7] == 5.0                       # initTime kept, time = tick
    nz = ((c_n * _f32(1.0)) + (c_o_a * _f32(1.0))) / w
    np.testing.assert_array_equal(m[1, 8:11], np.float32([0.0, 0.0, nz / np.sqrt(nz * nz)]))
    assert m[1, 11] == r_a                                                            # min(radii_n, r_o), :191
    # ---- K15
    np.testing.assert_array_equal(m[2, 0:3], pb)                                      # old position (identity pose)
    assert m[2, 3] == c_n + c_o_b
    assert bits(m[2, 4]) == (7 << 24 | 10 << 16 | 20 << 8 | 30)                       # old colour
    assert m[2, 6] == 2.0 and m[2, 7] == 5.0
    np.testing.assert_array_equal(m[2, 8:11], np.float32([0.0, 0.0, 1.0]))
    assert m[2, 11] == r_b
    np.testing.assert_array_equal(m[0], model[0])


# ---------------------------------------------------------------- K16 src/GlobalModel.cpp:54-57 (conflictVbo = W*H records)
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cap", [1, 0])
def test_k16_first_wh_conflicts_only_hand_derived(backend, cap):
    """150 surfels in view, all measured farther => every one but id 0 conflicts (conflict.vert:64-73, conflict.geom:15).
    conflictVbo holds W*H = 128 records and transform feedback stops writing when it is full: ids
    1..128 are decremented (0.9 - 1 <= 0 => culled by back_map.geom:17), ids 129..149 keep their confidence 0.9
    untouched, conflictCount = 128.  With the cap off all 149 are culled.  Both the per-pass API and processFrame."""
    W, H = 16, 8
    _, o = mk(backend, W=W, H=H, conflict_cap=cap, max_sqrt_vertices=64)
    fx, cxx, cyy = 100.0, W / 2 - 0.5, H / 2 - 0.5
    n = 150
    model = np.stack([surfel(((k % W) + 0.5 - cxx) * 5.0 / fx, (((k // W) % H) + 0.5 - cyy) * 5.0 / fx, 5.0, conf=0.9) for k in range(n)])
    dm = np.full((H, W), 20.0, np.float32)
    o.upload_model(model)
    o.set_frame(depth_metric=dm, sem=np.zeros((H, W), np.uint8))
    o.stage_process_conflict(IDENT, 1.0, 30.0, 0.0, 0)
    assert o.counts()["conflict_count"] == (128 if cap else 149)
    o.stage_update_conflict(); o.stage_back_mapping(); o.stage_build_model_map()
    m = o.download_model()
    if cap:
        assert m.shape[0] == 1 + (149 - 128)
        np.testing.assert_array_equal(m[0], model[0])
        np.testing.assert_array_equal(m[1:], model[129:])              # untouched: confidence still 0.9
    else:
        assert m.shape[0] == 1
    # the same through processFrame (frame path: conflict + cull + splat + associate + append)
    _, o2 = mk(backend, W=W, H=H, conflict_cap=cap, max_sqrt_vertices=64)
    o2.upload_model(model)
    o2.set_tick(3)
    rgb = np.zeros((H, W, 3), np.uint8)
    o2.process_frame(rgb, np.full((H, W), 20000, np.uint16), np.zeros((H, W), np.uint8), IDENT)
    c = o2.counts()
    assert c["conflict_count"] == (128 if cap else 149)
    assert c["offset"] == (22 if cap else 1)
    m2 = o2.download_model()
    np.testing.assert_array_equal(m2[:c["offset"]], m)


# ---------------------------------------------------------------- K18 geometry.glsl:12-24 at the image border
def _k18_depth_mm(W, H):
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    return (4000 + 50 * i + 30 * j).astype(np.uint16)              # tilted both ways: 5 cm per column, 3 cm per row


def _k18_surfel(zmm, i, j, f, cx, cy, reading):
    """(position, unit normal, radius) of the new surfel of pixel (i, j) in float64.  getVertex geometry.glsl:5-9, getNormal
    :12-24, getRadius surfels.glsl:19-32; `reading` says what a neighbour OUTSIDE the image is taken to be:
      'edge'      GL_CLAMP_TO_EDGE as the shader has it: the texel fetch clamps, i.e. the depth is the pixel's own (one step
                  out of the image lands on the pixel's own texel), while the coordinate handed to getVertex stays x +- 1, y +- 1
      'coord'     the coordinate is clamped to the image, [0, cols] x [0, rows], as well
      'one-sided' the neighbour is the pixel's own vertex: a one-sided difference
      'zero'      the depth outside the image reads as 0"""
    H, W = zmm.shape
    x, y = i + 0.5, j + 0.5                                         # data.vert:62-63 at a texel centre
    z = zmm.astype(np.float64) / 1000.0

    def vertex(zz, xx, yy):
        return np.array([(xx - cx) * zz / f, (yy - cy) * zz / f, zz])

    own = vertex(z[j, i], x, y)

    def neighbour(di, dj):
        ii, jj = i + di, j + dj
        if 0 <= ii < W and 0 <= jj < H:
            return vertex(z[jj, ii], x + di, y + dj)
        if reading == "edge":
            return vertex(z[j, i], x + di, y + dj)
        if reading == "coord":
            return vertex(z[j, i], min(max(x + di, 0.0), float(W)), min(max(y + dj, 0.0), float(H)))
        if reading == "one-sided":
            return own
        return vertex(0.0, x + di, y + dj)

    n = np.cross(neighbour(-1, 0) - neighbour(1, 0), neighbour(0, -1) - neighbour(0, 1))
    n /= np.linalg.norm(n)
    r = own[2] / f * 1.41421356237                                  # meanFocal = f: fx == fy
    return own, n, min(2.0 * r, r / abs(n[2]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_k18_border_normals_clamp_to_edge_hand_derived(backend):
    """New surfels of the pixels ON the image border: their out-of-image neighbour has the pixel's own depth at the coordinate
    x +- 1 / y +- 1.  Expected values from the shader lines in float64; the float32 cross product and normalisation of a
    unit vector lose at most a few 1e-7 per component, hence atol 1e-5 (K7 uses 1e-6 for positions).  The three other readings
    one could have of the border are shown to be more than 1e-2 away at every one of these pixels, so the tolerance tells
    them apart a thousand times over."""
    W, H, f = 16, 12, 100.0
    cfg, o = mk(backend, W=W, H=H)
    zmm = _k18_depth_mm(W, H)
    rgb, _, sem = plane_frame(cfg, 0)
    o.process_frame(rgb, zmm, sem, IDENT)
    o.process_frame(rgb, zmm, sem, IDENT)
    m = o.download_model()
    i = np.rint(m[:, 0] / m[:, 2] * f + cfg.cx - 0.5).astype(int)
    j = np.rint(m[:, 1] / m[:, 2] * f + cfg.cy - 0.5).astype(int)
    at = {(a, b): k for k, (a, b) in enumerate(zip(i.tolist(), j.tolist()))}
    border = [(a, b) for a in range(W) for b in range(H) if (a + b) % 2 == 1 and (a in (0, W - 1) or b in (0, H - 1))]
    for must in [(0, 5), (W - 1, 4), (5, 0), (4, H - 1), (W - 1, 0), (0, H - 1), (1, 0), (0, 1), (W - 2, H - 1), (W - 1, H - 2)]:
        assert must in border        # column 0, column W-1, row 0, row H-1, the two corners on the checkerboard, corner-adjacent ones
    assert len(at) == m.shape[0] == W * H // 2                      # every checkerboard pixel is emitted (K3), the border's included
    for px in border:
        assert px in at, f"border pixel {px} was not emitted"
        pos, n, r = _k18_surfel(zmm, *px, f, cfg.cx, cfg.cy, "edge")
        for other in ("coord", "one-sided", "zero"):
            n_other = _k18_surfel(zmm, *px, f, cfg.cx, cfg.cy, other)[1]
            assert not np.all(np.isfinite(n_other)) or np.abs(n_other - n).max() > 1e-2, (px, other, n, n_other)
        got = m[at[px]]
        np.testing.assert_allclose(got[0:3], pos, rtol=0, atol=1e-6, err_msg=f"position at {px}")
        np.testing.assert_allclose(got[8:11], n, rtol=0, atol=1e-5, err_msg=f"normal at {px}")
        assert got[11] == pytest.approx(r, rel=1e-5), f"radius at {px}"
    # an interior pixel for comparison: every reading agrees there, and so must the backend
    pos, n, r = _k18_surfel(zmm, 6, 5, f, cfg.cx, cfg.cy, "zero")
    np.testing.assert_allclose(m[at[(6, 5)]][8:11], n, rtol=0, atol=1e-5)


# ---------------------------------------------------------------- K19 conflict.vert:35 (the edges of the view test are inclusive)
@pytest.mark.parametrize("backend", BACKENDS)
def test_k19_conflict_view_edges_hand_derived(backend):
    """conflict.vert:35 `if(u < stereoBorder || u > cols || v < 0 || v > rows || z <= minDepth || z >= maxDepth)` skips a surfel:
    u and v exactly ON an edge are tested, the depth limits themselves are not.  fx = fy = 64, z = 4, cx = 15.5, cy = 7.5 and
    coordinates that are short binary fractions make u = fx * (x / z) + cx = 16 x + 15.5 exact in float32 (two scalings by powers
    of two, then one addition whose result is representable -- or, for the neighbours, rounds as worked out below).
    A surfel at u == cols samples texcoord 1.0, i.e. texel floor(1.0 * cols) clamped to the LAST column (GL_NEAREST,
    GL_CLAMP_TO_EDGE); likewise v == rows and the last row."""
    W, H = 32, 16
    f32 = np.float32
    inst = make(backend, W, H, 64.0, 64.0, W / 2 - 0.5, H / 2 - 0.5, stereo_border=8.0, preprocess=0)
    e = 2.0 ** -25
    #                x                     y                     z     tested?
    cases = [
        (-0.46875,            0.0,                  4.0,  True),     # 1  16 x + 15.5 = 8 = stereoBorder exactly
        (-0.46875 - e,        0.0,                  4.0,  False),    # 2  x one ulp (2^-25) down: 8 - 2^-21, the float32 below 8
        (1.03125,             0.0,                  4.0,  True),     # 3  16 x + 15.5 = 32 = cols exactly
        (1.03125 + 8 * e,     0.0,                  4.0,  False),    # 4  x two ulps (2^-22) up: 32 + 2^-18, the float32 above 32 (one ulp
                                                                     #    of x gives 32 + 2^-19, a tie that rounds back to the even 32)
        (0.0,                 -0.46875,             4.0,  True),     # 5  16 y + 7.5 = 0 exactly
        (0.0,                 -0.46875 - e,         4.0,  False),    # 6  y one ulp down: v = -2^-21, the nearest v below 0 this form can give
        (0.0,                 0.53125,              4.0,  True),     # 7  16 y + 7.5 = 16 = rows exactly
        (0.0,                 0.53125 + 4 * e,      4.0,  False),    # 8  y two ulps (2^-23) up: 16 + 2^-19, the float32 above 16
        (0.0,                 0.0,                  1.0,  False),    # 9  z == minDepth
        (0.0,                 0.0,                  float(np.nextafter(f32(1.0), f32(2.0))), True),      # 10
        (0.0,                 0.0,                  30.0, False),    # 11 z == maxDepth
        (0.0,                 0.0,                  float(np.nextafter(f32(30.0), f32(0.0))), True),     # 12
    ]
    # the derivation above, replayed in float32 (conflict.vert:27-33: xl = x / z, u = cam.z * xl + cam.x)
    def uv(x, y, z):
        return f32(64.0) * (f32(x) / f32(z)) + f32(15.5), f32(64.0) * (f32(y) / f32(z)) + f32(7.5)
    assert [f32(c[0]) == c[0] and f32(c[1]) == c[1] for c in cases] == [True] * len(cases)        # every coordinate IS a float32
    assert uv(*cases[0][:3])[0] == f32(8.0) and uv(*cases[1][:3])[0] == np.nextafter(f32(8.0), f32(0.0))
    assert uv(*cases[2][:3])[0] == f32(32.0) and uv(*cases[3][:3])[0] == np.nextafter(f32(32.0), f32(64.0))
    assert uv(*cases[4][:3])[1] == f32(0.0) and uv(*cases[5][:3])[1] == f32(-2.0 ** -21)
    assert uv(*cases[6][:3])[1] == f32(16.0) and uv(*cases[7][:3])[1] == np.nextafter(f32(16.0), f32(32.0))
    model = np.stack([surfel(0, 0, 9.0)] + [surfel(x, y, z, conf=1.8) for x, y, z, _ in cases])    # id 0 never conflicts (K6)
    expect = np.array([False] + [c[3] for c in cases])
    sem = np.zeros((H, W), np.uint8)

    def conflicts(dm):
        inst.upload_model(model)
        inst.set_frame(depth_metric=dm, sem=sem)
        inst.stage_process_conflict(IDENT, 1.0, 30.0, 0.0, 0)
        n = inst.counts()["conflict_count"]
        inst.stage_update_conflict(); inst.stage_back_mapping()
        m = inst.download_model()
        assert m.shape[0] == model.shape[0]                         # 1.8 - 1 > 0: nobody dies, the order stands
        hit = m[:, 3] == f32(1.8) - f32(1.0)
        assert np.all(hit | (m[:, 3] == model[:, 3])) and hit.sum() == n
        return hit

    # a zero depth reads as maxDepth + 20 (conflict.vert:56-59): every surfel the view test lets through conflicts
    np.testing.assert_array_equal(conflicts(np.zeros((H, W), np.float32)), expect)
    # which texel u == cols and v == rows sample: the measurement equals the surfels' depth (4 * lambda - 4 * lambda = 0, not > 0)
    # everywhere but in one column / one row, where it is farther
    def only(col=None, row=None):
        dm = np.full((H, W), 4.0, np.float32)
        if col is not None:
            dm[:, col] = 5.0
        if row is not None:
            dm[row, :] = 5.0
        hit = conflicts(dm)
        return set(np.flatnonzero(hit).tolist())
    near = {10}                                    # (surfel 10 at z = 1 + ulp is in front of a measurement of 4 m wherever that is)
    assert only() == near
    assert only(col=W - 1) == near | {3}           # surfel 3 (u == cols) reads the last column ...
    assert only(col=W - 2) == near                 # ... and nothing else
    assert only(row=H - 1) == near | {7}           # surfel 7 (v == rows) reads the last row
    assert only(row=H - 2) == near
    assert only(col=8) == near | {1}               # u == stereoBorder == 8.0 reads column 8
    assert only(col=7) == near
    assert only(row=0) == near | {5}               # v == 0 reads row 0
    assert only(row=1) == near
