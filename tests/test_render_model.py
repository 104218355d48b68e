"""The model view (GlobalModel::renderModel, src/GlobalModel.cpp:683-758; sm_render_model).  Hand-derived known answers on
the numpy restatement (tests/model_view_ref.py, CPU) and on the HIP core (-m gpu) with the same assertions; bit-exact parity of
the HIP images against the restatement on a map fused by the core; no side effects on the model; argument checks (CPU)."""
import ctypes as C
import math

import numpy as np
import pytest

import model_view_ref as ref
from backends import assert_models_equal

f32 = np.float32
BACKENDS = ["ref", pytest.param("hip", marks=pytest.mark.gpu)]


def surfel(x, y, z, r, n=(0.0, 0.0, 1.0), conf=2.0, sem=3, rgb=(10, 20, 30), t=1.0):
    s = np.zeros(12, f32)
    s[0:3] = (x, y, z)
    s[3] = conf
    s[4] = np.array([(sem << 24) | (rgb[0] << 16) | (rgb[1] << 8) | rgb[2]], np.uint32).view(f32)[0]
    s[6] = s[7] = t
    s[8:11] = n
    s[11] = r
    return s


def render(backend, model, mvp, mv_inv, w, h, **kw):
    """(rgba, depth, ids) of one view"""
    model = np.ascontiguousarray(np.stack(model) if isinstance(model, list) else model, f32)
    if backend == "ref":
        return ref.render_model(model, mvp, mv_inv, w, h, **kw)
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(64, 48, 50.0, 50.0, 31.5, 23.5, max_sqrt_vertices=200))
    m.upload_model(model)
    return m.render_model(mvp, mv_inv, w, h, depth=True, ids=True, **kw)


# Orthographic 32 x 32 view (w = 1: affine texcoords): window x = world x, window y = world y, clip z = -0.1 * world z, so a
# visible clip z is <= 1 and every disc takes the near branch.  MVINV: identity rotation, eye at (16, 16, 10) on the axis of a
# disc at (16, 16, z) with normal +-z, so cosAngle = +-1 exactly.
ORTHO = np.array([[1 / 16, 0, 0, -1], [0, 1 / 16, 0, -1], [0, 0, -0.1, 0], [0, 0, 0, 1]])
EYE = np.eye(4)
EYE[:3, 3] = (16.0, 16.0, 10.0)
O_MVP, O_INV = ORTHO.T.reshape(16).astype(f32), EYE.T.reshape(16).astype(f32)


def _disc_80():
    """Pixels (i, j) of a 32x32 image whose centres (i + 0.5, j + 0.5) lie within 5 px of (16, 16): per quadrant the
    half-integer offsets a = 0.5 .. 4.5 admit b <= 4.5, 4.5, 3.5, 3.5, 1.5 (a^2 + b^2 <= 25), 20 pixels, 80 in all; a^2 + b^2
    is never 25 for half-integers (nearest: 24.5 inside, 26.5 outside), so the set does not depend on rounding."""
    m = np.zeros((32, 32), bool)
    for j in range(32):
        for i in range(32):
            m[j, i] = (i + 0.5 - 16.0) ** 2 + (j + 0.5 - 16.0) ** 2 <= 25.0
    assert m.sum() == 80
    return m


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("nz", [1.0, -1.0])
def test_ortho_near_branch_disc_is_the_80_pixel_set(backend, nz):
    """draw_surface_adaptive.geom:105-111: cosAngle = +-1, radius = 7.5 / 1.5 = 5 px; the strip P+x, P+y, P-y, P-x with
    texcoords (-1,-1), (1,-1), (-1,1), (1,1) is an affine map with |texcoord|^2 = |offset|^2 / 25 (draw_surface.frag:30)."""
    rgba, depth, ids = render(backend, [surfel(16.0, 16.0, 0.0, 7.5, n=(0.0, 0.0, nz), rgb=(11, 22, 33))], O_MVP, O_INV, 32, 32,
                              color_type=2, clear=(1, 2, 3, 4))
    want = _disc_80()
    assert np.array_equal(ids == 0, want)
    assert np.all(rgba[want] == (11, 22, 33, 255)) and np.all(rgba[~want] == (1, 2, 3, 4))
    assert np.all(depth[want] == f32(8388608) / f32(16777215)) and np.all(depth[~want] == 1.0)   # zw = 0.5
    assert np.all(ids[~want] == -1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_perspective_far_branch_disc_area_and_centre(backend):
    """posLocal.z > 5: a camera-facing disc of world radius r (draw_surface_adaptive.geom:97-101): 64 * 1 / 10 = 6.4 px."""
    P = ref.projection(64, 64, 64.0, 64.0, 32.0, 32.0, 0.1, 1000.0)
    MV = ref.look_at(0, 0, 0, 0, 0, 1, 0, -1, 0)
    mvp, inv = ref.view_mats(P, MV)
    rgba, depth, ids = render(backend, [surfel(0.0, 0.0, 10.0, 1.0, n=(0.6, 0.0, 0.8))], mvp, inv, 64, 64)
    m = ids == 0
    rad = 64.0 * 1.0 / 10.0
    assert abs(m.sum() - math.pi * rad ** 2) < 0.08 * math.pi * rad ** 2
    ys, xs = np.nonzero(m)
    assert abs(xs.mean() + 0.5 - 32.0) < 0.6 and abs(ys.mean() + 0.5 - 32.0) < 0.6


@pytest.mark.parametrize("backend", BACKENDS)
def test_colour_bytes(backend):
    """shaded 0.5 |n.x + n.y + n.z| + 0.1 (geom:85), colours srgb.yzw / 255 (:54-55), semantic palette (:57-81,
    src/GlobalModel.cpp:718-736), normals (:50), window x 0.25 (:88-91), RGBA8 = floor(clamp(c) * 255 + 0.5)"""
    def centre(n=(0.0, 0.0, 1.0), **kw):
        s = dict(sem=kw.pop("sem", 3), rgb=kw.pop("rgb", (10, 20, 30)), t=kw.pop("t", 1.0))
        rgba, _, _ = render(backend, [surfel(16.0, 16.0, 0.0, 7.5, n=n, **s)], O_MVP, O_INV, 32, 32, **kw)
        return tuple(int(c) for c in rgba[16, 16])
    assert centre(n=(0.6, 0.0, 0.8), color_type=0) == (204, 204, 204, 255)           # floor(0.8 * 255 + 0.5)
    assert centre(rgb=(200, 100, 50), color_type=2) == (200, 100, 50, 255)
    assert centre(rgb=(0, 255, 7), color_type=2) == (0, 255, 7, 255)
    assert centre(sem=13, color_type=3) == (255, 0, 0, 255)
    assert centre(sem=12, color_type=3) == (245, 222, 179, 255)
    assert centre(sem=19, color_type=3) == (0, 0, 0, 255)
    assert centre(n=(0.48, -0.36, 0.8), color_type=1) == (122, 0, 204, 255)        # floor(122.4 + 0.5), 0, floor(204 + 0.5)
    # window: time - surfel.time = 10 - 1 > 5 -> x 0.25 before rounding (204 / 4 = 51, 100 / 4 = 25, 52 / 4 = 13)
    assert centre(rgb=(204, 100, 52), color_type=2, window=True, time=10, time_delta=5) == (51, 25, 13, 255)
    assert centre(rgb=(204, 100, 52), color_type=2, window=True, time=6, time_delta=5) == (204, 100, 52, 255)
    assert centre(rgb=(204, 100, 52), color_type=2, window=False, time=10, time_delta=5) == (204, 100, 52, 255)


@pytest.mark.parametrize("backend", BACKENDS)
def test_gates(backend):
    s = surfel(16.0, 16.0, 0.0, 7.5, conf=0.9)
    # conf == threshold: not drawn unless unstable (draw_surface.vert:47)
    assert np.all(render(backend, [s], O_MVP, O_INV, 32, 32, threshold=0.9, unstable=False)[2] == -1)
    assert np.sum(render(backend, [s], O_MVP, O_INV, 32, 32, threshold=0.9, unstable=True)[2] == 0) == 80
    # points ignore unstable (draw_feedback.vert:38); above the threshold one fragment at (floor(xw), floor(yw))
    assert np.all(render(backend, [s], O_MVP, O_INV, 32, 32, threshold=0.9, unstable=True, points=True)[2] == -1)
    ids = render(backend, [s], O_MVP, O_INV, 32, 32, threshold=0.5, unstable=False, points=True)[2]
    assert np.sum(ids == 0) == 1 and ids[16, 16] == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_depth_order_and_ties(backend):
    near, far = surfel(16.0, 16.0, 1.0, 7.5, rgb=(1, 1, 1)), surfel(16.0, 16.0, 0.0, 7.5, rgb=(2, 2, 2))
    ids = render(backend, [far, near], O_MVP, O_INV, 32, 32)[2]
    assert np.sum(ids == 1) == 80 and np.sum(ids == 0) == 0                 # the nearer disc (higher id) wins
    ids = render(backend, [far, far, far], O_MVP, O_INV, 32, 32)[2]
    assert np.sum(ids == 0) == 80 and np.sum(ids > 0) == 0                  # the same d24: the lower id
    # a disc straddling the eye plane: a vertex with clip w <= 0 -> not drawn
    P = ref.projection(64, 64, 64.0, 64.0, 32.0, 32.0, 0.1, 1000.0)
    mvp, inv = ref.view_mats(P, ref.look_at(0, 0, 0, 0, 0, 1, 0, -1, 0))
    rgba, depth, ids = render(backend, [surfel(0.0, 0.0, 0.3, 1.0, n=(1.0, 0.0, 0.0))], mvp, inv, 64, 64, clear=(9, 8, 7, 6))
    assert np.all(ids == -1) and np.all(rgba == (9, 8, 7, 6)) and np.all(depth == 1.0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_ids_name_the_aos_row(backend):
    model = [surfel(8.0 + 16.0 * (k % 2), 8.0 + 16.0 * (k // 2), 0.0, 4.5) for k in range(4)]
    ids = render(backend, model, O_MVP, O_INV, 32, 32)[2]
    for k in range(4):
        assert ids[int(model[k][1]), int(model[k][0])] == k


# ---------------------------------------------------------------------------------------------------------------------
# bit-exact parity against the restatement on a map fused by the core
# ---------------------------------------------------------------------------------------------------------------------
CAM = dict(width=160, height=120, fx=100.0, fy=100.0, cx=79.5, cy=59.5)


def _views(w, h):
    """a GUI-like view behind and above the trajectory (gui/GUI.cpp:46-47), a side view, and one inside the map whose discs
    cross the near plane and cover more than a thousand pixels"""
    P = ref.projection(w, h, 420.0 * w / 640, 420.0 * h / 480, 320.0 * w / 640, 240.0 * h / 480, 0.1, 1000.0)
    return {"gui": ref.view_mats(P, ref.look_at(0, -6, -10, 0, 0, 20, 0, -1, 0)),
            "side": ref.view_mats(P, ref.look_at(-6, -2, 5, 3, 1, 12, 0, -1, 0)),
            "inside": ref.view_mats(P, ref.look_at(0.5, 1.58, 7.0, 0.8, 1.62, 10.0, 0, -1, 0))}


@pytest.fixture(scope="module")
def fused():
    from surfelmapping_amd import capi, synth
    seq = synth.make_sequence(CAM, synth.kitti_trajectory(3), seed=5)
    m = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=400))
    for fr in seq:
        m.process_frame(*fr)
    return m, m.download_model()


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["gui", "side", "inside"])
@pytest.mark.parametrize("points", [False, True])
def test_parity_with_restatement(fused, view, points):
    m, model = fused
    assert 0 < model.shape[0] < 40000
    w, h = 160, 120
    mvp, inv = _views(w, h)[view]
    keys = ref.splat(model, mvp, inv, w, h, threshold=0.5, unstable=False, points=points)
    for ct in range(4):
        for window in (False, True):
            kw = dict(color_type=ct, points=points, window=window, time=3, time_delta=1, clear=(5, 6, 7, 8))
            want = ref.resolve(model, keys, w, h, **kw)
            got = m.render_model(mvp, inv, w, h, threshold=0.5, unstable=False, depth=True, ids=True, **kw)
            for g, e, name in zip(got, want, ("rgba", "depth", "ids")):
                assert g.dtype == e.dtype and np.array_equal(g.view(np.uint8), e.view(np.uint8)), (view, points, ct, window, name)
    assert (keys != ref.EMPTY).mean() > (0.01 if points else 0.05)


@pytest.mark.gpu
def test_overflow_path_runs_on_the_close_view(fused):
    m, model = fused
    mvp, inv = _views(160, 120)["inside"]
    rgba, ids = m.render_model(mvp, inv, 160, 120, unstable=True, ids=True)
    n_ovf, _ = m.render_model_stats()
    assert n_ovf > 0
    counts = np.bincount(ids[ids >= 0].ravel())
    assert counts.max() > 1000                                      # one disc covers more than a thousand pixels
    want = ref.render_model(model, mvp, inv, 160, 120, unstable=True)
    assert np.array_equal(rgba, want[0]) and np.array_equal(ids, want[2])


# ---------------------------------------------------------------------------------------------------------------------
# no side effects
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_render_changes_nothing():
    """renders after every 3rd frame, synchronous and asynchronous frames: the model equals the run without renders, bit for
    bit, with the same live-surfel count.  (The forced compaction before a render resets only the deferred-compaction
    schedule's cull counter, as every read-back does; it moves no surfel.)"""
    from surfelmapping_amd import capi, synth
    cam = dict(width=128, height=96, fx=80.0, fy=80.0, cx=63.5, cy=47.5)
    seq = synth.make_sequence(cam, synth.kitti_trajectory(30), seed=9)
    mvp, inv = _views(96, 64)["gui"]

    def run(render_every, async_frames):
        m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=600))
        for k, fr in enumerate(seq):
            (m.process_frame_async if async_frames else m.process_frame)(*fr)
            if render_every and k % render_every == render_every - 1:
                m.render_model(mvp, inv, 96, 64, color_type=k % 4)
        m.sync()
        return m.download_model(), m.counts()["count"]

    base, n0 = run(0, False)
    for async_frames in (False, True):
        got, n = run(3, async_frames)
        assert n == n0 == base.shape[0]
        assert_models_equal(got, base, f"async={async_frames}")


@pytest.mark.gpu
def test_device_entry_point_into_torch_tensors(fused):
    import torch
    m, _ = fused
    mvp, inv = _views(160, 120)["side"]
    want = m.render_model(mvp, inv, 160, 120, color_type=3, depth=True, ids=True)
    rgba = torch.empty((120, 160, 4), dtype=torch.uint8, device="cuda")
    dep = torch.empty((120, 160), dtype=torch.float32, device="cuda")
    ids = torch.empty((120, 160), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.render_model_device(mvp, inv, 160, 120, rgba.data_ptr(), dep.data_ptr(), ids.data_ptr(), color_type=3)
    m.sync()
    assert np.array_equal(rgba.cpu().numpy(), want[0])
    assert np.array_equal(dep.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(ids.cpu().numpy(), want[2])


# ---------------------------------------------------------------------------------------------------------------------
# arguments (CPU: the library loads without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
def test_arguments_rejected_before_any_device_call():
    from surfelmapping_amd import capi
    L = capi.load()
    rgba = np.zeros(32 * 32 * 4, np.uint8)

    def call(v, ctx=None, out=rgba, fn="sm_render_model"):
        rc = getattr(L, fn)(ctx, None if v is None else C.byref(v), None if out is None else out.ctypes.data_as(C.c_void_p), None, None)
        return rc, L.sm_last_error().decode()

    ok = capi.model_view(O_MVP, O_INV, 32, 32)
    for fn in ("sm_render_model", "sm_render_model_device"):
        assert call(ok, fn=fn) == (capi.SM_E_ARG, f"{fn}: null context")
        assert call(None, fn=fn) == (capi.SM_E_ARG, f"{fn}: null view")
        assert call(ok, out=None, fn=fn) == (capi.SM_E_ARG, f"{fn}: null rgba")
        for w, h in ((0, 32), (32, -1), (1 << 15, 1 << 14)):
            rc, msg = call(capi.model_view(O_MVP, O_INV, w, h), fn=fn)
            assert rc == capi.SM_E_ARG and "width and height" in msg
        rc, msg = call(capi.model_view(O_MVP, O_INV, 32, 32, color_type=4), fn=fn)
        assert rc == capi.SM_E_ARG and "color_type" in msg
        rc, msg = call(capi.model_view(O_MVP, O_INV, 32, 32, color_type=-1), fn=fn)
        assert rc == capi.SM_E_ARG and "color_type" in msg
