"""Views of a map set (sm_render_image_maps / sm_render_model_maps, SurfelMap.render_image_maps / render_model_maps; DESIGN.md
"4f. Views of a map set").  The definition: the streamed images equal, bit for bit, what the resident renderers give from a
context whose model is the concatenation of the set's sources.  CPU: the symbols, the methods, the struct layouts, the argument
rules that need no device, and the per-block view test restated in numpy against the per-surfel rules.  GPU: everything else."""
import ctypes as C
import os

import numpy as np
import pytest

import model_view_ref as ref
import retire_ref as rr
from backends import assert_models_equal

f32 = np.float32
CAM, OVER = rr.CAM, rr.OVER
IMG = (CAM["width"], CAM["height"], CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])
N_DRIVE = 45
# recorded on the CPU oracle (retire_ref.oracle_run(sequence(45), 0, True)): the four files of the drive and the model it ends with
DRIVE_FILES, DRIVE_LIVE = [24, 144, 4404, 25681], 110076
MW, MH = 160, 120
# ... and what image_views() / model_cams() show of their concatenation: covered pixels per novel view (oracle render_image);
# pixels per source (the four files, the live model) over the four model views in discs, threshold 0.5, unstable drawn
# (model_view_ref.splat)
IMAGE_COVERED = [23464, 23240, 22514, 21375, 10945, 29328, 0, 0]
MODEL_SOURCES = [15, 230, 589, 2218, 13000]


def write_map(path, rows, a=0, b=0):
    """a map file in GlobalModel::downloadMap's format"""
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 12)
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([a, b], np.int32).tobytes())
        f.write(rows.tobytes())
    return str(path)


def image_views():
    """along the drive, two looking back, one sideways, two that see nothing (above the map looking ahead; past its end)"""
    from surfelmapping_amd import synth
    P = synth.pose_matrix
    ps = [P(0, 0, 0.8 * 5), P(0, 0, 0.8 * 20, 3.0), P(0, 0, 0.8 * 40), P(0, 0, 0.8 * 44, 180.0), P(0.5, 0, 0.8 * 25, 175.0),
          P(0, 0, 0.8 * 30, 90.0), P(0, -400.0, 0, 0.0), P(0, 0, 400.0, 0.0)]
    return np.stack([synth.pose_to_colmajor(p) for p in ps])


def model_cams():
    """the GUI's camera behind and above the start (gui/GUI.cpp:46-47), one high above the middle of the drive looking down, one
    at the end looking back, and one that looks away from the map"""
    P = ref.projection(MW, MH, 420.0 * MW / 640, 420.0 * MH / 480, 320.0 * MW / 640, 240.0 * MH / 480, 0.1, 1000.0)
    mv = [ref.look_at(0, -6, -10, 0, 0, 20, 0, -1, 0), ref.look_at(0, -40, 18, 0, 0, 18.5, 0, 0, 1),
          ref.look_at(2, -3, 45, 0, 0, 0, 0, -1, 0), ref.look_at(0, -6, -10, 0, -6, -40, 0, -1, 0)]
    return [ref.view_mats(P, m) for m in mv]


def model_views(**kw):
    from surfelmapping_amd import capi
    return [capi.model_view(mvp, inv, MW, MH, **kw) for mvp, inv in model_cams()]


MODES = [dict(color_type=0), dict(color_type=1), dict(color_type=2), dict(color_type=3),
         dict(color_type=2, window=True, time=N_DRIVE, time_delta=20), dict(color_type=2, points=True),
         dict(color_type=0, threshold=5.0, unstable=False), dict(color_type=3, threshold=5.0, unstable=False, points=True)]


def _gpu(cap, **over):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=cap, **over))


def _env(**kv):
    """set / unset SM_RENDER_MAPS_* switches for the calls that follow (they are read per call)"""
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)


@pytest.fixture(autouse=True)
def _clean_env():
    _env(SM_RENDER_MAPS_NO_CULL=None, SM_RENDER_MAPS_KEY_MB=None)
    yield
    _env(SM_RENDER_MAPS_NO_CULL=None, SM_RENDER_MAPS_KEY_MB=None)


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def resident_image(big, views):
    out = [big.render_image(v, *IMG) for v in views]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def resident_model(big, kw):
    out = [big.render_model(mvp, inv, MW, MH, depth=True, ids=True, **kw) for mvp, inv in model_cams()]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ("sm_render_image_maps", "sm_render_model_maps", "sm_render_maps_stats"):
        assert getattr(L, name) is not None


def test_python_methods_exist():
    from surfelmapping_amd import capi
    for name in ("render_image_maps", "render_model_maps", "render_maps_stats"):
        assert callable(getattr(capi.SurfelMap, name))


def test_arguments_rejected_before_any_device_call():
    from surfelmapping_amd import capi
    L = capi.load()
    src = capi.map_source([])
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.sm_render_image_maps(None, C.byref(src), p, 1, 4, 4, 1.0, 1.0, 1.0, 1.0, p, p) == capi.SM_E_ARG
    assert "null context" in L.sm_last_error().decode()
    v = capi.model_view(np.eye(4), np.eye(4), 4, 4)
    assert L.sm_render_model_maps(None, C.byref(src), C.byref(v), 1, p, None, None) == capi.SM_E_ARG
    assert L.sm_render_maps_stats(None, None) == capi.SM_E_ARG


# --- the per-block view test (sm_k_render_maps.h: maps_box_outside_image / maps_box_outside_view) restated, fp32, same order ---
def _reach(rmax):
    return (f32(1.41421356) * rmax) * f32(1.0001)


def _corners(lo, hi):
    return [(hi[0] if c & 1 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 4 else lo[2]) for c in range(8)]


def _box_finite(lo, hi, *r):
    return bool(np.isfinite(np.asarray(lo, f32)).all() and np.isfinite(np.asarray(hi, f32)).all() and np.isfinite(np.asarray(r, f32)).all())


def block_box(rows):
    """k_maps_intake's box of one block: (lo, hi, rmax, rnorm); rnorm = the largest |r| * max(1, |n|), +inf when a centre, a
    radius or a normal of the block is not finite"""
    rows = np.asarray(rows, f32)
    with np.errstate(all="ignore"):
        ra = np.abs(rows[:, 11])
        nx, ny, nz = rows[:, 8], rows[:, 9], rows[:, 10]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        rn = ra * np.fmax(f32(1.0), ln)
        bad = not (np.isfinite(rows[:, 0:3]).all() and np.isfinite(ln).all() and np.isfinite(rn).all())
        return np.fmin.reduce(rows[:, 0:3]), np.fmax.reduce(rows[:, 0:3]), np.fmax.reduce(ra), f32(np.inf) if bad else np.fmax.reduce(rn)


def box_outside_image(lo, hi, rmax, t_inv, w, h, fx, fy, cx, cy):
    if not _box_finite(lo, hi, rmax):
        return False
    m = np.asarray(t_inv, f32)
    fx, fy, cx, cy, cols, rows = (f32(v) for v in (fx, fy, cx, cy, w, h))
    R = _reach(f32(rmax))
    mpx = f32(2.0) + f32(1.0e-4) * (abs(cx) + cols)
    mpy = f32(2.0) + f32(1.0e-4) * (abs(cy) + rows)
    cl, cr, ct, cb = cx + mpx, (cols + mpx) - cx, cy + mpy, (rows + mpy) - cy
    zmin, zmax, mag = f32(3.0e38), f32(-3.0e38), f32(0.0)
    fl = fr = ft = fb = f32(-3.0e38)
    al = ar = at = ab = f32(0.0)
    for x, y, z in _corners(lo, hi):
        x, y, z = f32(x), f32(y), f32(z)
        p = [((m[r] * x + m[r + 4] * y) + m[r + 8] * z) + m[r + 12] for r in range(3)]
        ax, ay, az = abs(x), abs(y), abs(z)
        mag = max(mag, max(((abs(m[r]) * ax + abs(m[r + 4]) * ay) + abs(m[r + 8]) * az) + abs(m[r + 12]) for r in range(3)))
        zmin, zmax = min(zmin, p[2]), max(zmax, p[2])
        fl = max(fl, fx * p[0] + cl * p[2]); al = max(al, abs(fx * p[0]) + abs(cl * p[2]))
        fr = max(fr, cr * p[2] - fx * p[0]); ar = max(ar, abs(fx * p[0]) + abs(cr * p[2]))
        ft = max(ft, fy * p[1] + ct * p[2]); at = max(at, abs(fy * p[1]) + abs(ct * p[2]))
        fb = max(fb, cb * p[2] - fy * p[1]); ab = max(ab, abs(fy * p[1]) + abs(cb * p[2]))
    E4 = f32(4.0e-6) * mag
    Rc = (R + E4) * f32(1.0001)
    if zmax + E4 < f32(1.0) or zmin - E4 > f32(200.0):
        return True
    gx = np.sqrt(fx * fx + max(cl * cl, cr * cr)) * f32(1.0001)
    gy = np.sqrt(fy * fy + max(ct * ct, cb * cb)) * f32(1.0001)
    return bool(fl + (gx * Rc + f32(4.0e-6) * al) < 0 or fr + (gx * Rc + f32(4.0e-6) * ar) < 0 or
                ft + (gy * Rc + f32(4.0e-6) * at) < 0 or fb + (gy * Rc + f32(4.0e-6) * ab) < 0)


def _clip_form(lo, hi, m, row, sgn, s, R):
    sgn, s = f32(sgn), f32(s)
    a = [sgn * m[row + 4 * j] + s * m[3 + 4 * j] for j in range(4)]
    q = [abs(m[row + 4 * j]) + s * abs(m[3 + 4 * j]) for j in range(4)]
    f, A = f32(-3.0e38), f32(0.0)
    for x, y, z in _corners(lo, hi):
        x, y, z = f32(x), f32(y), f32(z)
        f = max(f, ((a[0] * x + a[1] * y) + a[2] * z) + a[3])
        A = max(A, ((q[0] * abs(x) + q[1] * abs(y)) + q[2] * abs(z)) + q[3])
    g = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) * f32(1.0001)
    qn = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    return f + (g * R + f32(4.0e-6) * (A + qn * R))


def box_outside_view(lo, hi, rmax, rnorm, mvp, mv_inv, w, h):
    if not _box_finite(lo, hi, rmax, rnorm):
        return False
    m, inv = np.asarray(mvp, f32), np.asarray(mv_inv, f32)
    with np.errstate(all="ignore"):
        la = np.sqrt((inv[8] * inv[8] + inv[9] * inv[9]) + inv[10] * inv[10])
    if not np.isfinite(la):
        return False
    R = _reach(max(f32(rnorm), f32(rmax) * max(f32(1.0), la)))
    sx = f32(1.0) + f32(2.0) * (f32(2.0) + f32(1.0e-4) * f32(w)) / f32(w)
    sy = f32(1.0) + f32(2.0) * (f32(2.0) + f32(1.0e-4) * f32(h)) / f32(h)
    return bool(_clip_form(lo, hi, m, 3, 0.0, 1.0, R) < 0 or _clip_form(lo, hi, m, 0, 1.0, sx, R) < 0 or
                _clip_form(lo, hi, m, 0, -1.0, sx, R) < 0 or _clip_form(lo, hi, m, 1, 1.0, sy, R) < 0 or
                _clip_form(lo, hi, m, 1, -1.0, sy, R) < 0)


def image_accepts(rows, t_inv, w, h, fx, fy, cx, cy):
    """bool[n]: the records whose pixel box in the novel view is not empty -- render_surfel (sm_k_draw.h) up to raster_tri's
    loop bounds, fp32, the same order of operations"""
    m = np.asarray(t_inv, f32)
    fx, fy, cx, cy, cols, rows_ = (f32(v) for v in (fx, fy, cx, cy, w, h))
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    with np.errstate(all="ignore"):
        ph = [((m[r] * x + m[r + 4] * y) + m[r + 8] * z) + m[r + 12] for r in range(3)]
        ok = ~((ph[2] >= f32(200.0)) | (ph[2] <= f32(1.0)))
        nx, ny, nz = rows[:, 8], rows[:, 9], rows[:, 10]
        n = [(m[r] * nx + m[r + 4] * ny) + m[r + 8] * nz for r in range(3)]
        n = ref._normalize(n)
        r = rows[:, 11]
        S = f32(1.41421356)
        one, zero = np.ones_like(r), np.zeros_like(r)
        tn = [zero, zero, one]
        a = ref._normalize([tn[1] - tn[2], -tn[0], tn[0]])
        xf = [a[i] * r * S for i in range(3)]
        yf = ref._cross(tn, xf)
        cosang = ref._dot(ph, n) / (np.sqrt(ref._dot(ph, ph)) * np.sqrt(ref._dot(n, n)))
        radius = r / (f32(1.0) + f32(0.5) * np.abs(cosang))
        an = ref._normalize([n[1] - n[2], -n[0], n[0]])
        xn = [an[i] * radius * S for i in range(3)]
        yn = ref._cross(n, xn)
        far = ph[2] > f32(5.0)
        X_ = [np.where(far, xf[i], xn[i]) for i in range(3)]
        Y_ = [np.where(far, yf[i], yn[i]) for i in range(3)]
        Xs, Ys = [], []
        for sgn, vec in ((1, X_), (1, Y_), (-1, Y_), (-1, X_)):
            VX, VY, VZ = (ph[i] + (vec[i] if sgn > 0 else -vec[i]) for i in range(3))
            ok &= VZ > 0
            xnn = ((((fx * VX) / VZ) + cx) - (cols * f32(0.5))) / (cols * f32(0.5))
            ynn = ((((fy * VY) / VZ) + cy) - (rows_ * f32(0.5))) / (rows_ * f32(0.5))
            xw = (cols * f32(0.5)) * xnn + (cols * f32(0.5))
            yw = (rows_ * f32(0.5)) * ynn + (rows_ * f32(0.5))
            ok &= (np.abs(xw) < f32(1.0e6)) & (np.abs(yw) < f32(1.0e6))
            Xs.append(np.floor(np.where(ok, xw, 0).astype(np.float64) * 256.0 + 0.5).astype(np.int64))
            Ys.append(np.floor(np.where(ok, yw, 0).astype(np.float64) * 256.0 + 0.5).astype(np.int64))
    X, Y = np.stack(Xs), np.stack(Ys)
    x0, x1 = np.maximum((X.min(0) - 128) >> 8, 0), np.minimum((X.max(0) - 128) >> 8, w - 1)
    y0, y1 = np.maximum((Y.min(0) - 128) >> 8, 0), np.minimum((Y.max(0) - 128) >> 8, h - 1)
    return ok & (x0 <= x1) & (y0 <= y1)


def view_accepts(rows, mvp, mv_inv, w, h):
    """bool[n]: the records whose pixel box in the model view is not empty (view_disc), or whose point lands in the image"""
    m, inv = np.asarray(mvp, f32), np.asarray(mv_inv, f32)
    pos, nrm = [rows[:, 0], rows[:, 1], rows[:, 2]], [rows[:, 8], rows[:, 9], rows[:, 10]]
    V = ref._disc_setup(m, pos, nrm, rows[:, 11], inv, w, h)
    ok = V[0][4] & V[1][4] & V[2][4] & V[3][4]
    X, Y = np.stack([np.where(ok, V[q][0], 0) for q in range(4)]).astype(np.int64), np.stack([np.where(ok, V[q][1], 0) for q in range(4)]).astype(np.int64)
    x0, x1 = np.maximum((X.min(0) - 128) >> 8, 0), np.minimum((X.max(0) - 128) >> 8, w - 1)
    y0, y1 = np.maximum((Y.min(0) - 128) >> 8, 0), np.minimum((Y.max(0) - 128) >> 8, h - 1)
    disc = ok & (x0 <= x1) & (y0 <= y1)
    c = ref._clip(m, *pos)
    with np.errstate(all="ignore"):
        xw = ((c[0] / c[3]) * f32(0.5) + f32(0.5)) * f32(w)
        yw = ((c[1] / c[3]) * f32(0.5) + f32(0.5)) * f32(h)
        point = (c[3] > 0) & (np.floor(xw) >= 0) & (np.floor(xw) < w) & (np.floor(yw) >= 0) & (np.floor(yw) < h)
    return disc | point


def _random_blocks(rng, n_blocks, normal_scale=None):
    """blocks of 256 records clustered as a map's are: a centre anywhere around the views, a spread from centimetres to tens of
    metres, radii from millimetres to metres; unit normals, or normals of every length up to `normal_scale` (a map file is
    caller input, and the model view draws with the stored normal as it is)"""
    for _ in range(n_blocks):
        centre = rng.uniform(-120, 120, 3) * (1.0 if rng.random() < 0.8 else 0.05)
        spread = 10.0 ** rng.uniform(-2, 1.5)
        rows = np.zeros((256, 12), f32)
        rows[:, 0:3] = centre + rng.normal(0, spread, (256, 3))
        rows[:, 3] = 5.0
        nrm = rng.normal(0, 1, (256, 3))
        rows[:, 8:11] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
        if normal_scale:
            rows[:, 8:11] *= rng.uniform(0.1, normal_scale, (256, 1)).astype(f32)
        rows[:, 11] = 10.0 ** rng.uniform(-3, 0.3, 256)
        yield rows


def _scaled_inv(inv, k):
    """a model view's mv_inv with column 2 (the far discs' axis) k times as long: not rigid, and the caller's to give"""
    inv = np.array(inv, f32)
    with np.errstate(invalid="ignore"):
        inv[8:11] *= f32(k)
    return inv


def test_box_test_is_conservative():
    """no record the per-surfel rules accept lies in a block the box test rejects -- random blocks against the tests' own views
    and random ones; and the test does reject (it is not vacuous)"""
    from surfelmapping_amd import synth
    rng = np.random.default_rng(20250)
    w, h, fx, fy, cx, cy = IMG
    poses = [ol_inv(v) for v in image_views()]
    cams = model_cams()
    for _ in range(6):
        p = synth.pose_matrix(*rng.uniform(-60, 60, 3), rng.uniform(-180, 180))
        poses.append(ol_inv(synth.pose_to_colmajor(p)))
        e, l = rng.uniform(-60, 60, 3), rng.uniform(-60, 60, 3)
        P = ref.projection(MW, MH, 100.0, 100.0, MW / 2, MH / 2, 0.1, 1000.0)
        cams.append(ref.view_mats(P, ref.look_at(*e, *l, 0, -1, 0)))
    # ... and what the model view does not normalise: mv_inv column 2 of other lengths, normals of other lengths
    cams += [(mvp, _scaled_inv(inv, k)) for (mvp, inv), k in zip(cams[:8], (3.0, 0.3, 8.0, 3.0, 2.0, 5.0, 3.0, 1.5))]
    rej_i = rej_v = acc_i = acc_v = 0
    import itertools
    for rows in itertools.chain(_random_blocks(rng, 150), _random_blocks(rng, 100, normal_scale=4.0)):
        lo, hi, rmax, rnorm = block_box(rows)
        assert np.isfinite(rnorm) and rnorm >= rmax
        for t_inv in poses:
            acc = image_accepts(rows, t_inv, w, h, fx, fy, cx, cy)
            out = box_outside_image(lo, hi, rmax, t_inv, w, h, fx, fy, cx, cy)
            assert not (out and acc.any()), (lo, hi, rmax, t_inv)
            rej_i += out; acc_i += bool(acc.any())
        for mvp, inv in cams:
            acc = view_accepts(rows, mvp, inv, MW, MH)
            out = box_outside_view(lo, hi, rmax, rnorm, mvp, inv, MW, MH)
            assert not (out and acc.any()), (lo, hi, rmax, rnorm, mvp, inv)
            rej_v += out; acc_v += bool(acc.any())
    print(f"novel view: {rej_i} rejected, {acc_i} with a drawn record; model view: {rej_v} rejected, {acc_v} with a drawn record")
    assert rej_i > 200 and rej_v > 200 and acc_i > 50 and acc_v > 50
    # a non-finite bound is never rejected
    t_inv = poses[6]
    far_lo, far_hi = np.array([0, 0, -900], f32), np.array([1, 1, -800], f32)
    assert box_outside_image(far_lo, far_hi, 0.1, t_inv, w, h, fx, fy, cx, cy)
    vlo, vhi = np.array([0, 0, 800], f32), np.array([1, 1, 900], f32)        # behind the camera that looks away from the map
    assert box_outside_view(vlo, vhi, 0.1, 0.1, *cams[3], MW, MH)
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(3):
            lo2, hi2 = far_lo.copy(), far_hi.copy()
            (lo2 if bad != np.inf else hi2)[i] = bad
            assert not box_outside_image(lo2, hi2, 0.1, t_inv, w, h, fx, fy, cx, cy)
            lo2, hi2 = vlo.copy(), vhi.copy()
            (lo2 if bad != np.inf else hi2)[i] = bad
            assert not box_outside_view(lo2, hi2, 0.1, 0.1, *cams[3], MW, MH)
        assert not box_outside_image(far_lo, far_hi, abs(bad), t_inv, w, h, fx, fy, cx, cy)
        assert not box_outside_view(vlo, vhi, abs(bad), 0.1, *cams[3], MW, MH)
        assert not box_outside_view(vlo, vhi, 0.1, abs(bad), *cams[3], MW, MH)
        assert not box_outside_view(vlo, vhi, 0.1, 0.1, cams[3][0], _scaled_inv(cams[3][1], bad), MW, MH)
    # a record with a non-finite normal marks its block (the model view draws with it)
    rows = next(_random_blocks(rng, 1))
    for col, bad in ((8, np.nan), (9, np.inf), (10, 3.0e38), (0, np.nan), (11, np.inf)):
        r2 = rows.copy()
        r2[5, col] = bad
        assert block_box(r2)[3] == np.inf, (col, bad)


def ol_inv(view16):
    """world->camera of a column-major camera->world pose, fp32 (what sm_render_image* computes from `view16`; any inverse
    does for the restatement: both tests see the same matrix)"""
    return np.linalg.inv(np.asarray(view16, np.float64).reshape(4, 4).T).T.reshape(16).astype(f32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the definition, on a drive
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drive(tmp_path_factory):
    """the drive with periodic retirement: (context, map files, their records, live model, concatenation, a context that holds
    the concatenation)"""
    d = tmp_path_factory.mktemp("drive")
    g = _gpu(rr.CAPACITY[0])
    g.set_auto_retire(rr.EVERY, str(d / "m"), min_age=rr.MIN_AGE, min_distance=rr.MIN_DISTANCE)
    for fr in rr.sequence(N_DRIVE):
        g.process_frame(*fr)
    nfiles, _ = g.auto_retire_stats()
    paths = [str(d / f"m_{i:06d}.bin") for i in range(nfiles)]
    files = [rr.read_map(p)[0] for p in paths]
    live = g.download_model()
    assert [len(f) for f in files] == DRIVE_FILES and len(live) == DRIVE_LIVE
    concat = np.concatenate(files + [live])
    big = _gpu(400)
    big.upload_model(concat)
    return g, paths, files, live, concat, big


def _sources(ids, edges):
    """how many pixels of an id plane each source of the set owns"""
    v = ids[ids >= 0]
    return np.bincount(np.searchsorted(edges, v, side="right") - 1, minlength=len(edges) - 1)


@pytest.mark.gpu
def test_definition_novel_view(drive):
    import oracle_lib as ol
    g, paths, files, live, concat, big = drive
    views = image_views()
    bgr, sem = g.render_image_maps(paths, views, *IMG)
    want = resident_image(big, views)
    same(bgr, want[0], "bgr")
    same(sem, want[1], "sem")
    o = ol.Oracle(ol.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=400))
    o.upload_model(concat)
    for k, v in enumerate(views):
        ob, os_ = o.render_image(v, *IMG)
        same(bgr[k], ob, f"oracle bgr {k}")
        same(sem[k], os_, f"oracle sem {k}")
    covered = [(int((s > 0).sum())) for s in sem]
    print("covered pixels per view", covered)
    assert covered == IMAGE_COVERED                              # two views see nothing, the others a street


@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(len(MODES)))
def test_definition_model_view(drive, mode):
    g, paths, files, live, concat, big = drive
    kw = dict(threshold=0.5, unstable=True, clear=(5, 6, 7, 8))
    kw.update(MODES[mode])
    got = g.render_model_maps(paths, model_views(**kw), depth=True, ids=True)
    want = resident_model(big, kw)
    for a, b, name in zip(got, want, ("rgba", "depth", "ids")):
        same(a, b, (MODES[mode], name))
    edges = np.cumsum([0] + DRIVE_FILES + [DRIVE_LIVE])
    per = _sources(got[2], edges)
    print(MODES[mode], "pixels per source", per.tolist(), "per view", [int((i >= 0).sum()) for i in got[2]])
    assert (got[2][3] == -1).all() and (got[0][3] == (5, 6, 7, 8)).all() and (got[1][3] == 1.0).all()   # the view that looks away
    if mode == 0:
        assert per.tolist() == MODEL_SOURCES and (per > 0).sum() >= 3     # the compared views show every source of the set


# ---------------------------------------------------------------------------------------------------------------------
# 2. larger than the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_larger_than_the_context(drive):
    from surfelmapping_amd import capi
    g, paths, files, live, concat, big = drive
    small = _gpu(100)                                            # 10 000 slots: below the largest file, far below the set
    assert 100 * 100 < max(DRIVE_FILES) < sum(DRIVE_FILES)
    with pytest.raises(capi.SurfelMapError) as e:
        small.load_map(paths[3])
    assert e.value.rc == capi.SM_E_CAPACITY
    only_files = np.concatenate(files)
    big2 = _gpu(400)
    big2.upload_model(only_files)
    views = image_views()
    for inc in (False, True):                                    # (the small context's own model is empty)
        bgr, sem = small.render_image_maps(paths, views, *IMG, include_model=inc)
        want = resident_image(big2, views)
        same(bgr, want[0], "bgr")
        same(sem, want[1], "sem")
    kw = dict(threshold=0.5, unstable=True, color_type=2)
    got = small.render_model_maps(paths, model_views(**kw), depth=True, ids=True)
    for a, b, name in zip(got, resident_model(big2, kw), ("rgba", "depth", "ids")):
        same(a, b, name)
    assert (got[2] >= 0).sum() > 1000


# ---------------------------------------------------------------------------------------------------------------------
# 3. chunking and batching
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded_set(tmp_path_factory):
    """three files: more than one chunk plus a partial one (record counts that are multiples of neither 256 nor 64), no
    records at all, and a small one"""
    from surfelmapping_amd import synth
    d = tmp_path_factory.mktemp("seeded")
    n0, n2 = (1 << 20) + 70001, 12345
    rows = synth.seeded_model(n0 + n2, 50, seed=4)
    paths = [write_map(d / "a.bin", rows[:n0]), write_map(d / "empty.bin", rows[:0]), write_map(d / "c.bin", rows[n0:])]
    return paths, rows


def _seeded_views():
    from surfelmapping_amd import synth
    P = synth.pose_matrix
    return np.stack([synth.pose_to_colmajor(p) for p in
                     (P(0, 0, 0), P(10, 0, 100, 40.0), P(-20, 1, 200, 180.0), P(0, 0, 120, -90.0), P(0, -300, 0), P(5, 0, 50, 10.0), P(0, 0, 180, 170.0))])


@pytest.mark.gpu
def test_chunking_and_batching(seeded_set):
    paths, rows = seeded_set
    from surfelmapping_amd import capi
    g = _gpu(10)
    big = capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=1100))
    big.upload_model(rows)
    views = _seeded_views()
    bgr, sem = g.render_image_maps(paths, views, *IMG, include_model=False)
    st = g.render_maps_stats()
    print("one pass:", st)
    assert st["passes"] == 1 and st["chunks"] == 3 and st["surfels_read"] == len(rows)
    want = resident_image(big, views)
    same(bgr, want[0], "bgr")
    same(sem, want[1], "sem")
    assert (sem > 0).sum() > 10000
    # a key budget of 1 MiB holds 4 views of 312 x 94: 7 views take 2 passes ... and 3 at 640 x 480 (one view each)
    _env(SM_RENDER_MAPS_KEY_MB=1)
    b2, s2 = g.render_image_maps(paths, views, *IMG, include_model=False)
    st = g.render_maps_stats()
    assert st["passes"] == 2 and st["chunks"] == 6 and st["surfels_read"] == 2 * len(rows)
    same(b2, bgr, "bgr, two passes")
    same(s2, sem, "sem, two passes")
    cams = model_cams()[:3]
    kw = dict(threshold=0.5, unstable=True, color_type=2)
    mv = [capi.model_view(mvp, inv, 640, 480, **kw) for mvp, inv in cams]
    three = g.render_model_maps(paths, mv, include_model=False, depth=True, ids=True)
    st = g.render_maps_stats()
    print("three passes:", st)
    assert st["passes"] == 3 and st["chunks"] == 9
    _env(SM_RENDER_MAPS_KEY_MB=None)
    one = g.render_model_maps(paths, mv, include_model=False, depth=True, ids=True)
    assert g.render_maps_stats()["passes"] == 1
    for a, b, name in zip(three, one, ("rgba", "depth", "ids")):
        same(a, b, name)
    for k, (mvp, inv) in enumerate(cams):
        w3 = big.render_model(mvp, inv, 640, 480, depth=True, ids=True, **kw)
        for a, b, name in zip(one, w3, ("rgba", "depth", "ids")):
            same(a[k], b, (k, name))
    assert (one[2] >= (1 << 20)).sum() > 0 and (one[2] >= 0).sum() > 10000     # rows of the second chunk and the last file are seen


# ---------------------------------------------------------------------------------------------------------------------
# 4. culling
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_culling_changes_nothing_and_skips(drive, seeded_set):
    g, paths, files, live, concat, big = drive
    views = image_views()
    mv = model_views(threshold=0.5, unstable=True, color_type=2)
    mvp_ = model_views(threshold=0.5, unstable=True, color_type=2, points=True)
    on = {}
    for cull in (True, False):
        _env(SM_RENDER_MAPS_NO_CULL=None if cull else 1)
        res = {}
        res["image"] = g.render_image_maps(paths, views, *IMG)
        st_i = g.render_maps_stats()
        res["discs"] = g.render_model_maps(paths, mv, depth=True, ids=True)
        st_d = g.render_maps_stats()
        res["points"] = g.render_model_maps(paths, mvp_, depth=True, ids=True)
        res["seeded"] = g.render_image_maps(seeded_set[0], _seeded_views(), *IMG, include_model=False)
        st_s = g.render_maps_stats()
        res["seeded discs"] = g.render_model_maps(seeded_set[0], mv, include_model=False, depth=True, ids=True)
        print("cull", cull, "drive image", st_i, "drive discs", st_d, "seeded", st_s)
        blocks = sum((n + 255) // 256 for n in DRIVE_FILES)
        if cull:
            on = res
            assert st_i["pairs_tested"] == blocks * len(views) and 0 < st_i["pairs_skipped"] < st_i["pairs_tested"]
            assert st_d["pairs_tested"] == blocks * len(mv) and 0 < st_d["pairs_skipped"] < st_d["pairs_tested"]
            assert 0 < st_s["pairs_skipped"] < st_s["pairs_tested"]
        else:
            assert st_i["pairs_tested"] == 0 and st_i["pairs_skipped"] == 0 and st_d["pairs_skipped"] == 0 and st_s["pairs_skipped"] == 0
            for k in res:
                for a, b in zip(res[k], on[k]):
                    same(a, b, k)


@pytest.mark.gpu
def test_culling_with_normals_and_view_axes_of_any_length(tmp_path):
    """the model view draws with the stored normal and with mv_inv column 2 as they are: a file whose normals are up to 4 times
    the unit length, views whose mv_inv column 2 is up to 8 times it -- blocks are still skipped, and the images equal those
    without the box test and those of the resident renderer"""
    from surfelmapping_amd import capi
    rng = np.random.default_rng(77)
    near = []
    for rows in _random_blocks(rng, 250, normal_scale=4.0):      # around the cameras, discs of 0.3 .. 0.7 m: many blocks at a view's edge
        rows[:, 0:3] = (rows[:, 0:3] - rows[:, 0:3].mean(0)) * f32(0.05) + rng.uniform(-30, 30, 3).astype(f32) + np.array([0, -5, 15], f32)
        rows[:, 11] = rng.uniform(0.3, 0.7, 256).astype(f32)
        near.append(rows)
    rows = np.concatenate(list(_random_blocks(rng, 150, normal_scale=4.0)) + near)
    rows[:, 4] = rng.integers(0, 1 << 24, len(rows), dtype=np.uint32).view(f32)
    path = write_map(tmp_path / "long_normals.bin", rows)
    g, big = _gpu(10), _gpu(330)
    big.upload_model(rows)
    kw = dict(threshold=0.5, unstable=True, color_type=2)
    cams = model_cams()
    cams = cams + [(mvp, _scaled_inv(inv, k)) for (mvp, inv), k in zip(cams, (3.0, 0.3, 8.0, 3.0))]
    mv = [capi.model_view(mvp, inv, MW, MH, **kw) for mvp, inv in cams]
    on = g.render_model_maps([path], mv, include_model=False, depth=True, ids=True)
    st = g.render_maps_stats()
    print("normals and axes of any length:", st)
    assert st["pairs_tested"] == 400 * len(mv) and 0 < st["pairs_skipped"] < st["pairs_tested"]
    _env(SM_RENDER_MAPS_NO_CULL=1)
    off = g.render_model_maps([path], mv, include_model=False, depth=True, ids=True)
    for a, b, name in zip(on, off, ("rgba", "depth", "ids")):
        same(a, b, name)
    for k, (mvp, inv) in enumerate(cams):
        want = big.render_model(mvp, inv, MW, MH, depth=True, ids=True, **kw)
        for a, b, name in zip(on, want, ("rgba", "depth", "ids")):
            same(a[k], b, (k, name))
    assert all((on[2][k] >= 0).sum() > 500 for k in (0, 1, 2, 4, 5, 6))


@pytest.mark.gpu
def test_block_with_a_nan_is_tested_and_never_skipped(tmp_path):
    from surfelmapping_amd import synth
    g = _gpu(10)
    rows = synth.seeded_model(256, 5, seed=1)
    rows[:, 0:3] = (0.0, 0.0, -500.0)                            # far behind every view below
    rows[:, 0:3] += np.random.default_rng(1).uniform(-1, 1, (256, 3)).astype(f32)
    views = image_views()[:3]
    mv = model_views()[:1]
    clean = write_map(tmp_path / "clean.bin", rows)
    g.render_image_maps([clean], views, *IMG, include_model=False)
    st = g.render_maps_stats()
    assert (st["pairs_tested"], st["pairs_skipped"]) == (3, 3)
    g.render_model_maps([clean], mv, include_model=False)
    st = g.render_maps_stats()
    assert (st["pairs_tested"], st["pairs_skipped"]) == (1, 1)
    for col, bad in ((0, np.nan), (1, np.inf), (2, -np.inf), (11, np.nan), (11, np.inf), (8, np.nan), (9, np.inf), (10, 3.0e38)):
        r2 = rows.copy()
        r2[77, col] = bad
        p = write_map(tmp_path / "bad.bin", r2)
        bgr, sem = g.render_image_maps([p], views, *IMG, include_model=False)
        st = g.render_maps_stats()
        assert (st["pairs_tested"], st["pairs_skipped"]) == (3, 0), (col, bad, st)
        assert not sem.any()
        g.render_model_maps([p], mv, include_model=False)
        st = g.render_maps_stats()
        assert (st["pairs_tested"], st["pairs_skipped"]) == (1, 0), (col, bad, st)


# ---------------------------------------------------------------------------------------------------------------------
# 5. ties and order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_go_to_the_first_source(tmp_path):
    from test_render_model import O_INV, O_MVP, surfel
    from surfelmapping_amd import capi
    g = _gpu(10)
    a = write_map(tmp_path / "a.bin", [surfel(16.0, 16.0, 0.0, 7.5, rgb=(200, 10, 10))])
    b = write_map(tmp_path / "b.bin", [surfel(16.0, 16.0, 0.0, 7.5, rgb=(10, 200, 10))])
    v = [capi.model_view(O_MVP, O_INV, 32, 32, color_type=2)]
    rgba, ids = g.render_model_maps([a, b], v, include_model=False, ids=True)
    assert (ids[0] == 0).sum() == 80 and (ids[0] == 1).sum() == 0
    assert (rgba[0][ids[0] == 0] == (200, 10, 10, 255)).all()
    rgba, ids = g.render_model_maps([b, a], v, include_model=False, ids=True)
    assert (ids[0] == 0).sum() == 80 and (ids[0] == 1).sum() == 0
    assert (rgba[0][ids[0] == 0] == (10, 200, 10, 255)).all()
    # the same with the live model as the later source, and in the novel view (class + 1 tells the sources apart)
    g.upload_model(np.stack([surfel(16.0, 16.0, 0.0, 7.5, rgb=(10, 10, 200))]))
    rgba, ids = g.render_model_maps([b], v, ids=True)
    assert (ids[0] == 0).sum() == 80 and (rgba[0][ids[0] == 0] == (10, 200, 10, 255)).all()
    fa = write_map(tmp_path / "fa.bin", [surfel(0.0, 0.0, 10.0, 0.5, n=(0.0, 0.0, -1.0), sem=4, rgb=(1, 2, 3))])
    fb = write_map(tmp_path / "fb.bin", [surfel(0.0, 0.0, 10.0, 0.5, n=(0.0, 0.0, -1.0), sem=9, rgb=(4, 5, 6))])
    eye = np.eye(4, dtype=f32).reshape(1, 16)
    bgr, sem = g.render_image_maps([fa, fb], eye, *IMG, include_model=False)
    assert (sem[0] == 5).sum() > 50 and (sem[0] == 10).sum() == 0 and (bgr[0][sem[0] == 5] == (3, 2, 1)).all()
    bgr, sem = g.render_image_maps([fb, fa], eye, *IMG, include_model=False)
    assert (sem[0] == 10).sum() > 50 and (sem[0] == 5).sum() == 0 and (bgr[0][sem[0] == 10] == (6, 5, 4)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. invariance
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_streamed_renders_change_nothing(drive):
    """streamed renders after every 3rd frame, synchronous and asynchronous frames: model, counts, frame log and the frames that
    follow equal the run without them, bit for bit; and two identical calls give identical bytes"""
    from surfelmapping_amd import capi, synth
    _, paths, *_ = drive
    cam = dict(width=128, height=96, fx=80.0, fy=80.0, cx=63.5, cy=47.5)
    seq = synth.make_sequence(cam, synth.kitti_trajectory(30), seed=9)
    views = image_views()[:3]
    mv = model_views(color_type=2)[:2]

    def run(render_every, async_frames):
        m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=600))
        for k, fr in enumerate(seq):
            (m.process_frame_async if async_frames else m.process_frame)(*fr)
            if render_every and k % render_every == render_every - 1:
                if k % 2:
                    m.render_image_maps(paths[2:], views, *IMG)
                else:
                    m.render_model_maps(paths[2:], mv)
        m.sync()
        return m.download_model(), m.counts(), m.read_frame_log()

    base, c0, log0 = run(0, False)
    for async_frames in (False, True):
        got, c, log = run(3, async_frames)
        assert c == c0 and c["count"] == base.shape[0]
        assert_models_equal(got, base, f"async={async_frames}")
        for name in ("tick", "n_before", "n_after_cull", "n_kill", "conflict_count", "visible_count", "fused_count"):
            assert np.array_equal(log[name], log0[name]), (async_frames, name)
    g = drive[0]
    a = g.render_image_maps(paths, image_views(), *IMG)
    b = g.render_image_maps(paths, image_views(), *IMG)
    same(a[0], b[0], "bgr twice")
    same(a[1], b[1], "sem twice")
    a = g.render_model_maps(paths, model_views(), depth=True, ids=True)
    b = g.render_model_maps(paths, model_views(), depth=True, ids=True)
    for x, y in zip(a, b):
        same(x, y, "model view twice")


@pytest.mark.gpu
@pytest.mark.parametrize("rgb_term", [False, True])
def test_streamed_renders_leave_the_tracker_alone(drive, rgb_term):
    """tracked frames with no guess (the constant-velocity guess is the tracker's state), streamed renders before every track
    and between the track and its frame: poses, track infos and the model equal the run without the renders, bit for bit"""
    from surfelmapping_amd import capi, synth
    _, paths, *_ = drive
    cam = dict(width=320, height=120, fx=180.0, fy=180.0, cx=159.5, cy=59.5)
    seq = synth.make_sequence(cam, synth.kitti_trajectory(9), seed=4)
    views = image_views()[:2]
    mv = model_views(color_type=2)[:2]

    def run(render):
        m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, stereo_border=20.0, max_sqrt_vertices=500))
        out = []
        for k, (rgb, d, s, p16) in enumerate(seq):
            if render:
                m.render_image_maps(paths[2:], views, *IMG)
            if k < 2:
                m.process_frame(rgb, d, s, p16)
                continue
            pose, info = m.track_rgb(rgb, d) if rgb_term else m.track(d)
            if render:
                m.render_model_maps(paths[2:], mv, depth=True)
            m.process_frame(rgb, d, s, capi._mat16(pose))
            out.append((pose, info))
        return out, m.download_model(), m.counts()

    base, model0, c0 = run(False)
    got, model, c = run(True)
    print("track status:", [i["status"] for _, i in base])
    assert c == c0
    assert_models_equal(model, model0, "tracked run")
    for (p0, i0), (p1, i1) in zip(base, got):
        same(np.asarray(p0), np.asarray(p1), "pose")
        assert i0.keys() == i1.keys()
        for key in i0:
            x, y = np.asarray(i0[key]), np.asarray(i1[key])
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), key


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors and degenerate sets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_degenerate_sets(drive):
    g, paths, files, live, concat, big = drive
    views = image_views()[:4]
    bgr, sem = g.render_image_maps([], views, *IMG, include_model=True)
    for k, v in enumerate(views):
        wb, ws = g.render_image(v, *IMG)
        same(bgr[k], wb, "model alone, bgr")
        same(sem[k], ws, "model alone, sem")
    kw = dict(threshold=0.5, unstable=True, color_type=1, clear=(9, 8, 7, 6))
    got = g.render_model_maps([], model_views(**kw), depth=True, ids=True)
    for k, (mvp, inv) in enumerate(model_cams()):
        want = g.render_model(mvp, inv, MW, MH, depth=True, ids=True, **kw)
        for a, b in zip(got, want):
            same(a[k], b, "model alone")
    bgr, sem = g.render_image_maps([], views, *IMG, include_model=False)
    assert not bgr.any() and not sem.any()
    rgba, d, ids = g.render_model_maps([], model_views(**kw), include_model=False, depth=True, ids=True)
    assert (rgba == (9, 8, 7, 6)).all() and (d == 1.0).all() and (ids == -1).all()


@pytest.mark.gpu
def test_errors_leave_the_outputs_alone(drive, tmp_path):
    from surfelmapping_amd import capi
    g, paths, files, live, concat, big = drive
    L = g._L
    views = image_views()[:2]
    V = len(views)
    w, h = IMG[0], IMG[1]
    bgr, sem = np.full((V, h, w, 3), 0xA5, np.uint8), np.full((V, h, w), 0x5A, np.uint8)
    rgba, dep, ids = np.full((V, MH, MW, 4), 0xA5, np.uint8), np.full((V, MH, MW), 7.0, f32), np.full((V, MH, MW), 77, np.int32)
    mvs = (capi.SmModelView * V)(*model_views()[:V])
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def image(ctx, ps, views=views, n=V, out=(bgr, sem), inc=1, wh=(w, h)):
        src = capi.map_source(ps, inc)
        rc = L.sm_render_image_maps(ctx._h, C.byref(src), vp(views), n, wh[0], wh[1], *IMG[2:], vp(out[0]), vp(out[1]))
        return rc, L.sm_last_error().decode()

    def model(ctx, ps, views=mvs, n=V, out=rgba, inc=1):
        src = capi.map_source(ps, inc)
        rc = L.sm_render_model_maps(ctx._h, C.byref(src), views, n, vp(out), vp(dep), vp(ids))
        return rc, L.sm_last_error().decode()

    def untouched():
        return ((bgr == 0xA5).all() and (sem == 0x5A).all() and (rgba == 0xA5).all() and (dep == 7.0).all() and (ids == 77).all())

    missing = str(tmp_path / "nowhere.bin")
    short = str(tmp_path / "short.bin")
    with open(short, "wb") as f:
        f.write(open(paths[2], "rb").read()[:-48])                # one record fewer than the header says
    long_ = str(tmp_path / "long.bin")
    with open(long_, "wb") as f:
        f.write(open(paths[2], "rb").read() + b"\0" * 48)
    stub = str(tmp_path / "stub.bin")
    with open(stub, "wb") as f:
        f.write(b"\1\0\0\0")                                      # no whole header
    for bad in (missing, short, long_, stub):
        for ps in ([bad], [paths[0], paths[1], bad]):             # all headers are checked before anything is drawn
            for call in (image, model):
                rc, msg = call(g, ps)
                assert rc == capi.SM_E_ARG and os.path.basename(bad) in msg, (bad, msg)
                assert untouched()
    # the size limit: headers that add up to more than 2^31 - 1 (sparse files: only their length is looked at before)
    huge = []
    for k in range(2):
        p = str(tmp_path / f"huge{k}.bin")
        with open(p, "wb") as f:
            f.write(np.array([1 << 30, 0, 0], np.uint32).tobytes())
            f.truncate(12 + 48 * (1 << 30))
        huge.append(p)
    for call in (image, model):
        rc, msg = call(g, huge)
        assert rc == capi.SM_E_CAPACITY and "2^31" in msg and untouched()
    # null arguments with n_views > 0, mixed sizes, refused views
    assert image(g, paths, views=None)[0] == capi.SM_E_ARG and image(g, paths, out=(None, sem))[0] == capi.SM_E_ARG
    assert image(g, paths, out=(bgr, None))[0] == capi.SM_E_ARG and image(g, paths, wh=(0, h))[0] == capi.SM_E_ARG
    assert model(g, paths, views=None)[0] == capi.SM_E_ARG and model(g, paths, out=None)[0] == capi.SM_E_ARG
    mixed = (capi.SmModelView * 2)(*model_views()[:2])
    mixed[1].width = MW - 1
    rc, msg = model(g, paths, views=mixed)
    assert rc == capi.SM_E_ARG and "one width x height" in msg
    mixed[1].width, mixed[1].color_type = MW, 4
    rc, msg = model(g, paths, views=mixed)
    assert rc == capi.SM_E_ARG and "color_type" in msg
    src = capi.SmMapSource(None, 2, 1)
    assert L.sm_render_image_maps(g._h, C.byref(src), vp(views), V, w, h, *IMG[2:], vp(bgr), vp(sem)) == capi.SM_E_ARG
    assert L.sm_render_image_maps(g._h, None, vp(views), V, w, h, *IMG[2:], vp(bgr), vp(sem)) == capi.SM_E_ARG
    assert untouched()
    # n_views == 0 checks the set and draws nothing
    assert image(g, paths, views=None, n=0, out=(None, None))[0] == capi.SM_OK
    assert image(g, [missing], views=None, n=0, out=(None, None))[0] == capi.SM_E_ARG
    # between sm_stage_conflict and sm_stage_cull
    seq = rr.sequence(2)
    st = _gpu(200)
    for fr in seq:
        st.process_frame(*fr)
    st.stage_conflict(seq[1][3], 1.0, 30.0)
    for call in (image, model):
        rc, msg = call(st, paths[:1])
        assert rc == capi.SM_E_ARG and "sm_stage_conflict" in msg and untouched()
    st.stage_cull()
    assert image(st, paths[:1])[0] == capi.SM_OK
    bgr[:], sem[:] = 0xA5, 0x5A
    # a sharded context
    sh = _gpu(200)
    sh.shard_stream_configure(0, 1)
    for call in (image, model):
        rc, msg = call(sh, paths[:1])
        assert rc == capi.SM_E_UNSUPPORTED and "sharded" in msg and untouched()
    # the stats of a context that has made no call
    fresh = _gpu(10)
    with pytest.raises(capi.SurfelMapError):
        fresh.render_maps_stats()
