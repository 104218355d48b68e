"""numpy restatement of the model view (GlobalModel::renderModel, src/GlobalModel.cpp:683-758) -- the checker of
tests/test_render_model.py.  It restates draw_surface.vert + draw_surface_adaptive.geom + draw_surface.frag (surfels) and
draw_feedback.vert/.frag (points) with the raster rules and the float32 expression order written down above the kernels in
surfelmapping_amd/csrc/sm_k_view.h: every float32 step below is one IEEE float32 operation there (no contraction), every
float64 step a double one, so the images agree byte for byte."""
import numpy as np

f32 = np.float32
SQRT2 = f32(1.41421356)
EMPTY = np.uint64(0x7FFFFFFFFFFFFFFF)
# src/GlobalModel.cpp:718-736
PALETTE = np.array([(128, 128, 128), (0, 255, 0), (0, 0, 255), (255, 255, 0), (128, 0, 0), (255, 0, 255), (128, 128, 0),
                    (0, 128, 0), (128, 0, 128), (0, 128, 128), (0, 255, 255), (0, 0, 128), (245, 222, 179), (255, 0, 0),
                    (210, 105, 30), (244, 164, 96), (119, 136, 153), (255, 20, 147), (138, 43, 226)], np.uint32)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(v):
    l = np.sqrt(_dot(v, v))
    return [v[0] / l, v[1] / l, v[2] / l]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _clip(m, x, y, z):
    return [((m[r] * x + m[r + 4] * y) + m[r + 8] * z) + m[r + 12] for r in range(4)]


def _vert(m, w, h, x, y, z):
    """clip-space divide -> (X, Y 24.8 fixed point int64, zw, iw, ok)"""
    c = _clip(m, x, y, z)
    with np.errstate(all="ignore"):
        xw = ((c[0] / c[3]) * f32(0.5) + f32(0.5)) * f32(w)
        yw = ((c[1] / c[3]) * f32(0.5) + f32(0.5)) * f32(h)
        zw = (c[2] / c[3]) * f32(0.5) + f32(0.5)
        iw = f32(1.0) / c[3]
        ok = (c[3] > 0) & (np.abs(xw) < f32(1e6)) & (np.abs(yw) < f32(1e6)) & np.isfinite(zw) & np.isfinite(iw)
        X = np.floor(np.where(ok, xw, 0).astype(np.float64) * 256.0 + 0.5).astype(np.int64)
        Y = np.floor(np.where(ok, yw, 0).astype(np.float64) * 256.0 + 0.5).astype(np.int64)
    return X, Y, zw, iw, ok


def _edge(a, b, px, py):
    return (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])


def _top_left(a, b):
    dx, dy = b[0] - a[0], b[1] - a[1]
    return (dy == 0 and dx > 0) or (dy < 0)


def _tri(v0, v1, v2):
    """raster_tri's set-up; a vertex is (X, Y, zw, iw, tx, ty) with Python ints for X, Y"""
    area = _edge(v0, v1, v2[0], v2[1])
    a, b, c = v0, v1, v2
    if area < 0:
        b, c, area = v2, v1, -area
    return a, b, c, area, (0 if _top_left(b, c) else -1, 0 if _top_left(c, a) else -1, 0 if _top_left(a, b) else -1)


def _raster(tri, px, py, k, keys, w):
    """the per-pixel function (view_px_tri) over arrays of pixel coordinates"""
    a, b, c, area, (ba, bb, bc) = tri
    if area == 0:
        return
    cx, cy = px * 256 + 128, py * 256 + 128
    e0, e1, e2 = _edge(b, c, cx, cy), _edge(c, a, cx, cy), _edge(a, b, cx, cy)
    m = (e0 + ba >= 0) & (e1 + bb >= 0) & (e2 + bc >= 0)
    if not m.any():
        return
    px, py, e0, e1, e2 = px[m], py[m], e0[m], e1[m], e2[m]
    l0 = (e0.astype(np.float64) / float(area)).astype(f32)
    l1 = (e1.astype(np.float64) / float(area)).astype(f32)
    l2 = (e2.astype(np.float64) / float(area)).astype(f32)
    wl0, wl1, wl2 = l0 * a[3], l1 * b[3], l2 * c[3]
    s = (wl0 + wl1) + wl2
    tx = ((wl0 * a[4] + wl1 * b[4]) + wl2 * c[4]) / s
    ty = ((wl0 * a[5] + wl1 * b[5]) + wl2 * c[5]) / s
    zw = (l0 * a[2] + l1 * b[2]) + l2 * c[2]
    keep = ~(tx * tx + ty * ty > f32(1.0)) & (zw >= f32(0.0)) & (zw <= f32(1.0))
    d24 = np.floor(zw[keep].astype(np.float64) * 16777215.0 + 0.5).astype(np.uint64)
    px, py = px[keep], py[keep]
    k24 = d24 < 16777215
    key = (d24[k24] << np.uint64(32)) | np.uint64(k)
    np.minimum.at(keys, py[k24] * w + px[k24], key)


def _disc_setup(m, pos, nrm, rad, mvinv, w, h):
    """draw_surface_adaptive.geom:94-128 for all surfels at once -> 4 vertices (X, Y, zw, iw, ok) each"""
    zl = ((m[2] * pos[0] + m[6] * pos[1]) + m[10] * pos[2]) + m[14]
    far = zl > f32(5.0)
    a = [mvinv[8], mvinv[9], mvinv[10]]
    with np.errstate(all="ignore"):
        uf = _normalize([a[1] - a[2], -a[0], a[0]])
        uf = [np.broadcast_to(u, pos[0].shape) for u in uf]
        xf = [(u * rad) * SQRT2 for u in uf]
        yf = _cross(a, xf)
        e = [pos[0] - mvinv[12], pos[1] - mvinv[13], pos[2] - mvinv[14]]
        cosang = _dot(e, nrm) / (np.sqrt(_dot(e, e)) * np.sqrt(_dot(nrm, nrm)))
        radius = rad / (f32(1.0) + f32(0.5) * np.abs(cosang))
        un = _normalize([nrm[1] - nrm[2], -nrm[0], nrm[0]])
        xn = [(u * radius) * SQRT2 for u in un]
        yn = _cross(nrm, xn)
    x = [np.where(far, xf[i], xn[i]) for i in range(3)]
    y = [np.where(far, yf[i], yn[i]) for i in range(3)]
    return [_vert(m, w, h, pos[0] + x[0], pos[1] + x[1], pos[2] + x[2]),
            _vert(m, w, h, pos[0] + y[0], pos[1] + y[1], pos[2] + y[2]),
            _vert(m, w, h, pos[0] - y[0], pos[1] - y[1], pos[2] - y[2]),
            _vert(m, w, h, pos[0] - x[0], pos[1] - x[1], pos[2] - x[2])]


def splat(model, mvp, mv_inv, w, h, threshold=0.0, unstable=True, points=False):
    """the key buffer (h*w uint64, EMPTY where nothing is drawn) of one view"""
    m = np.asarray(mvp, f32).reshape(16)
    mvinv = np.asarray(mv_inv, f32).reshape(16)
    model = np.asarray(model, f32).reshape(-1, 12)
    keys = np.full(w * h, EMPTY, np.uint64)
    conf = model[:, 3]
    pos = [model[:, 0], model[:, 1], model[:, 2]]
    if points:                                                  # draw_feedback.vert:38,80 + glPointSize(1)
        sel = conf > f32(threshold)
        c = _clip(m, *pos)
        with np.errstate(all="ignore"):
            ok = sel & (c[3] > 0)
            for q in range(3):
                ok &= (-c[3] <= c[q]) & (c[q] <= c[3])
            xw = ((c[0] / c[3]) * f32(0.5) + f32(0.5)) * f32(w)
            yw = ((c[1] / c[3]) * f32(0.5) + f32(0.5)) * f32(h)
            zw = (c[2] / c[3]) * f32(0.5) + f32(0.5)
            px = np.floor(np.where(ok, xw, -1)).astype(np.int64)
            py = np.floor(np.where(ok, yw, -1)).astype(np.int64)
            d24 = np.floor(np.where(ok, zw, 1).astype(np.float64) * 16777215.0 + 0.5).astype(np.uint64)
        ok &= (px >= 0) & (py >= 0) & (px < w) & (py < h) & (d24 < 16777215)
        ids = np.nonzero(ok)[0]
        np.minimum.at(keys, py[ok] * w + px[ok], (d24[ok] << np.uint64(32)) | ids.astype(np.uint64))
        return keys
    sel = (conf > f32(threshold)) | bool(unstable)
    nrm = [model[:, 8], model[:, 9], model[:, 10]]
    V = _disc_setup(m, pos, nrm, model[:, 11], mvinv, w, h)
    ok = sel & V[0][4] & V[1][4] & V[2][4] & V[3][4]
    tc = ((-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0), (1.0, 1.0))
    for k in np.nonzero(ok)[0]:
        vs = [(int(V[q][0][k]), int(V[q][1][k]), V[q][2][k], V[q][3][k], f32(tc[q][0]), f32(tc[q][1])) for q in range(4)]
        X = [v[0] for v in vs]
        Y = [v[1] for v in vs]
        x0, x1 = max((min(X) - 128) >> 8, 0), min((max(X) - 128) >> 8, w - 1)
        y0, y1 = max((min(Y) - 128) >> 8, 0), min((max(Y) - 128) >> 8, h - 1)
        if x0 > x1 or y0 > y1:
            continue
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        px, py = px.ravel().astype(np.int64), py.ravel().astype(np.int64)
        _raster(_tri(vs[0], vs[1], vs[2]), px, py, int(k), keys, w)      # triangle strip
        _raster(_tri(vs[2], vs[1], vs[3]), px, py, int(k), keys, w)
    return keys


def _u8(c):
    return np.floor(np.fmin(np.fmax(c, f32(0.0)), f32(1.0)) * f32(255.0) + f32(0.5)).astype(np.uint8)


def resolve(model, keys, w, h, color_type=0, points=False, window=False, time=0, time_delta=0, clear=(0, 0, 0, 0)):
    """key -> id -> colour: (rgba uint8[h][w][4], depth float32[h][w], ids int32[h][w])"""
    model = np.asarray(model, f32).reshape(-1, 12)
    hit = keys != EMPTY
    ids = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(f32) / f32(16777215.0), f32(1.0)).astype(f32)
    rgba = np.empty((w * h, 4), np.uint8)
    rgba[:] = np.array(clear, np.uint8)
    k = ids[hit]
    s = model[k]
    sc = s[:, 4].view(np.uint32)
    if color_type == 1:
        col = [s[:, 8], s[:, 9], s[:, 10]]
    elif color_type == 2:
        col = [((sc >> 16) & 0xFF).astype(f32) / f32(255.0), ((sc >> 8) & 0xFF).astype(f32) / f32(255.0),
               (sc & 0xFF).astype(f32) / f32(255.0)]
    elif color_type == 3:
        cls = sc >> 24
        pal = np.where((cls <= 18)[:, None], PALETTE[np.minimum(cls, 18)], 0).astype(np.uint32)
        col = [pal[:, i].astype(f32) / f32(255.0) for i in range(3)]
    else:
        v = f32(0.5) * np.abs((s[:, 8] + s[:, 9]) + s[:, 10]) + f32(0.1)
        col = [v, v, v]
    if window and not points:
        dim = f32(time) - s[:, 7] > f32(time_delta)
        col = [np.where(dim, c * f32(0.25), c) for c in col]
    out = np.stack([_u8(c) for c in col] + [np.full(len(k), 255, np.uint8)], axis=1)
    rgba[hit] = out
    return rgba.reshape(h, w, 4), depth.reshape(h, w), ids.reshape(h, w)


def render_model(model, mvp, mv_inv, w, h, threshold=0.0, color_type=0, unstable=True, points=False, window=False, time=0,
                 time_delta=0, clear=(0, 0, 0, 0)):
    keys = splat(model, mvp, mv_inv, w, h, threshold, unstable, points)
    return resolve(model, keys, w, h, color_type, points, window, time, time_delta, clear)


# ---- cameras (pangolin's ProjectionMatrix / ModelViewLookAt, double precision, returned as float32[16] column-major) ----
def projection(w, h, fu, fv, u0, v0, zn, zf):
    """pangolin::ProjectionMatrix (ProjectionMatrixRUB_BottomLeft)"""
    L, R = -u0 * zn / fu, (w - u0) * zn / fu
    T, B = v0 * zn / fv, -(h - v0) * zn / fv
    P = np.zeros((4, 4))
    P[0, 0] = 2 * zn / (R - L)
    P[1, 1] = 2 * zn / (T - B)
    P[0, 2] = (R + L) / (L - R)
    P[1, 2] = (T + B) / (B - T)
    P[2, 2] = (zf + zn) / (zn - zf)
    P[3, 2] = -1.0
    P[2, 3] = (2 * zf * zn) / (zn - zf)
    return P


def look_at(ex, ey, ez, lx, ly, lz, ux, uy, uz):
    """pangolin::ModelViewLookAt (eye, target, up)"""
    e, l, u = np.array([ex, ey, ez], float), np.array([lx, ly, lz], float), np.array([ux, uy, uz], float)
    z = e - l
    z /= np.linalg.norm(z)
    x = np.cross(u, z)
    y = np.cross(z, x)
    x /= np.linalg.norm(x)
    y /= np.linalg.norm(y)
    M = np.eye(4)
    M[0, :3], M[1, :3], M[2, :3] = x, y, z
    M[0, 3], M[1, 3], M[2, 3] = -x @ e, -y @ e, -z @ e
    return M


def view_mats(P, MV):
    """(mvp, mv_inv) as float32[16] column-major, computed in double as the reference's pangolin matrices are"""
    return (np.ascontiguousarray((P @ MV).T.reshape(16)).astype(f32),
            np.ascontiguousarray(np.linalg.inv(MV).T.reshape(16)).astype(f32))
