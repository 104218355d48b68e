"""numpy restatement of the blended novel view (sm_render_image_blend; include/sm_c_api.h "blended views", DESIGN.md "4o. Blended
views") -- the checker of tests/test_blend.py.  The fragments are restated from render_surfel / raster_tri
(surfelmapping_amd/csrc/sm_k_draw.h): every float32 step below is one IEEE float32 operation there (no contraction), every float64
step a double one, every edge function an exact integer, so keys, sums and images agree bit for bit.  Steps 1-3 of the definition
are integer arithmetic on those fragments."""
import numpy as np

import model_view_ref as mv

f32 = np.float32
EMPTY = mv.EMPTY
DEFAULTS = dict(depth_tol_256=13, falloff=2)
MAX_DEPTH = f32(200.0)                                              # src/GlobalModel.cpp:797
TEX = ((-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0), (1.0, 1.0))


def _vertices(rows, t_inv, w, h, fx, fy, cx, cy):
    """render_surfel up to the four vertices, for all rows at once: ok[n], X[4][n], Y[4][n] (24.8 fixed point), ZW[4][n]"""
    m = np.asarray(t_inv, f32).reshape(16)
    fx, fy, cx, cy, cols, rows_ = (f32(v) for v in (fx, fy, cx, cy, w, h))
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    with np.errstate(all="ignore"):
        ph = [((m[r] * x + m[r + 4] * y) + m[r + 8] * z) + m[r + 12] for r in range(3)]
        ok = ~((ph[2] >= MAX_DEPTH) | (ph[2] <= f32(1.0)))
        nx, ny, nz = rows[:, 8], rows[:, 9], rows[:, 10]
        n = mv._normalize([(m[r] * nx + m[r + 4] * ny) + m[r + 8] * nz for r in range(3)])
        r = rows[:, 11]
        S = mv.SQRT2
        one, zero = np.ones_like(r), np.zeros_like(r)
        tn = [zero, zero, one]
        a = mv._normalize([tn[1] - tn[2], -tn[0], tn[0]])
        xf = [a[i] * r * S for i in range(3)]
        yf = mv._cross(tn, xf)
        cosang = mv._dot(ph, n) / (np.sqrt(mv._dot(ph, ph)) * np.sqrt(mv._dot(n, n)))
        radius = r / (f32(1.0) + f32(0.5) * np.abs(cosang))
        an = mv._normalize([n[1] - n[2], -n[0], n[0]])
        xn = [an[i] * radius * S for i in range(3)]
        yn = mv._cross(n, xn)
        far = ph[2] > f32(5.0)
        X_ = [np.where(far, xf[i], xn[i]) for i in range(3)]
        Y_ = [np.where(far, yf[i], yn[i]) for i in range(3)]
        Xs, Ys, ZWs = [], [], []
        for sgn, vec in ((1, X_), (1, Y_), (-1, Y_), (-1, X_)):
            VX, VY, VZ = (ph[i] + (vec[i] if sgn > 0 else -vec[i]) for i in range(3))
            ok &= VZ > 0
            xnn = ((((fx * VX) / VZ) + cx) - (cols * f32(0.5))) / (cols * f32(0.5))
            ynn = ((((fy * VY) / VZ) + cy) - (rows_ * f32(0.5))) / (rows_ * f32(0.5))
            zn = (f32(2.0) * VZ / MAX_DEPTH) - f32(1.0)
            xw = (cols * f32(0.5)) * xnn + (cols * f32(0.5))
            yw = (rows_ * f32(0.5)) * ynn + (rows_ * f32(0.5))
            ok &= (np.abs(xw) < f32(1.0e6)) & (np.abs(yw) < f32(1.0e6))
            Xs.append(np.floor(np.where(ok, xw, 0).astype(np.float64) * 256.0 + 0.5).astype(np.int64))
            Ys.append(np.floor(np.where(ok, yw, 0).astype(np.float64) * 256.0 + 0.5).astype(np.int64))
            ZWs.append(f32(0.5) * zn + f32(0.5))
    return ok, Xs, Ys, ZWs


def _tri_frags(tri, px, py, w):
    """raster_tri's pixel loop over arrays of pixel coordinates: (p, d24, q) of the accepted ones; a vertex is (X, Y, zw, tx, ty)"""
    a, b, c, area, (ba, bb, bc) = tri
    none = (np.zeros(0, np.int64), np.zeros(0, np.uint64), np.zeros(0, f32))
    if area == 0:
        return none
    cx, cy = px * 256 + 128, py * 256 + 128
    e0, e1, e2 = mv._edge(b, c, cx, cy), mv._edge(c, a, cx, cy), mv._edge(a, b, cx, cy)
    m = (e0 + ba >= 0) & (e1 + bb >= 0) & (e2 + bc >= 0)
    if not m.any():
        return none
    px, py, e0, e1, e2 = px[m], py[m], e0[m], e1[m], e2[m]
    l0 = (e0.astype(np.float64) / float(area)).astype(f32)
    l1 = (e1.astype(np.float64) / float(area)).astype(f32)
    l2 = (e2.astype(np.float64) / float(area)).astype(f32)
    tx = (l0 * a[3] + l1 * b[3]) + l2 * c[3]
    ty = (l0 * a[4] + l1 * b[4]) + l2 * c[4]
    q = tx * tx + ty * ty
    zw = (l0 * a[2] + l1 * b[2]) + l2 * c[2]
    keep = ~(q > f32(1.0)) & (zw >= f32(0.0)) & (zw <= f32(1.0))
    d24 = np.floor(np.where(keep, zw, 0).astype(np.float64) * 16777215.0 + 0.5).astype(np.uint64)
    keep &= d24 < 16777215
    return (py[keep] * w + px[keep]), d24[keep], q[keep].astype(f32)


def fragments(rows, t_inv, w, h, fx, fy, cx, cy):
    """every fragment of one view: dict of arrays p (pixel, y * w + x), d24, q (float32), k (row of `rows`).  t_inv: the inverse of
    the camera->world pose as the library computes it (oracle_lib.invert4)"""
    rows = np.asarray(rows, f32).reshape(-1, 12)
    ok, Xs, Ys, ZWs = _vertices(rows, t_inv, w, h, fx, fy, cx, cy)
    P, D, Q, K = [], [], [], []
    for k in np.nonzero(ok)[0]:
        vs = [(int(Xs[i][k]), int(Ys[i][k]), ZWs[i][k], f32(TEX[i][0]), f32(TEX[i][1])) for i in range(4)]
        X, Y = [v[0] for v in vs], [v[1] for v in vs]
        x0, x1 = max((min(X) - 128) >> 8, 0), min((max(X) - 128) >> 8, w - 1)
        y0, y1 = max((min(Y) - 128) >> 8, 0), min((max(Y) - 128) >> 8, h - 1)
        if x0 > x1 or y0 > y1:
            continue
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        px, py = px.ravel().astype(np.int64), py.ravel().astype(np.int64)
        for tri in (mv._tri(vs[0], vs[1], vs[2]), mv._tri(vs[2], vs[1], vs[3])):      # triangle strip
            p, d, q = _tri_frags(tri, px, py, w)
            P.append(p); D.append(d); Q.append(q); K.append(np.full(len(p), k, np.int64))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return dict(p=cat(P, np.int64), d24=cat(D, np.uint64), q=cat(Q, f32), k=cat(K, np.int64))


def weight(q, falloff):
    """step 2's weight of float32 q in 0..1: 1..256"""
    i = np.minimum(255, (np.asarray(q, f32) * f32(256.0)).astype(np.int32)).astype(np.int64)
    u = 256 - i
    return np.full_like(u, 256) if falloff == 0 else u if falloff == 1 else (u * u + 255) >> 8


def normalise(sw, sc):
    """step 3 on uint64 sums: (sc + sw / 2) / sw by floor division where sw > 0, 0 elsewhere"""
    sw, sc = np.asarray(sw, np.uint64), np.asarray(sc, np.uint64)
    safe = np.maximum(sw, np.uint64(1))
    return np.where(sw > 0, (sc + sw // np.uint64(2)) // safe, np.uint64(0)).astype(np.uint8)


def blend(frags, rows, w, h, params=None):
    """steps 1-3 over the fragments of one view -> dict: keys uint64[h*w], sums uint64[h*w][4] (SW, SB, SG, SR), bgr (blended),
    nearest (the plain view's bgr), sem uint8, contributors int64[h][w], stats (drawn, contributions, changed)"""
    p_ = dict(DEFAULTS, **(params or {}))
    tol, falloff = p_["depth_tol_256"], p_["falloff"]
    rows = np.asarray(rows, f32).reshape(-1, 12)
    sc = np.ascontiguousarray(rows[:, 4]).view(np.uint32)
    npix = w * h
    p, d24, q, k = frags["p"], frags["d24"], frags["q"], frags["k"]
    keys = np.full(npix, EMPTY, np.uint64)
    np.minimum.at(keys, p, (d24 << np.uint64(32)) | k.astype(np.uint64))
    hit = keys != EMPTY
    front = keys >> np.uint64(32)
    inside = d24 * np.uint64(256) <= front[p] * np.uint64(256 + tol)
    pc, kc = p[inside], k[inside]
    wt = weight(q[inside], falloff).astype(np.uint64)
    sums = np.zeros((npix, 4), np.uint64)
    np.add.at(sums[:, 0], pc, wt)
    for c in range(3):
        np.add.at(sums[:, c + 1], pc, wt * ((sc[kc] >> np.uint32(8 * c)) & np.uint32(0xFF)).astype(np.uint64))
    win = sc[(keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    nearest = np.zeros((npix, 3), np.uint8)
    nearest[hit] = np.stack([(win >> np.uint32(8 * c)) & np.uint32(0xFF) for c in range(3)], axis=1).astype(np.uint8)
    sem = np.zeros(npix, np.uint8)
    sem[hit] = (((win >> np.uint32(24)) & np.uint32(0xFF)) + np.uint32(1)).astype(np.uint8)
    bgr = np.zeros((npix, 3), np.uint8)
    for c in range(3):
        bgr[:, c] = np.where(hit, normalise(sums[:, 0], sums[:, c + 1]), 0)
    drawn = sem != 0
    stats = dict(drawn=int(drawn.sum()), contributions=int(inside.sum()), changed=int((drawn & np.any(bgr != nearest, axis=1)).sum()))
    return dict(keys=keys, sums=sums, bgr=bgr.reshape(h, w, 3), nearest=nearest.reshape(h, w, 3), sem=sem.reshape(h, w),
                contributors=np.bincount(pc, minlength=npix).reshape(h, w), stats=stats)


def render(rows, t_inv, w, h, fx, fy, cx, cy, params=None):
    return blend(fragments(rows, t_inv, w, h, fx, fy, cx, cy), rows, w, h, params)
