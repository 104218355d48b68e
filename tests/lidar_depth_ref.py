"""Lidar depth (include/sm_c_api.h "lidar depth") restated in numpy: the projection of a scan into the camera in
fp32, one rounding per operation in the order the header writes them, the z-buffer by (mm, index), and the chain of
morphological steps in integers on v = 65536 - mm (0 = empty).  Returns every intermediate plane, so a test can say which step
differs."""
import numpy as np

f32 = np.float32
MAX_POINTS = 1 << 24
DILATE, CLOSE, FILL_SMALL, EXTEND_TOP, FILL_LARGE, MEDIAN, SMOOTH = (1 << b for b in range(7))
STEPS = ("dilate", "close", "fill_small", "extend_top", "fill_large", "median", "smooth")
DEFAULT = dict(min_z=0.5, max_z=65.0, stages=127, large=31, tol_256=13)
B5 = (1, 4, 6, 4, 1)
DIAMOND = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if abs(dx) + abs(dy) <= 2]


def params(**over):
    p = dict(DEFAULT)
    for k, v in over.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def project(points, T, cam, min_z, max_z):
    """step 1: (sparse_mm uint16[H][W], index int32[H][W], landed = the points that reached the splat)"""
    W, H = int(cam["width"]), int(cam["height"])
    pts = np.ascontiguousarray(points, f32).reshape(-1, 4)
    T = np.asarray(T, f32).reshape(-1)[:12].reshape(3, 4)
    fx, fy, cx, cy = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    sparse, index = np.zeros((H, W), np.uint16), np.full((H, W), -1, np.int32)
    if not len(pts):
        return sparse, index, 0
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        X, Y, Z = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3))
        ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z >= f32(min_z)) & (Z <= f32(max_z))
        u, v = (fx * X) / Z + cx, (fy * Y) / Z + cy
        ok &= np.isfinite(u) & np.isfinite(v)
        ok &= (u >= f32(-0.5)) & (u < f32(W) - f32(0.5)) & (v >= f32(-0.5)) & (v < f32(H) - f32(0.5))
        px, py, mm = np.floor(u + f32(0.5)), np.floor(v + f32(0.5)), np.floor(Z * f32(1000.0) + f32(0.5))
    assert X.dtype == u.dtype == mm.dtype == f32
    ok &= (mm >= 1) & (mm <= 65535) & (px < W) & (py < H)
    i = np.nonzero(ok)[0]
    px, py, mm = px[i].astype(np.int64), py[i].astype(np.int64), mm[i].astype(np.int64)
    key = np.full(W * H, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(key, py * W + px, (mm << 32) | i)
    hit = key != np.iinfo(np.int64).max
    sparse.reshape(-1)[hit] = (key[hit] >> 32).astype(np.uint16)
    index.reshape(-1)[hit] = (key[hit] & 0xFFFFFFFF).astype(np.int32)
    return sparse, index, int(len(i))


def _shift(v, dx, dy, fill):
    """out[y][x] = v[y + dy][x + dx], `fill` where that tap lies outside the image"""
    H, W = v.shape
    out = np.full_like(v, fill)
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[yd, xd] = v[ys, xs]
    return out


def _window(v, taps, fill, op):
    out = None
    for dx, dy in taps:
        s = _shift(v, dx, dy, fill)
        out = s if out is None else op(out, s)
    return out


def _box(r):
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]


def dilate(v):
    return _window(v, DIAMOND, 0, np.maximum)


def close(v):
    return _window(_window(v, _box(2), 0, np.maximum), _box(2), 65536, np.minimum)


def fill_box(v, size):
    return np.where(v == 0, _window(v, _box(size // 2), 0, np.maximum), v)


def extend_top(v):
    H, W = v.shape
    has = v > 0
    top = np.where(has.any(axis=0), has.argmax(axis=0), H)
    rows = np.arange(H)[:, None]
    return np.where(rows < top[None, :], v[np.minimum(top, H - 1), np.arange(W)][None, :], v)


def median(v):
    taps = np.stack([_shift(v, dx, dy, 0) for dx, dy in _box(2)], axis=-1)
    n = (taps > 0).sum(axis=-1)
    taps = np.sort(taps, axis=-1)                                   # the empties first: the valid ones are the last n
    k = np.maximum(25 - n + (n - 1) // 2, 0)
    return np.where(v > 0, np.take_along_axis(taps, k[..., None], axis=-1)[..., 0], 0)


def smooth(v, tol_256):
    z0 = 65536 - v
    num, den = np.zeros(v.shape, np.int64), np.zeros(v.shape, np.int64)
    for dx, dy in _box(2):
        t = _shift(v, dx, dy, 0)
        z = 65536 - t
        layer = (t > 0) & (np.maximum(z, z0) * 256 <= np.minimum(z, z0) * (256 + tol_256))
        w = B5[dy + 2] * B5[dx + 2]
        num += np.where(layer, w * t, 0)
        den += np.where(layer, w, 0)
    return np.where(v > 0, (num + den // 2) // np.maximum(den, 1), 0)


def complete(sparse_mm, stages=127, large=31, tol_256=13):
    """step 2 on a sparse depth image: dict(v0, dilate, close, fill_small, extend_top, fill_large, median, smooth: the v plane
    after each step, int64; depth_mm uint16; stats)"""
    v = np.where(sparse_mm > 0, 65536 - sparse_mm.astype(np.int64), 0)
    out = dict(v0=v)
    fns = (dilate, close, lambda a: fill_box(a, 7), extend_top, lambda a: fill_box(a, large), median, lambda a: smooth(a, tol_256))
    filled = {}
    for b, (name, fn) in enumerate(zip(STEPS, fns)):
        if stages >> b & 1:
            nv = fn(v)
            filled[name] = int(((v == 0) & (nv > 0)).sum())
            v = nv
        else:
            filled[name] = 0
        out[name] = v
    out["depth_mm"] = np.where(v > 0, 65536 - v, 0).astype(np.uint16)
    out["stats"] = dict(measured=int((sparse_mm > 0).sum()), filled_small=filled["fill_small"], filled_top=filled["extend_top"],
                        filled_large=filled["fill_large"], left_empty=int((v == 0).sum()))
    return out


def lidar_depth(points, T, cam, **over):
    """The whole stage.  cam: dict(width, height, fx, fy, cx, cy).  Returns complete()'s dict with sparse_mm, index and the
    stats' points and landed added."""
    p = params(**over)
    sparse, index, landed = project(points, T, cam, p["min_z"], p["max_z"])
    out = complete(sparse, p["stages"], p["large"], p["tol_256"])
    out["sparse_mm"], out["index"] = sparse, index
    out["stats"].update(points=int(np.asarray(points).size // 4), landed=landed)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the analytic street of the tests and the probe: a ground plane, a wall and a box, scanned from beside the camera
# ---------------------------------------------------------------------------------------------------------------------
LIDAR_UP, LIDAR_BACK = 0.08, 0.27              # the lidar's origin in the camera frame (x right, y down, z ahead): (0, -up, -back)
CAM_HEIGHT = 1.65                              # the camera above the ground
WALL_Z, WALL_SLOPE = 20.0, 0.25                # the wall: z = WALL_Z + WALL_SLOPE * x, oblique so that its depth varies along a row
BOX = (-1.0, 1.0, 0.15, 1.65, 8.0)             # the box face's x0, x1, y0, y1 (y down) and z
STREET_CAM = dict(width=1242, height=375, fx=721.5, fy=721.5, cx=609.5, cy=172.85)   # the camera the quality is judged with
T_STREET = np.array([[1, 0, 0, 0], [0, 1, 0, -LIDAR_UP], [0, 0, 1, -LIDAR_BACK], [0, 0, 0, 1]], f32)


def _cast(o, d):
    """the first hit of the rays o + t d with the street, in camera coordinates: t (inf for none)"""
    with np.errstate(all="ignore"):
        t = np.where(d[:, 1] > 1e-9, (CAM_HEIGHT - o[1]) / d[:, 1], np.inf)                # ground y = CAM_HEIGHT
        den = d[:, 2] - WALL_SLOPE * d[:, 0]
        tw = np.where(den > 1e-9, (WALL_Z + WALL_SLOPE * o[0] - o[2]) / den, np.inf)
        t = np.minimum(t, tw)
        tb = np.where(d[:, 2] > 1e-9, (BOX[4] - o[2]) / d[:, 2], np.inf)
        hx, hy = o[0] + tb * d[:, 0], o[1] + tb * d[:, 1]
        tb = np.where((hx >= BOX[0]) & (hx <= BOX[1]) & (hy >= BOX[2]) & (hy <= BOX[3]), tb, np.inf)
    return np.minimum(t, tb)


def street_scan(rows=64, cols=1100, fov_h_deg=100.0, up_deg=3.0, down_deg=25.0):
    """the scan of the street by rows x cols beams: float32 [n][4] in the lidar frame (the camera frame moved by the offset)"""
    az = np.deg2rad(np.linspace(-fov_h_deg / 2, fov_h_deg / 2, cols))
    el = np.deg2rad(np.linspace(-up_deg, down_deg, rows))
    az, el = np.meshgrid(az, el)
    d = np.stack([np.sin(az) * np.cos(el), np.sin(el), np.cos(az) * np.cos(el)], axis=-1).reshape(-1, 3)
    o = np.array([0.0, -LIDAR_UP, -LIDAR_BACK])
    t = _cast(o, d)
    hit = np.isfinite(t)
    p = d[hit] * t[hit, None]                                                          # lidar frame: relative to its origin
    return np.concatenate([p, np.ones((len(p), 1))], axis=1).astype(f32)


def street_depth(cam):
    """the analytic depth (metres along z, 0 for none) of every pixel of the camera"""
    W, H = int(cam["width"]), int(cam["height"])
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones_like(u)], axis=-1).reshape(-1, 3)
    t = _cast(np.zeros(3), d)
    return np.where(np.isfinite(t), t, 0.0).reshape(H, W)


def street_quality(cam=None):
    """the whole stage on the street's scan against the analytic depth: dict(points, landed, measured, filled: fractions of the
    pixels; median, p90: relative error over the pixels that have both depths; out, true: the images)"""
    cam = STREET_CAM if cam is None else cam
    pts = street_scan()
    out, true = lidar_depth(pts, T_STREET, cam), street_depth(cam)
    depth = out["depth_mm"]
    judged = (true > 0) & (depth > 0)
    err = np.abs(depth[judged] / 1000.0 - true[judged]) / true[judged]
    return dict(points=len(pts), landed=out["stats"]["landed"], measured=float((out["sparse_mm"] > 0).mean()), filled=float((depth > 0).mean()),
                judged=float(judged.mean()), median=float(np.median(err)), p90=float(np.quantile(err, 0.9)), out=out, true=true)
