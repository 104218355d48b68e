"""numpy restatement of the stereo rules of include/sm_c_api.h ("stereo depth", rules 1-7): luminance, census, matching cost,
path costs, winner, sub-pixel, depth.  All integers up to the final division; vectorised over paths and disparities.  The GPU
tests compare every stage with it bit for bit; test_stereo.py checks it against a scalar loop written straight from the rules."""
from __future__ import annotations

import numpy as np

DEFAULT = dict(max_disp=128, paths=8, p1=7, p2=86, uniqueness=5, lr_max_diff=1, baseline=0.54)
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))
BIG = 1 << 20


def params(**over) -> dict:
    p = dict(DEFAULT)
    for k, v in over.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def luminance(rgb) -> np.ndarray:
    c = np.asarray(rgb, np.uint8).astype(np.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def census(Y) -> np.ndarray:
    Y = np.asarray(Y, np.uint8)
    H, W = Y.shape
    pad = np.pad(Y, ((3, 3), (4, 4)), mode="edge")
    code = np.zeros((H, W), np.uint64)
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dx == 0 and dy == 0:
                continue
            nb = pad[3 + dy:3 + dy + H, 4 + dx:4 + dx + W]
            code = (code << np.uint64(1)) | (nb < Y).astype(np.uint64)
    return code


def _popcount64(v) -> np.ndarray:
    b = np.ascontiguousarray(v, np.uint64).view(np.uint8).reshape(v.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(axis=-1).astype(np.int32)


def cost_volume(cl, cr, D) -> np.ndarray:
    """C[y][x][d], int32"""
    H, W = cl.shape
    C = np.full((H, W, D), 64, np.int32)
    for d in range(min(D, W)):
        C[:, d:, d] = _popcount64(cl[:, d:] ^ cr[:, :W - d])
    return C


def _step(Cp, prev, p1, p2):
    """one step of rule 4 for a set of pixels: Cp and prev are [n][D]"""
    m = prev.min(axis=1, keepdims=True)
    lo = np.full_like(prev, BIG)
    hi = np.full_like(prev, BIG)
    lo[:, 1:] = prev[:, :-1] + p1
    hi[:, :-1] = prev[:, 1:] + p1
    return Cp + np.minimum(np.minimum(prev, lo), np.minimum(hi, m + p2)) - m


def path_cost(C, r, p1, p2) -> np.ndarray:
    """L_r[y][x][d] of direction r = (dx, dy), int32"""
    H, W, D = C.shape
    dx, dy = r
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    x = np.arange(W)
    inside = (x - dx >= 0) & (x - dx < W)
    for i, y in enumerate(ys):
        if i == 0:
            L[y] = C[y]
            continue
        prev = L[y - dy][np.clip(x - dx, 0, W - 1)]
        L[y] = np.where(inside[:, None], _step(C[y], prev, p1, p2), C[y])
    return L


def aggregate(C, p) -> np.ndarray:
    """S[y][x][d], uint16"""
    S = np.zeros(C.shape, np.int32)
    for r in DIRECTIONS[:p["paths"]]:
        S += path_cost(C, r, p["p1"], p["p2"])
    assert S.max() <= 8 * (64 + 1023)                          # L <= C + p2 in every direction
    return S.astype(np.uint16)


def select(S, p) -> np.ndarray:
    """disp16[y][x], uint16 (rules 5 and 6)"""
    H, W, D = S.shape
    S = S.astype(np.int32)
    d = np.arange(D)
    x = np.arange(W)
    dstar = S.argmin(axis=2)                                   # the lowest d with the least S
    smin = np.take_along_axis(S, dstar[..., None], axis=2)[..., 0]
    # right view: S(xr + d, y, d) over the d with xr + d < W
    src = x[:, None] + d[None, :]
    SR = np.where((src < W)[None], S[:, np.minimum(src, W - 1), d[None, :]], BIG)
    dR = SR.argmin(axis=2)
    far = np.abs(d[None, None, :] - dstar[..., None]) > 1
    m2 = np.where(far, S, BIG).min(axis=2)
    unique = ~(m2 * (100 - p["uniqueness"]) < smin * 100)
    xr = x[None, :] - dstar
    lr = np.abs(np.take_along_axis(dR, np.clip(xr, 0, W - 1), axis=1) - dstar) <= p["lr_max_diff"]
    valid = (dstar >= 1) & (xr >= 0) & unique & lr
    q = 16 * dstar
    inner = (dstar >= 1) & (dstar <= D - 2)
    a = np.take_along_axis(S, np.clip(dstar - 1, 0, D - 1)[..., None], axis=2)[..., 0] - smin
    b = np.take_along_axis(S, np.clip(dstar + 1, 0, D - 1)[..., None], axis=2)[..., 0] - smin
    den = a + b
    sub = 16 * dstar - 8 + (32 * a + den) // np.maximum(2 * den, 1)
    q = np.where(inner & (den > 0), sub, q)
    return np.where(valid, q, 0).astype(np.uint16)


def depth_scale(fx, baseline) -> float:
    """K of rule 7: fx and baseline are the floats the library holds"""
    return (float(np.float32(fx)) * float(np.float32(baseline))) * 16000.0


def depth_of(disp16, fx, baseline) -> np.ndarray:
    q = disp16.astype(np.float64)
    with np.errstate(divide="ignore"):
        mm = np.floor(depth_scale(fx, baseline) / q + 0.5)
    return np.where((disp16 > 0) & (mm <= 65535), mm, 0).astype(np.uint16)


def stereo(rgb_left, rgb_right, fx, **over) -> dict:
    """every stage: census_left, census_right (uint64[H][W]), volume (uint16[H][W][D]), disp16, depth_mm (uint16[H][W])"""
    p = params(**over)
    cl, cr = census(luminance(rgb_left)), census(luminance(rgb_right))
    S = aggregate(cost_volume(cl, cr, p["max_disp"]), p)
    disp16 = select(S, p)
    return dict(census_left=cl, census_right=cr, volume=S, disp16=disp16, depth_mm=depth_of(disp16, fx, p["baseline"]))
