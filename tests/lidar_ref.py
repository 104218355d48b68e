"""Lidar sweeps restated in numpy (include/sm_c_api.h "lidar sweeps"; DESIGN.md "4k. Lidar sweeps"): brute force, every beam against
every row, in the header's fp32 expressions; and the footprint filter of sm_k_lidar.h, which the kernels put in front of the exact
test.  The sweep takes the direction table as an input, so a bit-for-bit comparison does not depend on two maths libraries agreeing."""
import numpy as np

import track_ref as tr

f32 = np.float32
PI = 3.14159265358979323846
KEY_EMPTY = np.uint64(0x7FFFFFFFFFFFFFFF)
# sm_k_lidar.h
R_REL, R_ABS, SLACK_RAD, HUGE, RAD2DEG = f32(1.0001), f32(1.0e-5), f32(1.0e-4), f32(1.0e18), f32(57.29577951308232)


def sensor(n_az=360, n_el=16, az0=0.0, step=1.0, el=None, min_range=1.0, max_range=60.0, min_conf=0.0):
    el = np.arange(-15, 1, dtype=f32) if el is None else np.ascontiguousarray(el, f32)
    assert len(el) == n_el
    return dict(n_az=int(n_az), n_el=int(n_el), az0=f32(az0), step=f32(step), el=el, min_range=f32(min_range), max_range=f32(max_range),
                min_conf=f32(min_conf))


def directions(sn):
    """the table by numpy's own sin / cos: n_el x n_az x 3 float32"""
    a = (np.float64(sn["az0"]) + np.arange(sn["n_az"], dtype=np.float64) * np.float64(sn["step"])) * PI / 180.0
    e = sn["el"].astype(np.float64) * PI / 180.0
    d = np.empty((sn["n_el"], sn["n_az"], 3), np.float64)
    d[:, :, 0] = np.sin(a)[None, :] * np.cos(e)[:, None]
    d[:, :, 1] = -np.sin(e)[:, None]
    d[:, :, 2] = np.cos(a)[None, :] * np.cos(e)[:, None]
    return d.astype(f32)


def tinv_of(pose16):
    """[R^T | -R^T t] in double, rounded to float (sm_old_in_view's)"""
    return tr.rigid_inv_d(np.asarray(pose16, f32)).astype(f32)


def surfels(model, pose16):
    """c, m, r of every row in the sensor frame (track_ref._xform / _rot over arrays)"""
    m = np.ascontiguousarray(model, f32)
    t = tinv_of(pose16)
    with np.errstate(all="ignore"):
        c = np.stack(tr._xform(t, m[:, 0], m[:, 1], m[:, 2]), axis=1)
        n = np.stack(tr._rot(t, m[:, 8], m[:, 9], m[:, 10]), axis=1)
    return c.astype(f32), n.astype(f32), m[:, 11].copy()


def hits(c, m, r, sn, dirs):
    """the exact rule: (rows, beams) bool and t, for surfels (c, m, r) against the table"""
    d = np.ascontiguousarray(dirs, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        num = (m[:, 0] * c[:, 0] + m[:, 1] * c[:, 1]) + m[:, 2] * c[:, 2]
        den = (m[:, 0, None] * d[None, :, 0] + m[:, 1, None] * d[None, :, 1]) + m[:, 2, None] * d[None, :, 2]
        t = num[:, None] / den
        qx, qy, qz = t * d[None, :, 0] - c[:, 0, None], t * d[None, :, 1] - c[:, 1, None], t * d[None, :, 2] - c[:, 2, None]
        qq = (qx * qx + qy * qy) + qz * qz
        hit = (t >= sn["min_range"]) & (t <= sn["max_range"]) & (qq <= (r * r)[:, None])
    assert t.dtype == f32 and qq.dtype == f32
    return hit, t


def sweep(model, pose16, sn, dirs, chunk=2048):
    """the four planes of one sweep: range (n_el, n_az) float32, id int32, rgb (.., 3) uint8, sem uint8"""
    model = np.ascontiguousarray(model, f32)
    c, m, r = surfels(model, pose16)
    with np.errstate(invalid="ignore"):
        live = model[:, 3] >= sn["min_conf"]
    nb = sn["n_el"] * sn["n_az"]
    best = np.full(nb, KEY_EMPTY, np.uint64)
    for k0 in range(0, len(model), chunk):
        k1 = min(len(model), k0 + chunk)
        hit, t = hits(c[k0:k1], m[k0:k1], r[k0:k1], sn, dirs)
        hit &= live[k0:k1, None]
        key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(k0, k1, dtype=np.uint64)[:, None]
        best = np.minimum(best, np.where(hit, key, KEY_EMPTY).min(axis=0))
    won = best != KEY_EMPTY
    ids = np.where(won, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    rng = np.where(won, (best >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(f32)
    col = np.where(won, model[:, 4].view(np.uint32)[np.maximum(ids, 0)], 0).astype(np.uint32) if len(model) else np.zeros(nb, np.uint32)
    rgb = np.stack([(col >> 16) & 0xFF, (col >> 8) & 0xFF, col & 0xFF], axis=1).astype(np.uint8)
    sem = np.where(won, ((col >> 24) & 0xFF) + 1, 0).astype(np.uint8)
    shape = (sn["n_el"], sn["n_az"])
    return dict(range=rng.reshape(shape), id=ids.reshape(shape), rgb=rgb.reshape(shape + (3,)), sem=sem.reshape(shape))


def _col_lo(x, n):
    c = np.ceil(x)
    return np.where(c > 0, np.where(c < n, c, n), 0).astype(np.int64)


def _col_hi(x, n):
    f = np.floor(x)
    return np.where(f >= 0, np.where(f < n - 1, f, n - 1), -1).astype(np.int64)


def footprint(c, r, sn):
    """sm_k_lidar.h lidar_footprint over arrays: (rows, n_el) and (rows, n_az) bool masks; a beam is inside iff both are set"""
    c = np.ascontiguousarray(c, f32)
    n_el, n_az = sn["n_el"], sn["n_az"]
    N = len(c)
    with np.errstate(all="ignore"):
        ra = np.abs(np.asarray(r, f32))
        nan = np.isnan(c).any(axis=1) | np.isnan(ra)
        huge = ~((np.abs(c) <= HUGE).all(axis=1) & (ra <= HUGE))
        D = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        R = ra * R_REL + R_ABS * D
        out = (D - R > sn["max_range"]) | (D + R < sn["min_range"])
        whole = ~(R / D < f32(1.0))
        rho = np.sqrt(c[:, 0] * c[:, 0] + c[:, 2] * c[:, 2])
        ec = np.arctan2(-c[:, 1], rho)
        al = np.arcsin(R / D) + SLACK_RAD
        el = (sn["el"].astype(np.float64) * PI / 180.0).astype(f32)
        i0 = np.searchsorted(el, ec - al, side="left")
        i1 = np.searchsorted(el, ec + al, side="right")
        pole = ~(R / rho < f32(1.0))
        w = (np.arcsin(R / rho) + SLACK_RAD) * RAD2DEG
        u0 = np.fmod(np.float64(sn["az0"]) + 180.0, 360.0)
        u0 = f32((u0 + 360.0 if u0 < 0 else u0) - 180.0)
        u = np.arctan2(c[:, 0], c[:, 2]) * RAD2DEG - u0
        u = np.where(u < 0, u + f32(360.0), u)
        sh = np.where(u + w >= f32(360.0), f32(-360.0), f32(360.0))
        step = sn["step"]
        a0, a1 = _col_lo((u - w) / step, n_az), _col_hi((u + w) / step, n_az)
        b0, b1 = _col_lo(((u - w) + sh) / step, n_az), _col_hi(((u + w) + sh) / step, n_az)
        assert u.dtype == f32 and w.dtype == f32 and al.dtype == f32
    ri, ci = np.arange(n_el)[None, :], np.arange(n_az)[None, :]
    rows = (ri >= i0[:, None]) & (ri < i1[:, None])
    cols = ((ci >= a0[:, None]) & (ci <= a1[:, None])) | ((ci >= b0[:, None]) & (ci <= b1[:, None]))
    cols |= pole[:, None]
    every = (huge | whole) & ~nan
    rows |= every[:, None]
    cols |= every[:, None]
    none = nan | (out & ~huge)
    rows &= ~none[:, None]
    cols &= ~none[:, None]
    assert rows.shape == (N, n_el) and cols.shape == (N, n_az)
    return rows, cols
