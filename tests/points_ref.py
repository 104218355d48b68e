"""The point query of sm_query_points_maps restated in numpy (include/sm_c_api.h "point queries"): every point against every record in
float32, in the header's order, no index -- query().  And the voxel index's filter restated from the rules of csrc/sm_k_points.h, in
float64 as the kernels compute it: the registration is the ray casts' (rule (3) of csrc/sm_k_rays.h: rays_ref.classify, box_of,
registered, restated there and used as they are), the reach G and the cells a point visits in a chunk's box are (P3)-(P5) --
reach(), visited().  tests/test_points_filter_math.py checks the superset property on these; tests/test_points.py compares the
library against query() bit for bit."""
import numpy as np

import rays_ref as rf

f32, f64 = np.float32, np.float64
REL, ABS = 1.0e-6, 1.0e-6
DROP, REG, WIDE = rf.DROP, rf.REG, rf.WIDE
cell_edge, classify, box_of, registered, budget, wide_count = rf.cell_edge, rf.classify, rf.box_of, rf.registered, rf.budget, rf.wide_count
PLANES = ("d2", "id", "centre", "normal", "radius", "rgb", "sem")


def valid(pts):
    """points float32[n][4] = (position, reach) -> bool[n]"""
    p = np.asarray(pts, f32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return np.isfinite(p[:, 0:3]).all(axis=1) & (p[:, 3] >= 0)


def takes_part(model, min_conf=0.0):
    """bool[n_records]: the gate, no NaN in centre, normal and radius, nn > 0 and finite"""
    m = np.asarray(model, f32).reshape(-1, 12)
    with np.errstate(all="ignore"):
        n = m[:, 8:11]
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        return (m[:, 3] >= f32(min_conf)) & ~np.isnan(m[:, [0, 1, 2, 8, 9, 10, 11]]).any(axis=1) & (nn > 0) & np.isfinite(nn)


def near(model, pts, min_conf=0.0):
    """(near bool[n_pts][n_records], dd float32[n_pts][n_records]) of the exact rule; rows of invalid points and columns of records
    that take no part are all False"""
    m = np.asarray(model, f32).reshape(-1, 12)
    q = np.asarray(pts, f32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        p, n, rad = m[None, :, 0:3], m[None, :, 8:11], np.abs(m[None, :, 11])
        x, R = q[:, None, 0:3], q[:, None, 3]
        c = x - p
        nn = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        h = (n[..., 0] * c[..., 0] + n[..., 1] * c[..., 1]) + n[..., 2] * c[..., 2]
        h2 = (h * h) / nn
        cc = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
        rho2 = cc - h2
        rho2 = np.where(rho2 > 0, rho2, f32(0.0))
        e = np.sqrt(rho2) - rad
        e = np.where(e > 0, e, f32(0.0))
        dd = h2 + e * e
        assert dd.dtype == f32 and e.dtype == f32 and h2.dtype == f32
        ok = (dd <= R * R) & (dd < f32(np.inf))
    return ok & valid(q)[:, None] & takes_part(m, min_conf)[None, :], dd


def query(model, pts, min_conf=0.0, block=128):
    """dict(d2, id, centre, normal, radius, rgb, sem): per point the near record with the least (bits(dd + 0), id); the empty values
    elsewhere"""
    m = np.asarray(model, f32).reshape(-1, 12)
    q = np.asarray(pts, f32).reshape(-1, 4)
    n = len(q)
    out = dict(d2=np.full(n, np.inf, f32), id=np.full(n, -1, np.int32), centre=np.zeros((n, 3), f32), normal=np.zeros((n, 3), f32),
               radius=np.zeros(n, f32), rgb=np.zeros((n, 3), np.uint8), sem=np.zeros(n, np.uint8))
    if not len(m):
        return out
    ids = np.arange(len(m), dtype=np.uint64)
    empty = np.uint64(0x7FFFFFFFFFFFFFFF)
    for a in range(0, n, block):
        ok, dd = near(m, q[a:a + block], min_conf)
        with np.errstate(all="ignore"):
            db = (dd + f32(0.0)).view(np.uint32).astype(np.uint64)
        key = np.where(ok, (db << np.uint64(32)) | ids[None, :], empty).min(axis=1)
        won = key != empty
        k = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)[won]
        at = a + np.flatnonzero(won)
        out["d2"][at] = (key[won] >> np.uint64(32)).astype(np.uint32).view(f32)
        out["id"][at] = k
        out["centre"][at], out["normal"][at], out["radius"][at] = m[k, 0:3], m[k, 8:11], m[k, 11]
        sc = m[k, 4].view(np.uint32)
        out["rgb"][at] = np.stack([(sc >> 16) & 255, (sc >> 8) & 255, sc & 255], axis=1).astype(np.uint8)
        out["sem"][at] = (((sc >> 24) & 255) + 1).astype(np.uint8)
    return out


# ---- the filter (csrc/sm_k_points.h rules (P3), (P4), (P5))

def reach(R, best_dd=None):
    """(P3): G, in double, of a reach and the dd of the best key so far (None: no key)"""
    rho = float(f32(R))
    if best_dd is not None:
        rho = min(rho, float(np.sqrt(f64(f32(best_dd)))))
    return rho * (1.0 + REL) + ABS


def _gap(xs, k, C):
    return max(k * C - xs, xs - (k + 1) * C, 0.0)


def visited(point, V, origin, box, n, best_dd=None):
    """(P3)-(P5): the set of cells (x, y, z) a valid point visits in the box (lo, hi) of a chunk of n records, under the G of
    best_dd throughout (the kernel's G only shrinks further as its best improves, and by (P4) loses no cell it needs); the empty
    set where the cube misses the box; None where the walk is given up and the chunk's regular records are tested one by one"""
    point = np.asarray(point, f32)
    lo, hi = box
    C = V / 65536.0
    G = reach(point[3], best_dd)
    xs = [float(point[k]) - float(f32(origin[k])) for k in range(3)]
    c0, c1, cm = [], [], []
    miss = False
    for k in range(3):
        if xs[k] + G < lo[k] * C or xs[k] - G > (hi[k] + 1) * C:
            miss = True
        c0.append(rf.cell_in(xs[k] - G, V, lo[k], hi[k]))
        c1.append(rf.cell_in(xs[k] + G, V, lo[k], hi[k]))
        cm.append(rf.cell_in(xs[k], V, c0[k], c1[k]))
    if miss:
        return set()
    if (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1) > budget(n):
        return None
    G2 = G * G
    out = {tuple(cm)}
    for cx in range(c0[0], c1[0] + 1):
        dx = _gap(xs[0], cx, C)
        if dx * dx > G2:
            continue
        for cy in range(c0[1], c1[1] + 1):
            dxy = dx * dx + _gap(xs[1], cy, C) ** 2
            if dxy > G2:
                continue
            for cz in range(c0[2], c1[2] + 1):
                s = max(abs(cx - cm[0]), abs(cy - cm[1]), abs(cz - cm[2]))      # the shell of the cell: a shell with (s - 1) C > G ends the walk
                if not dxy + _gap(xs[2], cz, C) ** 2 > G2 and not (s - 1) * C > G:
                    out.add((cx, cy, cz))
    return out
