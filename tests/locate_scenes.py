"""Scenes for tests/test_locate.py, in a z-up world (up = 4) with normals that point out of the surface (normal_sign = +1), built
with tests/register_scenes.py's rigid() and records().  Everything is a function of the arguments (seeded).

yard_pair(truth): a yawed yard -- ground 40 x 8 m, a wall along one long side, a wall along half of the other, one end wall, two
box faces -- sampled twice with 1 cm of noise along the normals; the source sampling is expressed in a world of its own, moved by
the inverse of `truth` (any yaw about z, tens of metres, a height).  Nothing about the yard repeats under a half turn or a shift.
court_pair(truth): the symmetric one -- ground and four walls, a closed rectangle that a half turn maps onto itself."""
import math

import numpy as np

import locate_ref as lr
import register_scenes as sc

F32, F64 = np.float32, np.float64
LENGTH, HALF_W, WALL_H = 40.0, 4.0, 3.0
UP = dict(up=4, normal_sign=1)


def _surfaces(symmetric):
    L, W, Hh = LENGTH, HALF_W, WALL_H
    # (weight, origin, edge u, edge v, normal) in the yard's own frame: x along it, z up
    surf = [(L * 2 * W, (-L / 2, -W, 0), (L, 0, 0), (0, 2 * W, 0), (0, 0, 1)),
            (L * Hh, (-L / 2, -W, 0), (L, 0, 0), (0, 0, Hh), (0, 1, 0)),
            (2 * W * Hh, (L / 2, -W, 0), (0, 2 * W, 0), (0, 0, Hh), (-1, 0, 0))]
    if symmetric:
        surf += [(L * Hh, (-L / 2, W, 0), (L, 0, 0), (0, 0, Hh), (0, -1, 0)),
                 (2 * W * Hh, (-L / 2, -W, 0), (0, 2 * W, 0), (0, 0, Hh), (1, 0, 0))]
    else:
        surf += [(L / 2 * Hh, (-L / 2, W, 0), (L / 2, 0, 0), (0, 0, Hh), (0, -1, 0)),
                 (3.0 * 2.0 * 4, (-8.0, -1.0, 0), (0, 3.0, 0), (0, 0, 2.0), (-1, 0, 0)),          # (box faces: four times as densely)
                 (3.0 * 2.0 * 4, (6.0, 1.0, 0), (3.0, 0, 0), (0, 0, 2.0), (0, -1, 0))]
    return surf


def points(n, seed, symmetric=False, yaw_deg=20.0, noise=0.01, centre=(3.0, -2.0, 0.5)):
    """n points of the scene in the target world: (pos float64[n, 3], nrm float64[n, 3])"""
    rng = np.random.default_rng(seed)
    surf = _surfaces(symmetric)
    area = np.array([s[0] for s in surf])
    which = rng.choice(len(surf), n, p=area / area.sum())
    a, b = rng.random(n), rng.random(n)
    o, u, v, nn = (np.array([s[i] for s in surf], F64)[which] for i in (1, 2, 3, 4))
    p = o + a[:, None] * u + b[:, None] * v + rng.normal(0.0, noise, n)[:, None] * nn
    Wd = sc.rigid(rz_deg=yaw_deg, t=centre)
    return p @ Wd[:3, :3].T + Wd[:3, 3], nn @ Wd[:3, :3].T


def truth_of(yaw_deg, t):
    """a yaw about the z axis through the world's origin, then the translation t"""
    return sc.rigid(rz_deg=yaw_deg, t=t)


def pair(truth, n_target=20000, n_source=3000, seed=1, symmetric=False, **scene):
    """(source rows, target rows, params): the params are what a caller would choose without knowing `truth` -- the target window
    around the target's records, source_origin at the middle of the source's"""
    tp, tn = points(n_target, seed, symmetric, **scene)
    sp, sn = points(n_source, seed + 1000, symmetric, **scene)
    inv = np.linalg.inv(truth)
    sp, sn = sp @ inv[:3, :3].T + inv[:3, 3], sn @ inv[:3, :3].T
    rng = np.random.default_rng(seed + 2000)
    src, tgt = sc.records(sp, sn, rng), sc.records(tp, tn, rng)
    cell = lr.DEFAULTS["cell_mm"] / 1000.0
    lo, hi = tgt[:, :2].min(axis=0), tgt[:, :2].max(axis=0)
    origin = (math.floor(lo[0]) - 1.0, math.floor(lo[1]) - 1.0, 0.0)
    nu, nv = (int(math.ceil((hi[k] - origin[k] + 1.0) / cell)) for k in (0, 1))
    mid = 0.5 * (src[:, :3].min(axis=0) + src[:, :3].max(axis=0))
    source_origin = tuple(float(np.round(v)) for v in (mid[0], mid[1], 0.0))
    return src, tgt, dict(UP, origin=origin, nu=nu, nv=nv, source_origin=source_origin)


def yard_pair(truth, **kw):
    return pair(truth, symmetric=False, **kw)


def court_pair(truth, **kw):
    return pair(truth, symmetric=True, **kw)


def expected(truth, params, n_yaw=lr.DEFAULTS["n_yaw"], cell_mm=lr.DEFAULTS["cell_mm"]):
    """(k, du, dv, height) of `truth` as real numbers: the coarse row, the offsets in cells and the height in metres that the pose of
    sm_locate_maps would need to equal it"""
    yaw = math.degrees(math.atan2(truth[1, 0], truth[0, 0])) % 360.0
    So, O = np.asarray(params["source_origin"], F64), np.asarray(params["origin"], F64)
    off = truth[:3, :3] @ So + truth[:3, 3] - O
    cm = lr.gr.q16(cell_mm) / 65536.0
    return yaw / (360.0 / n_yaw), off[0] / cm, off[1] / cm, off[2]
