"""Scenes for tests/test_register.py: a street -- ground, two walls and three box faces across it -- sampled twice with 1 cm of
noise along the normals and yawed against the grid, the second sampling expressed in a world of its own (moved by the inverse of
`truth`).  Registering source onto target must give `truth`.  Everything is a function of the arguments (seeded)."""
import math

import numpy as np

F32 = np.float32


def rigid(rx_deg=0.0, ry_deg=0.0, rz_deg=0.0, t=(0.0, 0.0, 0.0), about=(0.0, 0.0, 0.0)):
    """4x4 float64: rotation Rz Ry Rx about the point `about`, then the translation t"""
    rx, ry, rz = (math.radians(v) for v in (rx_deg, ry_deg, rz_deg))
    Rx = np.array([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]])
    Ry = np.array([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]])
    Rz = np.array([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    a = np.asarray(about, np.float64)
    T[:3, 3] = a - T[:3, :3] @ a + np.asarray(t, np.float64)
    return T


def records(pos, nrm, rng):
    """map-file rows: conf 1, a colour word whose class varies (the registration ignores it), times 0 / 1, radius 5 cm"""
    n = len(pos)
    rows = np.zeros((n, 12), F32)
    rows[:, 0:3] = pos
    rows[:, 3] = 1.0
    rows[:, 4] = ((rng.integers(0, 20, n).astype(np.uint32) << 24) | np.uint32(0x808080)).view(F32)
    rows[:, 7] = 1.0
    rows[:, 8:11] = nrm
    rows[:, 11] = 0.05
    return rows


def street_points(n, seed, length=40.0, yaw_deg=20.0, noise=0.01, centre=(3.0, -2.0, 0.5)):
    """n points of the street in the world: (pos float64[n][3], nrm float64[n][3])"""
    rng = np.random.default_rng(seed)
    half_w, wall_h, box_w, box_h = 4.0, 4.0, 3.0, 2.0
    # (area, origin, edge u, edge v, normal) in the street's own frame: x along it, z up
    surf = [(length * 2 * half_w, (-length / 2, -half_w, 0), (length, 0, 0), (0, 2 * half_w, 0), (0, 0, 1)),
            (length * wall_h, (-length / 2, -half_w, 0), (length, 0, 0), (0, 0, wall_h), (0, 1, 0)),
            (length * wall_h, (-length / 2, half_w, 0), (length, 0, 0), (0, 0, wall_h), (0, -1, 0))]
    for bx, by in ((-12.0, -3.0), (0.5, 0.0), (11.0, -1.0)):
        surf.append((box_w * box_h * 4, (bx, by, 0), (0, box_w, 0), (0, 0, box_h), (-1, 0, 0)))     # (sampled four times as densely)
    area = np.array([s[0] for s in surf])
    which = rng.choice(len(surf), n, p=area / area.sum())
    a, b = rng.random(n), rng.random(n)
    o = np.array([s[1] for s in surf], np.float64)[which]
    u = np.array([s[2] for s in surf], np.float64)[which]
    v = np.array([s[3] for s in surf], np.float64)[which]
    nn = np.array([s[4] for s in surf], np.float64)[which]
    p = o + a[:, None] * u + b[:, None] * v + rng.normal(0.0, noise, n)[:, None] * nn
    W = rigid(rz_deg=yaw_deg, t=centre)
    return p @ W[:3, :3].T + W[:3, 3], nn @ W[:3, :3].T


def street_pair(n_target=20000, n_source=3000, seed=1, truth=None, **street):
    """(source rows, target rows, truth 4x4 float64, pivot): two samplings of one street, the source in its own world"""
    centre = street.get("centre", (3.0, -2.0, 0.5))
    pivot = (centre[0], centre[1], centre[2] + 1.0)
    if truth is None:
        truth = rigid(rx_deg=0.4, ry_deg=-0.3, rz_deg=1.5, t=(0.35, -0.3, 0.1), about=pivot)
    tp, tn = street_points(n_target, seed, **street)
    sp, sn = street_points(n_source, seed + 1000, **street)
    inv = np.linalg.inv(truth)
    sp, sn = sp @ inv[:3, :3].T + inv[:3, 3], sn @ inv[:3, :3].T
    rng = np.random.default_rng(seed + 2000)
    return records(sp, sn, rng), records(tp, tn, rng), truth, pivot


def plane_pair(n_target=6000, n_source=1500, seed=5):
    """a lone plane (the ground), sampled twice: three motions slide along it unnoticed"""
    rng = np.random.default_rng(seed)

    def pts(n):
        p = np.stack([rng.uniform(-10, 10, n), rng.uniform(-10, 10, n), rng.normal(0.0, 0.01, n)], axis=1)
        return p, np.tile([0.0, 0.0, 1.0], (n, 1))
    (tp, tn), (sp, sn) = pts(n_target), pts(n_source)
    return records(sp, sn, rng), records(tp, tn, rng)


def loose_rows(rng, n):
    """records that are not regular: a NaN coordinate, a zero normal, a cell out of range (20 km away is past the
    cells of a 0.2 m grid and inside those of a 0.4 m one: a record that is loose at one level and regular at another)"""
    rows = records(rng.uniform(-5, 5, (n, 3)), np.tile([0.0, 0.0, 1.0], (n, 1)), rng)
    kind = np.arange(n) % 3
    rows[kind == 0, 1] = np.nan
    rows[kind == 1, 8:11] = 0.0
    rows[kind == 2, 0] = 20000.0
    return rows
