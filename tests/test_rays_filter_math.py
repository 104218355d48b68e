"""The voxel index of the ray casts may leave out a (ray, record) pair only where the exact test fails (csrc/sm_k_rays.h rules
(1)-(4), restated in tests/rays_ref.py): for every pair that hits by the brute-force restatement, the record is wide or one of the
cells it is registered in is a cell the ray visits.  CPU only, numpy; random and adversarial rays and discs."""
import numpy as np
import pytest

import rays_ref as rf

f32 = np.float32


def _row(c, n, r, conf=1.0):
    m = np.zeros(12, f32)
    m[0:3], m[3], m[8:11], m[11] = c, conf, n, r
    return m


def _ray(o, d, t_min=0.0, t_max=1e30):
    return np.array([o[0], o[1], o[2], t_min, d[0], d[1], d[2], t_max], f32)


def _check(model, rays, cell_mm, origin, least):
    """-> (hitting pairs, those of regular records)"""
    model, rays = np.asarray(model, f32).reshape(-1, 12), np.asarray(rays, f32).reshape(-1, 8)
    V = rf.cell_edge(cell_mm)
    box, kinds = rf.box_of(model, V, origin)
    hit, _ = rf.hits(model, rays)
    pairs = np.argwhere(hit)
    vis, regular = {}, 0
    for i, j in pairs:
        kind, c0, c1 = kinds[j]
        assert kind != rf.DROP, (i, j)
        if kind == rf.WIDE:
            continue
        regular += 1
        if i not in vis:
            vis[i] = rf.visited(rays[i], V, origin, box)
        assert rf.registered(c0, c1) & vis[i], (cell_mm, origin, "ray", i, rays[i], "record", j, model[j], c0, c1, sorted(vis[i])[:8])
    assert regular >= least, (len(pairs), regular)
    return len(pairs), regular


def _random_scene(rng, cell_mm, base, n=40):
    C = cell_mm / 1000.0
    centres = np.asarray(base, np.float64) + rng.uniform(-10 * C, 10 * C, (n, 3))
    snap = np.round(centres / C) * C
    centres[::3] = snap[::3]                                                # every third centre on a lattice corner of an origin-0 grid
    centres[1::6, 0] = snap[1::6, 0]                                        # ... and some on a lattice plane
    nrm = rng.normal(size=(n, 3))
    nrm[::4] = np.eye(3)[rng.integers(0, 3, len(nrm[::4]))]                 # axis-aligned discs
    rad = rng.uniform(0.0, 0.8 * C, n)
    rad[1::2] *= 0.05                                                       # (small against the slack of far coordinates in 1 mm cells)
    model = np.stack([_row(centres[i], nrm[i], rad[i]) for i in range(n)])
    rays = []
    for i in range(n):
        c, nn, r = model[i, 0:3].astype(np.float64), model[i, 8:11].astype(np.float64), float(model[i, 11])
        e = np.cross(nn, rng.normal(size=3))
        e /= np.linalg.norm(e)
        target = c + e * r * rng.uniform(0.0, 1.0)                           # in the disc's plane, up to its rim
        dirn = rng.normal(size=3)
        if i % 5 == 0:
            dirn[rng.integers(0, 3)] = 0.0                                  # one zero component
        if i % 7 == 0:
            dirn = np.eye(3)[rng.integers(0, 3)] * rng.choice([-1.0, 1.0])  # two
        dirn /= np.linalg.norm(dirn)
        dist = rng.uniform(0.0, 30 * C)
        scale = 10.0 ** rng.uniform(-3, 3)
        t_hit = dist / scale
        t_max = [1e30, t_hit * 1.5 + 1e-3 / scale, t_hit * (1 + 1e-6)][i % 3]   # leaves the grid; ends inside the box; ends at the disc
        rays.append(_ray(target - dirn * dist, dirn * scale, 0.0 if i % 2 else t_hit * 0.5, t_max))
    return model, np.stack(rays)


@pytest.mark.parametrize("cell_mm", [1, 10, 250, 1000, 10000])
@pytest.mark.parametrize("base", [(0.0, 0.0, 0.0), (1000.0, -1000.0, 999.99994), (-999.5, 3.0, 1000.0)])
def test_random_hits_share_a_cell(cell_mm, base):
    rng = np.random.default_rng(cell_mm * 7 + int(abs(base[0])))
    total = 0
    for origin in ((0.0, 0.0, 0.0), (0.1, -0.033, 7.77)):
        model, rays = _random_scene(rng, cell_mm, base)
        # (1000 m from the grid's origin lies beyond cell 65535 of a 1 or 10 mm grid: every record there is loose, so wide, and the
        # property holds by definition; test_far_coordinates_and_small_cells moves the grid's origin there)
        pairs, regular = _check(model, rays, cell_mm, origin, least=0 if cell_mm <= 10 and base[0] != 0.0 else 8)
        total += regular
    print(cell_mm, base, "regular hitting pairs:", total)


def test_lattice_planes_edges_and_corners():
    """250 mm cells are 0.25 m exactly (V = 16384): centres, origins and hit points on lattice planes, edges and corners; axis-parallel
    rays lying in a cell-boundary plane; diagonals through lattice points"""
    C = 0.25
    model, rays = [], []
    for k, (i, j, l) in enumerate([(0, 0, 0), (4, 0, 0), (4, 4, 4), (-3, 2, 8), (1, 1, 1), (-8, -8, -8), (7, -2, 3)]):
        c = np.array([i, j, l]) * C
        for ax in range(3):
            model.append(_row(c, np.eye(3)[ax], [0.0, 0.05, 0.25, 0.1][(k + ax) % 4]))
        model.append(_row(c, (1, 1, 1), 0.05))
        for ax in range(3):                                                 # along every axis through the centre, from both sides, in a boundary plane
            for sgn in (1.0, -1.0):
                d = np.eye(3)[ax] * sgn
                rays.append(_ray(c - d * 2.0, d))                           # starts on a lattice point
                rays.append(_ray(c - d * 2.125, d * 0.5, 0.0, 4.25))        # ends exactly at the centre
                rays.append(_ray(c, d, 0.0, 0.0))                           # starts and ends on the disc
        for diag in ((1, 1, 1), (1, -1, 1), (1, 1, 0), (0, 1, -1), (-1, -1, -1)):
            d = np.array(diag, np.float64)
            rays.append(_ray(c - d * 1.0, d))                               # a diagonal through lattice points, hits at t = 1
            rays.append(_ray(c - d * 0.5, d * 0.25, 1.0, 2.0))              # ... at t = 2 = t_max
    rays.append(_ray((-100.0, 0.0, 0.0), (1.0, 0.0, 0.0)))                  # from far outside the box
    rays.append(_ray((0.0, 0.0, -1e6), (0.0, 0.0, 1e3)))
    for origin in ((0.0, 0.0, 0.0), (0.125, 0.125, 0.125), (-0.25, 1000.0, 0.1)):
        pairs, regular = _check(model, rays, 250, origin, least=150)
        print(origin, pairs, regular)


def test_far_coordinates_and_small_cells():
    """near +-1000 m float32 steps are 6e-5 m: with 10 mm cells and discs of 1 mm a coordinate's rounding is a sizeable part of both"""
    rng = np.random.default_rng(3)
    base = np.array([1000.0, -1000.0, 1000.0])
    model, rays = [], []
    for i in range(60):
        c = (base + rng.uniform(-0.02, 0.02, 3)).astype(f32)
        n = rng.normal(size=3)
        model.append(_row(c, n, rng.uniform(0.0005, 0.002)))
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        dist = rng.uniform(0.0, 0.05) if i % 2 else rng.uniform(500.0, 3000.0)     # near origins, and origins a long way off
        rays.append(_ray(c.astype(np.float64) - d * dist, d))
    pairs, regular = _check(model, rays, 10, (0.0, 0.0, 0.0), least=0)         # (cell 100000: off the grid, every record is loose)
    print(pairs, regular)
    _check(model, rays, 10, (999.9, -1000.1, 1000.0), least=10)
    _check(model, rays, 1, (0.0, 0.0, 0.0), least=0)


def test_classification_rules():
    V = rf.cell_edge(100)
    nan, inf = float("nan"), float("inf")
    kind = lambda row, **kw: rf.classify(row, V, (0.0, 0.0, 0.0), **kw)[0]
    assert kind(_row((0.05, 0.05, 0.05), (0, 0, 1), 0.01)) == rf.REG
    assert kind(_row((0.05, 0.05, 0.05), (0, 0, 1), 2.0)) == rf.WIDE                 # 40 cells across
    assert kind(_row((0.05, 0.05, 0.05), (0, 0, 1), inf)) == rf.WIDE and kind(_row((0.05, 0.05, 0.05), (0, 0, 1), -inf)) == rf.WIDE
    assert kind(_row((1e10, 0, 0), (0, 0, 1), 0.01)) == rf.WIDE and kind(_row((0, inf, 0), (0, 0, 1), 0.01)) == rf.WIDE
    assert kind(_row((nan, 0, 0), (0, 0, 1), 0.01)) == rf.DROP and kind(_row((0, 0, 0), (0, 0, 1), nan)) == rf.DROP
    assert kind(_row((0, 0, 0), (0, 0, 1), 0.01, conf=nan)) == rf.DROP and kind(_row((0, 0, 0), (0, 0, 1), 0.01, conf=1.0), min_conf=2.0) == rf.DROP
    assert kind(_row((0.05, 0.05, 0.05), (0, 0, 0), 0.01)) == rf.REG                 # a zero normal hits nothing, and is registered all the same
    # a cube over exactly 2 x 2 x 2 cells is regular, one over 3 x 1 x 3 is wide
    k8, c0, c1 = rf.classify(_row((0.1, 0.1, 0.1), (0, 0, 1), 0.04), V, (0.0, 0.0, 0.0))
    assert k8 == rf.REG and len(rf.registered(c0, c1)) == 8
    assert kind(_row((0.15, 0.05, 0.15), (0, 0, 1), 0.06)) == rf.WIDE
    assert rf.cell(-1e-9, V) == -1 and rf.cell(0.0, V) == 0 and rf.cell(16777216.0, V) is None and rf.cell(6554.0, V) is None
