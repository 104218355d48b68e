"""The voxel index of the point queries may leave out a (point, record) pair only where the exact rule does not call it near
(csrc/sm_k_points.h rules (P1)-(P4) over rule (3) of csrc/sm_k_rays.h, restated in tests/points_ref.py): for every pair that is near by
the brute-force restatement, the record is wide or one of the cells it is registered in is a cell the point visits -- under the
reach the point came with, and under the reach shrunk to that very pair's dd, which is the least a walk can have shrunk to while
the pair still matters.  CPU only, numpy; random and adversarial points and discs.  (The budget of (P5) is put out of the way: a
walk that is given up tests every regular record.)"""
import numpy as np

import points_ref as pr

f32 = np.float32
NO_BUDGET = 1 << 40


def _row(c, n, r, conf=1.0):
    m = np.zeros(12, f32)
    m[0:3], m[3], m[8:11], m[11] = c, conf, n, r
    return m


def _check(model, pts, cell_mm, origin):
    """-> (pairs, near pairs, those of regular records)"""
    model, pts = np.asarray(model, f32).reshape(-1, 12), np.asarray(pts, f32).reshape(-1, 4)
    V = pr.cell_edge(cell_mm)
    box, kinds = pr.box_of(model, V, origin)
    ok, dd = pr.near(model, pts)
    pairs = np.argwhere(ok)
    vis, regular = {}, 0
    for i, j in pairs:
        kind, c0, c1 = kinds[j]
        assert kind != pr.DROP, (i, j)
        if kind == pr.WIDE:
            continue
        regular += 1
        reg = pr.registered(c0, c1)
        if i not in vis:
            vis[i] = pr.visited(pts[i], V, origin, box, NO_BUDGET)
        assert reg & vis[i], (cell_mm, origin, "point", i, pts[i], "record", j, model[j], c0, c1, sorted(vis[i])[:8])
        shrunk = pr.visited(pts[i], V, origin, box, NO_BUDGET, best_dd=dd[i, j])
        assert reg & shrunk and shrunk <= vis[i], (cell_mm, origin, "point", i, pts[i], "record", j, model[j], dd[i, j], c0, c1, sorted(shrunk)[:8])
    return ok.size, len(pairs), regular


def _scene(rng, C, base, n=60, m=300, reach_cells=2.5):
    """n discs in a cube of 6 cells around base, m points aimed at them from all sides: a third with the reach within a few ulp of
    the distance (dd == R*R to the last bits), a third with reaches of 1e-3 .. reach_cells cells, a third with reaches of half a cell
    to reach_cells cells, which many discs are within"""
    centres = np.asarray(base, np.float64) + rng.uniform(-3 * C, 3 * C, (n, 3))
    snap = np.round(centres / C) * C
    centres[::3] = snap[::3]                                                # every third centre on a lattice corner of an origin-0 grid
    centres[1::6, 0] = snap[1::6, 0]                                        # ... and some on a lattice plane
    nrm = rng.normal(size=(n, 3))
    nrm[::4] = np.eye(3)[rng.integers(0, 3, len(nrm[::4]))]                 # axis-aligned discs
    nrm[1::7] *= 1e-20                                                      # nn in the denormals: h2 is rough there, the filter must not care
    nrm[2::9] *= 1e15
    rad = rng.uniform(0.0, 0.8 * C, n)
    rad[1::2] *= 0.05
    rad[3::10] *= -1.0
    model = np.stack([_row(centres[i], nrm[i], rad[i]) for i in range(n)])
    pts = np.zeros((m, 4), f32)
    for i in range(m):
        j = i % n
        c, nn, r = model[j, 0:3].astype(np.float64), model[j, 8:11].astype(np.float64), abs(float(model[j, 11]))
        e = np.cross(nn / np.linalg.norm(nn), rng.normal(size=3))
        e /= np.linalg.norm(e)
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if i % 5 == 0:
            u = nn / np.linalg.norm(nn) * rng.choice([-1.0, 1.0])            # straight over the disc
        if i % 5 == 1:
            u = e                                                            # in its plane, past the rim
        g = C * 10.0 ** rng.uniform(-3.0, np.log10(reach_cells))
        pts[i, 0:3] = c + e * r * rng.uniform(0.0, 1.0) + u * g
        pts[i, 3] = C * 10.0 ** rng.uniform(-3.0, np.log10(reach_cells))
        if i % 3 == 2:
            pts[i, 3] = C * rng.uniform(0.5, reach_cells)
        if i % 3 == 0:
            _, dd = pr.near(model[j], np.array([[pts[i, 0], pts[i, 1], pts[i, 2], np.inf]], f32))
            R = np.sqrt(dd[0, 0])
            for _ in range(abs(i // 3 % 5 - 2)):
                R = np.nextafter(R, f32(np.inf) if i // 3 % 5 > 2 else f32(0.0))
            pts[i, 3] = R
    return model, pts


def test_every_near_pair_shares_a_visited_registered_cell():
    """1 mm to 16 m cells (and 500 m cells for reaches up to 1e3 m), coordinates up to 1e4 m from the world's origin, grid origins
    that are no multiples of the cell"""
    totals = np.zeros(3, np.int64)
    cases = [(cell_mm, base) for cell_mm in (1, 10, 250, 1000, 16000) for base in ((0.0, 0.0, 0.0), (1000.0, -1000.0, 999.99994), (-9999.5, 3.0, 10000.0))]
    cases += [(500000, (0.0, 0.0, 0.0)), (500000, (-9999.5, 3.0, 10000.0))]
    for cell_mm, base in cases:
        rng = np.random.default_rng(cell_mm * 7 + int(abs(base[0])))
        C = cell_mm / 1000.0
        for shift in ((0.0, 0.0, 0.0), (0.1 * C + 0.01, -0.033 * C, 7.77 * C)):
            # (the grid's origin goes with the discs: 1000 m from it lies beyond cell 65535 of a 1 or 10 mm grid, where every record is
            # loose, so wide, and the property holds by definition)
            origin = tuple(float(f32(base[k] + shift[k])) for k in range(3))
            model, pts = _scene(rng, C, base)
            got = _check(model, pts, cell_mm, origin)
            totals += got
            print(cell_mm, base, origin, "pairs, near, regular near:", got)
    print("total:", totals)
    assert totals[0] >= 200000 and totals[1] >= 10000 and totals[2] >= 8000, totals


def test_lattice_points_and_reaches_that_end_on_cell_faces():
    """250 mm cells are 0.25 m exactly (V = 16384): centres and points on lattice corners, reaches that are whole cells, so the
    cube's faces are cell faces"""
    C = 0.25
    model, pts = [], []
    for k, (i, j, l) in enumerate([(0, 0, 0), (4, 0, 0), (4, 4, 4), (-3, 2, 8), (1, 1, 1), (-8, -8, -8), (7, -2, 3)]):
        c = np.array([i, j, l]) * C
        for ax in range(3):
            model.append(_row(c, np.eye(3)[ax], [0.0, 0.05, 0.25, 0.1][(k + ax) % 4]))
        model.append(_row(c, (1, 1, 1), 0.05))
        for d in ((1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1), (-2, 1, 0), (0, 0, 0)):
            x = c + np.array(d) * C
            for R in (0.0, C, 2 * C, np.sqrt(2.0) * C, np.sqrt(3.0) * C, 0.2, 3 * C):
                pts.append([x[0], x[1], x[2], R])
    for origin in ((0.0, 0.0, 0.0), (0.125, 0.125, 0.125), (-0.25, 1000.0, 0.1)):
        pairs, near, regular = _check(model, pts, 250, origin)
        print(origin, pairs, near, regular)
        assert regular >= 500                                                # (the check is not vacuous)


def test_reach_and_the_cube_that_misses_the_box():
    assert pr.reach(1.0) == 1.0 * (1.0 + 1e-6) + 1e-6 and pr.reach(np.inf) == np.inf and pr.reach(5.0, best_dd=4.0) == pr.reach(2.0)
    assert pr.reach(1.0, best_dd=4.0) == pr.reach(1.0) and pr.reach(0.0) == 1e-6
    V = pr.cell_edge(250)
    box = ([0, 0, 0], [3, 3, 3])                                             # 1 m of cells
    assert pr.visited([2.0, 0.5, 0.5, 0.5], V, (0, 0, 0), box, 1000) == set()    # half a metre short of the box
    assert pr.visited([1.4, 0.5, 0.5, 0.5], V, (0, 0, 0), box, 1000)             # reaches into it
    assert pr.visited([0.5, 0.5, 0.5, np.inf], V, (0, 0, 0), box, 0) == {(x, y, z) for x in range(4) for y in range(4) for z in range(4)}
    assert pr.visited([0.5, 0.5, 0.5, np.inf], V, (0, 0, 0), box, 0, best_dd=1e-4) == {(x, y, z) for x in (1, 2) for y in (1, 2) for z in (1, 2)}
    assert pr.visited([0.5, 0.5, 0.5, np.inf], V, (0, 0, 0), ([0, 0, 0], [4, 3, 3]), 0) is None    # 80 cells > 64 + 0
    # a sphere, not a cube: the corner cells of a reach of a cell and a half are passed over
    got = pr.visited([0.625, 0.625, 0.625, 0.4], V, (0, 0, 0), ([-8, -8, -8], [8, 8, 8]), 1000)
    assert (2, 2, 2) in got and (1, 2, 2) in got and (0, 2, 2) in got and (0, 0, 0) not in got and (1, 1, 1) in got and len(got) < 125
