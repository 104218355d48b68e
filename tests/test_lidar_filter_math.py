"""The footprint in front of the lidar sweep's exact test (sm_k_lidar.h lidar_footprint, restated in tests/lidar_ref.py) is a
superset: every beam the exact rule hits lies inside it.  10^5 random (surfel, pose, sensor) draws and the cases the filter is most
likely to get wrong; and the exact rule's known answers, derived by hand below.  CPU only."""
import math

import numpy as np

import lidar_ref as lr
import track_ref as tr

f32 = np.float32


def _pose(rng, spread=30.0):
    """a rigid sensor->world pose, column-major float32[16]: any rotation, a position within `spread` metres"""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = rng.uniform(-spread, spread, 3)
    return tr.colmajor(m.astype(f32))


def _sensor(rng):
    """a random grid: full or partial sweeps, any az0, uniform or jittered rows"""
    n_az = int(rng.integers(8, 120))
    full = rng.random() < 0.5
    step = 360.0 / n_az if full else rng.uniform(0.2, 360.0 / n_az)
    n_el = int(rng.integers(1, 24))
    lo = rng.uniform(-80, 20)
    el = np.sort(lo + np.cumsum(rng.uniform(0.3, 4.0, n_el)))
    el = el[el < 89.0]
    lo_r = rng.uniform(0.2, 3.0)
    return lr.sensor(n_az=n_az, n_el=len(el), az0=rng.uniform(-400, 400), step=f32(step) if f32(step) * n_az <= 360 else np.nextafter(f32(step), f32(0)),
                     el=el, min_range=lo_r, max_range=lo_r + rng.uniform(0.0, 60.0))


def _rows_near(rng, pose16, n):
    """n model rows around the sensor: centres at 0.05..80 m in any direction, radii from millimetres to metres, any normal"""
    P = np.asarray(pose16, np.float64).reshape(4, 4).T
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    dist = np.exp(rng.uniform(math.log(0.05), math.log(80.0), n))
    c = (d * dist[:, None]) @ P[:3, :3].T + P[:3, 3]
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    # half of the normals roughly towards the sensor, so that discs are seen face-on often enough to be hit
    face = rng.random(n) < 0.5
    towards = -(d @ P[:3, :3].T)
    nrm[face] = towards[face] + 0.3 * nrm[face]
    m = np.zeros((n, 12), f32)
    m[:, 0:3] = c
    m[:, 3] = 1.0
    m[:, 8:11] = nrm
    m[:, 11] = np.exp(rng.uniform(math.log(0.003), math.log(4.0), n)) * np.where(rng.random(n) < 0.1, dist, 1.0)
    return m


def _check(model, pose16, sn, what):
    """every exact hit inside the footprint; returns (rows with a hit, hits, beams inside the footprint)"""
    dirs = lr.directions(sn)
    c, m, r = lr.surfels(model, pose16)
    hit, _ = lr.hits(c, m, r, sn, dirs)
    rows, cols = lr.footprint(c, r, sn)
    inside = (rows[:, :, None] & cols[:, None, :]).reshape(len(model), -1)
    missed = hit & ~inside
    assert not missed.any(), (what, np.argwhere(missed)[:5], c[np.argwhere(missed)[:5, 0]], r[np.argwhere(missed)[:5, 0]])
    return int(hit.any(axis=1).sum()), int(hit.sum()), int(inside.sum())


def test_footprint_is_a_superset_on_random_draws():
    rng = np.random.default_rng(20260419)
    draws = hit_rows = hits = inside = beams = 0
    for k in range(250):
        pose, sn = _pose(rng), _sensor(rng)
        model = _rows_near(rng, pose, 400)
        a, b, c = _check(model, pose, sn, f"draw {k}")
        draws += len(model); hit_rows += a; hits += b; inside += c; beams += len(model) * sn["n_el"] * sn["n_az"]
    print(f"{draws} draws, {hit_rows} with a hit, {hits} hits, {inside} beams inside the footprints of {beams}")
    assert draws == 100000
    assert hit_rows >= draws // 100, "the generator must produce hits, or a filter that rejects everything would pass"
    assert inside < beams // 4, "the filter must filter"


def _row(c, n, r, conf=1.0):
    m = np.zeros(12, f32)
    m[0:3], m[3], m[8:11], m[11] = c, conf, n, r
    return m


IDENT = np.eye(4, dtype=f32).T.reshape(16).copy()


def test_footprint_adversarial_cases():
    full = lr.sensor(n_az=360, n_el=16, az0=-180.0, step=1.0)
    steep = lr.sensor(n_az=90, n_el=12, az0=0.0, step=4.0, el=[-88, -80, -60, -45, -30, -29, -10, 0, 3, 40, 70, 88], min_range=0.05, max_range=100.0)
    part = lr.sensor(n_az=45, n_el=8, az0=-45.0, step=1.0, el=np.arange(-14, 1, 2))
    tilt = tr.colmajor(np.array([[1, 0, 0, 0], [0, 0.8, -0.6, 1.5], [0, 0.6, 0.8, 0], [0, 0, 0, 1]], f32))
    cases = {
        # the sensor inside the disc's sphere: every beam may hit
        "inside": (steep, IDENT, [_row((0.2, 0.3, 0.1), (0, 1, 0), 5.0), _row((0, 0.5, 0), (0.1, 1, 0.1), 2.0), _row((0, 0, 0), (0, 1, 0), 1.0)]),
        # over the pole of the grid: hypot(c.x, c.z) <= R, every column
        "pole": (steep, IDENT, [_row((0.1, 3.0, -0.2), (0, 1, 0), 0.8), _row((0.0, -4.0, 0.0), (0, 1, 0.05), 1.0), _row((0.5, 2.0, 0.5), (0.2, 1, 0), 0.72)]),
        # a cap across the +-180 degree seam, seen from grids that start at -180, at 0 and at 170
        "seam": (full, IDENT, [_row((0.05, 0.5, -6.0), (0, 0, 1), 1.5), _row((-0.3, 1.0, -10.0), (0.1, 0.2, 1), 0.4)]),
        "seam0": (lr.sensor(n_az=360, n_el=16, az0=0.0, step=1.0), IDENT, [_row((0.05, 0.5, 6.0), (0, 0, 1), 1.5), _row((-0.3, 1.0, 10.0), (0.1, 0.2, 1), 0.4)]),
        "seam170": (lr.sensor(n_az=360, n_el=16, az0=170.0, step=1.0), IDENT, [_row((1.0, 0.5, -6.0), (0, 0, 1), 1.5), _row((-0.5, 0.5, -6.0), (0, 0, 1), 0.3)]),
        # a sweep narrower than 360 degrees: discs at both edges and behind
        "partial": (part, IDENT, [_row((-5.0, 0.6, 5.0), (1, 0, -1), 0.5), _row((0.0, 0.6, 7.0), (0, 0, 1), 0.5), _row((0.0, 0.5, -6.0), (0, 0, 1), 3.0)]),
        # the ground under a tilted sensor, wide and close
        "ground": (full, tilt, [_row((0.0, 2.0, 1.0), (0, 1, 0), 2.0), _row((3.0, 2.0, 4.0), (0, 1, 0), 0.3)]),
        # at the range limits
        "range": (full, IDENT, [_row((0, 0, 60.04), (0, 0, 1), 0.1), _row((0, 0, 0.98), (0, 0, 1), 0.1), _row((0, 1.0, 59.99), (0.0, 0.02, 1), 0.05)]),
    }
    for name, (sn, pose, rows) in cases.items():
        n_hit, hits, _ = _check(np.stack(rows), pose, sn, name)
        assert n_hit >= 1, name
    c = lambda rows: lr.surfels(np.stack(rows), IDENT)
    # inside the sphere: the whole grid; over the pole: every column of some rows
    cc, _, rr = c(cases["inside"][2])
    rows, cols = lr.footprint(cc, rr, steep)
    assert rows.all() and cols.all()
    cc, _, rr = c(cases["pole"][2])
    rows, cols = lr.footprint(cc, rr, steep)
    assert cols.all() and rows.any(axis=1).all() and not rows.all(axis=1).any()
    # the seam: two runs of columns, at both ends of the grid
    cc, _, rr = c(cases["seam"][2])
    rows, cols = lr.footprint(cc, rr, full)
    assert cols[0, 0] and cols[0, -1] and cols[1, 0] and not cols[:, 180].any()
    # the partial sweep: a disc behind the sensor has no column at all -- nothing wraps
    cc, _, rr = c(cases["partial"][2])
    rows, cols = lr.footprint(cc, rr, part)
    assert not cols[2].any() and cols[0, 0] and not cols[0, -1] and cols[1, -1]
    # hostile values: an empty or a whole footprint, never an exception
    bad = np.stack([_row((np.nan, 0, 5), (0, 0, 1), 0.1), _row((0, 0, 5), (0, 0, 1), np.nan), _row((np.inf, 0, 5), (0, 0, 1), 0.1),
                    _row((0, 0, 5), (0, 0, 1), 1e30), _row((0, 0, 5), (0, 0, 1), np.inf), _row((1e30, 0, 5), (0, 0, 1), 1e30)])
    cc, _, rr = lr.surfels(bad, IDENT)
    rows, cols = lr.footprint(cc, rr, full)
    assert [bool(a.all() and b.all()) for a, b in zip(rows, cols)] == [False, False, False, True, True, True]    # (inf * 0 in the transform makes the infinite centre a NaN)
    assert not rows[:3].any()
    _check(bad, IDENT, full, "hostile")


def test_known_answers():
    """A disc at (0, 0, 5) with normal (0, 0, -1) and r = 0.1, seen from the origin with the identity pose.  Beam az a, el 0 is
    d = (sin a, 0, cos a): den = -cos a, num = -5, t = 5 / cos a, and the hit point lies 5 tan a from the centre in the disc's plane."""
    disc = _row((0, 0, 5), (0, 0, -1), 0.1)
    sn = lr.sensor(n_az=4, n_el=1, az0=0.0, step=0.5, el=[0.0])
    dirs = lr.directions(sn)
    out = lr.sweep(disc[None], IDENT, sn, dirs)
    # az 0: t = 5 exactly; az 0.5 deg: 5 tan = 0.0436 < 0.1, t = 5 / cos; az 1 deg: 0.0873 < 0.1; az 1.5 deg: 0.1309 > 0.1, a miss
    assert out["range"][0, 0] == f32(5.0)
    assert list(out["id"][0]) == [0, 0, 0, -1]
    np.testing.assert_allclose(out["range"][0, 1:3], [5 / math.cos(math.radians(0.5)), 5 / math.cos(math.radians(1.0))], rtol=1e-6)
    assert out["range"][0, 3] == 0 and out["sem"][0, 3] == 0 and (out["rgb"][0, 3] == 0).all()
    # colour word 0x02112233: class 2 -> sem 3, bytes >>16, >>8, >>0
    disc[4] = np.array([0x02112233], np.uint32).view(f32)[0]
    out = lr.sweep(disc[None], IDENT, sn, dirs)
    assert out["sem"][0, 0] == 3 and list(out["rgb"][0, 0]) == [0x11, 0x22, 0x33]
    # two-sided: the normal turned round gives the same return
    back = lr.sweep(_row((0, 0, 5), (0, 0, 1), 0.1)[None], IDENT, sn, dirs)
    assert np.array_equal(back["range"], out["range"])
    # edge-on: the normal (1, 0, 0) is perpendicular to beam 0, den = 0 and num = 0: t is a NaN, no return; the other beams meet the
    # plane x = 0 at t = 0, below min_range
    edge = lr.sweep(_row((0, 0, 5), (1, 0, 0), 0.1)[None], IDENT, sn, dirs)
    assert (edge["id"] == -1).all() and (edge["range"] == 0).all()
    # edge-on and off the plane: c = (0.05, 0, 5), num = 0.05, den = 0 on beam 0: t = +inf, no return
    edge = lr.sweep(_row((0.05, 0, 5), (1, 0, 0), 0.1)[None], IDENT, sn, dirs)
    assert edge["id"][0, 0] == -1
    # two coincident discs: the lower id wins; a nearer one wins whatever its id
    two = np.stack([disc, disc])
    assert (lr.sweep(two, IDENT, sn, dirs)["id"][0, :3] == 0).all()
    near = np.stack([disc, _row((0, 0, 3), (0, 0, -1), 0.1)])
    got = lr.sweep(near, IDENT, sn, dirs)
    assert got["id"][0, 0] == 1 and got["range"][0, 0] == f32(3.0) and got["id"][0, 2] == 1    # 3 tan 1 deg = 0.052 < 0.1: at 1 deg the nearer wins too
    # range limits are inclusive; conf below min_conf and a NaN conf take no part
    assert lr.sweep(disc[None], IDENT, dict(sn, max_range=f32(5.0)), dirs)["id"][0, 0] == 0
    assert lr.sweep(disc[None], IDENT, dict(sn, max_range=f32(4.999)), dirs)["id"][0, 0] == -1
    assert lr.sweep(disc[None], IDENT, dict(sn, min_range=f32(5.0)), dirs)["id"][0, 0] == 0
    assert lr.sweep(disc[None], IDENT, dict(sn, min_conf=f32(2.0)), dirs)["id"][0, 0] == -1
    nanc = disc.copy(); nanc[3] = np.nan
    assert lr.sweep(nanc[None], IDENT, sn, dirs)["id"][0, 0] == -1
    # a pose: the sensor 2 m further back and turned 90 degrees about y (x_s = -z_w, z_s = x_w): the disc at world (7, 0, 0) facing -x
    pose = tr.colmajor(np.array([[0, 0, 1, 2], [0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 1]], f32))
    got = lr.sweep(_row((7, 0, 0), (-1, 0, 0), 0.1)[None], pose, sn, dirs)
    assert got["range"][0, 0] == f32(5.0) and list(got["id"][0]) == [0, 0, 0, -1]
