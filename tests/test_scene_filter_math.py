"""The widened world box of an actor block (sm_k_scene.h: scene_box_world, restated in tests/scene_ref.py: box_world) against the
per-record rule: over seeded (block, near-rigid pose) pairs every placed float centre lies inside the box, and every placed
normal's length times the radius is within the widened rmax.  CPU only."""
import numpy as np

import scene_ref as sr

f32 = np.float32
N_PAIRS = 10000


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _non_orthonormality(C):
    R = C.reshape(3, 4)[:, :3].astype(np.float64)
    return np.abs(R.T @ R - np.eye(3)).max(), np.linalg.det(R)


def _pose(rng, kind):
    R = _rotation(rng)
    if kind % 3 == 1:
        # pushed to the 1e-3 limit of sm_loop_spread's test: a stretch along a random axis, backed off until the float pose passes
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        g = 0.9995e-3 / np.abs(np.outer(u, u)).max()                      # R^T R - I = g u u^T: its largest entry at the limit
        while True:
            S = np.eye(3) + (np.sqrt(1 + g) - 1) * np.outer(u, u)
            if _non_orthonormality(np.concatenate([(R @ S), np.zeros((3, 1))], axis=1).astype(f32).reshape(12))[0] <= 1e-3:
                R = R @ S
                break
            g *= 0.999
    t = rng.uniform(-1, 1, 3) * (1.0e4 if kind % 4 == 2 else 50.0)
    return np.concatenate([R, t[:, None]], axis=1).astype(f32).reshape(12)


def _block(rng, kind):
    n = 1 if kind % 5 == 3 else int(rng.integers(2, 257))
    centre = rng.uniform(-1, 1, 3) * (3.0 if kind % 2 else 300.0)
    rows = np.zeros((n, 12), f32)
    rows[:, 0:3] = centre + rng.normal(0, rng.uniform(0.01, 3.0), (n, 3))
    nrm = rng.normal(size=(n, 3))
    rows[:, 8:11] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)        # unit normals (to float rounding), as the mapper stores them
    rows[:, 11] = rng.uniform(0.005, 0.5, n)
    return rows


def _intake_box(rows):
    """k_maps_intake's box: (lo, hi, rmax, rnorm)"""
    ra = np.abs(rows[:, 11])
    nx, ny, nz = rows[:, 8], rows[:, 9], rows[:, 10]
    ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
    return rows[:, 0:3].min(axis=0), rows[:, 0:3].max(axis=0), ra.max(), (ra * np.maximum(f32(1.0), ln)).max()


def test_placed_records_lie_inside_the_widened_world_box():
    rng = np.random.default_rng(2024)
    worst_centre, worst_normal, limit_poses, far_poses, single = 0.0, 0.0, 0, 0, 0
    for k in range(N_PAIRS):
        pose, rows = _pose(rng, k), _block(rng, k)
        dev, det = _non_orthonormality(pose)
        assert dev <= 1e-3 and det > 0                                       # a pose the call accepts
        limit_poses += dev > 0.99e-3
        far_poses += np.abs(pose[[3, 7, 11]]).max() > 5.0e3
        single += len(rows) == 1
        lo, hi, rmax, rnorm = _intake_box(rows)
        wlo, whi, wrmax, wrnorm = sr.box_world(lo, hi, rmax, rnorm, pose)
        assert np.isfinite(wrnorm)
        placed = sr.place_rows(pose, rows)
        c = placed[:, 0:3]
        assert (c >= wlo).all() and (c <= whi).all(), (k, pose, lo, hi)
        # how much of the widening the float error used (1 = all of it), against the box of the exact corner images
        n = placed[:, 8:11].astype(np.float64)
        reach = np.sqrt((n * n).sum(axis=1)) * np.abs(rows[:, 11].astype(np.float64))
        assert (reach <= float(wrmax)).all() and (reach <= float(wrnorm)).all(), (k, reach.max(), wrmax)
        worst_normal = max(worst_normal, float((reach / np.abs(rows[:, 11])).max()))
        exact = rows[:, 0:3].astype(np.float64) @ pose.reshape(3, 4)[:, :3].astype(np.float64).T + pose.reshape(3, 4)[:, 3].astype(np.float64)
        mag = float((np.abs(pose.reshape(3, 4)[:, :3]).astype(np.float64) @ np.abs(np.stack([lo, hi])).max(axis=0) + np.abs(pose.reshape(3, 4)[:, 3])).max())
        worst_centre = max(worst_centre, float(np.abs(c.astype(np.float64) - exact).max() / (float(sr.BOX_ERR) * mag)))
    print(f"{limit_poses} poses at the limit, {far_poses} with translations of 1e4 m, {single} one-record blocks; "
          f"largest centre error {worst_centre:.3f} of E, longest placed normal {worst_normal:.6f}")
    assert limit_poses > 2000 and far_poses > 1500 and single > 1500
    assert worst_centre < 0.5                                                # the float error stays well inside E
    assert 1.0004 < worst_normal < 1.002                                     # the limit poses stretch normals, within the growth


def test_boxes_that_cannot_be_bounded_are_never_skipped():
    lo, hi = np.array([-1, -1, -1], f32), np.array([1, 1, 1], f32)
    ident = sr.rigid(0, 0, 0)
    assert np.isinf(sr.box_world(lo, hi, 0.1, np.inf, ident)[3])                                  # a non-finite member (k_maps_intake's flag)
    assert np.isinf(sr.box_world(np.array([np.nan, 0, 0], f32), hi, 0.1, 0.1, ident)[3])
    assert np.isinf(sr.box_world(lo, np.array([1, 3e38, 1], f32), 0.1, 0.1, sr.rigid(0, 0, 0, 45.0))[3])   # terms beyond 1e18
    assert np.isinf(sr.box_world(lo, hi, 0.1, 0.1, sr.rigid(2e18, 0, 0))[3])
    wlo, whi, rmax, rnorm = sr.box_world(lo, hi, 0.1, 0.1, sr.rigid(10, 20, 30))
    assert np.isfinite(rnorm) and (wlo < [9, 19, 29]).all() and (whi > [11, 21, 31]).all() and (whi - wlo < 2.001).all()
    assert rmax == f32(0.1) * sr.NORMAL_GROWTH
