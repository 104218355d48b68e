"""Lidar depth without a GPU (include/sm_c_api.h "lidar depth"): the numpy restatement of the rules
(lidar_depth_ref.py) against answers derived by hand and against a per-pixel loop written from the header, and the quality of the
rules on an analytic street at KITTI size."""
import numpy as np
import pytest

import lidar_depth_ref as lr

f32 = np.float32
KITTI = lr.STREET_CAM
DIAMOND = {(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if abs(dx) + abs(dy) <= 2}


def _sparse(w, h, pts):
    s = np.zeros((h, w), np.uint16)
    for x, y, mm in pts:
        s[y, x] = mm
    return s


def _set(depth, mm=None):
    """the (x, y) of the pixels that are not empty (or hold mm)"""
    ys, xs = np.nonzero(depth if mm is None else depth == mm)
    return set(zip(xs.tolist(), ys.tolist()))


def test_one_point_dilates_to_the_diamond_and_corners_to_clipped_ones():
    w, h = 11, 9
    out = lr.complete(_sparse(w, h, [(5, 4, 5000)]), stages=lr.DILATE)
    assert _set(out["depth_mm"]) == {(5 + dx, 4 + dy) for dx, dy in DIAMOND} and len(DIAMOND) == 13
    assert set(out["depth_mm"][out["depth_mm"] > 0].tolist()) == {5000}
    corners = [(0, 0, 1000), (w - 1, 0, 2000), (0, h - 1, 3000), (w - 1, h - 1, 4000)]
    out = lr.complete(_sparse(w, h, corners), stages=lr.DILATE)
    for x, y, mm in corners:
        want = {(x + dx, y + dy) for dx, dy in DIAMOND if 0 <= x + dx < w and 0 <= y + dy < h}
        assert _set(out["depth_mm"], mm) == want and len(want) == 6, (x, y)
    assert out["stats"]["measured"] == 4 and out["stats"]["left_empty"] == w * h - 24


def test_close_fills_a_hole_and_keeps_an_isolated_diamond():
    w, h = 40, 21
    block = [(x, y, 7000) for x in range(8, 13) for y in range(8, 13) if (x, y) != (10, 10)]
    out = lr.complete(_sparse(w, h, block + [(30, 10, 9000)]), stages=lr.DILATE | lr.CLOSE)
    assert out["depth_mm"][10, 10] == 7000
    assert out["depth_mm"][8:13, 8:13].min() == 7000 == out["depth_mm"][8:13, 8:13].max()
    assert _set(out["depth_mm"], 9000) == {(30 + dx, 10 + dy) for dx, dy in DIAMOND}
    # without the dilation: the closing alone fills the one-pixel hole and adds nothing around the block or the point
    out = lr.complete(_sparse(w, h, block + [(30, 10, 9000)]), stages=lr.CLOSE)
    assert _set(out["depth_mm"], 7000) == {(x, y) for x in range(8, 13) for y in range(8, 13)}
    assert _set(out["depth_mm"], 9000) == {(30, 10)}


def test_extend_top_and_fill_large_with_one_measured_column():
    w, h, mm = 15, 12, 6000
    s = _sparse(w, h, [(7, y, mm + y) for y in range(5, h)])
    out = lr.complete(s, stages=lr.EXTEND_TOP)
    assert np.array_equal(out["depth_mm"][:5, 7], np.full(5, mm + 5)) and np.array_equal(out["depth_mm"][5:], s[5:])
    assert out["stats"]["filled_top"] == 5 and _set(out["depth_mm"]) == {(7, y) for y in range(h)}
    out = lr.complete(s, stages=lr.FILL_LARGE, large=5)
    assert _set(out["depth_mm"]) == {(x, y) for x in range(5, 10) for y in range(3, h)}
    assert out["depth_mm"][3, 5] == mm + 5 and out["depth_mm"][9, 9] == mm + 7          # the nearest of the window's taps
    assert out["stats"]["filled_large"] == 5 * 9 - 7
    out = lr.complete(s, stages=lr.EXTEND_TOP | lr.FILL_LARGE, large=5)
    assert _set(out["depth_mm"]) == {(x, y) for x in range(5, 10) for y in range(h)}
    assert out["stats"]["filled_top"] == 5 and out["stats"]["filled_large"] == 4 * h and out["stats"]["left_empty"] == 10 * h
    assert not lr.complete(np.zeros((h, w), np.uint16), stages=127)["depth_mm"].any()    # columns without a pixel stay empty


def test_lower_median_with_one_two_and_twenty_five_taps():
    w, h = 30, 9
    vals = np.arange(25) * 37 % 25                                                      # a permutation of 0..24
    block = [(20 + k % 5, 2 + k // 5, 4000 + 10 * int(vals[k])) for k in range(25)]
    out = lr.complete(_sparse(w, h, [(3, 4, 5000), (9, 4, 5000), (10, 4, 6000)] + block), stages=lr.MEDIAN)["depth_mm"]
    assert out[4, 3] == 5000
    assert out[4, 9] == 6000 and out[4, 10] == 6000          # of two, the lower v: the greater depth
    assert out[4, 22] == 4000 + 10 * 12                      # element 12 of 25 ascending in v is element 12 descending in depth
    assert (out > 0).sum() == 28


def test_smooth_averages_the_pixels_own_layer_only():
    w, h = 12, 7
    s = np.zeros((h, w), np.uint16)
    s[:, :6] = 2000 + 3 * np.arange(6)[None, :] + 7 * np.arange(h)[:, None]
    s[:, 6:] = 10000 + 40 * np.arange(6)[None, :]
    out = lr.complete(s, stages=lr.SMOOTH, tol_256=13)["depth_mm"]
    for x, y in ((5, 3), (6, 3), (4, 2)):                    # windows that hold both layers
        num = den = 0
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if (x + dx < 6) == (x < 6):
                    wt = lr.B5[dy + 2] * lr.B5[dx + 2]
                    num, den = num + wt * (65536 - int(s[y + dy, x + dx])), den + wt
        assert out[y, x] == 65536 - (num + den // 2) // den, (x, y)
    assert out[3, 5] < 2100 and out[3, 6] > 9900
    # tol_256 = 0: only taps of exactly the pixel's depth
    assert np.array_equal(lr.complete(s, stages=lr.SMOOTH, tol_256=0)["depth_mm"][:, 6:], s[:, 6:])


def _scalar(sparse, stages, large, tol):
    """the steps as the header writes them, one pixel at a time, in Python integers: the v plane after each"""
    H, W = sparse.shape
    v = [[65536 - int(sparse[y, x]) if sparse[y, x] else 0 for x in range(W)] for y in range(H)]
    box = lambda r: [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]

    def taps(p, x, y, offs):
        return [p[y + dy][x + dx] for dx, dy in offs if 0 <= x + dx < W and 0 <= y + dy < H]

    def each(fn):
        return [[fn(x, y) for x in range(W)] for y in range(H)]

    def top_of(p, x):
        return next((y for y in range(H) if p[y][x] > 0), None)

    def med(p, x, y):
        t = sorted(a for a in taps(p, x, y, box(2)) if a > 0)
        return t[(len(t) - 1) // 2] if p[y][x] > 0 else 0

    def smo(p, x, y):
        if p[y][x] == 0:
            return 0
        z0, num, den = 65536 - p[y][x], 0, 0
        for dx, dy in box(2):
            if 0 <= x + dx < W and 0 <= y + dy < H and p[y + dy][x + dx] > 0:
                z = 65536 - p[y + dy][x + dx]
                if max(z, z0) * 256 <= min(z, z0) * (256 + tol):
                    wt = lr.B5[dy + 2] * lr.B5[dx + 2]
                    num, den = num + wt * p[y + dy][x + dx], den + wt
        return (num + den // 2) // den

    out = {}
    for b, name in enumerate(lr.STEPS):
        if stages >> b & 1:
            p = v
            if name == "dilate":
                v = each(lambda x, y: max(taps(p, x, y, sorted(DIAMOND))))
            elif name == "close":
                m = each(lambda x, y: max(taps(p, x, y, box(2))))
                v = each(lambda x, y: min(taps(m, x, y, box(2))))
            elif name in ("fill_small", "fill_large"):
                r = 3 if name == "fill_small" else large // 2
                v = each(lambda x, y: p[y][x] if p[y][x] else max(taps(p, x, y, box(r))))
            elif name == "extend_top":
                tops = [top_of(p, x) for x in range(W)]
                v = each(lambda x, y: p[tops[x]][x] if tops[x] is not None and y < tops[x] else p[y][x])
            elif name == "median":
                v = each(lambda x, y: med(p, x, y))
            else:
                v = each(lambda x, y: smo(p, x, y))
        out[name] = np.array(v, np.int64)
    return out


@pytest.mark.parametrize("stages,large,tol", [(127, 31, 13), (127, 5, 0), (127, 9, 255)] + [(1 << b, 7, 13) for b in range(7)] + [(0, 31, 13)])
def test_every_step_equals_a_per_pixel_loop(stages, large, tol):
    rng = np.random.default_rng(stages * 100 + large)
    w, h = 23, 11
    s = np.where(rng.random((h, w)) < (0.08 if stages == 127 else 0.4), rng.choice([1, 1500, 1600, 9000, 30000, 65535], (h, w)), 0).astype(np.uint16)
    s[:3, :5] = 0
    got, want = lr.complete(s, stages, large, tol), _scalar(s, stages, large, tol)
    for name in lr.STEPS:
        assert np.array_equal(got[name], want[name]), name
    assert np.array_equal(got["depth_mm"], np.where(want["smooth"] > 0, 65536 - want["smooth"], 0))
    if stages == 0:
        assert np.array_equal(got["depth_mm"], s)


def test_projection_rules_one_point_at_a_time():
    cam = dict(width=20, height=9, fx=10.0, fy=10.0, cx=9.5, cy=4.0)
    I = np.eye(4, dtype=f32)
    nan, inf = float("nan"), float("inf")
    pts = np.array([
        [0.0, 0.0, 2.0, 0.5],          # 0: u = 9.5 -> px 10 (floor(10.0)), py 4
        [0.0, 0.0, 2.0, 0.9],          # 1: the same pixel and mm: the lower index wins
        [0.0, 0.0, 1.9996, 0.0],       # 2: mm 2000 as well (1999.6 + 0.5 floors to 2000)
        [0.0, 0.0, 3.0, 0.0],          # 3: behind the others
        [-2.0, 0.0, 2.0, 0.0],         # 4: u = -0.5 exactly: px 0
        [2.0, 0.0, 2.0, 0.0],          # 5: u = 19.5 = W - 0.5: dropped
        [nan, 0.0, 2.0, 0.0], [0.0, inf, 2.0, 0.0], [0.0, 0.0, -2.0, 0.0], [0.0, 0.0, 0.0, 0.0],   # 6..9
        [0.0, 0.0, 0.5, 0.0],          # 10: Z = min_z: kept, mm 500
        [0.1, 0.0, 65.0, 0.0],         # 11: Z = max_z: kept, mm 65000, but behind the winner of its pixel
        [0.0, 0.0, 0.499, 0.0], [0.0, 0.0, 65.01, 0.0],                                          # 12, 13: outside the range
    ], f32)
    sparse, index, landed = lr.project(pts, I, cam, 0.5, 65.0)
    assert landed == 7
    assert sparse[4, 10] == 500 and index[4, 10] == 10
    assert sparse[4, 0] == 2000 and index[4, 0] == 4
    assert (sparse > 0).sum() == 2 and (index >= 0).sum() == 2
    sparse, index, landed = lr.project(pts[:4], I, cam, 0.5, 65.0)
    assert sparse[4, 10] == 2000 and index[4, 10] == 0 and landed == 4
    sparse, index, landed = lr.project(pts[2:4], I, cam, 0.5, 65.0)
    assert sparse[4, 10] == 2000 and index[4, 10] == 0
    # T moves the points: the third row's translation alone carries the lidar's offset along z
    T = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1.0]], f32)
    sparse, index, _ = lr.project(pts[:1], T, cam, 0.5, 65.0)
    assert sparse[4, 10] == 3000 and lr.project(np.zeros((0, 4), f32), T, cam, 0.5, 65.0)[2] == 0


def test_near_grid_occludes_the_far_points_between():
    w, h = 44, 28
    pts = [(x, y, 3000 if (x % 4 == 0 and y % 4 == 0) else 20000) for y in range(4, 21) for x in range(8, 37)]
    out = lr.complete(_sparse(w, h, pts))
    assert np.array_equal(out["depth_mm"][4:21, 8:37], np.full((17, 29), 3000))
    assert (out["dilate"][4:21, 8:37] == 65536 - 20000).any()                # the dilation alone leaves far pixels inside the hull


def test_quality_on_the_analytic_street_at_kitti_size():
    """Measured with this restatement (64 x 1100 beams of which 35001 land, the lidar 8 cm above and 27 cm behind the camera,
    1242 x 375): 0.0751 of the pixels measured, every pixel filled, median relative error 0.00097, 90th percentile 0.0140.  The
    bound is twice the measured median (tools/lidar_depth_probe.py prints the same figures into profiles/lidar_depth_probe.txt)."""
    q = lr.street_quality()
    depth, sparse = q["out"]["depth_mm"], q["out"]["sparse_mm"]
    top = np.nonzero(sparse.any(axis=1))[0][0]
    assert (depth[top:] > 0).all()
    print(f"points {q['points']}, landed {q['landed']}, measured {q['measured']:.4f}, filled {q['filled']:.4f}, median {q['median']:.5f}, p90 {q['p90']:.5f}")
    assert q["judged"] > 0.9 and q["measured"] > 0.03
    assert q["median"] < 0.00194
    # no far depth inside the box face: the wall and the ground the lidar sees past the box's edges do not show through
    u0, u1 = (KITTI["fx"] * lr.BOX[0] / lr.BOX[4] + KITTI["cx"], KITTI["fx"] * lr.BOX[1] / lr.BOX[4] + KITTI["cx"])
    v0, v1 = (KITTI["fy"] * lr.BOX[2] / lr.BOX[4] + KITTI["cy"], KITTI["fy"] * lr.BOX[3] / lr.BOX[4] + KITTI["cy"])
    face = depth[int(v0) + 4:int(v1) - 3, int(u0) + 4:int(u1) - 3]
    assert face.size > 10000 and face.max() <= 8100 and face.min() >= 7900
