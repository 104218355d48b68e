"""Scenes (include/sm_c_api.h "scenes") restated in numpy: the placed row, the id rule, the scene S_i of a view, and the
widened world box of an actor block (sm_k_scene.h: scene_box_world).  Everything fp32 in the stated order unless it says otherwise."""
import numpy as np

f32 = np.float32
ACTOR_CLASS = 7                       # a class the synthetic street lacks (it has 0, 2 and 13)
BOX_ERR, NORMAL_GROWTH, HUGE = f32(4.0e-6), f32(1.002), f32(1.0e18)


def pose12(m):
    """float32[12], row-major 3x4 [R|t], from that or from a 4x4 matrix (numpy row / column indexed)"""
    m = np.asarray(m, f32)
    return np.ascontiguousarray(m.reshape(4, 4)[:3, :] if m.size == 16 else m).reshape(12)


def place_rows(pose, rows):
    """sm_warp_by_time's row rule with one table row, applied to every row: the centre ((C0 x + C1 y) + C2 z) + C3, the normal the
    same without the translation; everything else bit-identical"""
    C = pose12(pose)
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 12)
    out = rows.copy()
    x, y, z, nx, ny, nz = (rows[:, k] for k in (0, 1, 2, 8, 9, 10))
    with np.errstate(all="ignore"):
        for r in range(3):
            c = C[4 * r:4 * r + 4]
            out[:, r] = ((c[0] * x + c[1] * y) + c[2] * z) + c[3]
            out[:, 8 + r] = (c[0] * nx + c[1] * ny) + c[2] * nz
    return out


def _fma(a, b, c):
    """fl32(a * b + c) as a fused multiply-add gives it: the product of two floats is exact in double, the sum is rounded to double
    and then to float (the double rounding can differ from a true fma only on a 2^-29 sliver of inputs)"""
    with np.errstate(all="ignore"):
        return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(f32)


def place_rows_contracted(pose, rows):
    """what a compiler that contracts a*b + c into fma would make of the rule (clang's pattern: the LAST product of each sum fused
    with the sum before it) -- NOT the definition: the tests use it to pick inputs on which contraction shows"""
    C = pose12(pose)
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 12)
    out = rows.copy()
    x, y, z, nx, ny, nz = (rows[:, k] for k in (0, 1, 2, 8, 9, 10))
    for r in range(3):
        c = C[4 * r:4 * r + 4]
        out[:, r] = _fma(z, c[2], _fma(y, c[1], c[0] * x)) + c[3]
        out[:, 8 + r] = _fma(nz, c[2], _fma(ny, c[1], c[0] * nx))
    return out


def id_bases(static_total, counts):
    """the id of row 0 of every actor: A + the records of the actors before it, present or not"""
    return [int(static_total + sum(counts[:j])) for j in range(len(counts))]


def scene_rows(static_rows, actors, view):
    """S_i: the static rows, then for every actor present in `view`, in list order, its placed rows.  actors: (rows, poses[V][12 or
    4x4], present[V] or None).  Returns (rows of S_i, scene id of each of them) -- with an actor absent the concatenation's row
    numbers and the scene ids part ways."""
    static_rows = np.ascontiguousarray(static_rows, f32).reshape(-1, 12)
    parts, ids = [static_rows], [np.arange(len(static_rows), dtype=np.int64)]
    bases = id_bases(len(static_rows), [len(a[0]) for a in actors])
    for (rows, poses, present), base in zip(actors, bases):
        if present is not None and not present[view]:
            continue
        parts.append(place_rows(poses[view], rows))
        ids.append(base + np.arange(len(rows), dtype=np.int64))
    return np.concatenate(parts), np.concatenate(ids)


def box_world(lo, hi, rmax, rnorm, pose):
    """scene_box_world: (lo', hi', rmax', rnorm') of a block's box under a pose; rnorm' = +inf: never skipped"""
    C = pose12(pose)
    never = (np.asarray(lo, f32), np.asarray(hi, f32), f32(rmax), f32(np.inf))
    if not np.isfinite(np.concatenate([np.asarray(lo, f32), np.asarray(hi, f32), [f32(rmax), f32(rnorm)]])).all():
        return never
    qlo, qhi, mag = np.full(3, f32(3.0e38)), np.full(3, f32(-3.0e38)), f32(0.0)
    aC = np.abs(C)
    with np.errstate(all="ignore"):
        for c in range(8):
            x, y, z = (f32(hi[k]) if c & (1 << k) else f32(lo[k]) for k in range(3))
            ax, ay, az = abs(x), abs(y), abs(z)
            for r in range(3):
                a = C[4 * r:4 * r + 4]
                q = ((a[0] * x + a[1] * y) + a[2] * z) + a[3]
                b = aC[4 * r:4 * r + 4]
                mag = max(mag, ((b[0] * ax + b[1] * ay) + b[2] * az) + b[3])
                qlo[r], qhi[r] = min(qlo[r], q), max(qhi[r], q)
        if not mag <= HUGE:
            return never
        E = BOX_ERR * mag
        return (qlo - E).astype(f32), (qhi + E).astype(f32), f32(rmax) * NORMAL_GROWTH, f32(rnorm) * NORMAL_GROWTH


def actor_box(n, size=(1.7, 1.5, 3.8), radius=0.12, seed=0, rgb=(40, 200, 250)):
    """an actor in its own frame: n records on the faces of a box centred at the origin, outward normals, class ACTOR_CLASS"""
    rng = np.random.default_rng(0xAC70 + seed)
    s = np.asarray(size, np.float64)
    area = np.array([s[1] * s[2], s[0] * s[2], s[0] * s[1]])
    axis = rng.choice(3, size=n, p=area / area.sum())
    sign = rng.choice([-1.0, 1.0], size=n)
    p = rng.uniform(-0.5, 0.5, size=(n, 3)) * s
    nrm = np.zeros((n, 3))
    p[np.arange(n), axis] = sign * s[axis] / 2
    nrm[np.arange(n), axis] = sign
    rows = np.zeros((n, 12), f32)
    rows[:, 0:3], rows[:, 3], rows[:, 8:11], rows[:, 11] = p, 10.0, nrm, radius
    word = np.uint32(rgb[2] | (rgb[1] << 8) | (rgb[0] << 16) | (ACTOR_CLASS << 24))      # B low, then G, R, the class on top
    rows[:, 4] = np.array([word], np.uint32).view(f32)[0]
    rows[:, 7] = np.arange(n) % 5
    return rows


def rigid(tx, ty, tz, yaw_deg=0.0):
    """float32[12]: a yaw about the y axis and a translation"""
    a = np.radians(yaw_deg)
    c, s = np.cos(a), np.sin(a)
    return np.array([c, 0, s, tx, 0, 1, 0, ty, -s, 0, c, tz], f32)


def street_setup(model, poses16):
    """The scenario the scene tests share, from the 10-frame street's model (tests/retire_ref.py) and its frames' poses: the static
    set -- the street's records within 5 m of the road's axis and between 2 and 22 m ahead of the first camera, thinned to every
    other one, in two files' worth of rows --, three views from the first three even frames, and five actors in front of them:
    P (600 records: two full blocks and a partial one) twice, Q (one large record), Z (none), and P again as `P2`."""
    model = np.asarray(model, f32).reshape(-1, 12)
    near = (np.abs(model[:, 0]) < 5.0) & (model[:, 2] > 2.0) & (model[:, 2] < 22.0)
    static = model[near][::2]
    cut = len(static) * 2 // 5
    views = np.stack([np.asarray(poses16[k], f32).reshape(16) for k in (0, 2, 4)])
    P = actor_box(600)
    Q = actor_box(1, seed=1, rgb=(250, 60, 60))
    Q[0, 0:3], Q[0, 8:11], Q[0, 11] = (0, 0, 0), (0, 0, -1), 0.45
    Z = np.zeros((0, 12), f32)
    z0 = [float(v[14]) for v in views]                                        # the cameras' z
    y = 1.65 - 0.75                                                           # the box stands on the road
    actors = [
        ("P", P, np.stack([rigid(-2.2, y, z + 9.0, 10.0 * i) for i, z in enumerate(z0)]), None),
        ("Q", Q, np.stack([rigid(0.6, 0.4, z + 3.5) for z in z0]), np.array([1, 0, 1], np.uint8)),
        ("Z", Z, np.stack([rigid(0, 0, z + 5.0) for z in z0]), None),
        ("P", P, np.stack([rigid(2.4, y + 0.6, z + 13.0, -25.0) for z in z0]), np.array([1, 1, 0], np.uint8)),   # sunk 0.6 m into the road
        ("P", P, np.stack([rigid(0.3, y, z + 17.0 + i, 90.0) for i, z in enumerate(z0)]), np.array([0, 1, 1], np.uint8)),
    ]
    return dict(static=(static[:cut], static[cut:]), views=views, actors=actors)
