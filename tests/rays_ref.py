"""The ray cast of sm_cast_rays_maps restated in numpy (include/sm_c_api.h "ray casts"): every ray against every record in float32, in
the header's order, no index -- cast().  And the voxel index's filter restated from the numbered rules of csrc/sm_k_rays.h, in
float64 as the kernels compute it: the cell of a coordinate (cell), what becomes of a record and where it is registered (classify),
the chunk's box (box_of) and the cells a ray visits in it (visited).  tests/test_rays_filter_math.py checks the superset property
on these; tests/test_rays.py compares the library against cast() bit for bit."""
import numpy as np

f32, f64 = np.float32, np.float64
R_REL, REL, ABS = 1.0001, 2.5e-7, 1.0e-6
GRID = 16777216.0
MAX_CELLS = 8
DROP, REG, WIDE = 0, 1, 2


def valid(rays):
    """rays float32[n][8] = (origin, t_min, dir, t_max) -> bool[n]"""
    r = np.asarray(rays, f32).reshape(-1, 8)
    return np.isfinite(r).all(axis=1) & (r[:, 3] >= 0) & (r[:, 7] >= r[:, 3]) & ~(r[:, 4:7] == 0).all(axis=1)


def hits(model, rays, min_conf=0.0):
    """(hit bool[n_rays][n_records], t float32[n_rays][n_records]) of the exact test; rows of invalid rays are all False"""
    m = np.asarray(model, f32).reshape(-1, 12)
    r = np.asarray(rays, f32).reshape(-1, 8)
    ok = valid(r)
    takes = m[:, 3] >= f32(min_conf)
    with np.errstate(all="ignore"):
        p, n, rad = m[None, :, 0:3], m[None, :, 8:11], m[None, :, 11]
        o, d = r[:, None, 0:3], r[:, None, 4:7]
        c = p - o
        den = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
        num = (n[..., 0] * c[..., 0] + n[..., 1] * c[..., 1]) + n[..., 2] * c[..., 2]
        t = num / den
        q = t[..., None] * d - c
        qq = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
        assert t.dtype == f32 and qq.dtype == f32
        hit = (t >= r[:, None, 3]) & (t <= r[:, None, 7]) & (qq <= rad * rad)
    return hit & ok[:, None] & takes[None, :], t


def cast(model, rays, min_conf=0.0, block=128):
    """dict(t, id, rgb, sem, normal): per ray the hitting record with the least (bits(t + 0), id); the empty values elsewhere"""
    m = np.asarray(model, f32).reshape(-1, 12)
    r = np.asarray(rays, f32).reshape(-1, 8)
    n = len(r)
    out = dict(t=np.zeros(n, f32), id=np.full(n, -1, np.int32), rgb=np.zeros((n, 3), np.uint8), sem=np.zeros(n, np.uint8),
               normal=np.zeros((n, 3), f32))
    if not len(m):
        return out
    ids = np.arange(len(m), dtype=np.uint64)
    empty = np.uint64(0x7FFFFFFFFFFFFFFF)
    for a in range(0, n, block):
        hit, t = hits(m, r[a:a + block], min_conf)
        with np.errstate(all="ignore"):
            tb = (t + f32(0.0)).view(np.uint32).astype(np.uint64)
        key = np.where(hit, (tb << np.uint64(32)) | ids[None, :], empty).min(axis=1)
        won = key != empty
        k = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)[won]
        at = a + np.flatnonzero(won)
        out["t"][at] = (key[won] >> np.uint64(32)).astype(np.uint32).view(f32)
        out["id"][at] = k
        sc = m[k, 4].view(np.uint32)
        out["rgb"][at] = np.stack([(sc >> 16) & 255, (sc >> 8) & 255, sc & 255], axis=1).astype(np.uint8)
        out["sem"][at] = (((sc >> 24) & 255) + 1).astype(np.uint8)
        out["normal"][at] = m[k, 8:11]
    return out


# ---- the filter (csrc/sm_k_rays.h rules (1), (3), (4))

def cell_edge(cell_mm):
    """V: the cell edge in 2^-16 m, as the simplification's grid has it"""
    return (int(cell_mm) * 65536 + 500) // 1000


def cell(y, V):
    """(1): the cell of a shifted coordinate (a float), or None off the grid"""
    y = float(y)
    if not abs(y) < GRID:
        return None
    c = int(np.floor(y * 65536.0)) // V                  # (Python's // is the floor division)
    return c if -65536 <= c <= 65535 else None


def cell_in(y, V, lo, hi):
    y = float(y)
    if not y > -GRID:
        return lo
    if not y < GRID:
        return hi
    return min(max(int(np.floor(y * 65536.0)) // V, lo), hi)


def classify(row, V, origin, min_conf=0.0):
    """(3): (DROP | REG | WIDE, c0, c1) of one record of 12 floats; c0, c1: its cells per axis when REG"""
    row = np.asarray(row, f32)
    p, conf, r = row[0:3], row[3], row[11]
    if not conf >= f32(min_conf) or np.isnan(p).any() or np.isnan(r):
        return DROP, None, None
    ra = abs(r)
    if not np.isfinite(ra):
        return WIDE, None, None
    with np.errstate(all="ignore"):
        m = max(abs(float(p[0])), abs(float(p[1])), abs(float(p[2])))
        R = (float(ra) * R_REL + REL * m) + ABS
        c0, c1, cells = [], [], 1
        for i in range(3):
            y = float(p[i]) - float(f32(origin[i]))
            a, b = cell(y - R, V), cell(y + R, V)
            if a is None or b is None:
                return WIDE, None, None
            c0.append(a); c1.append(b)
            cells *= b - a + 1
    return (WIDE if cells > MAX_CELLS else REG), c0, c1


def box_of(model, V, origin, min_conf=0.0):
    """the chunk's box in cells over its regular records: (lo[3], hi[3]), or None without any; and the list of classify()'s results"""
    kinds = [classify(row, V, origin, min_conf) for row in np.asarray(model, f32).reshape(-1, 12)]
    reg = [(c0, c1) for k, c0, c1 in kinds if k == REG]
    if not reg:
        return None, kinds
    lo = [min(c0[i] for c0, _ in reg) for i in range(3)]
    hi = [max(c1[i] for _, c1 in reg) for i in range(3)]
    return (lo, hi), kinds


def visited(ray, V, origin, box):
    """(4): the set of cells (x, y, z) a valid ray visits in the chunk box (lo, hi), without the early stop"""
    ray = np.asarray(ray, f32)
    lo, hi = box
    C = V / 65536.0
    o, tmin, d, tmax = ray[0:3], float(ray[3]), ray[4:7], float(ray[7])
    oy = [float(o[k]) - float(f32(origin[k])) for k in range(3)]
    dd = [float(d[k]) for k in range(3)]
    S = 0.0
    for k in range(3):
        W = max(abs(lo[k] * C), abs((hi[k] + 1) * C)) + abs(float(f32(origin[k])))
        S = max(S, REL * (2.0 * abs(float(o[k])) + W))
    S += ABS
    ta, tb = tmin, tmax
    for k in range(3):
        L, U = lo[k] * C - S, (hi[k] + 1) * C + S
        if dd[k] == 0.0:
            if oy[k] < L or oy[k] > U:
                return set()
        else:
            t1, t2 = (L - oy[k]) / dd[k], (U - oy[k]) / dd[k]
            ta, tb = max(ta, min(t1, t2)), min(tb, max(t1, t2))
    if not ta <= tb:
        return set()
    m = 0
    if abs(dd[1]) > abs(dd[m]):
        m = 1
    if abs(dd[2]) > abs(dd[m]):
        m = 2
    u, v = (1 if m == 0 else 0), (1 if m == 2 else 2)
    ya, yb = oy[m] + ta * dd[m], oy[m] + tb * dd[m]
    kA, kB = cell_in(min(ya, yb) - S, V, lo[m], hi[m]), cell_in(max(ya, yb) + S, V, lo[m], hi[m])
    out = set()
    for k in range(kA, kB + 1):
        t1, t2 = (k * C - S - oy[m]) / dd[m], ((k + 1) * C + S - oy[m]) / dd[m]
        tl, th = max(ta, min(t1, t2)), min(tb, max(t1, t2))
        if not tl <= th:
            continue
        ua, ub = oy[u] + tl * dd[u], oy[u] + th * dd[u]
        va, vb = oy[v] + tl * dd[v], oy[v] + th * dd[v]
        u0, u1 = cell_in(min(ua, ub) - S, V, lo[u], hi[u]), cell_in(max(ua, ub) + S, V, lo[u], hi[u])
        v0, v1 = cell_in(min(va, vb) - S, V, lo[v], hi[v]), cell_in(max(va, vb) + S, V, lo[v], hi[v])
        for cu in range(u0, u1 + 1):
            for cv in range(v0, v1 + 1):
                c = [0, 0, 0]
                c[m], c[u], c[v] = k, cu, cv
                out.add(tuple(c))
    return out


def budget(n):
    """(6): the cells a ray may visit in a chunk of n records before it gives the walk up and tests the chunk's regular records
    one by one (which finds every hit the walk would have found, and more tests)"""
    return 64 + n // 8


def registered(c0, c1):
    return {(x, y, z) for x in range(c0[0], c1[0] + 1) for y in range(c0[1], c1[1] + 1) for z in range(c0[2], c1[2] + 1)}


def wide_count(model, cell_mm, origin=(0.0, 0.0, 0.0), min_conf=0.0):
    """stats.wide of a set that is one chunk, by rule (3) (a table that is not overfull)"""
    V = cell_edge(cell_mm)
    return sum(1 for row in np.asarray(model, f32).reshape(-1, 12) if classify(row, V, origin, min_conf)[0] == WIDE)
