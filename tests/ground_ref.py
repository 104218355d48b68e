"""A map set as a planner's ground map, restated (sm_ground_maps; include/sm_c_api.h, "ground map"; DESIGN.md "4v. Ground map").  This
file is the contract the HIP path is compared with, bit for bit.  Integers are int64 (nothing below leaves its range); the float32
and float64 steps of the record quantities are numpy's of that type, one at a time.

A set is a list of (global id, record) pairs; a record is 12 float32 (48 bytes): x y z conf | colour word, -, t0, t1 | nx ny nz radius.

Units.     Q(mm) = (mm * 65536 + 500) // 1000.  C = Q(cell_mm), B = Q(band_mm), L = Q(clear_lo_mm), Hi = Q(clear_hi_mm), S = Q(step_mm).
Axes.      a = up >> 1, sgn = -1 if up & 1 else +1; the horizontal axes are the other two, ascending: ua < va.
Records.   The simplification's regular-record test on the fields and |float64(p[k]) - float64(origin[k])| < 2^24 (not its cell range);
           X[k] = floor((float64(p[k]) - float64(origin[k])) * 65536.0); ni[k], w and c = colour word >> 24 as there.  Not regular: LOOSE.
Placement. cu = X[ua] // C, cv = X[va] // C, H = sgn * X[a].  cu outside [0, nu), cv outside [0, nv) or |H| >= 2^30: OUTSIDE.
Ground-like. c has its bit in ground_mask and normal_sign * sgn * ni[a] >= min_up (normal_sign -1: normals stored pointing into the surface).
Reading 1. Z[cell] = min H over the cell's ground-like records; such a cell has ground.
Reference. R[cell] = Z[cell] with ground; else Z of the cell (u', v') with ground that minimises (du^2 + dv^2, v', u') among |du|, |dv| <=
           fill_cells inside the window; else none.
Reading 2. d = H - R[cell]; the first that applies: no R: UNREFERENCED.  Ground-like, the cell has ground, 0 <= d <= B: GROUND (SW += w,
           SH += w d, SC[ch] += w channel[ch], best = max(best, w << 40 | (0x7FFFFFFF - id) << 8 | c)).  L < d < Hi: OBSTACLE (n_obst += 1,
           top = max(top, d)).  Else IGNORED.
Planes.    With ground: ground = Z + (SH + SW // 2) // SW, bgr[ch] = (SC[ch] + SW // 2) // SW, cls = best & 255.  Without: NONE, 0, 255.
State.     OBSTACLE (2): n_obst >= min_obstacle.  UNKNOWN (0): no ground.  STEP (3): step_mm > 0 and a 4-neighbour in the window has
           ground with |ground - ground'| > S.  FREE (1).
Clearance. clear2 = min(reach_cells^2, min over blocking cells of du^2 + dv^2); blocking: OBSTACLE, STEP, UNKNOWN if unknown_blocks.

Worked by hand: EXAMPLE below (the header's)."""
import numpy as np

F32, F64 = np.float32, np.float64
DEFAULTS = dict(cell_mm=100, up=3, origin=(0.0, 0.0, 0.0), nu=256, nv=256, min_up=11585, ground_mask=(0xFFFFFFFF,) * 8, band_mm=200,
                clear_lo_mm=150, clear_hi_mm=2000, min_obstacle=2, fill_cells=3, step_mm=150, reach_cells=32, unknown_blocks=0, normal_sign=-1)
KINDS = ("GROUND", "OBSTACLE", "IGNORED", "UNREFERENCED", "OUTSIDE", "LOOSE")
STATES = ("UNKNOWN", "FREE", "OBSTACLE", "STEP")
UNKNOWN, FREE, OBSTACLE, STEP = range(4)
NONE = -(1 << 31)
PLANES = ("ground", "top", "state", "cls", "bgr", "clear2")


def q16(mm):
    return (int(mm) * 65536 + 500) // 1000


def axes(up):
    """(a, sgn, ua, va)"""
    a = up >> 1
    ua, va = [k for k in range(3) if k != a]
    return a, (-1 if up & 1 else 1), ua, va


def quantities(rows, origin):
    """(regular: bool[n], X: int64[n, 3], ni: int64[n, 3], w: int64[n], col: int64[n]) -- the simplification's record quantities"""
    rows = np.asarray(rows, F32).reshape(-1, 12)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(rows[:, [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]]).all(axis=1)
        ok = fin & (rows[:, 3] > 0) & (rows[:, 6] >= 0) & (rows[:, 7] >= 0) & (rows[:, 11] >= 0) & (rows[:, 11] < 32768)
        ok &= ~((rows[:, 8] == 0) & (rows[:, 9] == 0) & (rows[:, 10] == 0))
        o = np.asarray([F32(v) for v in origin], F32).astype(F64)
        d = rows[:, :3].astype(F64) - o[None, :]
        ok &= (np.abs(d) < 2.0 ** 24).all(axis=1)
        d = np.where(ok[:, None], d, 0.0)
        X = np.floor(d * F64(65536.0)).astype(np.int64)
        n = np.where(ok[:, None], rows[:, 8:11], F32(0))
        ni = np.minimum(np.maximum(np.floor(n * F32(16384.0) + F32(0.5)), F32(-4194304.0)), F32(4194304.0)).astype(np.int64)
        t = np.where(ok, rows[:, 3], F32(1)) * F32(16.0)
        w = np.where(t >= F32(255.0), 255, np.maximum(1, np.minimum(t, F32(255.0)).astype(np.int64)))
    col = rows[:, 4].copy().view(np.uint32).astype(np.int64)
    return ok, X, ni, w, col


def fill(Z, has, fill_cells):
    """(R, has_R): Z where the cell has ground, else Z of the nearest cell with ground in the (2 fill_cells + 1)^2 window, ties to
    the lower v', then the lower u'"""
    nv, nu = Z.shape
    R, got = Z.copy(), has.copy()
    F = int(fill_cells)
    offs = sorted((du * du + dv * dv, dv, du) for dv in range(-F, F + 1) for du in range(-F, F + 1) if du or dv)
    pz = np.zeros((nv + 2 * F, nu + 2 * F), np.int64)
    ph = np.zeros((nv + 2 * F, nu + 2 * F), bool)
    pz[F:F + nv, F:F + nu], ph[F:F + nv, F:F + nu] = Z, has
    for _, dv, du in offs:                                                    # (for one cell v' rises with dv and u' with du)
        if got.all():
            break
        sz, sh = pz[F + dv:F + dv + nv, F + du:F + du + nu], ph[F + dv:F + dv + nv, F + du:F + du + nu]
        take = ~got & sh
        R[take] = sz[take]
        got |= take
    return R, got


def states(ground, n_obst, min_obstacle, step_mm):
    has = ground != NONE
    S = q16(step_mm)
    step = np.zeros(ground.shape, bool)
    if step_mm > 0:
        for axis in (0, 1):
            a, b = [slice(None)] * 2, [slice(None)] * 2
            a[axis], b[axis] = slice(0, -1), slice(1, None)
            a, b = tuple(a), tuple(b)
            differs = has[a] & has[b] & (np.abs(ground[a] - ground[b]) > S)
            step[a] |= differs
            step[b] |= differs
    st = np.where(has, np.where(step, STEP, FREE), UNKNOWN)
    return np.where(n_obst >= min_obstacle, OBSTACLE, st).astype(np.uint8)


def blocking(state, unknown_blocks):
    return (state == OBSTACLE) | (state == STEP) | ((state == UNKNOWN) & bool(unknown_blocks))


def clearance(block, reach_cells):
    """uint32[nv, nu]: min(reach^2, the squared distance in cells to the nearest True of `block`), by columns then rows: exact, since a
    cell nearer than reach has |du| and |dv| below it and a capped column distance adds reach^2 or more"""
    nv, nu = block.shape
    reach = int(reach_cells)
    g = np.full((nv, nu), reach, np.int64)
    d = np.full(nu, reach, np.int64)
    for v in range(nv):
        d = np.where(block[v], 0, np.minimum(d + 1, reach))
        g[v] = d
    d = np.full(nu, reach, np.int64)
    for v in range(nv - 1, -1, -1):
        d = np.where(block[v], 0, np.minimum(d + 1, reach))
        g[v] = np.minimum(g[v], d)
    best = np.full((nv, nu), reach * reach, np.int64)
    span = min(reach, nu - 1)
    pad = np.full((nv, nu + 2 * span), reach, np.int64)
    pad[:, span:span + nu] = g
    for du in range(-span, span + 1):
        best = np.minimum(best, du * du + pad[:, span + du:span + du + nu] ** 2)
    return best.astype(np.uint32)


def ground(rows, ids=None, **params):
    """dict(ground, top, state, cls, bgr, clear2, info) of the set {(ids[i], rows[i])}; ids default to 0..n-1"""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise KeyError(sorted(unknown))
    p = dict(DEFAULTS, **params)
    rows = np.asarray(rows, F32).reshape(-1, 12)
    ids = np.arange(len(rows), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    nu, nv = int(p["nu"]), int(p["nv"])
    N = nu * nv
    C, B, L, Hi = q16(p["cell_mm"]), q16(p["band_mm"]), q16(p["clear_lo_mm"]), q16(p["clear_hi_mm"])
    a, sgn, ua, va = axes(int(p["up"]))
    ok, X, ni, w, col = quantities(rows, p["origin"])
    cu, cv, H = X[:, ua] // C, X[:, va] // C, sgn * X[:, a]
    inside = ok & (cu >= 0) & (cu < nu) & (cv >= 0) & (cv < nv) & (np.abs(H) < (1 << 30))
    c = col >> 24
    mask = np.asarray([int(v) for v in p["ground_mask"]], np.int64)
    like = inside & ((mask[c >> 5] >> (c & 31)) & 1).astype(bool) & (int(p["normal_sign"]) * sgn * ni[:, a] >= int(p["min_up"]))
    cell = np.where(inside, cv * nu + cu, 0)

    # reading 1
    big = 1 << 40
    Z = np.full(N, big, np.int64)
    np.minimum.at(Z, cell[like], H[like])
    has = Z != big
    R, has_R = fill(Z.reshape(nv, nu), has.reshape(nv, nu), p["fill_cells"])
    R, has_R = R.reshape(-1), has_R.reshape(-1)

    # reading 2
    d = H - R[cell]
    unref = inside & ~has_R[cell]
    is_ground = inside & ~unref & like & has[cell] & (d >= 0) & (d <= B)
    is_obst = inside & ~unref & ~is_ground & (d > L) & (d < Hi)
    ignored = inside & ~unref & ~is_ground & ~is_obst
    SW, SH, SC, best = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros((3, N), np.int64), np.zeros(N, np.int64)
    gi = np.flatnonzero(is_ground)
    np.add.at(SW, cell[gi], w[gi])
    np.add.at(SH, cell[gi], w[gi] * d[gi])
    for ch in range(3):
        np.add.at(SC[ch], cell[gi], w[gi] * ((col[gi] >> (8 * ch)) & 255))
    np.maximum.at(best, cell[gi], (w[gi] << 40) | ((0x7FFFFFFF - ids[gi]) << 8) | c[gi])
    n_obst, top = np.zeros(N, np.int64), np.zeros(N, np.int64)
    oi = np.flatnonzero(is_obst)
    np.add.at(n_obst, cell[oi], 1)
    np.maximum.at(top, cell[oi], d[oi])

    # planes
    sw = np.maximum(SW, 1)
    assert (SW[has] >= 1).all()                                               # (a cell's lowest ground-like record lies in its band)
    gr = np.where(has, Z + (SH + sw // 2) // sw, NONE)
    bgr = np.where(has[None, :], (SC + sw[None, :] // 2) // sw[None, :], 0).T.astype(np.uint8)
    cls = np.where(has, best & 255, 255).astype(np.uint8)
    state = states(gr.reshape(nv, nu), n_obst.reshape(nv, nu), int(p["min_obstacle"]), int(p["step_mm"]))
    clear2 = clearance(blocking(state, p["unknown_blocks"]), p["reach_cells"])
    counts = [int(v.sum()) for v in (is_ground, is_obst, ignored, unref, ok & ~inside, ~ok)]
    info = dict(records=len(rows), counts_by_kind=counts, cells_by_state=[int((state == k).sum()) for k in range(4)])
    return dict(ground=gr.reshape(nv, nu).astype(np.int32), top=top.reshape(nv, nu).astype(np.int32), state=state, cls=cls.reshape(nv, nu),
                bgr=np.ascontiguousarray(bgr).reshape(nv, nu, 3), clear2=clear2, info=info,
                Z=np.where(has, Z, NONE).reshape(nv, nu), R=np.where(has_R, R, NONE).reshape(nv, nu))


def ground_set(parts, **params):
    """of a set given as its files (and the live model last): ids run through the parts in order"""
    parts = [np.asarray(q, F32).reshape(-1, 12) for q in parts]
    return ground(np.concatenate(parts) if parts else np.zeros((0, 12), F32), **params)


def record(x, y, z, conf=1.0, sem=3, bgr=(10, 100, 200), t0=1.0, t1=1.0, n=(0, 0, -1), r=0.0078125):
    s = np.zeros(12, F32)
    s[0:3] = (x, y, z)
    s[3] = conf
    s[4:5].view(np.uint32)[0] = (sem << 24) | (bgr[2] << 16) | (bgr[1] << 8) | bgr[0]
    s[6], s[7] = t0, t1
    s[8:11] = n
    s[11] = r
    return s


# The header's example: cell_mm 1000, up 3, origin 0, 5 x 1 cells, normals that point out of the surface, the rest at the defaults
EXAMPLE_PARAMS = dict(cell_mm=1000, up=3, nu=5, nv=1, normal_sign=1)
EXAMPLE_ROWS = np.stack([record(0.5, 1, 0.5, n=(0, -1, 0), sem=0), record(1.5, 1, 0.5, n=(0, -1, 0), sem=0), record(1.5, 0.875, 0.5, n=(0, -1, 0), sem=1),
                         record(2.5, 0, 0.5, n=(-1, 0, 0)), record(2.5, -0.5, 0.5, n=(-1, 0, 0)), record(3.5, 1, 0.5, n=(0, -1, 0)),
                         record(4.5, 0.5, 0.5, n=(0, -1, 0))])


def permute_axes(rows, up):
    """the rows of a world whose up direction is -y (up 3) moved into one whose up direction is `up`, with the horizontal axes (x, z)
    going to (ua, va): the planes are then the same"""
    a, sgn, ua, va = axes(up)
    rows = np.asarray(rows, F32).reshape(-1, 12)
    out = rows.copy()
    for base in (0, 8):
        out[:, base + ua], out[:, base + va], out[:, base + a] = rows[:, base + 0], rows[:, base + 2], F32(-sgn) * rows[:, base + 1]
    return out
