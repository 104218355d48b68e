"""One map set found in another without a guess, restated (sm_locate_maps; include/sm_c_api.h, "locating one map set in another";
DESIGN.md "4ab. Locating").  This file is the contract the HIP path is compared with, bit for bit.  Integers are int64 (nothing
below leaves its range); the record quantities are tests/ground_ref.py's.  The rotation table is an INPUT (`table`, int64[n_fine, 2]
of (c, s) in 2^-30; sm_locate_rotations gives the library's): nothing below calls a cosine, unless no table is given.

Units.     Q(mm) = (mm * 65536 + 500) // 1000, C = Q(cell_mm).  a = up >> 1, sgn = -1 if up & 1 else +1, ua < va the other axes.
Records.   The ground map's: regular or LOOSE; X[k] = floor((float64(p[k]) - float64(o[k])) * 65536), ni, class c; cu = X[ua] // C,
           cv = X[va] // C, H = sgn * X[a].  o is `origin` for the target set and `source_origin` for the source set.
           OUTSIDE: |H| >= 2^30; target: cu outside [0, nu) or cv outside [0, nv); source: |cu| > 4095 or |cv| > 4095.
Kinds.     structure-like: c in structure_mask and |ni[a]| <= max_up.  ground-like: c in ground_mask and normal_sign * sgn * ni[a] >=
           min_up.  A record may be both (it then adds to both rasters) or neither.  Counted as STRUCTURE if structure-like, else
           GROUND if ground-like, else OTHER.
Target.    n_t[cell] = its structure-like records; occ0 = n_t >= min_records; occ = occ0 dilated by `dilate` cells (Chebyshev), inside
           the window; Zt[cell] = min H of its ground-like records.
Source.    S = the cells with >= min_records structure-like records in (cv, cu) order, n_s = |S|; G = the cells with a ground-like
           record, in (cv, cu) order, with Zs = min H.
Rotation.  x = cu * C + C // 2, y = cv * C + C // 2; xr = (c x - s y + 2^29) >> 30, yr = (s x + c y + 2^29) >> 30; ru = xr // C, rv = yr // C.
Score.     score(j, du, dv) = the cells of S with (ru + du, rv + dv) in the window and occ set there.
Range.     R = (3 * max over S of max(|x|, |y|) // 2) // C + 2; du in [-R, nu - 1 + R], dv in [-R, nv - 1 + R].
Coarse.    over j = k * refine, k < n_yaw, and the range: the largest score, of equal ones the smallest (k, dv, du).
Refine.    over dj in (-refine, refine), j = (k* refine + dj) mod n_fine, and |du - du*| <= 1, |dv - dv*| <= 1 (not cut to the range):
           the largest score, of equal ones the smallest (|dj|, dj, dv, du).
Runner-up. the largest coarse score over circular |k - k*| > sep_yaw or max(|du - du*|, |dv - dv*|) > sep_cells (0 without such a
           candidate); sep_cells < 0: not searched, 0.
Height.    the cells of G whose rotated cell (row j) plus (du, dv) is a window cell with Zt: d = Zt - Zs; m of them; dh = sorted(d)[(m - 1) // 2],
           0 with m < min_ground.
Status.    NO_TARGET (no occ cell), NO_SOURCE (n_s = 0) -- for both every result field is 0 and nothing is searched --, NONE (score *
           256 < n_s * min_overlap_256), AMBIGUOUS (runner_up * 256 > coarse_score * ambiguity_256), OK.
Pose.      OK and AMBIGUOUS: float32 of the doubles M with c = c_j * 2^-30, s = s_j * 2^-30, Cm = C * 2^-16, O = float64(origin), So =
           float64(source_origin): M[ua][ua] = c, M[ua][va] = -s, M[va][ua] = s, M[va][va] = c, M[a][a] = 1,
           M[ua][3] = (O[ua] + du * Cm) - (c * So[ua] - s * So[va]), M[va][3] = (O[va] + dv * Cm) - (s * So[ua] + c * So[va]),
           M[a][3] = (O[a] + sgn * dh * 2^-16) - So[a].  Otherwise the identity.

Worked by hand: EXAMPLE below (the header's)."""
import numpy as np

import ground_ref as gr

F32, F64 = np.float32, np.float64
ALL = (0xFFFFFFFF,) * 8
DEFAULTS = dict(cell_mm=500, up=3, origin=(0.0, 0.0, 0.0), source_origin=(0.0, 0.0, 0.0), nu=256, nv=256, structure_mask=ALL, max_up=8192,
                ground_mask=ALL, min_up=11585, normal_sign=-1, min_records=2, dilate=1, n_yaw=360, refine=8, sep_yaw=10, sep_cells=8,
                min_ground=16, min_overlap_256=128, ambiguity_256=218, max_source_cells=1 << 18, max_nodes=1 << 20)
STATUS = ("OK", "AMBIGUOUS", "NONE", "NO_TARGET", "NO_SOURCE")
KINDS = ("STRUCTURE", "GROUND", "OTHER", "OUTSIDE", "LOOSE")
SPAN = 4095
RESULT_FIELDS = ("row", "du", "dv", "score", "coarse_k", "coarse_du", "coarse_dv", "coarse_score", "runner_up", "height_pairs", "dh")


def rotations(n_yaw, refine):
    """int64[n_fine, 2]: (c, s) as the library's host computes them.  Tests that compare with the GPU pass the library's own."""
    n = int(n_yaw) * int(refine)
    ang = 2.0 * np.pi * np.arange(n, dtype=F64) / F64(n)
    return np.stack([np.rint(np.cos(ang) * 2.0 ** 30), np.rint(np.sin(ang) * 2.0 ** 30)], axis=1).astype(np.int64)


def rotate(cu, cv, c, s, C):
    """the rotated cells (ru, rv) of the cells (cu, cv) under the table row (c, s)"""
    cu, cv = np.asarray(cu, np.int64), np.asarray(cv, np.int64)
    x, y = cu * C + C // 2, cv * C + C // 2
    xr, yr = (c * x - s * y + (1 << 29)) >> 30, (s * x + c * y + (1 << 29)) >> 30
    return xr // C, yr // C


def _bit(mask, c):
    mask = np.asarray([int(v) for v in mask], np.int64)
    return ((mask[c >> 5] >> (c & 31)) & 1).astype(bool)


def classify(rows, origin, p, window):
    """per record: (cu, cv, H, structure-like, ground-like, counts by KINDS); window: (nu, nv) for the target, None for the source"""
    rows = np.asarray(rows, F32).reshape(-1, 12)
    C = gr.q16(p["cell_mm"])
    a, sgn, ua, va = gr.axes(int(p["up"]))
    ok, X, ni, _, col = gr.quantities(rows, origin)
    cu, cv, H = X[:, ua] // C, X[:, va] // C, sgn * X[:, a]
    if window is None:
        inside = ok & (np.abs(cu) <= SPAN) & (np.abs(cv) <= SPAN)
    else:
        inside = ok & (cu >= 0) & (cu < window[0]) & (cv >= 0) & (cv < window[1])
    inside &= np.abs(H) < (1 << 30)
    c = col >> 24
    st = inside & _bit(p["structure_mask"], c) & (np.abs(ni[:, a]) <= int(p["max_up"]))
    gd = inside & _bit(p["ground_mask"], c) & (int(p["normal_sign"]) * sgn * ni[:, a] >= int(p["min_up"]))
    counts = [int(v.sum()) for v in (st, gd & ~st, inside & ~st & ~gd, ok & ~inside, ~ok)]
    return cu, cv, H, st, gd, counts


def target_raster(rows, p):
    """(occ bool[nv, nu], has_Z bool[nv, nu], Zt int64[nv, nu], counts)"""
    nu, nv = int(p["nu"]), int(p["nv"])
    cu, cv, H, st, gd, counts = classify(rows, p["origin"], p, (nu, nv))
    n_t = np.zeros(nu * nv, np.int64)
    np.add.at(n_t, (cv * nu + cu)[st], 1)
    occ0 = (n_t >= int(p["min_records"])).reshape(nv, nu)
    big = 1 << 40
    Z = np.full(nu * nv, big, np.int64)
    np.minimum.at(Z, (cv * nu + cu)[gd], H[gd])
    return dilate(occ0, int(p["dilate"])), (Z != big).reshape(nv, nu), Z.reshape(nv, nu), counts


def dilate(occ0, d):
    nv, nu = occ0.shape
    pad = np.zeros((nv + 2 * d, nu + 2 * d), bool)
    pad[d:d + nv, d:d + nu] = occ0
    out = np.zeros((nv, nu), bool)
    for dv in range(2 * d + 1):
        for du in range(2 * d + 1):
            out |= pad[dv:dv + nv, du:du + nu]
    return out


def source_cells(rows, p):
    """(S int64[n_s, 2] of (cu, cv), G int64[n_g, 3] of (cu, cv, Zs), counts); both in (cv, cu) order"""
    cu, cv, H, st, gd, counts = classify(rows, p["source_origin"], p, None)
    W = 2 * SPAN + 1
    key = (cv + SPAN) * W + (cu + SPAN)
    ks, n = np.unique(key[st], return_counts=True)
    ks = ks[n >= int(p["min_records"])]
    S = np.stack([ks % W - SPAN, ks // W - SPAN], axis=1).reshape(-1, 2)
    kg = np.unique(key[gd])
    Zs = np.full(len(kg), 1 << 40, np.int64)
    np.minimum.at(Zs, np.searchsorted(kg, key[gd]), H[gd])
    G = np.stack([kg % W - SPAN, kg // W - SPAN, Zs], axis=1).reshape(-1, 3)
    return S, G, counts


def search_range(S, C):
    x, y = S[:, 0] * C + C // 2, S[:, 1] * C + C // 2
    return int((3 * int(max(np.abs(x).max(), np.abs(y).max())) // 2) // C + 2)


def score_at(S, occ, row, du, dv, C):
    """the score of one candidate, literally"""
    nv, nu = occ.shape
    ru, rv = rotate(S[:, 0], S[:, 1], int(row[0]), int(row[1]), C)
    u, v = ru + du, rv + dv
    ok = (u >= 0) & (u < nu) & (v >= 0) & (v < nv)
    return int(occ[v[ok], u[ok]].sum())


def candidate_keys(S, occ, row, R, C):
    """int64[..]: (dv + R) * (nu + 2 R) + (du + R) of every pair of an occupied target cell and a rotated source cell whose difference
    (du, dv) lies in the range: a candidate's score is the number of times its key occurs"""
    nv, nu = occ.shape
    Wu, Wv = nu + 2 * R, nv + 2 * R
    ru, rv = rotate(S[:, 0], S[:, 1], int(row[0]), int(row[1]), C)
    tv, tu = np.nonzero(occ)
    du = (tu[None, :] - ru[:, None] + R).reshape(-1)
    dv = (tv[None, :] - rv[:, None] + R).reshape(-1)
    ok = (du >= 0) & (du < Wu) & (dv >= 0) & (dv < Wv)
    return dv[ok] * Wu + du[ok]


def score_plane(S, occ, row, R, C):
    """int64[nv + 2 R, nu + 2 R]: the scores of one row over the range, entry (dv + R, du + R) -- the histogram of the differences
    between occupied target cells and rotated source cells"""
    nv, nu = occ.shape
    Wu, Wv = nu + 2 * R, nv + 2 * R
    return np.bincount(candidate_keys(S, occ, row, R, C), minlength=Wu * Wv).reshape(Wv, Wu)


def best_of(keys, Wu, R):
    """(score, dv, du) of the most frequent key, of equal ones the smallest; without keys every candidate scores 0 and the first wins"""
    if not len(keys):
        return 0, -R, -R
    ks, n = np.unique(keys, return_counts=True)
    i = int(n.argmax())                                                       # (the first of equal ones: the smallest key)
    return int(n[i]), int(ks[i]) // Wu - R, int(ks[i]) % Wu - R


def score_plane_literal(S, occ, row, R, C):
    """the same by the triple loop of the definition"""
    nv, nu = occ.shape
    out = np.zeros((nv + 2 * R, nu + 2 * R), np.int64)
    for dv in range(-R, nv + R):
        for du in range(-R, nu + R):
            out[dv + R, du + R] = score_at(S, occ, row, du, dv, C)
    return out


def circular(d, n):
    d = abs(int(d)) % n
    return min(d, n - d)


def pose_of(p, row, du, dv, dh):
    """float64[4, 4] by the stated operations"""
    C = gr.q16(p["cell_mm"])
    a, sgn, ua, va = gr.axes(int(p["up"]))
    c, s, Cm = F64(int(row[0])) * F64(2.0 ** -30), F64(int(row[1])) * F64(2.0 ** -30), F64(C) * F64(2.0 ** -16)
    O = np.asarray([F32(v) for v in p["origin"]], F32).astype(F64)
    So = np.asarray([F32(v) for v in p["source_origin"]], F32).astype(F64)
    M = np.zeros((4, 4), F64)
    M[3, 3] = 1.0
    M[ua, ua], M[ua, va], M[va, ua], M[va, va], M[a, a] = c, -s, s, c, 1.0
    M[ua, 3] = (O[ua] + F64(du) * Cm) - (c * So[ua] - s * So[va])
    M[va, 3] = (O[va] + F64(dv) * Cm) - (s * So[ua] + c * So[va])
    M[a, 3] = (O[a] + F64(sgn * dh) * F64(2.0 ** -16)) - So[a]
    return M


def locate(source_rows, target_rows, table=None, **params):
    """dict(pose float64[4, 4], info) of the two sets' records; the info's fields are sm_locate_info's"""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise KeyError(sorted(unknown))
    p = dict(DEFAULTS, **params)
    C = gr.q16(p["cell_mm"])
    n_yaw, refine = int(p["n_yaw"]), int(p["refine"])
    n_fine = n_yaw * refine
    table = rotations(n_yaw, refine) if table is None else np.asarray(table, np.int64).reshape(n_fine, 2)
    occ, has_Z, Zt, tcounts = target_raster(target_rows, p)
    S, G, scounts = source_cells(source_rows, p)
    if len(S) > int(p["max_source_cells"]):
        raise OverflowError("more than max_source_cells source cells")
    nv, nu = occ.shape
    info = dict(status="OK", n_s=len(S), target_cells=int(occ.sum()), source_counts=scounts, target_counts=tcounts, **{k: 0 for k in RESULT_FIELDS})
    if not occ.any() or not len(S):
        info["status"] = "NO_SOURCE" if occ.any() else "NO_TARGET"
        info["status_code"] = STATUS.index(info["status"])
        return dict(pose=np.eye(4), info=info, S=S, G=G, occ=occ)
    R = search_range(S, C)
    Wu = nu + 2 * R
    # coarse: per row the largest score and its first place in (dv, du) order (the sparse form of score_plane)
    best, keys = None, []
    for k in range(n_yaw):
        keys.append(candidate_keys(S, occ, table[k * refine], R, C))
        sc, dv, du = best_of(keys[k], Wu, R)
        if best is None or sc > best[0]:
            best = (sc, k, dv, du)
    cs, ck, cdv, cdu = best
    runner = 0
    if int(p["sep_cells"]) >= 0:
        sep = int(p["sep_cells"])
        for k in range(n_yaw):
            ks = keys[k]
            if circular(k - ck, n_yaw) <= int(p["sep_yaw"]):
                ks = ks[np.maximum(np.abs(ks // Wu - R - cdv), np.abs(ks % Wu - R - cdu)) > sep]
            runner = max(runner, best_of(ks, Wu, R)[0])
    # refinement
    fine = None
    for dj in sorted(range(-refine + 1, refine), key=lambda d: (abs(d), d)):
        j = (ck * refine + dj) % n_fine
        for dv in (cdv - 1, cdv, cdv + 1):
            for du in (cdu - 1, cdu, cdu + 1):
                sc = score_at(S, occ, table[j], du, dv, C)
                if fine is None or sc > fine[0]:
                    fine = (sc, j, du, dv)
    score, j, du, dv = fine
    # height
    gu, gv = rotate(G[:, 0], G[:, 1], int(table[j][0]), int(table[j][1]), C)
    gu, gv = gu + du, gv + dv
    ok = (gu >= 0) & (gu < nu) & (gv >= 0) & (gv < nv)
    ok[ok] = has_Z[gv[ok], gu[ok]]
    d = np.sort(Zt[gv[ok], gu[ok]] - G[ok, 2])
    m = len(d)
    dh = int(d[(m - 1) // 2]) if m >= int(p["min_ground"]) and m else 0
    if score * 256 < len(S) * int(p["min_overlap_256"]):
        info["status"] = "NONE"
    elif runner * 256 > cs * int(p["ambiguity_256"]):
        info["status"] = "AMBIGUOUS"
    info.update(row=j, du=du, dv=dv, score=score, coarse_k=ck, coarse_du=cdu, coarse_dv=cdv, coarse_score=cs, runner_up=runner, height_pairs=m, dh=dh)
    info["status_code"] = STATUS.index(info["status"])
    pose = pose_of(p, table[j], du, dv, dh) if info["status"] in ("OK", "AMBIGUOUS") else np.eye(4)
    return dict(pose=pose, info=info, S=S, G=G, occ=occ, R=R)


def locate_set(source_parts, target_parts, table=None, **params):
    """of sets given as their files (and the live model last)"""
    cat = lambda parts: np.concatenate([np.asarray(q, F32).reshape(-1, 12) for q in parts]) if len(parts) else np.zeros((0, 12), F32)
    return locate(cat(source_parts), cat(target_parts), table, **params)


def wall(x, y, z=-1.0, n=(1, 0, 0), sem=3):
    """a structure-like record of the example's world (up 3: -y is up, the horizontal axes are x and z): a vertical surface"""
    return gr.record(x, z, y, sem=sem, n=n)


# The header's example: cell_mm 1000, up 3, a window of 6 x 4 cells at the origin, one record a cell suffices, no dilation, 4 coarse
# rows of 8 fine rows each (the table's rows 0, 8, 16, 24 are exact quarter turns), no runner-up separation in yaw.
#   target: cells (1, 1), (2, 1), (4, 1), (5, 1) occupied.     source: cells (0, 0), (1, 0).
#   row k = 0 (identity): both source cells land on occupied cells at (du, dv) = (1, 1) and at (4, 1): score 2 twice, the tie goes to
#   the smaller (k, dv, du): (0, 1, 1).  k = 2 (half a turn): the cells become (-1, -1), (-2, -1): score 2 at (3, 2) and (6, 2), both
#   later in the order.  k = 1, 3 put the pair along v: score 1 at most.  Coarse winner (0, 1, 1), score 2.
#   Refinement: dj = 0 gives 2 at (1, 1); dj = -1 and +1 (11.25 degrees either way) leave both cell centres in their cells and give 2 at
#   (1, 1) as well; the tie goes to the smaller (|dj|, dj, dv, du): dj = 0, row 0.
#   Runner-up (sep_yaw 0, sep_cells 1): (0, 1, 4) is 3 cells away: 2.  2 * 256 > 2 * 218: AMBIGUOUS.
EXAMPLE_PARAMS = dict(cell_mm=1000, up=3, nu=6, nv=4, min_records=1, dilate=0, n_yaw=4, refine=8, sep_yaw=0, sep_cells=1, min_ground=1)
EXAMPLE_TARGET = np.stack([wall(1.5, 1.5), wall(2.5, 1.5), wall(4.5, 1.5), wall(5.5, 1.5),
                           gr.record(1.5, 0.25, 1.5, n=(0, 1, 0)), gr.record(2.5, 0.5, 1.5, n=(0, 1, 0))])
EXAMPLE_SOURCE = np.stack([wall(0.5, 0.5), wall(1.5, 0.5), gr.record(0.5, 1.25, 0.5, n=(0, 1, 0)), gr.record(1.5, 1.0, 0.5, n=(0, 1, 0))])
#   Height: ground cells (0, 0) and (1, 0) of the source land on (1, 1) and (2, 1): H = -y * 65536: Zt = -16384, -32768; Zs = -81920,
#   -65536: d = 65536, 32768; m = 2, dh = sorted(d)[0] = 32768 (half a metre up).
EXAMPLE_INFO = dict(status="AMBIGUOUS", row=0, du=1, dv=1, score=2, coarse_k=0, coarse_du=1, coarse_dv=1, coarse_score=2, runner_up=2, n_s=2,
                    target_cells=4, height_pairs=2, dh=32768, source_counts=[2, 2, 0, 0, 0], target_counts=[4, 2, 0, 0, 0])
