"""Registration of one map set against another restated in numpy (include/sm_c_api.h "registration"; DESIGN.md "4q.
Registration") -- the checker of tests/test_register.py.  Integers where the specification has integers (int64: exact for the
sizes the tests use), float64 and float32 arrays one IEEE operation at a time in the header's order.  The lookups are vectorised:
a level's keys are sorted and the eight candidates of every sample found by searchsorted.  Every evaluated system also reports how
close any sample came to a threshold that decides something (`margins`, all relative: reach -- the distance to the reach;
angle -- the dot product to the cosine; half and cell -- the coordinate in units of 2^-16 m, before it is floored, to the middle
and to the faces of its cell, over the cell edge; tie -- the two nearest candidates' squared distances)."""
import math

import numpy as np

import track_ref as tr

F32, F64, I64 = np.float32, np.float64, np.int64
DEFAULTS = dict(voxel_mm=200, levels=3, max_iters=20, min_inliers=1000, angle_thresh=30.0, reach_cells=1.0, stride=0,
                max_samples=1 << 22, max_cells=1 << 24, origin=(0.0, 0.0, 0.0), pivot=(0.0, 0.0, 0.0))
BOUND = 1e-4                     # SM_TRACK_DEGENERATE_BOUND
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


class Capacity(Exception):
    """more keys at a level than max_cells"""


def cell_edge(voxel_mm, level=0):
    return ((int(voxel_mm) << level) * 65536 + 500) // 1000


def fields_ok(rows):
    """the simplification's tests of a record's fields (everything but the cell range): bool[N]"""
    r = np.asarray(rows, F32).reshape(-1, 12)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(r[:, [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]]).all(axis=1)
        ok &= (r[:, 3] > 0) & (r[:, 6] >= 0) & (r[:, 7] >= 0) & (r[:, 11] >= 0) & (r[:, 11] < 32768)
        ok &= ~((r[:, 8] == 0) & (r[:, 9] == 0) & (r[:, 10] == 0))
    return ok


def grid(q, V, origin):
    """q float64[N][3] -> (ok bool[N], cell int64[N][3], off int64[N][3]): |q - origin| < 2^24 and the cell in range"""
    o = np.asarray(origin, F32).astype(F64)
    with np.errstate(invalid="ignore"):
        d = q - o[None, :]
        ok = (np.abs(d) < 2.0 ** 24).all(axis=1)
        X = np.floor(np.where(ok[:, None], d, 0.0) * 65536.0).astype(I64)
    cell = X // V
    off = X - cell * V
    ok &= ((cell >= -65536) & (cell <= 65535)).all(axis=1)
    return ok, cell, off


def face_of(n):
    """the simplification's face of the normals n[N][3] (float32 or float64): the axis of the largest |n|, ties to the lower"""
    a = np.abs(n)
    ax = np.zeros(len(n), I64)
    ax = np.where(a[:, 1] > a[np.arange(len(n)), ax], 1, ax)
    ax = np.where(a[:, 2] > a[np.arange(len(n)), ax], 2, ax)
    return 2 * ax + (n[np.arange(len(n)), ax] < 0)


def pack(cell, face):
    c = (cell + 65536).astype(np.uint64)
    k3 = (c[:, 0] << np.uint64(34)) | (c[:, 1] << np.uint64(17)) | c[:, 2]
    return (k3 << np.uint64(11)) | (face.astype(np.uint64) << np.uint64(8))


def table(rows, V, origin):
    """the target table of one level: dict(keys uint64[K] ascending, pos float32[K][3], nrm float32[K][3], SW, SP, SN int64)"""
    r = np.asarray(rows, F32).reshape(-1, 12)
    r = r[fields_ok(r)]
    ok, cell, off = grid(r[:, 0:3].astype(F64), V, origin)
    r, cell, off = r[ok], cell[ok], off[ok]
    key = pack(cell, face_of(r[:, 8:11]))
    t = r[:, 3] * F32(16.0)
    w = np.where(t >= 255, 255, np.maximum(1, t.astype(np.int32))).astype(I64)
    ni = np.clip(np.floor(r[:, 8:11] * F32(16384.0) + F32(0.5)), F32(-4194304.0), F32(4194304.0)).astype(I64)
    keys, inv = np.unique(key, return_inverse=True)
    K = len(keys)
    SW, SP, SN = np.zeros(K, I64), np.zeros((K, 3), I64), np.zeros((K, 3), I64)
    np.add.at(SW, inv, w)
    np.add.at(SP, inv, w[:, None] * off)
    np.add.at(SN, inv, w[:, None] * ni)
    kc = np.stack([(keys >> np.uint64(45)) & np.uint64(0x1FFFF), (keys >> np.uint64(28)) & np.uint64(0x1FFFF),
                   (keys >> np.uint64(11)) & np.uint64(0x1FFFF)], axis=1).astype(I64) - 65536
    X = kc * V + (SP + (SW // 2)[:, None]) // SW[:, None]
    pos = (np.asarray(origin, F32).astype(F64)[None, :] + X.astype(F64) * (1.0 / 65536.0)).astype(F32)
    big = np.abs(SN).max(axis=1) if K else np.zeros(0, I64)
    s = np.array([max(0, int(b).bit_length() - 24) for b in big], I64)
    f = (SN >> s[:, None]).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2])
        nrm = f / ln[:, None]
    nrm[(f == 0).all(axis=1)] = 0
    assert nrm.dtype == F32 and pos.dtype == F32
    return dict(keys=keys, pos=pos, nrm=nrm, SW=SW, SP=SP, SN=SN, V=V)


class Problem:
    """tables and samples of one call: `source`, `target` the sets' rows in id order (float32[N][12])"""

    def __init__(self, source, target, **params):
        self.p = p = dict(DEFAULTS, **params)
        source = np.ascontiguousarray(source, F32).reshape(-1, 12)
        target = np.ascontiguousarray(target, F32).reshape(-1, 12)
        self.stride = p["stride"] or max(1, -(-len(source) // p["max_samples"]))
        s = source[::self.stride]
        self.n_samples = len(s)
        self.regular = fields_ok(s)
        self.pos, self.nrm = s[:, 0:3].astype(F64), s[:, 8:11].astype(F64)
        self.levels = [table(target, cell_edge(p["voxel_mm"], l), p["origin"]) for l in range(p["levels"])]
        for t in self.levels:
            if len(t["keys"]) > p["max_cells"]:
                raise Capacity(len(t["keys"]))
        self.cells = [len(t["keys"]) for t in self.levels]
        self.cos_angle = math.cos(float(F32(p["angle_thresh"])) * (math.pi / 180.0))
        self.pivot = np.asarray(p["pivot"], F32).astype(F64)

    def rows(self, T, level):
        """the pairs at the pose T (4x4 float64) on `level`: (J float32[n][6], r float32[n], sample index int64[n], margins)"""
        p, L = self.p, self.levels[level]
        V = L["V"]
        T = np.asarray(T, F64)
        x, n = self.pos, self.nrm
        with np.errstate(invalid="ignore", over="ignore"):
            q = np.stack([((T[k, 0] * x[:, 0] + T[k, 1] * x[:, 1]) + T[k, 2] * x[:, 2]) + T[k, 3] for k in range(3)], axis=1)
            nq = np.stack([(T[k, 0] * n[:, 0] + T[k, 1] * n[:, 1]) + T[k, 2] * n[:, 2] for k in range(3)], axis=1)
            ok, cell, off = grid(q, V, p["origin"])
        ok &= self.regular
        idx = np.nonzero(ok)[0]
        q, nq, cell, off = q[idx], nq[idx], cell[idx], off[idx]
        N = len(idx)
        g = (q - np.asarray(p["origin"], F32).astype(F64)[None, :]) * 65536.0          # the coordinate the cell and off are cut from
        nb = np.where(2 * off >= V, cell + 1, cell - 1)
        face = face_of(nq)
        K = len(L["keys"])
        best_d2 = np.full(N, np.inf)
        best_key = np.full(N, NO_KEY)
        best_at = np.zeros(N, I64)
        second = np.full(N, np.inf)                       # the nearest of the other candidates, for the tie margin
        for j in range(8):
            cand = np.stack([np.where(j & 1, nb[:, 0], cell[:, 0]), np.where((j >> 1) & 1, nb[:, 1], cell[:, 1]),
                             np.where(j >> 2, nb[:, 2], cell[:, 2])], axis=1)
            inr = ((cand >= -65536) & (cand <= 65535)).all(axis=1)
            ck = pack(np.where(inr[:, None], cand, 0), face)
            at = np.minimum(np.searchsorted(L["keys"], ck), max(K - 1, 0))
            hit = inr & (L["keys"][at] == ck) if K else np.zeros(N, bool)
            c = L["pos"][at].astype(F64) if K else np.zeros((N, 3))
            e = q - c
            d2 = np.where(hit, (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2], np.inf)
            better = hit & ((d2 < best_d2) | ((d2 == best_d2) & (ck < best_key)))
            second = np.where(better, np.minimum(second, best_d2), np.minimum(second, d2))
            best_d2 = np.where(better, d2, best_d2)
            best_key = np.where(better, ck, best_key)
            best_at = np.where(better, at, best_at)
        found = best_key != NO_KEY
        reach = float(F32(p["reach_cells"])) * (float(V) * (1.0 / 65536.0))
        c = L["pos"][best_at].astype(F64) if K else np.zeros((N, 3))
        m = L["nrm"][best_at].astype(F64) if K else np.zeros((N, 3))
        e = q - c
        with np.errstate(invalid="ignore"):
            dist = np.sqrt(np.where(found, best_d2, 0.0))
            dot = (nq[:, 0] * m[:, 0] + nq[:, 1] * m[:, 1]) + nq[:, 2] * m[:, 2]
        near = found & (dist <= reach)
        keep = near & (dot >= self.cos_angle)
        r = ((m[:, 0] * e[:, 0] + m[:, 1] * e[:, 1]) + m[:, 2] * e[:, 2]).astype(F32)
        u = q - self.pivot[None, :]
        J = np.stack([m[:, 0], m[:, 1], m[:, 2], u[:, 1] * m[:, 2] - u[:, 2] * m[:, 1], u[:, 2] * m[:, 0] - u[:, 0] * m[:, 2],
                      u[:, 0] * m[:, 1] - u[:, 1] * m[:, 0]], axis=1).astype(F32)
        # the smallest relative distance of any sample to a deciding threshold
        def rel(a, b):
            return float(np.min(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if len(a) else math.inf
        margins = dict(reach=rel(dist[found], np.full(found.sum(), reach)),
                       angle=rel(dot[near], np.full(near.sum(), self.cos_angle)),
                       half=float(np.min(np.abs(g - (cell * V + V / 2.0)) / V)) if N else math.inf,
                       cell=float(np.min(np.minimum(g - cell * V, (cell + 1) * V - g) / V)) if N else math.inf,
                       tie=rel(second[found & np.isfinite(second)], best_d2[found & np.isfinite(second)]))
        return J[keep], r[keep], idx[keep], margins

    def terms(self, T, level):
        J, r, _, _ = self.rows(T, level)
        return tr.products(J, r)


def start_pose(guess):
    return np.eye(4) if guess is None else tr.start_pose(guess)


def step(sys29, T, pivot):
    """the trackers' solve and the step about the pivot, in the header's operation order: (T', xi), or (None, None)"""
    A, b = tr.unpack(sys29)
    L, d = tr._ldlt(A)
    if L is None:
        return None, None
    y, xi = np.zeros(6), np.zeros(6)
    for i in range(6):
        y[i] = -b[i] - sum(L[i, k] * y[k] for k in range(i))
    for i in range(5, -1, -1):
        xi[i] = y[i] / d[i] - sum(L[k, i] * xi[k] for k in range(i + 1, 6))
    E = tr.se3_exp(xi)
    R, t = E[:3, :3], E[:3, 3]
    pv = np.asarray(pivot, F64)
    tp = np.array([(t[r] + pv[r]) - ((R[r, 0] * pv[0] + R[r, 1] * pv[1]) + R[r, 2] * pv[2]) for r in range(3)])
    T = np.asarray(T, F64)
    Tn = np.eye(4)
    for r in range(3):
        for c in range(3):
            Tn[r, c] = (R[r, 0] * T[0, c] + R[r, 1] * T[1, c]) + R[r, 2] * T[2, c]
        Tn[r, 3] = ((R[r, 0] * T[0, 3] + R[r, 1] * T[1, 3]) + R[r, 2] * T[2, 3]) + tp[r]
    return Tn, xi


def register(source, target, guess=None, **params):
    """sm_register_maps: (pose 4x4 float64 -- the guess unless status is OK --, info) with info = status, iterations and cells per
    level, inliers, rmse, pivot_ratio, samples, stride, and for the tests poses (level, T before the system) of every system,
    counts (its pairs) and margin (the smallest of all systems' margins)"""
    pb = Problem(source, target, **params)
    p = pb.p
    g = np.eye(4) if guess is None else np.asarray(guess, F32).astype(F64)
    info = dict(status="OK", iterations=[0] * p["levels"], cells=pb.cells, inliers=0, rmse=0.0, pivot_ratio=0.0,
                samples=int(pb.regular.sum()), stride=pb.stride, poses=[], counts=[], margin=math.inf, problem=pb)
    if min(pb.cells) == 0:
        info["status"] = "NO_TARGET"
        return g, info
    if info["samples"] == 0:
        info["status"] = "NO_SOURCE"
        return g, info
    T = start_pose(guess)
    for level in range(p["levels"] - 1, -1, -1):
        for it in range(p["max_iters"]):
            J, r, _, mg = pb.rows(T, level)
            terms = tr.products(J, r)
            sys = tr.exact_system(terms)
            n = len(terms)
            info["poses"].append((level, T.copy()))
            info["counts"].append(n)
            info["margin"] = min(info["margin"], *mg.values())
            info["iterations"][level] += 1
            info.update(inliers=n, rmse=math.sqrt(sys[27] / n) if n else 0.0)
            if n < p["min_inliers"] or n < 6:
                info["status"] = "LOST"
                return g, info
            T1, xi = step(sys, T, pb.pivot)
            if T1 is None:
                info["status"] = "DEGENERATE"
                return g, info
            T = T1
            if np.linalg.norm(xi[3:]) < 1e-6 and np.linalg.norm(xi[:3]) < 1e-6:
                break
    info["pivot_ratio"] = tr.pivot_ratio(sys, (0.0, 0.0, 0.0))
    if not info["pivot_ratio"] >= BOUND:
        info["status"] = "DEGENERATE"
        return g, info
    return T, info
