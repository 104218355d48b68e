"""Change detection between two map sets restated in numpy (include/sm_c_api.h "change detection"; DESIGN.md "4r. Change
detection") -- the checker of tests/test_compare.py.  The fine table is registration's (tests/register_ref.py `table`, per class
where match_class keeps it), the cells, faces and keys are its functions; every float64 step is one IEEE operation in the header's
order.  The lookups are vectorised: the keys are sorted and every candidate found by searchsorted.  `primary_only` cuts the
candidate faces down to the simplification's face of the moved normal -- a switch of this restatement alone, for the test that
shows what the several faces are for."""
import math

import numpy as np

import register_ref as rr

F32, F64, I64 = np.float32, np.float64, np.int64
DEFAULTS = dict(voxel_mm=100, cover_shift=3, reach_cells=2.0, plane_mm=50, angle_thresh=30.0, match_class=0, write_mask=2,
                max_cells=1 << 24, origin=(0.0, 0.0, 0.0))
SUPPORTED, CHANGED, OUTSIDE, LOOSE = 0, 1, 2, 3
NAMES = ("SUPPORTED", "CHANGED", "OUTSIDE", "LOOSE")


class Capacity(Exception):
    """more keys in a table than max_cells"""


def _rows(x):
    return np.ascontiguousarray(x, F32).reshape(-1, 12)


def classes(rows):
    return (np.ascontiguousarray(_rows(rows)[:, 4]).view(np.uint32) >> np.uint32(24)).astype(np.uint64)


def fine_table(rows, V, origin, match_class):
    """registration's table of one level; with match_class one per class, the class in the keys' low eight bits"""
    r = _rows(rows)
    if not match_class:
        return rr.table(r, V, origin)
    cls = classes(r)
    parts = []
    for c in np.unique(cls):
        t = rr.table(r[cls == c], V, origin)
        parts.append((t["keys"] | c, t["pos"], t["nrm"]))
    if not parts:
        return rr.table(r, V, origin)
    keys, pos, nrm = (np.concatenate([p[i] for p in parts]) for i in range(3))
    order = np.argsort(keys, kind="stable")
    return dict(keys=keys[order], pos=pos[order], nrm=nrm[order], V=V)


def cover_table(rows, V, origin):
    """the keys (cell alone, face 0, class 0) of the cells that hold a record regular with V: uint64[K] ascending"""
    r = _rows(rows)
    r = r[rr.fields_ok(r)]
    ok, cell, _ = rr.grid(r[:, 0:3].astype(F64), V, origin)
    return np.unique(rr.pack(cell[ok], np.zeros(int(ok.sum()), I64)))


def _candidates(cell, off, V):
    """the eight cells of every point: (cell int64[8][N][3], in range bool[8][N])"""
    nb = np.where(2 * off >= V, cell + 1, cell - 1)
    out, inr = [], []
    for j in range(8):
        c = np.stack([np.where(j & 1, nb[:, 0], cell[:, 0]), np.where((j >> 1) & 1, nb[:, 1], cell[:, 1]),
                      np.where(j >> 2, nb[:, 2], cell[:, 2])], axis=1)
        ok = ((c >= -65536) & (c <= 65535)).all(axis=1)
        out.append(np.where(ok[:, None], c, 0))
        inr.append(ok)
    return out, inr


def compare(query, reference, pose=None, primary_only=False, **params):
    """sm_compare_maps of the sets' rows in id order (float32[N][12]); pose: 4x4, query world -> reference world, as the float32
    matrix the call gets.  Returns dict(labels uint8[N], counts [4], cells_fine, cells_cover, written float32[M][12])."""
    p = dict(DEFAULTS, **params)
    qr, ref = _rows(query), _rows(reference)
    V0 = rr.cell_edge(p["voxel_mm"])
    V1 = rr.cell_edge(int(p["voxel_mm"]) << int(p["cover_shift"]))
    fine = fine_table(ref, V0, p["origin"], p["match_class"])
    cover = cover_table(ref, V1, p["origin"])
    if len(fine["keys"]) > p["max_cells"] or len(cover) > p["max_cells"]:
        raise Capacity((len(fine["keys"]), len(cover)))
    T = np.eye(4) if pose is None else np.asarray(pose, F32).astype(F64).reshape(4, 4)
    N = len(qr)
    labels = np.full(N, LOOSE, np.uint8)
    regular = rr.fields_ok(qr)
    x, n = qr[:, 0:3].astype(F64), qr[:, 8:11].astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.stack([((T[k, 0] * x[:, 0] + T[k, 1] * x[:, 1]) + T[k, 2] * x[:, 2]) + T[k, 3] for k in range(3)], axis=1)
        nq = np.stack([(T[k, 0] * n[:, 0] + T[k, 1] * n[:, 1]) + T[k, 2] * n[:, 2] for k in range(3)], axis=1)
        ok0, cell, off = rr.grid(q, V0, p["origin"])
        ok1, ccell, coff = rr.grid(q, V1, p["origin"])
    labels[regular] = OUTSIDE
    idx = np.nonzero(regular & ok0 & ok1)[0]
    q, nq, cell, off, ccell, coff = q[idx], nq[idx], cell[idx], off[idx], ccell[idx], coff[idx]
    M = len(idx)
    cls = classes(qr)[idx] if p["match_class"] else np.zeros(M, np.uint64)
    reach = float(F32(p["reach_cells"])) * (float(V0) * (1.0 / 65536.0))
    cos_angle = math.cos(float(F32(p["angle_thresh"])) * (math.pi / 180.0))
    plane = float(int(p["plane_mm"])) / 1000.0
    an = np.abs(nq)
    m = an.max(axis=1) if M else np.zeros(0)
    primary = rr.face_of(nq) // 2 if M else np.zeros(0, I64)
    K = len(fine["keys"])
    sup = np.zeros(M, bool)
    cands, inr = _candidates(cell, off, V0)
    for a in range(3):
        use = (primary == a) if primary_only else (4.0 * an[:, a] >= m)
        face = 2 * a + (nq[:, a] < 0)
        for j in range(8):
            if not K:
                break
            ck = rr.pack(cands[j], face) | cls
            at = np.minimum(np.searchsorted(fine["keys"], ck), K - 1)
            hit = use & inr[j] & (fine["keys"][at] == ck)
            e = q - fine["pos"][at].astype(F64)
            nc = fine["nrm"][at].astype(F64)
            d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            r = (nc[:, 0] * e[:, 0] + nc[:, 1] * e[:, 1]) + nc[:, 2] * e[:, 2]
            dot = (nq[:, 0] * nc[:, 0] + nq[:, 1] * nc[:, 1]) + nq[:, 2] * nc[:, 2]
            sup |= hit & (np.sqrt(d2) <= reach) & (dot >= cos_angle) & (np.abs(r) <= plane)
    near = np.zeros(M, bool)
    cands, inr = _candidates(ccell, coff, V1)
    for j in range(8):
        if not len(cover):
            break
        ck = rr.pack(cands[j], np.zeros(M, I64))
        at = np.minimum(np.searchsorted(cover, ck), len(cover) - 1)
        near |= inr[j] & (cover[at] == ck)
    labels[idx] = np.where(sup, SUPPORTED, np.where(near, CHANGED, OUTSIDE))
    keep = ((int(p["write_mask"]) >> labels.astype(I64)) & 1).astype(bool)
    return dict(labels=labels, counts=[int((labels == l).sum()) for l in range(4)], cells_fine=K, cells_cover=len(cover),
                written=qr[keep].copy())


def compare_sets(query_parts, reference_parts, pose=None, **params):
    """sets: the parts (files in order, then the live model) get consecutive ids"""
    cat = lambda parts: np.concatenate([_rows(x) for x in parts]) if len(parts) else np.zeros((0, 12), F32)
    return compare(cat(query_parts), cat(reference_parts), pose, **params)
