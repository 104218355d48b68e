"""Voxel-cell simplification restated in numpy and Python integers (include/sm_c_api.h "simplification"; DESIGN.md "4p.
Simplification") -- the checker of tests/test_simplify.py.  Everything that the specification states in integers is a Python int
here; the float32 and float64 steps are numpy scalars of that type, one operation at a time."""
import math

import numpy as np

DEFAULTS = dict(voxel_mm=50, split_normals=1, origin=(0.0, 0.0, 0.0), max_cells=1 << 26)
F32, F64 = np.float32, np.float64


class Capacity(Exception):
    """more distinct cells than max_cells"""


def cell_edge(voxel_mm):
    return (int(voxel_mm) * 65536 + 500) // 1000


def _bits(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def classify(row, V, split, origin):
    """None for a loose record, else (key, off): key = (cx, cy, cz, face, class)"""
    x, y, z, conf, col, _, t0, t1, nx, ny, nz, rad = (F32(v) for v in row)
    if not all(np.isfinite(v) for v in (x, y, z, conf, t0, t1, nx, ny, nz, rad)):
        return None
    if not (conf > 0 and t0 >= 0 and t1 >= 0 and 0 <= rad < 32768) or (nx == 0 and ny == 0 and nz == 0):
        return None
    cell, off = [], []
    for p, o in zip((x, y, z), origin):
        d = F64(p) - F64(F32(o))
        if not abs(d) < 2.0 ** 24:
            return None
        X = int(math.floor(d * F64(65536.0)))
        c = X // V
        if not -65536 <= c <= 65535:
            return None
        cell.append(c)
        off.append(X - c * V)
    face = 0
    if split:
        n = (nx, ny, nz)
        a = 0
        if abs(n[1]) > abs(n[a]):
            a = 1
        if abs(n[2]) > abs(n[a]):
            a = 2
        face = 2 * a + (1 if n[a] < 0 else 0)
    return (cell[0], cell[1], cell[2], face, _bits(col) >> 24), off


def contribution(row, off, gid):
    conf, col = F32(row[3]), _bits(row[4])
    t = conf * F32(16.0)
    w = 255 if t >= 255 else max(1, int(t))
    ni = [int(min(max(np.floor(F32(n) * F32(16384.0) + F32(0.5)), F32(-4194304.0)), F32(4194304.0))) for n in row[8:11]]
    return dict(n=1, SW=w, SP=[w * o for o in off], SN=[w * v for v in ni], SC=[w * ((col >> (8 * c)) & 255) for c in range(3)],
                lo=list(off), hi=list(off), Rmax=int(math.floor(F64(F32(row[11])) * F64(65536.0))), conf=_bits(row[3]), time=_bits(row[7]),
                init=_bits(row[6]), first=gid)


def merge(a, b):
    for k in ("n", "SW"):
        a[k] += b[k]
    for k in ("SP", "SN", "SC"):
        a[k] = [x + y for x, y in zip(a[k], b[k])]
    a["lo"] = [min(x, y) for x, y in zip(a["lo"], b["lo"])]
    a["hi"] = [max(x, y) for x, y in zip(a["hi"], b["hi"])]
    for k in ("Rmax", "conf", "time"):
        a[k] = max(a[k], b[k])
    a["init"] = min(a["init"], b["init"])
    a["first"] = min(a["first"], b["first"])


def finish(key, c, V, origin, first_row):
    """the record of a cell with two or more contributors"""
    out = np.zeros(12, F32)
    SW = c["SW"]
    for k in range(3):
        X = key[k] * V + (c["SP"][k] + SW // 2) // SW
        out[k] = F32(F64(F32(origin[k])) + F64(X) * F64(2.0 ** -16))
    col = key[4] << 24
    for ch in range(3):
        col |= ((c["SC"][ch] + SW // 2) // SW) << (8 * ch)
    out.view(np.uint32)[3:8] = (c["conf"], col, 0, c["init"], c["time"])      # (bit patterns, as they are)
    s = max(0, max(abs(v) for v in c["SN"]).bit_length() - 24)
    f = [F32(v >> s) for v in c["SN"]]
    if all(v == 0 for v in f):
        out[8:11] = first_row[8:11]
    else:
        ln = np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
        assert ln.dtype == F32
        out[8:11] = [v / ln for v in f]
    e = [h - l for h, l in zip(c["hi"], c["lo"])]
    R = max(c["Rmax"], (math.isqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) + 1) // 2)
    out[11] = F32(F64(R) * F64(2.0 ** -16))
    return out


def simplify(rows, ids=None, **params):
    """rows: float32[N][12] with global ids `ids` (default: 0..N-1), in any order.  Returns (float32[M][12], stats)."""
    p = dict(DEFAULTS, **params)
    rows = np.ascontiguousarray(rows, F32).reshape(-1, 12)
    ids = list(range(len(rows))) if ids is None else [int(i) for i in ids]
    V = cell_edge(p["voxel_mm"])
    cells, reps = {}, []                                   # reps: (id, key or None)
    by_id = {}
    for row, gid in zip(rows, ids):
        by_id[gid] = row
        got = classify(row, V, p["split_normals"], p["origin"])
        if got is None:
            reps.append((gid, None))
            continue
        key, off = got
        c = contribution(row, off, gid)
        if key in cells:
            merge(cells[key], c)
        else:
            cells[key] = c
    if len(cells) > p["max_cells"]:
        raise Capacity(len(cells))
    reps += [(c["first"], key) for key, c in cells.items()]
    reps.sort(key=lambda r: r[0])
    out = np.zeros((len(reps), 12), F32)
    for i, (gid, key) in enumerate(reps):
        if key is None or cells[key]["n"] == 1:
            out[i] = by_id[gid]
        else:
            out[i] = finish(key, cells[key], V, p["origin"], by_id[gid])
    ns = [c["n"] for c in cells.values()]
    stats = dict(records_in=len(rows), records_out=len(reps), cells_merged=sum(1 for n in ns if n >= 2), loose=len(reps) - len(cells),
                 largest_cell=max(ns, default=0))
    return out, stats


def simplify_set(parts, **params):
    """a set: the parts (files in order, then the live model) get consecutive ids"""
    parts = [np.ascontiguousarray(x, F32).reshape(-1, 12) for x in parts]
    return simplify(np.concatenate(parts) if parts else np.zeros((0, 12), F32), **params)
