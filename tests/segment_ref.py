"""Segmentation of a map set into connected voxel components, restated (sm_segment_maps; include/sm_c_api.h, "segmentation";
DESIGN.md "4t. Segmentation").  This file is the contract the HIP path is compared with, bit for bit.

A set is a list of (global id, record) pairs; a record is 12 float32 (48 bytes): x y z conf | colour word, -, t0, t1 | nx ny nz radius.

Grid.      V = (voxel_mm * 65536 + 500) // 1000;  X[k] = floor((float64(p[k]) - float64(origin[k])) * 65536.0);  cell[k] = X[k] // V
           (floor division).
Regular.   The simplification's test: every field finite, conf > 0, t0 >= 0, t1 >= 0, 0 <= radius < 32768, a normal that is not
           (0, 0, 0), |float64(p[k]) - float64(origin[k])| < 2^24, every cell[k] in [-65536, 65535].  c = colour word >> 24.
Label.     The first rule that applies: LOOSE if the record is not regular; SKIPPED if bit c & 31 of class_mask[c >> 5] is clear;
           otherwise it belongs to the node (cell, kc), kc = c with by_class, else 0.
Edges.     Two nodes with the same kc whose cells differ by d in {-1, 0, 1}^3 \\ {0} with |d|_1 <= 1 (connectivity 6), 2 (18), 3 (26).
           A cell outside [-65536, 65535] on an axis does not exist.
Component. A connected component: records (in its nodes), cells (its nodes), first (the smallest id among its records), cell_lo and
           cell_hi (the box of its cells), sum_cell[k] (the sum over its records of cell[k] + 65536), cls (kc with by_class, else -1).
Small.     records < min_records: its records are SMALL, it has no number and no row.
Numbers.   The other components 0, 1, ... in ascending `first`; their records carry the number.
File.      The records whose kind (0 a number, 1 SMALL, 2 SKIPPED, 3 LOOSE) has its bit in write_mask, in id order.

Worked by hand, voxel_mm = 1000 (V = 65536), origin 0, one class, ids 0..4:
  A (.5, .5, .5) cell (0,0,0);  B (1.5, .5, .5) (1,0,0);  C (2.5, 1.5, .5) (2,1,0);  D (3.5, 2.5, 1.5) (3,2,1);  E (5.5, .5, .5) (5,0,0)
  A-B differ by (1,0,0): |d|_1 = 1.  B-C by (1,1,0): 2.  C-D by (1,1,1): 3.  D-E by (2,..): no edge.
  6: {A,B} {C} {D} {E};  18: {A,B,C} {D} {E};  26: {A,B,C,D} {E}.
  26 with min_records 2: E is SMALL; one row: first 0, records 4, cells 4, cell_lo (0,0,0), cell_hi (3,2,1),
  sum_cell (4 * 65536 + 0+1+2+3, 4 * 65536 + 0+0+1+2, 4 * 65536 + 0+0+0+1)."""
import itertools
import struct

import numpy as np

LOOSE, SMALL, SKIPPED = 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
KIND_CODE = (None, SMALL, SKIPPED, LOOSE)
DEFAULTS = dict(voxel_mm=200, connectivity=26, by_class=1, class_mask=(0xFFFFFFFF,) * 8, min_records=1, write_mask=1, max_cells=1 << 24,
                origin=(0.0, 0.0, 0.0))
COMPONENT = np.dtype([("first", "<u4"), ("records", "<u4"), ("cells", "<u4"), ("cls", "<i4"), ("cell_lo", "<i4", 3), ("cell_hi", "<i4", 3),
                      ("sum_cell", "<u8", 3)])


class Capacity(Exception):
    """more nodes than max_cells"""


def cell_edge(voxel_mm):
    return (int(voxel_mm) * 65536 + 500) // 1000


def class_mask(classes):
    words = [0] * 8
    for c in classes:
        words[c >> 5] |= 1 << (c & 31)
    return tuple(words)


def cells(rows, voxel_mm=200, origin=(0.0, 0.0, 0.0)):
    """(regular as bool, cell as int64[n, 3] (0 where the row is loose), class as int64) per row"""
    rows = np.asarray(rows, np.float32).reshape(-1, 12)
    V = cell_edge(voxel_mm)
    conf, t0, t1, rad, nrm = rows[:, 3], rows[:, 6], rows[:, 7], rows[:, 11], rows[:, 8:11]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(rows[:, [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]]).all(axis=1)
        ok &= (conf > 0) & (t0 >= 0) & (t1 >= 0) & (rad >= 0) & (rad < 32768) & ~(nrm == 0).all(axis=1)
        cell = np.zeros((len(rows), 3), np.int64)
        for k in range(3):
            d = rows[:, k].astype(np.float64) - np.float64(np.float32(origin[k]))
            fine = np.isfinite(d) & (np.abs(d) < 16777216.0)
            X = np.floor(np.where(fine, d, 0.0) * 65536.0).astype(np.int64)
            c = X // V                                                       # (numpy's // on integers is floor division)
            fine &= (c >= -65536) & (c <= 65535)
            cell[:, k] = np.where(fine, c, 0)
            ok &= fine
    cell[~ok] = 0
    cls = (np.ascontiguousarray(rows[:, 4]).view(np.uint32) >> np.uint32(24)).astype(np.int64)
    return ok, cell, cls


def offsets(connectivity):
    max_l1 = {6: 1, 18: 2, 26: 3}[connectivity]
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(v) for v in d) <= max_l1]


def _pack(cell, kc):
    """(cell + 65536 per axis, 17 bits each, x highest) << 8 | kc: one int64 per node, its order is of no consequence"""
    u = cell + 65536
    return (((u[:, 0] << 17 | u[:, 1]) << 17 | u[:, 2]) << 8) | kc


def segment(rows, ids=None, voxel_mm=200, connectivity=26, by_class=1, class_mask=(0xFFFFFFFF,) * 8, min_records=1, write_mask=1,
            max_cells=1 << 24, origin=(0.0, 0.0, 0.0)):
    """-> dict(labels: uint32 per row, in the order the rows were given; components: COMPONENT rows; info; kept: the file's rows).
    ids: the rows' global ids (default: their positions)"""
    rows = np.asarray(rows, np.float32).reshape(-1, 12)
    n = len(rows)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    ok, cell, cls = cells(rows, voxel_mm, origin)
    words = np.asarray(class_mask, np.uint64)
    takes_part = ((words[cls >> 5] >> (cls & 31).astype(np.uint64)) & np.uint64(1)).astype(bool)
    kind = np.where(~ok, 3, np.where(~takes_part, 2, 0))
    labels = np.zeros(n, np.uint32)
    labels[kind == 3], labels[kind == 2] = LOOSE, SKIPPED

    idx = np.flatnonzero(kind == 0)
    kc = cls[idx] if by_class else np.zeros(len(idx), np.int64)
    packed = _pack(cell[idx], kc)
    nodes, first_at, node_of = np.unique(packed, return_index=True, return_inverse=True)
    if len(nodes) > max_cells:
        raise Capacity("more than max_cells nodes")
    ncell, nkc = cell[idx][first_at], kc[first_at]       # a node's cell and class, from one of its records

    # union-find over the nodes: every edge from its lower end
    parent = list(range(len(nodes)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for d in offsets(connectivity):
        if d <= (0, 0, 0):
            continue                                                         # (the other half of the neighbourhood gives the same pairs)
        nb = ncell + np.asarray(d, np.int64)
        exists = ((nb >= -65536) & (nb <= 65535)).all(axis=1)                # dropped before it is packed: no carry into another field
        want = _pack(np.where(exists[:, None], nb, 0), nkc)
        at = np.searchsorted(nodes, want)
        at[at == len(nodes)] = 0
        hit = exists & (nodes[at] == want) if len(nodes) else exists & False
        for a, b in zip(np.flatnonzero(hit).tolist(), at[hit].tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    root = np.asarray([find(x) for x in range(len(nodes))], np.int64)
    roots, comp_of_node = np.unique(root, return_inverse=True)
    comp = comp_of_node[node_of]                         # per record of idx
    C = len(roots)
    records = np.bincount(comp, minlength=C).astype(np.int64)
    ncells = np.bincount(comp_of_node, minlength=C).astype(np.int64)
    first = np.full(C, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, comp, ids[idx])
    lo, hi = np.full((C, 3), 1 << 20, np.int64), np.full((C, 3), -(1 << 20), np.int64)
    np.minimum.at(lo, comp_of_node, ncell)
    np.maximum.at(hi, comp_of_node, ncell)
    sums = np.zeros((C, 3), np.int64)
    np.add.at(sums, comp, cell[idx] + 65536)

    numbered = records >= min_records
    order = np.argsort(np.where(numbered, first, np.iinfo(np.int64).max), kind="stable")[:int(numbered.sum())]
    number = np.full(C, -1, np.int64)
    number[order] = np.arange(len(order))
    lab = number[comp]
    kind[idx[lab < 0]] = 1
    labels[idx] = np.where(lab < 0, SMALL, lab).astype(np.uint32)
    table = np.zeros(len(order), COMPONENT)
    table["first"], table["records"], table["cells"] = first[order], records[order], ncells[order]
    table["cls"] = nkc[roots[order]] if by_class else -1
    table["cell_lo"], table["cell_hi"], table["sum_cell"] = lo[order], hi[order], sums[order]

    keep = np.flatnonzero((write_mask >> kind) & 1)
    keep = keep[np.argsort(ids[keep], kind="stable")]
    info = dict(records=n, counts_by_kind=[int((kind == k).sum()) for k in range(4)], written=len(keep), cells=len(nodes), components=len(order),
                small_components=int((~numbered).sum()), largest=int(records.max()) if C else 0)
    return dict(labels=labels, components=table, info=info, kept=rows[keep])


def segment_set(parts, **params):
    """the segmentation of a set given as its parts in order (files, then the live model): ids run on across them"""
    parts = [np.asarray(p, np.float32).reshape(-1, 12) for p in parts]
    return segment(np.concatenate(parts) if parts else np.zeros((0, 12), np.float32), **params)


def file_bytes(rows, start_id=0, end_id=0):
    """a map file with these rows: u32 count | i32 startId | i32 endId | the records"""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 12)
    return struct.pack("<Iii", len(rows), start_id, end_id) + rows.tobytes()
