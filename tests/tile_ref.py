"""Spatial tiling of a map set, restated (sm_tile_maps; include/sm_c_api.h, "tiling"; DESIGN.md "4s. Spatial tiling").  This file
is the contract the HIP path is compared with, byte for byte.

A set is a list of (global id, record) pairs; a record is 12 float32 (48 bytes) and only its first three, the centre, are examined.

Grid.    V = (cell_mm * 65536 + 500) // 1000;  X[k] = floor((float64(p[k]) - float64(origin[k])) * 65536.0);  cell[k] = X[k] // V
         (floor division).
Placed.  x, y, z finite, |float64(p[k]) - float64(origin[k])| < 2^24 and every cell[k] in [-65536, 65535].  Every other record is
         loose.  conf <= 0, a NaN normal, a negative radius do not matter.
Key.     u[k] = cell[k] + 65536 in [0, 2^17); bit 3 i + k of M is bit i of u[k] (x lowest): 51 bits.
Tile.    M >> (3 * tile_shift).
Order.   Placed records in ascending (M, id), then the loose ones in ascending id.
Files.   Tiles in ascending id; a file takes successive whole tiles while its count stays <= max_file_records; a tile with more
         records is written alone as consecutive files of max_file_records records, the last shorter; the loose records form one
         last file.  An empty set has no file.

Worked by hand, cell_mm = 1000 (V = 65536), origin 0, so that cell[k] = floor(p[k]):
  A (.5, .5, .5)    cells (0, 0, 0),  u = (65536, 65536, 65536) = bit 16 of each: bits 48, 49, 50 of M = 0x7000000000000
  G (-0.0, .5, .5)  -0.0 - 0.0 = -0.0, floor(-0.0 * 65536) = -0.0 -> X = 0, cell 0: the same key as A
  F (-.5, .5, .5)   X = -32768, cell -1, u[0] = 65535 = bits 0..15: bits 0, 3, .., 45 of M = 0x0249249249249; y, z as A: bits 49, 50
                    = 0x6000000000000; M = 0x6249249249249
  B (1.5, .5, .5)   u[0] = 65537 = bits 16 and 0: M = 0x7000000000000 | 1 << 0 = 0x7000000000001
  C (.5, 1.5, .5)   bit 0 of u[1]: bit 1 of M: 0x7000000000002
  D (.5, .5, 1.5)   bit 0 of u[2]: bit 2 of M: 0x7000000000004
  E (2.5, .5, .5)   u[0] = 65538 = bits 16 and 1: bit 3 of M: 0x7000000000008
Order: F, then A and G by id, then B, C, D, E.  With tile_shift = 1 (M >> 3): A, G, B, C, D share tile 0xE00000000000, E has
0xE00000000001, F has 0xC49249249249.
Other edges: cell_mm 100 -> V = 6554, 200 -> 13107, 10 -> 655 (65536 cells of 655 / 65536 m: the grid ends at +-429 m)."""
import struct

import numpy as np

DEFAULTS = dict(cell_mm=200, tile_shift=7, origin=(0.0, 0.0, 0.0), max_file_records=1 << 20, max_tiles=1 << 20)
SORT_RECORDS = 1 << 22


class Capacity(Exception):
    pass


def cell_edge(cell_mm):
    return (int(cell_mm) * 65536 + 500) // 1000


def keys(rows, cell_mm=200, origin=(0.0, 0.0, 0.0)):
    """(M as uint64, placed as bool) per row; M is 0 where the row is loose"""
    rows = np.asarray(rows, np.float32).reshape(-1, 12)
    V = cell_edge(cell_mm)
    placed = np.ones(len(rows), bool)
    M = np.zeros(len(rows), np.uint64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            d = rows[:, k].astype(np.float64) - np.float64(np.float32(origin[k]))
            ok = np.isfinite(rows[:, k]) & (np.abs(d) < 16777216.0)
            X = np.floor(np.where(ok, d, 0.0) * 65536.0).astype(np.int64)
            cell = X // V                                                    # (numpy's // on integers is floor division)
            ok &= (cell >= -65536) & (cell <= 65535)
            u = np.where(ok, cell + 65536, 0).astype(np.uint64)
            for i in range(17):
                M |= ((u >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i + k)
            placed &= ok
    M[~placed] = 0
    return M, placed


def plan_files(counts, limit):
    """records per file for the tiles' record counts, the tiles in ascending id"""
    files, cur = [], 0
    for n in counts:
        n = int(n)
        if n > limit:
            if cur:
                files.append(cur)
            cur = 0
            while n:
                files.append(min(n, limit))
                n -= min(n, limit)
            continue
        if cur + n > limit:
            files.append(cur)
            cur = 0
        cur += n
    if cur:
        files.append(cur)
    return files


def plan_batches(counts, capacity):
    """records per batch: maximal runs of successive whole tiles of at most `capacity` records; a larger tile is Capacity"""
    batches = []
    for n in counts:
        n = int(n)
        if n > capacity:
            raise Capacity("a tile above the sort capacity")
        if not batches or batches[-1] + n > capacity:
            batches.append(0)
        batches[-1] += n
    return batches


def tile(rows, ids=None, cell_mm=200, tile_shift=7, origin=(0.0, 0.0, 0.0), max_file_records=1 << 20, max_tiles=1 << 20, capacity=SORT_RECORDS):
    """-> (the files' rows, a list of float32 arrays in order; the tally).  ids: the rows' global ids (default: their positions)"""
    rows = np.asarray(rows, np.float32).reshape(-1, 12)
    ids = np.arange(len(rows), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    M, placed = keys(rows, cell_mm, origin)
    pi, li = np.flatnonzero(placed), np.flatnonzero(~placed)
    pi = pi[np.lexsort((ids[pi], M[pi]))]                                    # (the last key is the primary one)
    li = li[np.argsort(ids[li], kind="stable")]
    tiles, counts = np.unique(M[pi] >> np.uint64(3 * tile_shift), return_counts=True)
    if len(tiles) > max_tiles:
        raise Capacity("more than max_tiles tiles")
    batches = plan_batches(counts, capacity)
    want = plan_files(counts, max_file_records)
    ordered = rows[pi]
    files, at = [], 0
    for n in want:
        files.append(ordered[at:at + n])
        at += n
    assert at == len(pi)
    if len(li):
        files.append(rows[li])
    stats = dict(records_in=len(rows), placed=len(pi), loose=len(li), tiles=len(tiles), largest_tile=int(counts.max()) if len(counts) else 0,
                 files_written=len(files), batches=batches, file_records=want)
    return files, stats


def tile_set(parts, **params):
    """the tiling of a set given as its parts in order (files, then the live model): ids run on across them"""
    parts = [np.asarray(p, np.float32).reshape(-1, 12) for p in parts]
    return tile(np.concatenate(parts) if parts else np.zeros((0, 12), np.float32), **params)


def file_bytes(rows, start_id=0, end_id=0):
    """a map file with these rows: u32 count | i32 startId | i32 endId | the records"""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 12)
    return struct.pack("<Iii", len(rows), start_id, end_id) + rows.tobytes()


def spans_a_batch_boundary(stats):
    """does a file of the plan hold records of two batches?"""
    cuts, at = set(), 0
    for n in stats["batches"][:-1]:
        at += n
        cuts.add(at)
    at = 0
    for n in stats["file_records"]:
        if any(at < c < at + n for c in cuts):
            return True
        at += n
    return False
