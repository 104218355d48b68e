"""The packed map-file format (include/sm_c_api.h, "packed map files") restated in numpy: the encoder and the decoder, bit for bit.
Every float operation below is a single IEEE fp32 operation in the written order (numpy float32 arrays, no fused multiply-add),
which is what the kernels of csrc/sm_k_pack.h compute under the library's -ffp-contract=off.

  encode(rows, start_id, end_id, pos_step_log2=-10) -> (file bytes, raw flag per block)
  decode(file bytes)                                -> (rows float32[n, 12], (start_id, end_id), raw flag per block)
"""
from __future__ import annotations

import numpy as np

MAGIC = 0x4B504D53          # "SMPK", little-endian
VERSION = 1
BLOCK = 256
HEADER_BYTES = 32
DIR_BYTES = 32
PACKED_BYTES = 20
RAW_BYTES = 48
DIR_DTYPE = np.dtype([("origin", "<f4", 3), ("time_base", "<f4"), ("init_base", "<f4"), ("flags", "<u4"), ("offset", "<u8")])
assert DIR_DTYPE.itemsize == DIR_BYTES

f32 = np.float32


# ---- the normal: octahedral, 10 + 10 bits
def oct_encode(n):
    """n: float32[k, 3] -> (ou, ov) uint32[k] in 0..1023"""
    n = np.asarray(n, f32)
    with np.errstate(all="ignore"):
        a = (np.abs(n[:, 0]) + np.abs(n[:, 1])) + np.abs(n[:, 2])
        px, py = n[:, 0] / a, n[:, 1] / a
        sx = np.where(px >= f32(0), f32(1), f32(-1))
        sy = np.where(py >= f32(0), f32(1), f32(-1))
        fx, fy = (f32(1) - np.abs(py)) * sx, (f32(1) - np.abs(px)) * sy
        lower = n[:, 2] < f32(0)
        px, py = np.where(lower, fx, px), np.where(lower, fy, py)

        def code(p):
            v = np.floor((p * f32(0.5) + f32(0.5)) * f32(1023) + f32(0.5))
            v = np.where(v >= f32(0), v, f32(0))             # (a NaN becomes 0: such a record is never packed)
            return np.minimum(v, f32(1023)).astype(np.uint32)
        return code(px), code(py)


def oct_decode(ou, ov):
    """(ou, ov) in 0..1023 -> float32[k, 3]: the fold in integers on the codes, then one fp32 normalisation"""
    ui = 2 * np.asarray(ou, np.int64) - 1023
    vi = 2 * np.asarray(ov, np.int64) - 1023
    zi = 1023 - np.abs(ui) - np.abs(vi)
    t = np.maximum(-zi, 0)
    xi = np.where(ui >= 0, ui - t, ui + t)
    yi = np.where(vi >= 0, vi - t, vi + t)
    ln = np.sqrt((xi * xi + yi * yi + zi * zi).astype(f32))  # (the sum is < 2^22: exact in fp32)
    return np.stack([xi.astype(f32) / ln, yi.astype(f32) / ln, zi.astype(f32) / ln], axis=1)


# ---- the blocks
def _block_min(v, starts):
    return np.minimum.reduceat(v, starts) if len(v) else np.zeros(0, f32)


def _block_all(ok, starts):
    return np.logical_and.reduceat(ok, starts) if len(ok) else np.zeros(0, bool)


def plan(rows, pos_step_log2=-10):
    """What the encoder decides per block of 256 records: dict(raw bool[nb], origin float32[nb, 3], time_base, init_base float32[nb]);
    the bases of a RAW block are 0."""
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 12)
    n = len(rows)
    starts = np.arange(0, n, BLOCK)
    nb = len(starts)
    blk = np.arange(n) // BLOCK
    up, down = f32(2.0 ** -pos_step_log2), f32(2.0 ** pos_step_log2)
    bits = rows.view(np.uint32)
    with np.errstate(all="ignore"):
        x, c, it, t, nrm, r = rows[:, 0:3], rows[:, 3], rows[:, 6], rows[:, 7], rows[:, 8:11], rows[:, 11]
        ok = np.isfinite(rows[:, [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11]]).all(axis=1)          # (m[4] is a colour word: any bits)
        ok &= (np.abs(x) < f32(8192)).all(axis=1)
        ok &= (r >= f32(0)) & (np.floor(r * f32(8192) + f32(0.5)) <= f32(65535))
        ok &= (c >= f32(0)) & (np.floor(c * f32(16) + f32(0.5)) <= f32(4095))
        ok &= bits[:, 5] == 0
        for k in (6, 7):                                     # (as bits: +0 .. below 2^24)
            ok &= (bits[:, k] < 0x4B800000) & (np.floor(rows[:, k]) == rows[:, k])
        n2 = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        ok &= np.abs(n2 - f32(1)) <= f32(2.0 ** -10)
        origin = np.floor(np.stack([_block_min(x[:, k], starts) for k in range(3)], axis=1) * up) * down + f32(0) if nb else np.zeros((0, 3), f32)
        tb, ib = _block_min(t, starts), _block_min(it, starts)
        q = np.floor((x - origin[blk]) * up + f32(0.5))
        ok &= (q <= f32(65535)).all(axis=1)
        ok &= (t - tb[blk] <= f32(65535)) & (it - ib[blk] <= f32(65535))
    raw = ~_block_all(ok, starts)
    origin = np.where(raw[:, None], f32(0), origin).astype(f32)
    return dict(raw=raw, origin=origin, time_base=np.where(raw, f32(0), tb).astype(f32), init_base=np.where(raw, f32(0), ib).astype(f32))


def encode(rows, start_id=0, end_id=0, pos_step_log2=-10):
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 12)
    n = len(rows)
    pl = plan(rows, pos_step_log2)
    raw = pl["raw"]
    nb = len(raw)
    blk = np.arange(n) // BLOCK
    m = np.minimum(BLOCK, n - np.arange(nb) * BLOCK)
    size = np.where(raw, RAW_BYTES, PACKED_BYTES).astype(np.uint64) * m.astype(np.uint64)
    d = np.zeros(nb, DIR_DTYPE)
    d["origin"], d["time_base"], d["init_base"], d["flags"] = pl["origin"], pl["time_base"], pl["init_base"], raw.astype(np.uint32)
    d["offset"] = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.uint64) if nb else 0
    up = f32(2.0 ** -pos_step_log2)
    with np.errstate(all="ignore"):
        q = np.floor((rows[:, 0:3] - pl["origin"][blk]) * up + f32(0.5))
        qr = np.floor(rows[:, 11] * f32(8192) + f32(0.5))
        qc = np.floor(rows[:, 3] * f32(16) + f32(0.5))
        dt, di = rows[:, 7] - pl["time_base"][blk], rows[:, 6] - pl["init_base"][blk]
        ou, ov = oct_encode(rows[:, 8:11])
        keep = ~raw[blk]

        def u(v):
            return np.where(keep, v, 0).astype(np.int64).astype(np.uint32)
        w = np.zeros((n, 5), np.uint32)
        w[:, 0] = u(q[:, 0]) | u(q[:, 1]) << 16
        w[:, 1] = u(q[:, 2]) | u(qr) << 16
        w[:, 2] = rows.view(np.uint32)[:, 4]
        w[:, 3] = ou | ov << 10 | u(qc) << 20
        w[:, 4] = u(dt) | u(di) << 16
    payload = bytearray()
    for b in range(nb):
        sl = slice(b * BLOCK, b * BLOCK + int(m[b]))
        payload += rows[sl].tobytes() if raw[b] else w[sl].astype("<u4").tobytes()
    head = np.array([MAGIC, VERSION, n, start_id & 0xFFFFFFFF, end_id & 0xFFFFFFFF, pos_step_log2 & 0xFFFFFFFF, nb, 0], "<u4")
    return head.tobytes() + d.tobytes() + bytes(payload), raw


def decode(data):
    data = bytes(data)
    head = np.frombuffer(data, "<u4", 8)
    assert head[0] == MAGIC and head[1] == VERSION and head[7] == 0, "not a packed map file"
    n, nb = int(head[2]), int(head[6])
    start_id, end_id, s = (int(np.int32(v)) for v in head[3:6].view(np.int32))
    assert nb == (n + BLOCK - 1) // BLOCK and -14 <= s <= -6
    d = np.frombuffer(data, DIR_DTYPE, nb, HEADER_BYTES)
    base = HEADER_BYTES + DIR_BYTES * nb
    down = f32(2.0 ** s)
    rows = np.zeros((n, 12), f32)
    at = 0
    for b in range(nb):
        m = min(BLOCK, n - b * BLOCK)
        raw = bool(d["flags"][b] & 1)
        assert d["flags"][b] <= 1 and int(d["offset"][b]) == at, "bad directory"
        sl = slice(b * BLOCK, b * BLOCK + m)
        if raw:
            rows[sl] = np.frombuffer(data, "<f4", m * 12, base + at).reshape(m, 12)
            at += m * RAW_BYTES
            continue
        w = np.frombuffer(data, "<u4", m * 5, base + at).reshape(m, 5)
        at += m * PACKED_BYTES
        out = rows[sl]
        q = np.stack([w[:, 0] & 0xFFFF, w[:, 0] >> 16, w[:, 1] & 0xFFFF], axis=1).astype(f32)
        out[:, 0:3] = d["origin"][b] + q * down
        out[:, 3] = (w[:, 3] >> 20).astype(f32) * f32(1.0 / 16)
        out.view(np.uint32)[:, 4] = w[:, 2]
        out[:, 5] = 0
        out[:, 6] = d["init_base"][b] + (w[:, 4] >> 16).astype(f32)
        out[:, 7] = d["time_base"][b] + (w[:, 4] & 0xFFFF).astype(f32)
        out[:, 8:11] = oct_decode(w[:, 3] & 1023, (w[:, 3] >> 10) & 1023)
        out[:, 11] = (w[:, 1] >> 16).astype(f32) * f32(1.0 / 8192)
    assert len(data) == base + at, "length"
    return rows, (start_id, end_id), (d["flags"] & 1).astype(bool)


def packed_size(n, raw):
    """bytes of a packed file of n records with the given RAW flags"""
    m = np.minimum(BLOCK, n - np.arange(len(raw)) * BLOCK)
    return HEADER_BYTES + DIR_BYTES * len(raw) + int(np.where(raw, RAW_BYTES, PACKED_BYTES) @ m)


def plain_bytes(rows, start_id=0, end_id=0):
    rows = np.ascontiguousarray(rows, "<f4").reshape(-1, 12)
    return np.array([len(rows), start_id & 0xFFFFFFFF, end_id & 0xFFFFFFFF], "<u4").tobytes() + rows.tobytes()


# ---- the fixtures the tests share
def fixture_a(n, seed=0, tick=1000):
    """n rows of synth.seeded_model with integer times as the fusion writes them, drawn into a box that one block can span (a
    block packs only below 64 m of extent at the default step): every block of it packs"""
    from surfelmapping_amd import synth
    rows = synth.seeded_model(n, tick, seed)
    rows[:, 0] *= f32(0.25)                                  # x in [-15, 15], y in [-3, 5], z in [-10, 50]
    rows[:, 2] *= f32(0.2)
    return rows


RAW_CAUSES = ("nan_centre", "extent", "far", "conf_256", "conf_negative", "radius", "time_fraction", "time_span", "normal_length", "m5")


B_ROWS = (len(RAW_CAUSES) + 1) * BLOCK + 100


def fixture_b(seed=1, base=None):
    """(rows, the blocks that must be RAW): a clean block, one block for each cause of RAW, a clean short block; base: B_ROWS
    rows every block of which packs, in place of fixture_a's"""
    rows = fixture_a(B_ROWS, seed) if base is None else np.array(base, f32).reshape(B_ROWS, 12)
    for i, cause in enumerate(RAW_CAUSES):
        r = rows[(i + 1) * BLOCK + 17 * (i + 1) % BLOCK]     # one record of block i + 1
        if cause == "nan_centre":
            r[1] = np.nan
        elif cause == "extent":
            r[0] += f32(70)
        elif cause == "far":
            r[2] = f32(9000)
        elif cause == "conf_256":
            r[3] = f32(256)
        elif cause == "conf_negative":
            r[3] = f32(-1)
        elif cause == "radius":
            r[11] = f32(8.5)
        elif cause == "time_fraction":
            r[7] += f32(0.5)
        elif cause == "time_span":
            r[7] = f32(70000)
        elif cause == "normal_length":
            r[8:11] *= f32(1.1)
        elif cause == "m5":
            r[5] = f32(1)
    return rows, np.arange(1, len(RAW_CAUSES) + 1)
