"""Hole filling through the drop-in facade (SurfelMapping::setFillHoles / setWriteDepth and both acquireImages overloads;
tests/cpp/fill_demo.cpp).  CPU: the caller compiles with plain g++ against the C-ABI only.  GPU: with both switches the PNGs in
image/, semantic/ and depth/ decode to the binding's arrays; without them the two old folders hold, byte for byte, the files the
writer has always produced for the plain renderers' output, and no depth/ appears."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import test_fill as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
CAM = (tf.RW, tf.RH, tf.RF, tf.RF, tf.RCX, tf.RCY)


def build_demo(tmp_path):
    exe = str(tmp_path / "fill_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "fill_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_fill_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def read_png(path):
    """an 8-bit grey / RGB or 16-bit grey PNG as sm_png.h writes it (filter 0 on every row, big-endian samples)"""
    b = open(path, "rb").read()
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(b):
        n, typ = struct.unpack(">I4s", b[pos:pos + 8])
        body = b[pos + 8:pos + 8 + n]
        assert zlib.crc32(typ + body) == struct.unpack(">I", b[pos + 8 + n:pos + 12 + n])[0]
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        if typ == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype = hdr[:4]
    ch = 3 if ctype == 2 else 1
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w * ch * depth // 8 + 1)
    assert depth in (8, 16) and np.all(raw[:, 0] == 0)
    if depth == 16:
        assert ch == 1
        return np.ascontiguousarray(raw[:, 1:]).view(">u2").astype(np.uint16)
    return raw[:, 1:].reshape(h, w, ch)


def png_bytes(img):
    """the file sm_png::write has always produced for an 8-bit image [h][w] or [h][w][3]: stored deflate blocks of 65535 bytes"""
    h, w = img.shape[:2]
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))
    z = b"\x78\x01"
    for pos in range(0, len(raw), 65535):
        blk = raw[pos:pos + 65535]
        z += bytes([1 if pos + 65535 >= len(raw) else 0]) + struct.pack("<HH", len(blk), len(blk) ^ 0xFFFF) + blk
    z += struct.pack(">I", zlib.adler32(raw))

    def chunk(typ, body):
        return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0)) + chunk(b"IDAT", z) +
            chunk(b"IEND", b""))


def model_image(bgr, sem):
    """fill_demo's line about the image that the live-model overload leaves in the model"""
    h, w = sem.shape
    return f"model image {w} x {h} bgr {bgr.size} sum {int(bgr.sum(dtype=np.int64))} sem {sem.size} sum {int(sem.sum(dtype=np.int64))}\n"


@pytest.mark.gpu
def test_facade_dumps_equal_the_binding(tmp_path):
    rows = tf.scene_rows()
    n0, n1 = 60, 150
    files = [tf.write_map(tmp_path / "a.bin", rows[:n0]), tf.write_map(tmp_path / "b.bin", rows[n0:n1])]
    live = tf.write_map(tmp_path / "live.bin", rows[n1:])
    views = tf.scene_views()
    with open(tmp_path / "views.bin", "wb") as f:
        f.write(np.array([len(views)], np.uint32).tobytes() + views.astype(np.float32).tobytes())
    exe = build_demo(tmp_path)
    levels = 4

    def run(fill, depth, out):
        r = subprocess.run([exe, live, "64", str(tmp_path / "views.bin")] + [repr(float(x)) if i >= 2 else str(x) for i, x in enumerate(CAM)] +
                           [str(fill), str(levels), str(depth), str(out)] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout

    m = tf._model(rows[n1:])
    p = dict(levels=levels)
    # ---- both switches on
    out = tmp_path / "on"
    stdout = run(1, 1, out)
    want_live = [m.render_image(v, *CAM, fill=p, depth=True) for v in views]
    want_set = m.render_image_maps(files, views, *CAM, fill=p, depth=True)
    st = m.fill_stats()
    assert (f"views {len(views)} valid {st['valid']} seen_through {st['seen_through']} filled {st['filled']} left_empty {st['left_empty']} "
            f"launches {st['launches']}\n") in stdout, stdout
    for k in range(len(views)):
        for sub, first, (bgr, sem, dep) in (("live", 0, want_live[k]), ("set", 5, [a[k] for a in want_set])):
            name = f"{first + k:06d}.png"
            assert np.array_equal(read_png(out / sub / "image" / name), bgr[..., ::-1]), (sub, k)
            assert np.array_equal(read_png(out / sub / "semantic" / name)[..., 0], sem), (sub, k)
            assert np.array_equal(read_png(out / sub / "depth" / name), dep), (sub, k)
    assert (want_set[2] > 0).any() and (want_set[1] > 0).mean() > 0.3
    assert model_image(want_live[-1][0], want_live[-1][1]) in stdout, stdout      # the model keeps the last view, as written
    # ---- each switch alone
    out = tmp_path / "depth_only"
    run(0, 1, out)
    bgr, sem, dep = m.render_image_maps(files, views[:1], *CAM, depth=True)
    assert np.array_equal(read_png(out / "set" / "depth" / "000005.png"), dep[0])
    assert open(out / "set" / "semantic" / "000005.png", "rb").read() == png_bytes(sem[0])
    out = tmp_path / "fill_only"
    run(1, 0, out)
    assert np.array_equal(read_png(out / "live" / "semantic" / "000000.png")[..., 0], want_live[0][1]) and not (out / "live" / "depth").exists()
    # ---- both off: the files of the plain renderers, and no depth/
    out = tmp_path / "off"
    stdout = run(0, 0, out)
    assert model_image(*m.render_image(views[-1], *CAM)) in stdout, stdout
    bgr, sem = m.render_image_maps(files, views, *CAM)
    for k, v in enumerate(views):
        b1, s1 = m.render_image(v, *CAM)
        for sub, first, (b, s) in (("live", 0, (b1, s1)), ("set", 5, (bgr[k], sem[k]))):
            name = f"{first + k:06d}.png"
            assert open(out / sub / "image" / name, "rb").read() == png_bytes(np.ascontiguousarray(b[..., ::-1])), (sub, k)
            assert open(out / sub / "semantic" / name, "rb").read() == png_bytes(s), (sub, k)
            assert not (out / sub / "depth").exists()
    m.close()
