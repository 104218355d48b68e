"""Views of a map set through the drop-in facade (SurfelMapping::acquireImages and GlobalModel::renderModelImage with a list of
map files; surfelmapping_amd/csrc/facade).  CPU: a caller compiles with plain g++ against the C-ABI only.  GPU: the PNGs and the
model views it writes equal SurfelMap.render_image_maps / render_model_maps for the same files and views, with processFrame
synchronous and asynchronous (SM_FACADE_ASYNC)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import retire_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "render_maps_demo.cpp")
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
N, SQRT, EVERY, MIN_AGE, MIN_DISTANCE = 45, 440, 10, 8, 15.0


def build_demo(tmp_path):
    exe = str(tmp_path / "render_maps_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC,
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_render_maps_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def read_png(path):
    """an 8-bit grey or RGB PNG as sm_png.h writes it (filter 0 on every row)"""
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
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w * ch + 1)
    assert depth == 8 and np.all(raw[:, 0] == 0)
    return raw[:, 1:].reshape(h, w, ch)


@pytest.mark.gpu
@pytest.mark.parametrize("facade_async", ["0", "1"])
def test_facade_views_of_the_map_set_equal_python(tmp_path, facade_async):
    import model_view_ref as ref
    from surfelmapping_amd import capi, synth
    cam, seq = rr.CAM, rr.sequence(N)
    frames = tmp_path / "frames.bin"
    with open(frames, "wb") as f:
        f.write(np.array([cam["width"], cam["height"], len(seq)], np.uint32).tobytes())
        f.write(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32).tobytes())
        for rgb, d, s, p in seq:
            f.write(rgb.tobytes()); f.write(d.tobytes()); f.write(s.tobytes()); f.write(p.astype(np.float32).tobytes())
    P = synth.pose_matrix
    views = np.stack([synth.pose_to_colmajor(p) for p in (P(0, 0, 4.0), P(0, 0, 35.0, 180.0), P(0, 0, 20.0, 90.0), P(0, -400.0, 0))])
    with open(tmp_path / "views.bin", "wb") as f:
        f.write(np.array([len(views)], np.uint32).tobytes() + views.astype(np.float32).tobytes())
    w, h = 200, 150
    Pm = ref.projection(w, h, 420.0 * w / 640, 420.0 * h / 480, 320.0 * w / 640, 240.0 * h / 480, 0.1, 1000.0)
    MV = ref.look_at(0.0, -12.0, -10.0, 0.0, -12.0, 20.0, 0, -1, 0)      # axis-aligned: its inverse is exact in any method
    with open(tmp_path / "camera.bin", "wb") as f:
        f.write((Pm @ MV).T.reshape(16).astype(np.float64).tobytes())
        f.write(MV.T.reshape(16).astype(np.float64).tobytes())
        f.write(np.array([w, h], np.int32).tobytes())
    out_dir, out_img = tmp_path / "views", tmp_path / "images.bin"
    out_dir.mkdir()
    r = subprocess.run([build_demo(tmp_path), str(frames), str(SQRT), str(EVERY), str(MIN_AGE), str(MIN_DISTANCE), str(tmp_path / "cpp"),
                        str(tmp_path / "views.bin"), str(tmp_path / "camera.bin"), str(out_dir), str(out_img)],
                       capture_output=True, text=True, env=dict(os.environ, SM_FACADE_ASYNC=facade_async))
    assert r.returncode == 0, r.stdout + r.stderr
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=SQRT))
    m.set_auto_retire(EVERY, str(tmp_path / "py"), min_age=MIN_AGE, min_distance=MIN_DISTANCE)
    for fr in seq:
        m.process_frame(*fr)
    files, surfels = m.auto_retire_stats()
    assert files == N // EVERY
    assert f"files {files} surfels {surfels} count {m.counts()['count']} views {len(views)}\n" in r.stdout, r.stdout
    paths = [str(tmp_path / f"cpp_{i:06d}.bin") for i in range(files)]        # the files the facade wrote
    bgr, sem = m.render_image_maps(paths, views, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    for k in range(len(views)):
        img = read_png(str(out_dir / "image" / f"{3 + k:06d}.png"))
        lab = read_png(str(out_dir / "semantic" / f"{3 + k:06d}.png"))
        assert np.array_equal(img, bgr[k][..., ::-1]) and np.array_equal(lab[..., 0], sem[k]), k
    assert (sem[:3] > 0).mean() > 0.3 and not sem[3].any()
    imgs = np.frombuffer(open(out_img, "rb").read(), np.uint8).reshape(4, h, w, 4)
    mvp, inv = ref.view_mats(Pm, MV)
    kw = dict(threshold=0.5, unstable=True, time=len(seq), time_delta=1, clear=(51, 102, 153, 255))
    modes = [(dict(color_type=0), True), (dict(color_type=3), True), (dict(color_type=2, points=True), True), (dict(color_type=0), False)]
    for img, (mode, inc) in zip(imgs, modes):
        want = m.render_model_maps(paths, [capi.model_view(mvp, inv, w, h, **kw, **mode)], include_model=inc)[0]
        assert np.array_equal(img, want), (mode, inc)
        cleared = (want == (51, 102, 153, 255)).all(-1)
        assert 0.02 < 1.0 - cleared.mean() < 1.0                      # something is drawn, something is not
    assert not np.array_equal(imgs[0], imgs[3])                       # the live model shows
