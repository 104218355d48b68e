"""Scenes through the drop-in facade (SurfelMapping::acquireSceneImages / acquireSceneSweeps; tests/cpp/scene_demo.cpp): the demo
compiles against the C-ABI alone; on the GPU its PNGs and velodyne files equal the planes of the Python calls, and with setBlend on
the scene call refuses."""
import os
import subprocess

import numpy as np
import pytest

import retire_ref as rr
import scene_ref as sr
from test_scene import CAM, IMG, OVER, STREET, write_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
DEMO = os.path.join(ROOT, "tests", "cpp", "scene_demo.cpp")
f32 = np.float32


def _build(tmp_path):
    exe = str(tmp_path / "scene_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, DEMO, "-L" + LIBDIR, "-lsurfelmapping_hip",
                           "-Wl,-rpath," + LIBDIR])
    return exe


def test_scene_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def _read_png(path):
    import struct
    import zlib
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, colour = head[:4]
    ch = {0: 1, 2: 3}[colour]
    bpp = ch * depth // 8
    data = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * bpp)
    assert (data[:, 0] == 0).all()                                        # the facade's writer uses filter 0 on every row
    px = data[:, 1:]
    if depth == 16:
        return px.reshape(h, w, 2).astype(np.uint16)[:, :, 0] << 8 | px.reshape(h, w, 2)[:, :, 1]
    return px.reshape(h, w, ch) if ch == 3 else px.reshape(h, w)


@pytest.mark.gpu
def test_facade_files_equal_the_python_planes(tmp_path):
    import oracle_lib as ol
    from surfelmapping_amd import capi
    exe = _build(tmp_path)
    seq = rr.sequence(10)
    cpu = ol.Oracle(ol.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=440))
    for fr in seq:
        cpu.process_frame(*fr)
    S = sr.street_setup(cpu.download_model(), [fr[3] for fr in seq])
    static = [write_map(tmp_path / f"static_{i}.bin", r) for i, r in enumerate(S["static"])]
    views = S["views"]
    with open(tmp_path / "views.bin", "wb") as f:
        f.write(np.array([len(views)], np.uint32).tobytes() + np.ascontiguousarray(views, f32).tobytes())
    args, actors = [], []
    for j, (name, rows, poses, present) in enumerate(S["actors"]):
        path = write_map(tmp_path / f"actor_{name}.bin", rows)
        m = np.tile(np.eye(4, dtype=f32), (len(poses), 1, 1))
        m[:, :3, :] = poses.reshape(-1, 3, 4)
        pr = np.ones(len(poses), np.uint8) if present is None else present
        with open(tmp_path / f"poses_{j}.bin", "wb") as f:
            f.write(np.array([len(poses)], np.uint32).tobytes() + np.ascontiguousarray(m.transpose(0, 2, 1)).tobytes() + pr.tobytes())
        args += [path, str(tmp_path / f"poses_{j}.bin")]
        actors.append((path, poses, present))
    out = tmp_path / "out"
    out.mkdir()
    w, h, fx, fy, cx, cy = IMG
    r = subprocess.run([exe, "440", str(tmp_path / "views.bin"), str(out), str(w), str(h), repr(fx), repr(fy), repr(cx), repr(cy), str(len(static))]
                       + static + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "views 3 actors 5 files 3 records 601" in r.stdout and "blended views draw no scenes" in r.stdout and "blend refused" in r.stdout

    ctx = capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=440))
    try:
        bgr, sem, depth = ctx.render_scene(static, actors, views, *IMG, include_model=False, fill=True, depth=True)
        sn = capi.lidar_sensor(**STREET)
        sweeps = ctx.lidar_sweep_scene(static, actors, views, sn, include_model=False)
        dirs = capi.lidar_directions(sn)
    finally:
        ctx.close()
    assert (sem == sr.ACTOR_CLASS + 1).any(axis=(1, 2)).all()
    for k in range(len(views)):
        name = f"{k:06d}"
        assert np.array_equal(_read_png(out / "image" / f"{name}.png"), bgr[k][:, :, ::-1]), k
        assert np.array_equal(_read_png(out / "semantic" / f"{name}.png"), sem[k]), k
        assert np.array_equal(_read_png(out / "depth" / f"{name}.png"), depth[k]), k
        pts = np.fromfile(out / "velodyne" / f"{name}.bin", f32).reshape(-1, 4)
        want = capi.lidar_points(sweeps["range"][k], dirs, sweeps["rgb"][k])
        assert len(want) > 100 and np.array_equal(pts.view(np.uint32), want.view(np.uint32)), k
