"""Point queries through the drop-in facade (SurfelMapping::queryPoints, GlobalModel::queryPoints; tests/cpp/points_demo.cpp): the demo
compiles against the C-ABI alone; on the GPU the planes it writes equal those of the Python call."""
import os
import subprocess

import numpy as np
import pytest

import points_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
DEMO = os.path.join(ROOT, "tests", "cpp", "points_demo.cpp")
f32 = np.float32


def _build(tmp_path):
    exe = str(tmp_path / "points_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, DEMO, "-L" + LIBDIR, "-lsurfelmapping_hip",
                           "-Wl,-rpath," + LIBDIR])
    return exe


def test_points_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def _write_map(path, rows):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([0, 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, f32).tobytes())
    return str(path)


@pytest.mark.gpu
def test_facade_planes_equal_python(tmp_path):
    from surfelmapping_amd import capi
    exe = _build(tmp_path)
    rng = np.random.default_rng(2)
    n = 3000
    model = np.zeros((n, 12), f32)
    model[:, 0:3] = rng.uniform(-5.0, 5.0, (n, 3))
    model[:, 3] = 1.0
    model[:, 4] = rng.integers(0, 1 << 29, n).astype(np.uint32).view(f32)
    model[:, 8:11] = rng.normal(size=(n, 3))
    model[:, 11] = rng.uniform(0.05, 0.3, n)
    pts = np.zeros((700, 4), f32)
    pts[:, 0:3] = rng.uniform(-6.0, 6.0, (700, 3))
    pts[:, 3] = rng.uniform(0.0, 1.0, 700)
    pts[::50, 3] = np.inf
    pts[5, 3] = -1.0                                                          # an invalid point
    files = [_write_map(tmp_path / "a.bin", model[:1000]), _write_map(tmp_path / "b.bin", model[1000:2200])]
    live = _write_map(tmp_path / "live.bin", model[2200:])
    with open(tmp_path / "points.bin", "wb") as f:
        f.write(np.array([len(pts)], np.uint32).tobytes() + pts.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, live, "200", str(tmp_path / "points.bin"), str(out)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "points 700 bad 1 records 3000 chunks 3" in r.stdout, r.stdout
    raw = open(out, "rb").read()
    N = len(pts)
    got = dict(d2=np.frombuffer(raw, f32, N, 0), id=np.frombuffer(raw, np.int32, N, 4 * N), centre=np.frombuffer(raw, f32, 3 * N, 8 * N).reshape(N, 3),
               normal=np.frombuffer(raw, f32, 3 * N, 20 * N).reshape(N, 3), radius=np.frombuffer(raw, f32, N, 32 * N),
               rgb=np.frombuffer(raw, np.uint8, 3 * N, 36 * N).reshape(N, 3), sem=np.frombuffer(raw, np.uint8, N, 39 * N))
    assert len(raw) == 40 * N
    ctx = capi.SurfelMap(capi.make_config(64, 48, 50.0, 50.0, 31.5, 23.5, max_sqrt_vertices=200))
    try:
        ctx.upload_model(model[2200:])
        want = ctx.query_points(pts, files)
        alone = ctx.query_points(pts)
    finally:
        ctx.close()
    ref = pr.query(model, pts)
    assert 100 < (want["id"] >= 0).sum() < 700
    for k in pr.PLANES:
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
        assert np.array_equal(ref[k].view(np.uint8), want[k].view(np.uint8)), k
    assert f"model answers {int((alone['id'] >= 0).sum())} of 700" in r.stdout, r.stdout
