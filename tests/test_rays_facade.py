"""Ray casts through the drop-in facade (SurfelMapping::castRays, GlobalModel::castRays; tests/cpp/rays_demo.cpp): the demo compiles
against the C-ABI alone; on the GPU the planes it writes equal those of the Python call."""
import os
import subprocess

import numpy as np
import pytest

import rays_ref as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
DEMO = os.path.join(ROOT, "tests", "cpp", "rays_demo.cpp")
f32 = np.float32


def _build(tmp_path):
    exe = str(tmp_path / "rays_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, DEMO, "-L" + LIBDIR, "-lsurfelmapping_hip",
                           "-Wl,-rpath," + LIBDIR])
    return exe


def test_rays_demo_compiles_against_c_abi_only(tmp_path):
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
    rays = np.zeros((700, 8), f32)
    rays[:, 0:3] = rng.uniform(-8.0, 8.0, (700, 3))
    rays[:, 4:7] = rng.normal(size=(700, 3))
    rays[:, 7] = 30.0
    rays[5, 4:7] = 0.0                                                        # an invalid ray
    files = [_write_map(tmp_path / "a.bin", model[:1000]), _write_map(tmp_path / "b.bin", model[1000:2200])]
    live = _write_map(tmp_path / "live.bin", model[2200:])
    with open(tmp_path / "rays.bin", "wb") as f:
        f.write(np.array([len(rays)], np.uint32).tobytes() + rays.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, live, "200", str(tmp_path / "rays.bin"), str(out)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rays 700 bad 1 records 3000 chunks 3" in r.stdout, r.stdout
    raw = open(out, "rb").read()
    N = len(rays)
    got = dict(t=np.frombuffer(raw, f32, N, 0), id=np.frombuffer(raw, np.int32, N, 4 * N), rgb=np.frombuffer(raw, np.uint8, 3 * N, 8 * N).reshape(N, 3),
               sem=np.frombuffer(raw, np.uint8, N, 11 * N), normal=np.frombuffer(raw, f32, 3 * N, 12 * N).reshape(N, 3))
    assert len(raw) == 24 * N
    ctx = capi.SurfelMap(capi.make_config(64, 48, 50.0, 50.0, 31.5, 23.5, max_sqrt_vertices=200))
    try:
        ctx.upload_model(model[2200:])
        want = ctx.cast_rays(rays, files, normal=True)
        alone = ctx.cast_rays(rays)
    finally:
        ctx.close()
    ref = rf.cast(model, rays)
    assert (want["id"] >= 0).sum() > 100
    for k in ("t", "id", "rgb", "sem", "normal"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
        assert np.array_equal(ref[k].view(np.uint8), want[k].view(np.uint8)), k
    assert f"model returns {int((alone['id'] >= 0).sum())} of 700" in r.stdout, r.stdout
