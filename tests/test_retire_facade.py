"""The periodic retirement through the drop-in facade (SurfelMapping::setAutoRetire, GlobalModel::retire;
surfelmapping_amd/csrc/facade).  CPU: a caller compiles with plain g++ against the C-ABI only.  GPU: the map files it writes, the
figures it prints and the map it saves equal SurfelMap's with the same policy, with processFrame synchronous and asynchronous
(SM_FACADE_ASYNC)."""
import os
import subprocess

import numpy as np
import pytest

import retire_ref as rr
from backends import assert_models_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "retire_demo.cpp")
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
N, SQRT, EVERY, MIN_AGE, MIN_DISTANCE = 45, 440, 10, 8, 15.0


def build_demo(tmp_path):
    exe = str(tmp_path / "retire_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC,
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_retire_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("facade_async", ["0", "1"])
def test_policy_through_the_facade_equals_python(tmp_path, facade_async):
    from surfelmapping_amd import capi
    cam, seq = rr.CAM, rr.sequence(N)
    frames = tmp_path / "frames.bin"
    with open(frames, "wb") as f:
        f.write(np.array([cam["width"], cam["height"], len(seq)], np.uint32).tobytes())
        f.write(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32).tobytes())
        for rgb, d, s, p in seq:
            f.write(rgb.tobytes()); f.write(d.tobytes()); f.write(s.tobytes()); f.write(p.astype(np.float32).tobytes())
    out_map = tmp_path / "map.bin"
    r = subprocess.run([build_demo(tmp_path), str(frames), str(SQRT), str(EVERY), str(MIN_AGE), str(MIN_DISTANCE),
                        str(tmp_path / "cpp"), str(out_map)], capture_output=True, text=True,
                       env=dict(os.environ, SM_FACADE_ASYNC=facade_async))
    assert r.returncode == 0, r.stdout + r.stderr
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=SQRT))
    m.set_auto_retire(EVERY, str(tmp_path / "py"), min_age=MIN_AGE, min_distance=MIN_DISTANCE)
    for fr in seq:
        m.process_frame(*fr)
    files, surfels = m.auto_retire_stats()
    assert files == N // EVERY and surfels > 1000
    assert f"files {files} surfels {surfels} count {m.counts()['count']}\n" in r.stdout, r.stdout
    for i in range(files):
        assert (tmp_path / f"cpp_{i:06d}.bin").read_bytes() == (tmp_path / f"py_{i:06d}.bin").read_bytes(), i
    rest = m.retire(pose=seq[-1][3], min_age=MIN_AGE, min_distance=MIN_DISTANCE)
    left = m.download_model()
    # refreshHostModel()'s callers see the model after the retirement
    assert f"retired at the end {len(rest)} count {len(left)} mirror {len(left)}\n" in r.stdout, r.stdout
    assert len(rest) > 0
    got, a, b = rr.read_map(out_map)
    assert (a, b) == (0, N - 1)
    assert_models_equal(got, left, "the saved map")
