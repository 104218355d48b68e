"""Paging in through the drop-in facade (SurfelMapping::setAutoRecall, GlobalModel::recall; surfelmapping_amd/csrc/facade).  CPU:
a caller compiles with plain g++ against the C-ABI only.  GPU: on a short drive the map files, the figures it prints and the map
it saves equal SurfelMap's with the same policies and the same two recalls."""
import os
import subprocess

import numpy as np
import pytest

import retire_ref as rr
from backends import assert_models_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "recall_demo.cpp")
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
N, SQRT, EVERY, MIN_AGE, MIN_DISTANCE, RADIUS, BACK = 45, 440, 10, 8, 15.0, 12.0, 20


def build_demo(tmp_path):
    exe = str(tmp_path / "recall_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC,
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_recall_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_recall_through_the_facade_equals_python(tmp_path):
    from surfelmapping_amd import capi
    cam, seq = rr.CAM, rr.sequence(N)
    frames = tmp_path / "frames.bin"
    with open(frames, "wb") as f:
        f.write(np.array([cam["width"], cam["height"], len(seq)], np.uint32).tobytes())
        f.write(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32).tobytes())
        for rgb, d, s, p in seq:
            f.write(rgb.tobytes()); f.write(d.tobytes()); f.write(s.tobytes()); f.write(p.astype(np.float32).tobytes())
    out_map = tmp_path / "map.bin"
    r = subprocess.run([build_demo(tmp_path), str(frames), str(SQRT), str(EVERY), str(MIN_AGE), str(MIN_DISTANCE), str(RADIUS),
                        str(tmp_path / "cpp"), str(BACK), str(out_map)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "setAutoRecall:" in r.stdout and "recall:" in r.stdout        # the refused radius and the missing file, printed
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=SQRT))
    m.set_auto_retire(EVERY, str(tmp_path / "py"), min_age=MIN_AGE, min_distance=MIN_DISTANCE)
    m.set_auto_recall(radius=RADIUS)
    for fr in seq:
        m.process_frame(*fr)
    (files, surfels), (rounds, recalled) = m.auto_retire_stats(), m.auto_recall_stats()
    assert files == N // EVERY == rounds and recalled > 0
    assert f"files {files} surfels {surfels} rounds {rounds} recalled {recalled} count {m.counts()['count']}\n" in r.stdout, r.stdout
    paths = [str(tmp_path / f"py_{i:06d}.bin") for i in range(files)]
    m.set_auto_retire(0, None)
    kept = m.recall(paths, pose=seq[BACK][3], mode="copy", radius=RADIUS)
    c1 = m.counts()["count"]
    moved = m.recall(paths, pose=seq[BACK][3], mode="move", radius=RADIUS)
    assert kept == moved > 1000
    assert f"copy {kept} count {c1} move {moved} count {m.counts()['count']}\n" in r.stdout, r.stdout
    for i in range(files):
        assert (tmp_path / f"cpp_{i:06d}.bin").read_bytes() == (tmp_path / f"py_{i:06d}.bin").read_bytes(), i
    got, a, b = rr.read_map(out_map)
    assert (a, b) == (0, N - 1)
    assert_models_equal(got, m.download_model(), "the saved map")
