"""Closing loops through the drop-in facade (SurfelMapping::closeLoop, GlobalModel::warpByTime; surfelmapping_amd/csrc/facade).
CPU: a caller compiles with plain g++ against the C-ABI only.  GPU: on test_loop.py's scenario the status, the measured
correction, the corrected pose, the map file that moved and the saved model equal SurfelMap.close_loop's with the same defaults."""
import os
import subprocess

import numpy as np
import pytest

import recall_ref as cr
import retire_ref as rr
import test_loop as tl
from backends import assert_models_equal
from test_loop import frames, old_map          # noqa: F401  (module-scoped fixtures: the scene and the old world)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "loop_demo.cpp")
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
f32 = np.float32


def build_demo(tmp_path):
    exe = str(tmp_path / "loop_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC,
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_loop_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def _floats(line):
    return np.array([float.fromhex(x) for x in line.split()[1:]], f32)


@pytest.mark.gpu
def test_loop_through_the_facade_equals_python(frames, old_map, tmp_path):     # noqa: F811
    cam, seq = frames["cam"], frames["seq"]
    G = tl._drift()
    drifted = [(fr[0], fr[1], fr[2], tl._moved(G, fr[3])) for fr in seq[4:11]]
    dump = tmp_path / "frames.bin"
    with open(dump, "wb") as f:
        f.write(np.array([cam["width"], cam["height"], len(drifted)], np.uint32).tobytes())
        f.write(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], f32).tobytes())
        for rgb, d, s, p in drifted:
            f.write(rgb.tobytes()); f.write(d.tobytes()); f.write(s.tobytes()); f.write(p.astype(f32).tobytes())
    f_path = str(tmp_path / "F.bin")
    cr.write_map(f_path, old_map[1], 0, 9)
    n_cpp, n_py, out_map = str(tmp_path / "N_cpp.bin"), str(tmp_path / "N_py.bin"), str(tmp_path / "map.bin")
    r = subprocess.run([build_demo(tmp_path), str(dump), "400", f_path, "500", n_cpp, out_map], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "warpByTime:" in r.stdout                                     # the missing file, printed
    lines = r.stdout.splitlines()
    # the same through the C-ABI binding
    from surfelmapping_amd import capi
    g = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    g.set_tick(400)
    for fr in drifted[:-1]:
        g.process_frame(*fr)
    g.save_map(n_py, 400, 405)
    n_old = g.recall([f_path], pose=drifted[-2][3], mode="copy", radius=500.0)
    assert f"recalled {n_old} count {g.counts()['count']}" in lines
    pose, info = g.close_loop(drifted[-1][1], drifted[-1][3], paths=[n_py])
    assert info["status"] == "CLOSED", info
    want = f"status {info['status_code']} t_a {info['t_a']} t_b {info['t_b']} track {info['track']['status_code']} inliers {info['track']['inliers']}"
    assert want in lines, r.stdout
    D = _floats([l for l in lines if l.startswith("D ")][0])
    P = _floats([l for l in lines if l.startswith("pose ")][0])
    assert np.array_equal(D.view(np.uint32), info["D"].T.reshape(16).view(np.uint32))
    assert np.array_equal(P.view(np.uint32), np.ascontiguousarray(pose.T).reshape(16).view(np.uint32))
    g.warp_by_time([n_py], info["t_a"], np.eye(3, 4, dtype=f32).reshape(1, 12))
    st = g.warp_stats()
    assert st["records_moved"] > 0 and st["model_moved"] > 0
    assert f"identity moved {st['records_moved'] + st['model_moved']}" in lines, r.stdout
    assert open(n_cpp, "rb").read() == open(n_py, "rb").read()
    got, a, b = rr.read_map(out_map)
    assert_models_equal(got, g.download_model(), "the saved map")
