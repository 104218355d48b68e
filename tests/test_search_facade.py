"""The pose search through the drop-in facade (SurfelMapping::setLoopSearch, honoured by closeLoop and setAutoLoop;
surfelmapping_amd/csrc/facade).  On the street of tests/retire_ref.py, with the facade's default configuration, a camera that
comes back 1.4 m from where it believes to be closes the loop after setLoopSearch(true), by closeLoop and by a processFrame
without a pose: status, correction, pose, the map file that moved and the saved model equal the C-ABI binding's."""
import os
import subprocess

import numpy as np
import pytest

import recall_ref as cr
import retire_ref as rr
import track_ref as tr
from backends import assert_models_equal
from test_search import _drift, _m4, _moved

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
f32 = np.float32
CAM = rr.CAM


def _build_demo(tmp_path):
    exe = str(tmp_path / "search_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "search_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_search_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def _floats(line):
    return np.array([float.fromhex(x) for x in line.split()[1:]], f32)


@pytest.fixture(scope="module")
def street():
    """frames 0..10 of the street and the old world: frames 0..9 fused with the facade's default configuration"""
    from surfelmapping_amd import capi
    seq = rr.sequence(11)
    m = capi.SurfelMap(capi.make_config(**CAM, preprocess=0))
    for fr in seq[:10]:
        m.process_frame(*fr)
    return seq, m.download_model()


def _scenario(street, tmp_path, mode):
    """the demo in `mode` and the same context through the binding, up to the recall"""
    from surfelmapping_amd import capi
    seq, rows_f = street
    G = _drift()
    drifted = [(x[0], x[1], x[2], _moved(G, x[3])) for x in seq[4:11]]
    dump = str(tmp_path / "frames.bin")
    with open(dump, "wb") as f:
        f.write(np.array([CAM["width"], CAM["height"], len(drifted)], np.uint32).tobytes())
        f.write(np.array([CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]], f32).tobytes())
        for rgb, d, s, p in drifted:
            f.write(rgb.tobytes()); f.write(d.tobytes()); f.write(s.tobytes()); f.write(p.astype(f32).tobytes())
    f_path = str(tmp_path / "F.bin")
    cr.write_map(f_path, rows_f, 0, 9)
    n_cpp, n_py, out_map = str(tmp_path / "N_cpp.bin"), str(tmp_path / "N_py.bin"), str(tmp_path / "map.bin")
    r = subprocess.run([_build_demo(tmp_path), dump, "400", f_path, "500", n_cpp, out_map, mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    g = capi.SurfelMap(capi.make_config(**CAM, preprocess=0))
    g.set_tick(400)
    for x in drifted[:-1]:
        g.process_frame(*x)
    g.save_map(n_py, 400, 405)
    n_old = g.recall([f_path], pose=drifted[-2][3], mode="copy", radius=500.0)
    assert f"recalled {n_old} count {g.counts()['count']}" in lines, r.stdout
    return lines, g, drifted, (n_cpp, n_py), out_map


def _check(lines, pose, info, files, out_map, g):
    want = f"status {info['status_code']} t_a {info['t_a']} t_b {info['t_b']} track {info['track']['status_code']} inliers {info['track']['inliers']}"
    assert want in lines, lines
    D = _floats([l for l in lines if l.startswith("D ")][0])
    P = _floats([l for l in lines if l.startswith("pose ")][0])
    assert np.array_equal(D.view(np.uint32), info["D"].T.reshape(16).view(np.uint32))
    assert np.array_equal(P.view(np.uint32), np.ascontiguousarray(pose.T).reshape(16).view(np.uint32))
    assert open(files[0], "rb").read() == open(files[1], "rb").read()
    assert_models_equal(rr.read_map(out_map)[0], g.download_model(), "the saved map")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "search"])
def test_facade_close_loop_honours_the_search(street, tmp_path, mode):
    lines, g, drifted, files, out_map = _scenario(street, tmp_path, mode)
    rgb, depth, believed = drifted[-1][0], drifted[-1][1], drifted[-1][3]
    pose, info = g.close_loop_rgb(rgb, depth, believed, paths=[files[1]], search=mode == "search")
    et, _ = tr.pose_error(info["D"].astype(np.float64) @ _drift(), np.eye(4))
    print(f"{mode}: {info['status']}, D * G {et:.3f} m from the identity")
    if mode == "search":
        assert info["status"] == "CLOSED" and et < 0.05, (info, et)
    else:
        assert info["status"] != "CLOSED" or et > 0.3, (info, et)
    _check(lines, pose, info, files, out_map, g)


@pytest.mark.gpu
def test_facade_auto_loop_honours_the_search(street, tmp_path):
    lines, g, drifted, files, out_map = _scenario(street, tmp_path, "auto")
    g.set_auto_loop(paths=[files[1]], search=True)
    pose, ti = g.process_frame_tracked_rgb(*drifted[-1][:3])
    st = g.auto_loop_stats()
    assert ti["status"] == "OK" and st["last"]["status"] == "CLOSED" and (st["checked"], st["attempts"], st["closed"]) == (1, 1, 1), (ti, st)
    assert f"checked 1 attempts 1 closed 1 census {st['last_census']}" in lines, lines
    et, er = tr.pose_error(pose, _m4(street[0][10][3]))
    assert et < 0.05 and er < 0.3, (et, er)
    _check(lines, pose, st["last"], files, out_map, g)
