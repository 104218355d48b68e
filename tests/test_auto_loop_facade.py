"""Closing loops unasked through the drop-in facade (SurfelMapping::setAutoLoop / autoLoopStats and closeLoop's rgb overload;
surfelmapping_amd/csrc/facade).  On test_loop.py's scenario a processFrame without a pose closes the loop by itself, and on the
corridor of test_track_rgb.py the rgb overload closes a loop depth alone cannot: status, tally, correction, pose, the map file that
moved and the saved model equal the C-ABI binding's with the same defaults."""
import os

import numpy as np
import pytest

import recall_ref as cr
import retire_ref as rr
import test_loop as tl
from backends import assert_models_equal
from test_auto_loop import _build_demo, corridor          # noqa: F401  (the corridor and its old world)
from test_loop import frames, old_map                      # noqa: F401  (the box scene and its old world)

f32 = np.float32


def _floats(line):
    return np.array([float.fromhex(x) for x in line.split()[1:]], f32)


def _dump(path, cam, drifted):
    with open(path, "wb") as f:
        f.write(np.array([cam["width"], cam["height"], len(drifted)], np.uint32).tobytes())
        f.write(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], f32).tobytes())
        for rgb, d, s, p in drifted:
            f.write(rgb.tobytes()); f.write(d.tobytes()); f.write(s.tobytes()); f.write(p.astype(f32).tobytes())


def _scenario(fr, rows_f, tmp_path, mode):
    """the demo in `mode` and the same context through the binding, up to the recall: (stdout lines, context, drifted frames,
    the two map files, the demo's saved model)"""
    import subprocess
    from surfelmapping_amd import capi
    cam, seq = fr["cam"], fr["seq"]
    G = tl._drift()
    drifted = [(x[0], x[1], x[2], tl._moved(G, x[3])) for x in seq[4:11]]
    dump = str(tmp_path / "frames.bin")
    _dump(dump, cam, drifted)
    f_path = str(tmp_path / "F.bin")
    cr.write_map(f_path, rows_f, 0, 9)
    n_cpp, n_py, out_map = str(tmp_path / "N_cpp.bin"), str(tmp_path / "N_py.bin"), str(tmp_path / "map.bin")
    r = subprocess.run([_build_demo(tmp_path), dump, "400", f_path, "500", n_cpp, out_map, mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    g = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
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
def test_facade_closes_the_loop_by_itself(frames, old_map, tmp_path):     # noqa: F811
    lines, g, drifted, files, out_map = _scenario(frames, old_map[1], tmp_path, "auto")
    g.set_auto_loop(paths=[files[1]])
    pose, ti = g.process_frame_tracked(*drifted[-1][:3])
    st = g.auto_loop_stats()
    assert ti["status"] == "OK" and st["last"]["status"] == "CLOSED" and (st["checked"], st["attempts"], st["closed"]) == (1, 1, 1), (ti, st)
    assert f"checked 1 attempts 1 closed 1 census {st['last_census']}" in lines, lines
    assert g.counts()["tick"] == 407
    _check(lines, pose, st["last"], files, out_map, g)


@pytest.mark.gpu
def test_facade_closes_the_corridor_loop_with_colour(corridor, tmp_path):     # noqa: F811
    fr, rows_f = corridor
    lines, g, drifted, files, out_map = _scenario(fr, rows_f, tmp_path, "rgb")
    pose, info = g.close_loop_rgb(drifted[-1][0], drifted[-1][1], drifted[-1][3], paths=[files[1]])
    assert info["status"] == "CLOSED", info
    _check(lines, pose, info, files, out_map, g)
