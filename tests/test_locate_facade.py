"""Locating through the drop-in facade (SurfelMapping::locateMaps; tests/cpp/locate_demo.cpp).  CPU: the caller compiles with plain
g++ against the C-ABI only.  GPU: what the demo prints of the yard is the restatement's, the pose it hands to registerMaps brings
the truth back, and the files stay as they are."""
import os
import subprocess

import numpy as np
import pytest

from surfelmapping_amd.capi import SmLocateParams  # noqa: F401  (the binding's symbol: without it nothing here can run)

import locate_ref as lr
import locate_scenes as ls
import recall_ref as cr
import test_locate as tl
import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "locate_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "locate_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_locate_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_locates_and_registers(tmp_path):
    truth = ls.truth_of(*tl.TRUTHS[0])
    src, tgt, params = ls.yard_pair(truth)
    want = lr.locate(src, tgt, tl._table(params), **params)
    i = want["info"]
    s, t = str(tmp_path / "s.bin"), str(tmp_path / "t.bin")
    cr.write_map(s, src)
    cr.write_map(t, tgt)
    before = open(s, "rb").read(), open(t, "rb").read()
    args = [s, t, str(params["up"]), str(params["normal_sign"])] + [repr(float(v)) for v in params["origin"]] + [str(params["nu"]), str(params["nv"])]
    args += [repr(float(v)) for v in params["source_origin"]] + [str(tl.MIN_INLIERS)]
    r = subprocess.run([build_demo(tmp_path)] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == (f"status 0 row {i['row']} du {i['du']} dv {i['dv']} score {i['score']} coarse {i['coarse_k']} {i['coarse_du']} {i['coarse_dv']} {i['coarse_score']}"
                        f" runner_up {i['runner_up']} n_s {i['n_s']} cells {i['target_cells']} pairs {i['height_pairs']} dh {i['dh']}"), lines
    pose = np.array([float(v) for v in lines[1].split()[1:]], np.float32).reshape(4, 4).T
    assert np.array_equal(pose.view(np.uint32), want["pose"].astype(np.float32).view(np.uint32))
    assert lines[2].startswith("register 0 inliers ")
    refined = np.array([float(v) for v in lines[3].split()[1:]], np.float64).reshape(4, 4).T
    dt, dr = tr.pose_error(refined, truth)
    print(lines, dt, dr)
    assert dt < 0.01 and dr < 0.03                        # (test_locate.py's end-to-end bound; the pivot is the window's middle)
    assert "locateMaps: sm_locate_maps: nu outside 1..4096" in r.stdout
    assert (open(s, "rb").read(), open(t, "rb").read()) == before
    assert sorted(os.listdir(tmp_path)) == ["locate_demo", "s.bin", "t.bin"]
