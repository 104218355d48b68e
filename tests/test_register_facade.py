"""Registration through the drop-in facade (SurfelMapping::registerMaps, SurfelMapping::alignMaps; tests/cpp/register_demo.cpp).
CPU: the caller compiles with plain g++ against the C-ABI only.  GPU: the pose it prints is the restatement's, registerMaps
leaves the files alone, and alignMaps + simplifyMaps leave what the Python calls leave."""
import os
import subprocess

import numpy as np
import pytest

import recall_ref as cr
import register_ref as rr
import register_scenes as sc
import retire_ref as ret
import test_register as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "register_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "register_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_register_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_registers_and_aligns(tmp_path):
    yaw, seed = tg.STREETS[0]
    src, tgt, truth, pivot = sc.street_pair(yaw_deg=yaw, seed=seed)
    T, want = rr.register(src, tgt, min_inliers=tg.MIN_INLIERS, pivot=pivot)
    s, t, out = str(tmp_path / "s.bin"), str(tmp_path / "t.bin"), str(tmp_path / "both.bin")
    cr.write_map(s, src)
    cr.write_map(t, tgt)
    before = open(s, "rb").read()
    exe = build_demo(tmp_path)
    args = [s, t, str(tg.MIN_INLIERS)] + [repr(float(v)) for v in pivot]

    def run(align):
        r = subprocess.run([exe] + args + [str(align), "200", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        lines = r.stdout.splitlines()
        pose = np.array([float(v) for v in lines[1].split()[1:]], np.float32).reshape(4, 4).T
        return lines, pose
    lines, pose = run(0)
    it = want["iterations"]
    assert lines[0] == f"status 0 iterations {it[0]} {it[1]} {it[2]} inliers {want['inliers']} samples {want['samples']}", lines
    tg._assert_pose(pose, T, "registerMaps")
    assert open(s, "rb").read() == before and not os.path.exists(out)
    # the same through Python on copies, then alignMaps + simplifyMaps on the files themselves
    s2 = str(tmp_path / "s2.bin")
    cr.write_map(s2, src)
    m = tg._ctx()
    pose_py, info = m.register_maps([s2], [t], apply=True, min_inliers=tg.MIN_INLIERS, pivot=pivot)
    st = m.simplify_maps([t, s2], str(tmp_path / "both_py.bin"), voxel_mm=200)
    m.close()
    lines, pose = run(1)
    assert np.array_equal(pose, pose_py) and info["applied"]
    assert open(s, "rb").read() == open(s2, "rb").read() != before
    assert lines[2] == f"merged {st['records_out']}"
    assert open(out, "rb").read() == open(str(tmp_path / "both_py.bin"), "rb").read()
    assert len(ret.read_map(out)[0]) == st["records_out"]
