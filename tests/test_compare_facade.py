"""Change detection through the drop-in facade (SurfelMapping::compareMaps, SurfelMapping::diffMaps; tests/cpp/compare_demo.cpp)
and SurfelMap.diff_maps.  CPU: the caller compiles with plain g++ against the C-ABI only.  GPU: the file compareMaps writes of
the street is the Python call's and the restatement's; diff_maps is its two compare_maps calls; diffMaps writes their files."""
import os
import subprocess

import numpy as np
import pytest

import compare_ref as cf
import retire_ref as ret
import test_compare as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
F32 = np.float32


@pytest.fixture(scope="module")
def street():
    case = tc.street_case()
    case["want"] = {6: cf.compare(case["query"], case["ref"], case["pose"], write_mask=6, **tc.STREET)}
    return case


def build_demo(tmp_path):
    exe = str(tmp_path / "compare_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "compare_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def _args(kw, mask):
    return [str(kw["voxel_mm"]), str(kw["cover_shift"]), repr(float(kw.get("reach_cells", 2.0))), str(kw.get("plane_mm", 50)), str(mask)]


def _pose_args(pose):
    return [repr(float(v)) for v in np.asarray(pose, F32).reshape(4, 4).T.ravel()]                  # column-major


def test_compare_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_compares_the_street(street, tmp_path):
    q, r = tc._write(tmp_path, "q.bin", street["query"]), tc._write(tmp_path, "r.bin", street["ref"])
    out, out_py = str(tmp_path / "out.bin"), str(tmp_path / "out_py.bin")
    want = street["want"][6]
    run = subprocess.run([build_demo(tmp_path), "compare", q, r] + _args(tc.STREET, 6) + [out] + _pose_args(street["pose"]),
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.splitlines()
    c = want["counts"]
    assert lines[0] == f"compared counts {c[0]} {c[1]} {c[2]} {c[3]} cells {want['cells_fine']} {want['cells_cover']} written {len(want['written'])}"
    assert lines[1] == f"changed {c[1]}"
    m = tc._ctx()
    lab, info = m.compare_maps([q], [r], pose=street["pose"], out_path=out_py, write_mask=6, **tc.STREET)
    m.close()
    assert open(out, "rb").read() == open(out_py, "rb").read()
    assert np.array_equal(ret.read_map(out)[0].view(np.uint32), want["written"].view(np.uint32))


@pytest.mark.gpu
def test_diff_is_two_compares(tmp_path):
    """a = the hand scene's reference, b = its query with the pose a -> b the inverse of the scene's (exact: a quarter turn and a
    dyadic shift): `appeared` is b against a, the scene itself; `vanished` is a against b"""
    qry, ref, pose, want = tc.hand_scene()
    a, b = tc._write(tmp_path, "a.bin", ref), tc._write(tmp_path, "b.bin", qry)
    a_to_b = np.linalg.inv(pose.astype(np.float64)).astype(F32)
    assert np.array_equal(np.linalg.inv(a_to_b.astype(np.float64)).astype(F32), pose)
    back = cf.compare(ref, qry, a_to_b, **tc.HAND)
    m = tc._ctx()
    outs = [str(tmp_path / n) for n in ("app.bin", "van.bin", "app2.bin", "van2.bin", "app3.bin", "van3.bin")]
    appeared, vanished = m.diff_maps([a], [b], a_to_b, outs[0], outs[1], **tc.HAND)
    lab_b, info_b = m.compare_maps([b], [a], pose=pose, out_path=outs[2], **tc.HAND)
    lab_a, info_a = m.compare_maps([a], [b], pose=a_to_b, out_path=outs[3], **tc.HAND)
    m.close()
    assert np.array_equal(appeared.pop("labels"), lab_b) and np.array_equal(vanished.pop("labels"), lab_a)
    assert appeared == info_b and vanished == info_a
    assert lab_b.tolist() == want.tolist() and lab_a.tolist() == back["labels"].tolist() and info_a["counts_by_code"] == back["counts"]
    assert open(outs[0], "rb").read() == open(outs[2], "rb").read() and open(outs[1], "rb").read() == open(outs[3], "rb").read()
    # the facade's diffMaps writes the same two files
    run = subprocess.run([build_demo(tmp_path), "diff", a, b] + _args(tc.HAND, 2) + outs[4:6] + _pose_args(a_to_b), capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr)
    lines = run.stdout.splitlines()
    for line, what, info in ((lines[0], "appeared", info_b), (lines[1], "vanished", info_a)):
        c = info["counts_by_code"]
        assert line == f"{what} counts {c[0]} {c[1]} {c[2]} {c[3]} cells {info['cells_fine']} {info['cells_cover']} written {info['written']}"
    assert open(outs[4], "rb").read() == open(outs[0], "rb").read() and open(outs[5], "rb").read() == open(outs[1], "rb").read()
