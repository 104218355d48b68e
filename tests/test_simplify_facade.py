"""Simplification through the drop-in facade (GlobalModel::simplify, SurfelMapping::simplifyMaps; tests/cpp/simplify_demo.cpp).
CPU: the caller compiles with plain g++ against the C-ABI only.  GPU: the files it writes hold the restatement's rows."""
import os
import subprocess

import pytest

import recall_ref as cr
import retire_ref as rr
import simplify_ref as sr
import test_simplify as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "simplify_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "simplify_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_simplify_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_files_equal_the_restatement(tmp_path):
    rows = ts.Scene().rows
    n0, n1 = 600, 1400
    files = [str(tmp_path / "a.bin"), str(tmp_path / "b.bin")]
    cr.write_map(files[0], rows[:n0])
    cr.write_map(files[1], rows[n0:n1])
    live = str(tmp_path / "live.bin")
    cr.write_map(live, rows[n1:])
    out = tmp_path / "out"
    before = [open(p, "rb").read() for p in files]
    r = subprocess.run([build_demo(tmp_path), live, "64", str(ts.BITE_MM), "0", str(out)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    want_set, st_set = sr.simplify(rows, voxel_mm=ts.BITE_MM, split_normals=0)
    want_live, st_live = sr.simplify(rows[n1:], voxel_mm=ts.BITE_MM, split_normals=0)
    ts.same_rows(rr.read_map(str(out / "set.bin"))[0], want_set, "set")
    ts.same_rows(rr.read_map(str(out / "live.bin"))[0], want_live, "live")
    for what, st in (("set", st_set), ("live", st_live)):
        line = (f"{what} {st['records_out']} in {st['records_in']} out {st['records_out']} merged {st['cells_merged']} loose {st['loose']} "
                f"largest {st['largest_cell']}\n")
        assert line in r.stdout, (line, r.stdout)
    assert "simplifyMaps:" in r.stdout and "a.bin" in r.stdout              # (the refusal of an output that is a source)
    assert [open(p, "rb").read() for p in files] == before
    assert sorted(os.listdir(out)) == ["live.bin", "set.bin"]
