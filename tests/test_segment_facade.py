"""Segmentation through the drop-in facade (SurfelMapping::segmentMaps; tests/cpp/segment_demo.cpp).  CPU: the caller compiles with
plain g++ against the C-ABI only.  GPU: two separated boxes of surfels are two components with the right counts, and the file it
writes holds the larger one when min_records lies between the two sizes."""
import os
import subprocess

import numpy as np
import pytest

import recall_ref as cr
import segment_ref as sg
from test_simplify import surfel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "segment_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "segment_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_segment_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def box(x0, nx, ny, nz, sem):
    """the faces of a box of nx x ny x nz cells of 200 mm at x0: one surfel per face cell"""
    rows = [surfel(x0 + 0.2 * i + 0.1, 0.2 * j + 0.1, 5.0 + 0.2 * k + 0.1, sem=sem, t0=float((i + j + k) % 7))
            for i in range(nx) for j in range(ny) for k in range(nz) if i in (0, nx - 1) or j in (0, ny - 1) or k in (0, nz - 1)]
    return np.stack(rows)


@pytest.mark.gpu
def test_facade_two_boxes(tmp_path):
    big, little = box(0.0, 8, 6, 5, 3), box(4.0, 3, 3, 3, 7)
    rs = np.random.RandomState(2)
    rows = np.concatenate([little[:10], big, little[10:]])
    rows = np.concatenate([rows[:5], rows[5:][rs.permutation(len(rows) - 5)]])           # (the little box is met first)
    files = [str(tmp_path / "a.bin"), str(tmp_path / "b.bin")]
    cr.write_map(files[0], rows[:100], 2, 5)
    cr.write_map(files[1], rows[100:], 4, 9)
    before = [open(p, "rb").read() for p in files]
    out = str(tmp_path / "objects.bin")
    between = (len(big) + len(little)) // 2
    r = subprocess.run([build_demo(tmp_path), "200", str(between), out] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    want = sg.segment(rows, voxel_mm=200)
    assert want["components"]["records"].tolist() == [len(little), len(big)] and want["components"]["cls"].tolist() == [7, 3]
    assert f"all: records {len(rows)} components 2 small 0 largest {len(big)}\n" in r.stdout, r.stdout
    for i, c in enumerate(want["components"]):
        line = (f"component {i} first {c['first']} records {c['records']} cells {c['cells']} class {c['cls']} box "
                f"{c['cell_lo'][0]} {c['cell_lo'][1]} {c['cell_lo'][2]} .. {c['cell_hi'][0]} {c['cell_hi'][1]} {c['cell_hi'][2]}\n")
        assert line in r.stdout, (line, r.stdout)
    assert f"kept: components 1 small 1 written {len(big)}\n" in r.stdout and f"labelled small {len(little)}\n" in r.stdout, r.stdout
    kept = sg.segment(rows, voxel_mm=200, min_records=between)
    assert kept["info"]["components"] == 1 and len(kept["kept"]) == len(big)
    assert open(out, "rb").read() == sg.file_bytes(kept["kept"], 2, 9)
    assert "segmentMaps:" in r.stdout and "a.bin" in r.stdout               # (the refusal of an output that is a source)
    assert [open(p, "rb").read() for p in files] == before
    assert sorted(os.listdir(tmp_path)) == ["a.bin", "b.bin", "objects.bin", "segment_demo"]
