"""The ground map through the drop-in facade (SurfelMapping::groundMaps, GlobalModel::groundMap; tests/cpp/ground_demo.cpp).  CPU: the
caller compiles with plain g++ against the C-ABI only.  GPU: the planes the demo prints are the restatement's of the same files, the
header's example among them."""
import os
import subprocess

import numpy as np
import pytest

from surfelmapping_amd.capi import SmGroundParams  # noqa: F401  (the binding's symbol: without it nothing here can run)

import ground_ref as gr
import recall_ref as cr
from test_ground import random_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "ground_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "ground_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def printed(want):
    """what ground_demo prints of a ground map"""
    i = want["info"]
    lines = [f"ground: records {i['records']} counts " + " ".join(str(v) for v in i["counts_by_kind"]) + " cells " + " ".join(str(v) for v in i["cells_by_state"])]
    for k in gr.PLANES:
        plane = want[k].reshape(want[k].shape[0], -1)
        lines += [f"{k} {r}: " + " ".join(str(int(v)) for v in row) for r, row in enumerate(plane)]
    return "\n".join(lines) + "\n"


def test_ground_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_example_and_two_files(tmp_path):
    exe = build_demo(tmp_path)
    example = str(tmp_path / "e.bin")
    cr.write_map(example, gr.EXAMPLE_ROWS)
    r = subprocess.run([exe, "1000", "3", "5", "1", "1", example], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    want = gr.ground(gr.EXAMPLE_ROWS, **gr.EXAMPLE_PARAMS)
    assert r.stdout.startswith(printed(want)), r.stdout
    assert "state 0: 1 1 2 3 3\n" in r.stdout and "clear2 0: 4 1 0 0 0\n" in r.stdout
    assert "model: records 0 unknown 5\n" in r.stdout and "groundMaps: sm_ground_maps: nu outside 1..8192" in r.stdout
    rows = random_rows(600, 41, span=(2.0, 1.2))
    files = [str(tmp_path / "a.bin"), str(tmp_path / "b.bin")]
    cr.write_map(files[0], rows[:250], 2, 5)
    cr.write_map(files[1], rows[250:], 4, 9)
    before = [open(p, "rb").read() for p in files]
    r = subprocess.run([exe, "100", "3", "20", "12", "-1"] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    want = gr.ground(rows, cell_mm=100, nu=20, nv=12)
    assert all(v > 0 for v in want["info"]["cells_by_state"][1:3]) and r.stdout.startswith(printed(want)), r.stdout
    assert [open(p, "rb").read() for p in files] == before
    assert sorted(os.listdir(tmp_path)) == ["a.bin", "b.bin", "e.bin", "ground_demo"]
