"""Spatial tiling through the drop-in facade (SurfelMapping::tileMaps; tests/cpp/tile_demo.cpp).  CPU: the caller compiles with
plain g++ against the C-ABI only.  GPU: the files it writes are the restatement's, byte for byte."""
import os
import subprocess

import pytest

import recall_ref as cr
import test_simplify as ts
import tile_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "tile_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "tile_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_tile_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_files_equal_the_restatement(tmp_path):
    rows = ts.Scene().rows
    n0, n1 = 600, 1400
    files = [str(tmp_path / "a_000000.bin"), str(tmp_path / "b.bin")]
    cr.write_map(files[0], rows[:n0], 2, 5)
    cr.write_map(files[1], rows[n0:n1], 4, 9)
    live = str(tmp_path / "live.bin")
    cr.write_map(live, rows[n1:])
    before = [open(p, "rb").read() for p in files]
    prefix = str(tmp_path / "tiled")
    r = subprocess.run([build_demo(tmp_path), live, "64", "100", "3", "256", prefix] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    want, st = tr.tile(rows, cell_mm=100, tile_shift=3, max_file_records=256)
    line = (f"tiled {st['records_in']} placed {st['placed']} loose {st['loose']} tiles {st['tiles']} largest {st['largest_tile']} "
            f"files {len(want)} readings 2\n")
    assert line in r.stdout, (line, r.stdout)
    for i, w in enumerate(want):
        name = "%s_%06d.bin" % (prefix, i)
        assert f"wrote {name}\n" in r.stdout
        assert open(name, "rb").read() == tr.file_bytes(w, 2, 9), i
    assert "tileMaps:" in r.stdout and "a_000000.bin" in r.stdout            # (the refusal of an output name that is a source)
    assert [open(p, "rb").read() for p in files] == before
    assert sorted(os.listdir(tmp_path)) == sorted(["a_000000.bin", "b.bin", "live.bin", "tile_demo"] + ["tiled_%06d.bin" % i for i in range(len(want))])
