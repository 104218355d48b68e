"""Meshing through the drop-in facade (SurfelMapping::meshMaps, GlobalModel::mesh; tests/cpp/mesh_demo.cpp).  CPU: the caller compiles
with plain g++ against the C-ABI only.  GPU: the PLY file the demo writes, read back with capi.read_ply, is the restatement's mesh of
the same files, and the counts it prints are the restatement's."""
import os
import subprocess

import pytest

import mesh_ref as mr
import recall_ref as cr
from test_mesh import sphere_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "mesh_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "mesh_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_mesh_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_sphere(tmp_path):
    from surfelmapping_amd import capi
    rows = sphere_rows(1500, 0.75)
    files = [str(tmp_path / "a.bin"), str(tmp_path / "b.bin")]
    cr.write_map(files[0], rows[:400], 2, 5)
    cr.write_map(files[1], rows[400:], 4, 9)
    before = [open(p, "rb").read() for p in files]
    out = str(tmp_path / "sphere.ply")
    r = subprocess.run([build_demo(tmp_path), "250", "2", out] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    want = mr.mesh(rows, voxel_mm=250, reach=2)
    i = want["info"]
    assert mr.topology(want["faces"], len(want["vertices"])) == dict(open_edges=0, bad_edges=0, repeated=0, euler=2)
    assert (f"mesh: records {len(rows)} used {len(rows)} cells {i['cells']} lattice {i['lattice_points']} cubes {i['cubes']} vertices {i['vertices']} "
            f"faces {i['faces']}\n") in r.stdout, r.stdout
    assert "model: faces 0\n" in r.stdout
    vertices, faces = capi.read_ply(out)
    assert vertices.tobytes() == want["vertices"].tobytes() and faces.tobytes() == want["faces"].tobytes()
    assert open(out, "rb").read() == mr.ply_bytes(want["vertices"], want["faces"])
    assert "meshMaps:" in r.stdout and "a.bin" in r.stdout                  # (the refusal of an output that is a source)
    assert [open(p, "rb").read() for p in files] == before
    assert sorted(os.listdir(tmp_path)) == ["a.bin", "b.bin", "mesh_demo", "sphere.ply"]
