"""Packed map files through the drop-in facade (SurfelMapping::packMaps / unpackMaps; tests/cpp/pack_demo.cpp).  CPU: the caller
compiles with plain g++ against the C-ABI only.  GPU: the files it writes are the restatement's, byte for byte, and the view of the
packed set is the view of its unpacked twin."""
import os
import subprocess

import numpy as np
import pytest

import pack_ref as pr
import recall_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "pack_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "pack_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_pack_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def _visible(m):
    m = m.copy()
    m[:, 0] *= np.float32(0.4)
    m[:, 1] *= np.float32(0.3)
    m[:, 2] = m[:, 2] * np.float32(0.5) + np.float32(10.0)
    m[:, 11] *= np.float32(3.0)
    return m


@pytest.mark.gpu
def test_facade_files_equal_the_restatement(tmp_path):
    a, live = _visible(pr.fixture_a(600, 60)), _visible(pr.fixture_a(300, 61))
    b, raw_b = pr.fixture_b(base=_visible(pr.fixture_a(pr.B_ROWS, 62)))
    files = [str(tmp_path / "a_000000.smp"), str(tmp_path / "b.bin")]               # (plain files, whatever their names say)
    cr.write_map(files[0], a, 2, 5)
    cr.write_map(files[1], b, 4, 9)
    live_path = str(tmp_path / "live.bin")
    cr.write_map(live_path, live)
    before = [open(p, "rb").read() for p in files]
    prefix = str(tmp_path / "out")
    r = subprocess.run([build_demo(tmp_path), live_path, "64", "-10", prefix] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    want = [pr.encode(a, 2, 5), pr.encode(b, 4, 9), pr.encode(live, 0, 0)]
    assert not want[0][1].any() and list(np.flatnonzero(want[1][1])) == list(raw_b) and not want[2][1].any()
    blocks, raws = sum(len(raw) for _, raw in want), len(raw_b)
    n = len(a) + len(b) + len(live)
    plain_bytes, packed_bytes = 2 * 12 + 48 * n, sum(len(w) for w, _ in want)
    assert f"packed files 3 records {n} blocks {blocks} raw {raws} bytes {plain_bytes} -> {packed_bytes}\n" in r.stdout, r.stdout
    assert f"unpacked files 3 records {n} bytes {packed_bytes} -> {plain_bytes + 12}\n" in r.stdout, r.stdout
    for i, ((data, _), ids) in enumerate(zip(want, ((2, 5), (4, 9), (0, 0)))):
        assert open("%s_%06d.smp" % (prefix, i), "rb").read() == data, i
        assert open("%s_%06d.bin" % (prefix, i), "rb").read() == pr.plain_bytes(pr.decode(data)[0], *ids), i
        assert "wrote %s_%06d.smp\n" % (prefix, i) in r.stdout and "wrote %s_%06d.bin\n" % (prefix, i) in r.stdout
    views = [open(prefix + s, "rb").read() for s in ("_packed.bgr", "_plain.bgr")]
    assert views[0] == views[1] and len(views[0]) == 160 * 60 * 3 and np.count_nonzero(np.frombuffer(views[0], np.uint8)) > 600
    assert "packMaps:" in r.stdout and "a_000000.smp" in r.stdout                    # (the refusal of an output name that is a source)
    assert [open(p, "rb").read() for p in files] == before
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
