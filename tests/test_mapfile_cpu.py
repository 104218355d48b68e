"""The map-file format's one reader, writer and chunk plan (surfelmapping_amd/csrc/sm_mapfile.h), without a GPU and without HIP:
tests/cpp/mapfile_check.cpp is compiled against that header alone.  The inputs are made with numpy, the outputs compared as bytes."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfelmapping_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "mapfile_check.cpp")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapfile") / "mapfile_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, SRC])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stdout, r.stderr)
        return r.stdout.splitlines()
    return run


def _rows(n, seed=0):
    return np.random.default_rng(seed).standard_normal((n, 12)).astype(np.float32)


def _file(rows, a, b, count=None):
    return (np.array([len(rows) if count is None else count], np.uint32).tobytes() + np.array([a, b], np.int32).tobytes() +
            np.ascontiguousarray(rows, np.float32).tobytes())


def test_header_includes_no_hip():
    text = open(os.path.join(CSRC, "sm_mapfile.h")).read()
    assert "#include <hip" not in text and '#include "sm_ctx.h"' not in text


def test_writer(check, tmp_path):
    rows = _rows(8, 1)
    src = tmp_path / "rows.f32"
    src.write_bytes(rows.tobytes())
    pieces = (0, 1, 5, 2)
    # a known count, rows in uneven pieces: exactly header + rows
    out = tmp_path / "known.bin"
    assert check("write", out, 8, -3, 9, src, "commit", *pieces) == ["ok 8"]
    assert out.read_bytes() == _file(rows, -3, 9)
    # an unknown count: the header carries the rows appended once the writer has committed
    out = tmp_path / "unknown.bin"
    assert check("write", out, "unknown", 4, 5, src, "commit", *pieces) == ["ok 8"]
    assert out.read_bytes() == _file(rows, 4, 5)
    out = tmp_path / "unknown_fewer.bin"
    assert check("write", out, "unknown", 4, 5, src, "commit", 0, 1, 5) == ["ok 6"]
    assert out.read_bytes() == _file(rows[:6], 4, 5)
    out = tmp_path / "unknown_none.bin"
    assert check("write", out, "unknown", 4, 5, src, "commit") == ["ok 0"]
    assert out.read_bytes() == _file(rows[:0], 4, 5)
    # a known count that the rows do not reach: refused by commit(), no file
    out = tmp_path / "short.bin"
    got = check("write", out, 8, 0, 0, src, "commit", 1, 5)
    assert got[0].startswith("err ") and "short.bin" in got[0] and not out.exists()
    # dropped without commit(): no file, whatever was appended
    for count in (8, "unknown"):
        out = tmp_path / "dropped.bin"
        assert check("write", out, count, 0, 0, src, "drop", *pieces) == ["ok 8"]
        assert not out.exists()
    # a path in a missing directory: the error names it, nothing is made
    out = tmp_path / "no_such_dir" / "x.bin"
    got = check("write", out, 8, 0, 0, src, "commit", *pieces)
    assert got == [f"err check: {out} is not open!"]
    assert not out.exists() and not out.parent.exists()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["known.bin", "rows.f32", "unknown.bin", "unknown_fewer.bin", "unknown_none.bin"]


def test_checked_open(check, tmp_path):
    rows = _rows(5, 2)
    whole = _file(rows, 7, 11)
    cases = dict(good=whole, empty=_file(rows[:0], 1, 2), stub=whole[:4], short=whole[:-48], long=whole + rows[:1].tobytes(),
                 stray=whole + b"\0" * 7, cut=whole[:-7])
    for name, data in cases.items():
        (tmp_path / f"{name}.bin").write_bytes(data)
    order = ["good", "empty", "missing", "stub", "short", "long", "stray", "cut"]
    paths = [str(tmp_path / f"{n}.bin") for n in order]
    strict = dict(zip(order, check("open", "strict", *paths)))
    assert strict["good"] == f"ok 5 7 11 {12 + 48 * 5} 12"           # count, ids, size; positioned at the first record
    assert strict["empty"] == "ok 0 1 2 12 12"
    for name in order[2:]:
        assert strict[name].startswith("err check: ") and f"{name}.bin" in strict[name], (name, strict[name])
    assert strict["missing"].endswith("missing.bin is not open!")
    assert strict["stub"].endswith("stub.bin read err!! (no header)")
    assert strict["short"].endswith(f"short.bin holds {12 + 48 * 4} bytes, its header's 5 records need {12 + 48 * 5}")
    assert strict["long"].endswith(f"long.bin holds {12 + 48 * 6} bytes, its header's 5 records need {12 + 48 * 5}")
    assert strict["stray"].endswith(f"stray.bin holds {12 + 48 * 5 + 7} bytes, its header's 5 records need {12 + 48 * 5}")
    # the lenient form (sm_load_map): trailing bytes are accepted, a file that is too short is not
    lenient = dict(zip(order, check("open", "lenient", *paths)))
    assert lenient["good"] == strict["good"] and lenient["empty"] == strict["empty"]
    assert lenient["long"] == f"ok 5 7 11 {12 + 48 * 6} 12" and lenient["stray"] == f"ok 5 7 11 {12 + 48 * 5 + 7} 12"
    for name in ("stub", "short", "cut"):
        assert lenient[name].endswith(f"{name}.bin read err!!"), (name, lenient[name])
    assert lenient["missing"].endswith("missing.bin is not open!")


def test_chunk_plan(check, tmp_path):
    chunk, sizes = 4, [0, 1, 3, 4, 5, 11]
    paths = []
    for i, n in enumerate(sizes):
        paths.append(str(tmp_path / f"p{i}.bin"))
        open(paths[-1], "wb").write(_file(_rows(n, i), i, i))
    want = [(i, first, min(chunk, n - first)) for i, n in enumerate(sizes) for first in range(0, n, chunk)]
    got = [tuple(int(x) for x in line.split()) for line in check("plan", chunk, *paths)]
    assert got == want
    assert all(first + n <= sizes[f] and 0 < n <= chunk for f, first, n in got)     # no job across a file boundary
    assert 0 not in {f for f, _, _ in got}                                          # none for the empty file
    assert [sum(n for f, _, n in got if f == i) for i in range(len(sizes))] == sizes
    # a list with a bad file has no plan: the error names the file
    open(paths[2], "r+b").truncate(12 + 48 * 2 + 7)
    got = check("plan", chunk, *paths)
    assert len(got) == 1 and got[0].startswith("err ") and "p2.bin" in got[0]


def test_policy_file_name(check):
    assert check("name", "/a/b/run", 7) == ["/a/b/run_000007.bin"]
    assert check("name", "m", 1234567) == ["m_1234567.bin"]
