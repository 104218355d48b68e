"""A listed set of map files on the host (surfelmapping_amd/csrc/sm_map_set.h), without a GPU and without HIP: the file index, the
two openings, MapFile::keep and its temporary, the look-ahead loop and the replacement pass.  tests/cpp/mapset_check.cpp is compiled
against that header alone, once plainly and once with the address and undefined-behaviour sanitizers (a stand-alone program);
every case runs on both.  The inputs are made with numpy, the outputs compared as bytes and as listed lines."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfelmapping_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "mapset_check.cpp")
CHUNK, SIZES = 4, [0, 1, 3, 4, 5, 11]
SANITIZE = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-g"]


class Session:
    """one run of the program: a command in, its lines out"""

    def __init__(self, exe):
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)

    def __call__(self, *words):
        self.p.stdin.write(" ".join(str(w) for w in words) + "\n")
        self.p.stdin.flush()
        out = []
        while True:
            line = self.p.stdout.readline()
            assert line, (words, out, self.close())
            if line == ".\n":
                return out
            out.append(line.rstrip("\n"))

    def close(self):
        if self.p.stdin:
            self.p.stdin.close()
        err = self.p.stderr.read()
        return self.p.wait(), err


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def session(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mapset") / f"mapset_check_{request.param}")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, SRC]
    if request.param == "sanitized":
        r = subprocess.run(cmd + SANITIZE, capture_output=True, text=True)
        if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
            pytest.skip("the compiler cannot link the sanitizers' runtime: " + r.stderr.strip().splitlines()[-1])
        assert r.returncode == 0, r.stderr
    else:
        subprocess.check_call(cmd)
    opened = []

    def start():
        opened.append(Session(exe))
        return opened[-1]
    yield start
    for s in opened:                   # (every session ended clean: the sanitizers report at exit, leaks included)
        assert s.close() == (0, ""), exe


def _rows(n, seed=0):
    return np.random.default_rng(seed).standard_normal((n, 12)).astype(np.float32)


def _file(rows, a, b, count=None):
    return (np.array([len(rows) if count is None else count], np.uint32).tobytes() + np.array([a, b], np.int32).tobytes() +
            np.ascontiguousarray(rows, np.float32).tobytes())


def _set(tmp_path, sizes=SIZES):
    paths, rows = [], []
    for i, n in enumerate(sizes):
        paths.append(str(tmp_path / f"p{i}.bin"))
        rows.append(_rows(n, i))
        open(paths[-1], "wb").write(_file(rows[-1], i, 10 + i))
    return paths, rows


def _plan(sizes, read=None):
    return [f"job {i} {first} {min(CHUNK, n - first)}" for i, n in enumerate(sizes) if read is None or i in read for first in range(0, n, CHUNK)]


def _stat(p):
    st = os.stat(p)
    return st.st_size, st.st_mtime_ns


def test_header_includes_no_hip():
    text = open(os.path.join(CSRC, "sm_map_set.h")).read()
    assert "#include <hip" not in text and '#include "sm_ctx.h"' not in text


def test_index(session, tmp_path, monkeypatch):
    s = session()
    p = str(tmp_path / "a.bin")
    open(p, "wb").write(_file(_rows(3, 1), 0, 1))
    assert s("valid", p) == ["none"]
    assert s("note", p, 17) == ["ok"]
    assert s("valid", p) == ["valid %d %d 17" % _stat(p)]
    # grown by a row
    open(p, "ab").write(_rows(1, 2).tobytes())
    assert s("valid", p) == ["none"]
    assert s("note_now", p, 18) == ["ok"]
    assert s("valid", p) == ["valid %d %d 18" % _stat(p)]
    # rewritten with the same size and a later mtime
    size, mtime = _stat(p)
    open(p, "wb").write(_file(_rows(4, 3), 0, 1))
    os.utime(p, ns=(mtime + 1_000_000_000, mtime + 1_000_000_000))
    assert _stat(p) == (size, mtime + 1_000_000_000)
    assert s("valid", p) == ["none"]
    os.utime(p, ns=(mtime, mtime))
    assert s("valid", p) == ["valid %d %d 18" % (size, mtime)]
    # erased
    assert s("erase", p) == ["ok"] and s("valid", p) == ["none"]
    # removed; "as it is now" of a missing file erases
    assert s("note", p, 19) == ["ok"] and s("valid", p)[0].startswith("valid ")
    os.remove(p)
    assert s("valid", p) == ["none"]
    open(p, "wb").write(_file(_rows(4, 3), 0, 1))
    os.utime(p, ns=(mtime, mtime))
    assert s("valid", p) == ["valid %d %d 19" % (size, mtime)]       # (the entry was still there)
    os.remove(p)
    assert s("note_now", p, 20) == ["ok"]
    open(p, "wb").write(_file(_rows(4, 3), 0, 1))
    os.utime(p, ns=(mtime, mtime))
    assert s("valid", p) == ["none"]


def test_index_switch(session, tmp_path, monkeypatch):
    """SM_RECALL_NO_INDEX=1 turns the opening's look-ups off, not the notes"""
    paths, _ = _set(tmp_path, [5, 6])
    monkeypatch.delenv("SM_RECALL_NO_INDEX", raising=False)
    for on in (True, False):
        if not on:
            monkeypatch.setenv("SM_RECALL_NO_INDEX", "1")
        s = session()
        assert s("note", paths[0], 3) == ["ok"]
        got = s("rewrite", CHUNK, -1, 10.0, *paths)
        assert got[0] == ("counters 2 1 1" if on else "counters 2 0 2"), got
        assert s("valid", paths[0]) == ["valid %d %d 3" % _stat(paths[0])]


def test_reading_set(session, tmp_path):
    s = session()
    paths, _ = _set(tmp_path)
    got = s("read", CHUNK, *paths)
    assert got == [f"file {i} {n} {sum(SIZES[:i])}" for i, n in enumerate(SIZES)] + _plan(SIZES) + [f"total {sum(SIZES)}"]
    open(paths[2], "r+b").truncate(12 + 48 * 2 + 7)
    os.remove(paths[4])                                                # (a later bad file: the first one's message)
    got = s("read", CHUNK, *paths)
    assert len(got) == 1 and got[0].startswith("err check: ") and "p2.bin holds" in got[0]


def test_rewriting_set(session, tmp_path):
    s = session()
    paths, _ = _set(tmp_path)
    for i in (1, 3, 4):
        assert s("note", paths[i], 5 if i != 4 else 50) == ["ok"]     # (file 4's entry is valid and not skipped: max_time >= t0)
    open(paths[3], "r+b").truncate(12 + 48 * 2 + 7)
    s("note", paths[3], 5)                                             # truncated AND skipped by its entry: not opened, not noticed
    got = s("rewrite", CHUNK, -1, 10.0, *paths)
    read = [0, 2, 4, 5]
    assert got[0] == "counters 6 2 4"
    assert got[1:7] == [f"file {i} {int(i not in read)} {SIZES[i] if i in read else 0} {len(range(0, SIZES[i], CHUNK)) if i in read else 0}"
                        for i in range(6)]
    assert got[7:] == _plan(SIZES, read)
    # a file the caller knows it need not read is skipped unasked
    got = s("rewrite", CHUNK, 5, 10.0, *paths)
    assert got[0] == "counters 6 3 3" and got[6] == "file 5 1 0 0"
    # a truncated file that is read is refused, and names itself
    open(paths[2], "r+b").truncate(12 + 48 * 2 + 7)
    got = s("rewrite", CHUNK, -1, 10.0, *paths)
    assert len(got) == 1 and got[0].startswith("err check: ") and "p2.bin holds" in got[0]


def test_lookahead_order(session):
    s = session()
    assert s("lookahead", 0, -1, -1) == ["rc 0"]
    assert s("lookahead", 1, -1, -1) == ["e0 f0 rc 0"]
    assert s("lookahead", 2, -1, -1) == ["e0 e1 f0 f1 rc 0"]
    assert s("lookahead", 5, -1, -1) == ["e0 e1 f0 e2 f1 e3 f2 e4 f3 f4 rc 0"]
    assert s("lookahead", 5, 2, -1) == ["e0 e1 f0 rc 7"]               # nothing finished after the failed enqueue
    assert s("lookahead", 5, -1, 1) == ["e0 e1 f0 e2 rc 9"]
    assert s("lookahead", 5, -1, 4) == ["e0 e1 f0 e2 f1 e3 f2 e4 f3 rc 9"]


def _keep_all(s, tmp_path, rows, path, first_changed, suffix, count, drop=lambda r: r):
    """11 rows in chunks of 4 through keep(); chunks from `first_changed` on are changed (kept: drop(rows of the chunk))"""
    kept = []
    for c, first in enumerate(range(0, 11, CHUNK)):
        chunk = rows[first:first + CHUNK]
        changed = first_changed is not None and c >= first_changed
        out = drop(chunk) if changed else chunk
        f = tmp_path / f"chunk{c}.f32"
        f.write_bytes(out.tobytes())
        got = s("keep", c, int(changed), suffix, count, f, len(out))
        last = c == 2
        is_open = first_changed is not None and c >= first_changed
        assert got == [f"ok {int(is_open and not last)} {int(is_open and last)} {2 - c}"], (c, got)
        if is_open:
            kept.append(out)
        elif first_changed is not None:
            kept.append(chunk)
        assert os.path.exists(path + suffix) == is_open
    return np.concatenate(kept) if kept else None


@pytest.mark.parametrize("first_changed", [None, 0, 1, 2])
def test_keep(session, tmp_path, first_changed):
    s = session()
    rows = _rows(11, 7)
    p = str(tmp_path / "f.bin")
    open(p, "wb").write(_file(rows, 3, 9))
    before = (open(p, "rb").read(), _stat(p))
    assert s("rewrite", CHUNK, -1, 0, p)[:2] == ["counters 1 0 1", "file 0 0 11 3"]
    # a known count: every chunk's rows replaced by others, as many
    new = _keep_all(s, tmp_path, rows, p, first_changed, ".warp.tmp", "file", drop=lambda r: r + np.float32(1))
    if first_changed is None:
        assert not os.path.exists(p + ".warp.tmp") and (open(p, "rb").read(), _stat(p)) == before
        assert s("replace", "leave") == ["replaced 0 first -"]
        assert (open(p, "rb").read(), _stat(p)) == before
        return
    want = np.concatenate([rows[:first_changed * CHUNK], rows[first_changed * CHUNK:] + np.float32(1)])     # head + kept rows
    assert open(p + ".warp.tmp", "rb").read() == _file(want, 3, 9) and np.array_equal(new, want)
    # the record goes away before the replacement pass: so does the temporary
    assert s("drop") == ["ok"]
    assert not os.path.exists(p + ".warp.tmp") and (open(p, "rb").read(), _stat(p)) == before
    # an unknown count with fewer rows kept: the header carries the rows appended
    assert s("rewrite", CHUNK, -1, 0, p)[0] == "counters 1 0 1"
    new = _keep_all(s, tmp_path, rows, p, first_changed, ".recall.tmp", "unknown", drop=lambda r: r[1:])
    assert len(new) == 11 - (3 - first_changed)
    assert open(p + ".recall.tmp", "rb").read() == _file(new, 3, 9)
    # the replacement pass: the file has the new bytes, the index the new stat
    assert s("replace", "remove") == ["replaced 1 first -"]
    assert open(p, "rb").read() == _file(new, 3, 9) and not os.path.exists(p + ".recall.tmp")
    assert s("valid", p) == ["valid %d %d -inf" % _stat(p)]
    assert s("drop") == ["ok"] and open(p, "rb").read() == _file(new, 3, 9)
    assert sorted(f for f in os.listdir(tmp_path) if not f.startswith("chunk")) == ["f.bin"]


def test_keep_temporary_name_taken(session, tmp_path):
    s = session()
    rows = _rows(11, 8)
    p = str(tmp_path / "f.bin")
    open(p, "wb").write(_file(rows, 0, 0))
    os.mkdir(p + ".warp.tmp")
    f = tmp_path / "chunk.f32"
    f.write_bytes(rows[:4].tobytes())
    assert s("rewrite", CHUNK, -1, 0, p)[0] == "counters 1 0 1"
    assert s("keep", 0, 0, ".warp.tmp", "file", f, 4) == ["ok 0 0 2"]
    assert s("keep", 1, 1, ".warp.tmp", "file", f, 4) == [f"err check: {p}.warp.tmp is not open!"]
    assert s("drop") == ["ok"]
    assert sorted(os.listdir(tmp_path)) == ["chunk.f32", "f.bin", "f.bin.warp.tmp"] and os.listdir(p + ".warp.tmp") == []
    assert open(p, "rb").read() == _file(rows, 0, 0)


@pytest.mark.parametrize("policy", ["remove", "leave"])
def test_replacement_pass_failed_rename(session, tmp_path, policy):
    """files 0 and 1 cannot be replaced (each is a non-empty directory by then), file 2 still is; the first failure is reported"""
    s = session()
    paths, rows = _set(tmp_path, [3, 2, 4])
    assert s("rewrite", CHUNK, -1, 0, *paths)[0] == "counters 3 0 3"
    suffix = ".warp.tmp" if policy == "leave" else ".recall.tmp"
    for c, r in enumerate(rows):
        f = tmp_path / f"chunk{c}.f32"
        f.write_bytes(r[1:].tobytes())
        assert s("keep", c, 1, suffix, "unknown", f, len(r) - 1) == ["ok 0 1 0"]
        os.remove(f)
    for p in paths[:2]:
        assert s("note", p, 1) == ["ok"]
        os.remove(p)
        os.mkdir(p)
        open(os.path.join(p, "x"), "w").close()
    assert s("replace", policy) == [f"replaced 1 first {paths[0]}"]
    assert open(paths[2], "rb").read() == _file(rows[2][1:], 2, 12)
    assert s("valid", paths[2]) == ["valid %d %d -inf" % _stat(paths[2])]
    assert s("drop") == ["ok"]
    left = sorted(os.listdir(tmp_path))
    tmps = [os.path.basename(p) + suffix for p in paths[:2]]
    assert left == sorted(["p0.bin", "p1.bin", "p2.bin"] + (tmps if policy == "leave" else []))
    if policy == "leave":
        for p, r, i in zip(paths[:2], rows, range(2)):
            assert open(p + suffix, "rb").read() == _file(r[1:], i, 10 + i)


def test_check_distinct_paths(session):
    s = session()
    assert s("distinct", "who", "/a/x", "/a/y", "/b/x") == ["ok"]
    assert s("distinct", "who") == ["ok"]
    assert s("distinct", "sm_warp_by_time", "/a/x", "/a/y", "/a/z", "/a/y", "/a/x") == ["err sm_warp_by_time: /a/y is listed twice"]
