"""The packed map-file format without a GPU: the numpy restatement of its codec (tests/pack_ref.py) against the error bounds the
format promises, the host decoders (capi.read_packed_map, sm_mapfile.h's) against it, and the checked open of sm_mapfile.h --
tests/cpp/packfile_check.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import pack_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfelmapping_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "packfile_check.cpp")


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def codes():
    c = np.arange(1 << 20)
    ou, ov = c & 1023, c >> 10
    return ou, ov, pr.oct_decode(ou, ov)


def test_every_normal_code_decodes_to_a_unit_vector(codes):
    _, _, d = codes
    assert d.dtype == np.float32 and np.isfinite(d).all()
    # each component is (integer / sqrt(integer)): one correctly rounded sqrt and one correctly rounded division, 2^-24 relative
    # each, so the length is 1 within 2 * 2^-24 = one fp32 ulp of 1
    length = np.linalg.norm(d.astype(np.float64), axis=1)
    print("largest | |n| - 1 |:", np.abs(length - 1).max())
    assert np.abs(length - 1).max() <= 2.0 ** -23


def test_decode_encode_decode_is_decode_for_every_normal_code(codes):
    _, _, d = codes
    again = pr.oct_decode(*pr.oct_encode(d))
    assert _same(again, d)


def test_normal_angle_of_random_unit_vectors():
    v = np.random.default_rng(5).normal(size=(200000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    d = pr.oct_decode(*pr.oct_encode(v.astype(np.float32))).astype(np.float64)
    angle = np.degrees(np.arccos(np.clip((d * v).sum(axis=1) / np.linalg.norm(d, axis=1), -1, 1)))
    print("largest angle [deg]:", angle.max())
    assert angle.max() <= 0.25


@pytest.mark.parametrize("step", [-10, -14, -6])
def test_packed_rows_keep_the_promised_bounds(step):
    rows = pr.fixture_a(769, seed=2)
    rows[:, 0:3] *= np.float32(min(1.0, 2.0 ** (step + 10)))  # (a block spans at most 65535 steps: 4 m at 2^-14)
    data, raw = pr.encode(rows, 3, 9, step)
    assert not raw.any() and len(raw) == 4
    assert len(data) == pr.packed_size(len(rows), raw) == 32 + 32 * 4 + 20 * 769
    got, ids, raw2 = pr.decode(data)
    assert ids == (3, 9) and not raw2.any()
    a, b = rows.astype(np.float64), got.astype(np.float64)
    pos = np.abs(b[:, 0:3] - a[:, 0:3])
    bound = 2.0 ** (step - 1) + np.spacing(np.abs(rows[:, 0:3])).astype(np.float64)      # half a step plus one fp32 ulp of the coordinate
    print("step", step, "position", pos.max(), "radius", np.abs(b[:, 11] - a[:, 11]).max(), "conf", np.abs(b[:, 3] - a[:, 3]).max())
    assert (pos <= bound).all()
    assert np.abs(b[:, 11] - a[:, 11]).max() <= 2.0 ** -14
    assert np.abs(b[:, 3] - a[:, 3]).max() <= 1.0 / 32
    assert np.array_equal(got.view(np.uint32)[:, 4], rows.view(np.uint32)[:, 4])            # the colour word
    assert np.array_equal(got[:, 5:8].view(np.uint32), rows[:, 5:8].view(np.uint32))        # m[5] and both times
    cosang = (b[:, 8:11] * a[:, 8:11]).sum(axis=1) / (np.linalg.norm(b[:, 8:11], axis=1) * np.linalg.norm(a[:, 8:11], axis=1))
    assert np.degrees(np.arccos(np.clip(cosang, -1, 1))).max() <= 0.25


def test_each_raw_cause_makes_its_block_raw_and_raw_blocks_are_verbatim():
    rows, want = pr.fixture_b()
    data, raw = pr.encode(rows, -2, 5)
    assert list(np.flatnonzero(raw)) == list(want)
    assert len(data) == pr.packed_size(len(rows), raw)
    got, ids, raw2 = pr.decode(data)
    assert ids == (-2, 5) and np.array_equal(raw, raw2)
    d = np.frombuffer(data, pr.DIR_DTYPE, len(raw), pr.HEADER_BYTES)
    for b in want:
        sl = slice(b * pr.BLOCK, (b + 1) * pr.BLOCK)
        assert np.array_equal(got[sl].view(np.uint32), rows[sl].view(np.uint32)), pr.RAW_CAUSES[b - 1]
        assert not d["origin"][b].any() and d["time_base"][b] == 0 and d["init_base"][b] == 0
    # and every cause alone is what did it: the same block without its one bad record packs
    clean = pr.fixture_a(len(rows), 1)
    assert not pr.encode(clean)[1].any()


@pytest.mark.parametrize("step", [-10, -14, -6])
def test_unpack_pack_unpack_is_unpack(step):
    for rows in (pr.fixture_a(769, 3), pr.fixture_b()[0], pr.fixture_a(0), pr.fixture_a(1)):
        first, ids, _ = pr.decode(pr.encode(rows, 1, 2, step)[0])
        again, ids2, _ = pr.decode(pr.encode(first, 1, 2, step)[0])
        assert ids == ids2 == (1, 2) and _same(first, again)


def test_a_coordinate_near_the_limit_survives_a_second_packing():
    rows = pr.fixture_a(300, 4)
    rows[:, 0] += np.float32(8180)                           # some decode to >= 8192: RAW the second time, the same rows
    rows[:, 0] = np.minimum(rows[:, 0], np.float32(8191.9995))
    first = pr.decode(pr.encode(rows)[0])[0]
    assert _same(first, pr.decode(pr.encode(first)[0])[0])


def test_read_packed_map_is_the_reference_decode(tmp_path):
    from surfelmapping_amd import capi
    for name, rows in (("a", pr.fixture_a(769, 6)), ("b", pr.fixture_b()[0]), ("empty", pr.fixture_a(0))):
        path = tmp_path / f"{name}.smp"
        path.write_bytes(pr.encode(rows, 4, 8, -9)[0])
        got, ids, raw = capi.read_packed_map(path)
        want, ids2, raw2 = pr.decode(path.read_bytes())
        assert ids == ids2 == (4, 8) and _same(got, want) and np.array_equal(raw, raw2)
        assert capi._map_records(path) == len(rows)
    plain = tmp_path / "plain.bin"
    plain.write_bytes(pr.plain_bytes(pr.fixture_a(7)))
    assert capi._map_records(plain) == 7
    with pytest.raises(ValueError):
        capi.read_packed_map(plain)
    cut = tmp_path / "cut.smp"
    cut.write_bytes(pr.encode(pr.fixture_a(300))[0][:-1])
    with pytest.raises(ValueError):
        capi.read_packed_map(cut)


# ---- the checked open of sm_mapfile.h
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("packfile") / "packfile_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, "-o", exe, SRC])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (args, r.stdout, r.stderr)
        return r.stdout.splitlines()
    return run


def _patched(data, at, value, fmt="<u4"):
    raw = np.array([value], fmt).tobytes()
    return data[:at] + raw + data[at + len(raw):]


def test_checked_open_of_packed_files(check, tmp_path):
    rows, _ = pr.fixture_b()
    good, raw = pr.encode(rows, 7, 11, -9)                   # (a block spans 128 m at this step: the block of 85 m packs)
    nb = len(raw)
    assert int(raw.sum()) == len(pr.RAW_CAUSES) - 1
    size = pr.packed_size(len(rows), raw)
    cases = dict(
        good=good, empty=pr.encode(rows[:0], 1, 2)[0], cut=good[:-1], long=good + b"\0", header_only=good[:32], stub=good[:20],
        offset=_patched(good, 32 + 32 * 3 + 24, 12345, "<u8"),          # block 3 somewhere else
        offsets_shifted=good[:32] + b"".join(_patched(good[32 + 32 * b:64 + 32 * b], 24, int(np.frombuffer(good, "<u8", 1, 32 + 32 * b + 24)[0]) + 20, "<u8")
                                             for b in range(nb)) + good[32 + 32 * nb:],
        flags=_patched(good, 32 + 32 * 2 + 20, 2), flipped=_patched(good, 32 + 20, 1),   # an unknown flag; block 0 RAW: another size
        blocks=_patched(good, 24, nb + 1), version=_patched(good, 4, 2), reserved=_patched(good, 28, 1), step=_patched(good, 20, -5, "<i4"))
    for name, data in cases.items():
        (tmp_path / f"{name}.smp").write_bytes(data)
    order = list(cases)
    both = dict(zip(order, check("open", "both", *[tmp_path / f"{n}.smp" for n in order])))
    assert both["good"] == f"ok 1 {len(rows)} 7 11 {size} {32 + 32 * nb} {nb} {int(raw.sum())} -9"  # positioned at the payload
    assert both["empty"] == "ok 1 0 1 2 32 32 0 0 -10"
    for name in order[2:]:
        assert both[name].startswith("err check: ") and f"{name}.smp is a packed map file, but " in both[name], (name, both[name])
    assert both["cut"].endswith(f"it holds {size - 1} bytes, its directory needs {size}")
    assert both["long"].endswith(f"it holds {size + 1} bytes, its directory needs {size}")
    assert "block 3 lies at offset 12345" in both["offset"] and "block 0 lies at offset 20" in both["offsets_shifted"]
    assert "unknown flags" in both["flags"] and "block 1 lies at offset" in both["flipped"]
    assert check("looks", tmp_path / "good.smp", tmp_path / "cut.smp", tmp_path / "missing.smp") == ["1", "1", "0"]
    # a caller that takes plain files only gets the refusal that names the way out, for a whole packed file and a broken one alike
    plain_only = check("open", "plain", tmp_path / "good.smp", tmp_path / "cut.smp")
    for line, name in zip(plain_only, ("good", "cut")):
        assert line == f"err check: {tmp_path / name}.smp is a packed map file; sm_unpack_maps makes a plain one"


def test_checked_open_still_opens_plain_files(check, tmp_path):
    rows = pr.fixture_a(5)
    whole = pr.plain_bytes(rows, 7, 11)
    (tmp_path / "good.bin").write_bytes(whole)
    (tmp_path / "short.bin").write_bytes(whole[:-48])
    for mode in ("plain", "both"):
        got = check("open", mode, tmp_path / "good.bin", tmp_path / "short.bin")
        assert got[0] == f"ok 0 5 7 11 {12 + 48 * 5} 12 0 0 0"
        assert got[1].endswith(f"short.bin holds {12 + 48 * 4} bytes, its header's 5 records need {12 + 48 * 5}")
    assert check("looks", tmp_path / "good.bin") == ["0"]


def test_host_decoder_of_the_header_is_the_reference_decode(check, tmp_path):
    for name, rows, step in (("a", pr.fixture_a(769, 8), -10), ("b", pr.fixture_b()[0], -12), ("empty", pr.fixture_a(0), -10)):
        path, out = tmp_path / f"{name}.smp", tmp_path / f"{name}.f32"
        path.write_bytes(pr.encode(rows, 0, 0, step)[0])
        assert check("decode", path, out) == [f"ok {len(rows)}"]
        assert _same(np.fromfile(out, np.float32).reshape(-1, 12), pr.decode(path.read_bytes())[0])


def test_header_stays_host_only():
    text = open(os.path.join(CSRC, "sm_mapfile.h")).read()
    assert "#include <hip" not in text and '#include "sm_ctx.h"' not in text
