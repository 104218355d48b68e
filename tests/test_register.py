"""Registration of one map set against another (sm_register_maps, sm_register_debug; include/sm_c_api.h "registration").
Without a GPU: the symbols, defaults, layouts and argument errors; the restatement (tests/register_ref.py) against answers
derived by hand and against the ground truth of the scenes (tests/register_scenes.py), with the margins that make the GPU
comparisons meaningful.  With one: sm_register_debug's sums pinned to the restatement's products (tests/track_ref.py
assert_system) at sample counts that take every branch of the reduction, bit-identical sums under reorderings and splits of the
sets, loose records, whole runs, every status, the capacity error, that nothing is touched, and register -> warp -> simplify."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import recall_ref as cr
import register_ref as rr
import register_scenes as sc
import retire_ref as ret
import simplify_ref as sr
import table_ref as tb
import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sm_default_register_params", "sm_register_maps", "sm_register_debug", "sm_register_stats")
F32, F64 = np.float32, np.float64
W, H, F = 96, 64, 60.0
MIN_INLIERS = 500            # the scenes' source sets hold 3000 records
# (yaw, seed) of the two streets: chosen on the CPU so that no sample of any system of the restatement's run lies within 1e-6
# (relative) of a deciding threshold (test_scenes_converge_with_margin asserts it): seeds 3 and 1 give 6.2e-6 and 7.2e-6, the
# neighbouring seeds 3e-7 .. 1.5e-6.  At 45 degrees the walls' normals sit on the tie of two faces, see DESIGN.md 4q "Left out".
STREETS = ((20.0, 3), (33.0, 1))
# The other pinned poses are chosen the same way, and test_pinned_poses_have_margin and test_run_from_a_guess_converges_with_margin
# assert the 1e-6 for each of them on the CPU.  sm_register_debug's systems are taken PE_FRAC of the way from the identity to the
# truth (0.9: the smallest margin of any pinned variant is 1.2e-5; at 0.8 it was 3.0e-6).  The run from a guess starts GUESS_FRAC
# of the way with every GUESS_KW["stride"]-th record on two levels (3.0e-5 and 1.3e-5 on the two streets; with a stride of 2 a
# sample of the 20 degree street ends 5.7e-8 from the middle of its cell).  The loose records of LOOSE_SEED leave the run's margin
# the street's own (6.2e-6; the seeds 11 and 13 put a far record 1.3e-6 and 6.8e-7 from a cell face at some iteration).
PE_FRAC, GUESS_FRAC, GUESS_KW, LOOSE_SEED = 0.9, 0.4, dict(stride=5, levels=2, min_inliers=MIN_INLIERS // 2), 12
# (samples, level) of the systems test_gpu_system_is_the_exact_sum pins
REDUCTIONS = ((200, 0), (3000, 0), (3000, 1), (3000, 2), (8000, 0), (40960, 1), (1100000, 0))
# test_gpu_smallest_table_with_wrap_around: found on the CPU, of the origins (0.37 k, 0.21 k, 0), k < 400, only k = 169, 170, 171
# carry a key past the end of the table
WRAP = dict(voxel_mm=1000, levels=1, origin=(0.37 * 169, 0.21 * 169, 0.0))
WRAP_TARGET_ROWS = 6000


def row(x, y, z, n=(0.0, 0.0, 1.0), conf=1.0, sem=3):
    s = np.zeros(12, F32)
    s[0:3] = (x, y, z); s[3] = conf
    s[4:5].view(np.uint32)[0] = (sem << 24) | 0x102030
    s[6], s[7] = 1.0, 1.0
    s[8:11] = n; s[11] = 0.01
    return s


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_defaults():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert name in capi.SYMBOLS and hasattr(L, name), name
    p = capi.default_register_params()
    assert (p.voxel_mm, p.levels, p.max_iters, p.min_inliers, p.stride) == (200, 3, 20, 1000, 0)
    assert (p.angle_thresh, p.reach_cells, p.max_samples, p.max_cells) == (30.0, 1.0, 1 << 22, 1 << 24)
    assert list(p.origin) == [0.0] * 3 and list(p.pivot) == [0.0] * 3
    d = rr.DEFAULTS
    assert all(getattr(p, k) == d[k] for k in d if k not in ("origin", "pivot"))
    assert L.sm_api_version() == 4


def test_null_arguments_without_a_device():
    from surfelmapping_amd import capi
    L = capi.load()
    p, src = capi.default_register_params(), capi.map_source([], include_model=False)
    out, info, n = np.zeros(16, F32), capi.SmRegisterInfo(), C.c_uint32()
    sys29 = np.zeros(29)
    assert L.sm_default_register_params(None) == capi.SM_E_ARG
    assert L.sm_register_maps(None, C.byref(src), C.byref(src), None, C.byref(p), out.ctypes.data, C.byref(info)) == capi.SM_E_ARG
    assert L.sm_register_debug(None, C.byref(src), C.byref(src), out.ctypes.data, 0, C.byref(p), sys29.ctypes.data, C.addressof(n)) == capi.SM_E_ARG
    assert L.sm_register_stats(None, None) == capi.SM_E_ARG
    assert b"sm_register_stats" in L.sm_last_error()


def _one(source, target, **params):
    """the pairs of a hand-made problem at the identity: one level of 1 m cells (V = 65536, an even edge)"""
    pb = rr.Problem(np.array(source), np.array(target), voxel_mm=1000, levels=1, **params)
    return pb, pb.rows(np.eye(4), 0)


def test_ref_one_cell_with_three_records():
    """weights 1, 2, 3 at x = 0.25, 0.75, 0.5: SW = 6, SP_x = 16384 + 2 * 49152 + 3 * 32768 = 212992, (212992 + 3) // 6 = 35499"""
    tgt = [row(0.25, 0.5, 0.5, conf=1 / 16), row(0.75, 0.5, 0.5, conf=2 / 16, sem=7), row(0.5, 0.5, 0.5, conf=3 / 16, sem=9)]
    pb, (J, r, idx, _) = _one([row(0.625, 0.5, 0.75)], tgt, pivot=(0.5, 0.0, 0.0))
    t = pb.levels[0]
    assert pb.cells == [1] and int(t["SW"][0]) == 6 and t["SP"][0].tolist() == [212992, 6 * 32768, 6 * 32768]
    assert t["SN"][0].tolist() == [0, 0, 6 * 16384]
    assert int(t["keys"][0]) == ((65536 << 34 | 65536 << 17 | 65536) << 11) | (4 << 8)          # cell (0, 0, 0), face +z, class 0
    assert t["pos"][0].tolist() == [F32(35499 / 65536), 0.5, 0.5] and t["nrm"][0].tolist() == [0.0, 0.0, 1.0]
    # e = (0.625 - 35499 / 65536, 0, 0.25); r = e_z; u = q - pivot = (0.125, 0.5, 0.75); u x n = (u1, -u0, 0)
    assert idx.tolist() == [0] and r.tolist() == [0.25] and J.tolist() == [[0.0, 0.0, 1.0, 0.5, -0.125, 0.0]]


def test_ref_sample_at_half_a_cell():
    """off == V / 2 takes the neighbour above, one unit below it the neighbour below: the cell of q is empty, the representative
    at x = -0.05 is the nearer one and is no candidate of the first sample"""
    tgt = [row(1.25, 0.25, 0.3125), row(-0.0625, 0.25, 0.1875)]
    src = [row(0.5, 0.25, 0.25), row(0.5 - 2.0 ** -16, 0.25, 0.25)]
    pb, (J, r, idx, mg) = _one(src, tgt)
    assert idx.tolist() == [0, 1] and r.tolist() == [-0.0625, 0.0625]
    assert mg["half"] == 0.0 and pb.levels[0]["pos"][:, 0].tolist() == [-0.0625, 1.25]


def test_ref_negative_cells():
    """-0.4f = -0.4000000059..: X = floor(-26214.4004) = -26215, cell -1 (floor division), off = 39321"""
    pb, (J, r, idx, _) = _one([row(-0.25, -0.25, -0.25)], [row(-0.4, -0.4, -0.4)])
    t = pb.levels[0]
    assert int(t["keys"][0]) == ((65535 << 34 | 65535 << 17 | 65535) << 11) | (4 << 8)
    assert t["SP"][0].tolist() == [16 * 39321] * 3 and t["pos"][0].tolist() == [F32(-26215 / 65536)] * 3
    assert idx.tolist() == [0] and r.tolist() == [F32(-0.25 + 26215 / 65536)]
    # a sample whose neighbour cell would be -65537 has that candidate dropped, not wrapped
    far = -65536.0 + 0.25
    pb, (J, r, idx, _) = _one([row(far, 0.25, 0.25)], [row(far + 0.125, 0.25, 0.25)])
    assert idx.tolist() == [0]


def test_ref_distance_tie_goes_to_the_lower_key():
    tilt = (0.0, math.sin(math.radians(10.0)), math.cos(math.radians(10.0)))
    for first, second in (((0.0, 0.0, 1.0), tilt), (tilt, (0.0, 0.0, 1.0))):
        pb, (J, r, idx, mg) = _one([row(0.875, 0.25, 0.25)], [row(0.75, 0.25, 0.25, n=first), row(1.0, 0.25, 0.25, n=second)])
        assert mg["tie"] == 0.0 and idx.tolist() == [0]
        assert J[0, :3].tolist() == pb.levels[0]["nrm"][0].tolist()                # keys ascend: [0] is the cell at x = 0.75
        assert abs(float(J[0, 1]) - first[1]) < 1e-4


def test_ref_loose_records_by_level():
    """20 km out is cell 100000 of the 0.2 m grid, past its range, and cell 50000 of the 0.4 m one, inside it"""
    rows = sc.loose_rows(np.random.default_rng(2), 9)
    assert rr.fields_ok(rows).tolist() == [False, False, True] * 3
    pb = rr.Problem(rows, rows, min_inliers=0)
    assert pb.cells == [0, 3, 3] and int(pb.regular.sum()) == 3


def _pose_near(truth, frac):
    """a pose part of the way from the identity to the truth, as the float32 matrix the call gets"""
    return (np.eye(4) + frac * (truth - np.eye(4))).astype(F32)


@pytest.fixture(scope="module")
def base():
    src, tgt, truth, pivot = sc.street_pair(yaw_deg=STREETS[0][0], seed=STREETS[0][1])
    return dict(src=src, tgt=tgt, truth=truth, pivot=pivot, pe=_pose_near(truth, PE_FRAC), params=dict(min_inliers=MIN_INLIERS, pivot=pivot))


def _spread(src, n):
    """n source rows for the large reductions: copies of the street's, every 16th copy in place and the others a kilometre up,
    where nothing pairs -- pairs all over the index range, and few enough of them for the exact sums to take no time"""
    reps = -(-n // len(src))
    out = np.tile(src, (reps, 1))[:n].copy()
    copy = np.arange(n) // len(src)
    out[copy % 16 != 0, 2] += 1000.0
    return out


def _reduction_problem(base, n):
    """(source rows, Problem) of test_gpu_system_is_the_exact_sum's system of n samples"""
    src = base["src"][:n] if n <= len(base["src"]) else _spread(base["src"], n)
    return src, rr.Problem(src, base["tgt"], **base["params"])


def _wrap_problem(base):
    """(target rows, Problem) of test_gpu_smallest_table_with_wrap_around"""
    tgt = base["tgt"][:WRAP_TARGET_ROWS]
    return tgt, rr.Problem(base["src"], tgt, **WRAP, **base["params"])


def _loose_problem(base):
    """(source rows, target rows, Problem) of test_gpu_loose_records_in_both_sets"""
    rng = np.random.default_rng(LOOSE_SEED)
    src = np.concatenate([base["src"][:1500], sc.loose_rows(rng, 30), base["src"][1500:]])
    tgt = np.concatenate([sc.loose_rows(rng, 30), base["tgt"]])
    return src, tgt, rr.Problem(src, tgt, **base["params"])


@pytest.fixture(scope="module", params=STREETS, ids=lambda s: f"yaw{s[0]:.0f}")
def street(request):
    yaw, seed = request.param
    src, tgt, truth, pivot = sc.street_pair(yaw_deg=yaw, seed=seed)
    T, info = rr.register(src, tgt, min_inliers=MIN_INLIERS, pivot=pivot)
    # a guess and a stride: the restatement from the same start
    g, kw2 = _pose_near(truth, GUESS_FRAC), dict(GUESS_KW, pivot=pivot)
    T2, info2 = rr.register(src, tgt, guess=g, **kw2)
    return dict(src=src, tgt=tgt, truth=truth, pivot=pivot, T=T, info=info, params=dict(min_inliers=MIN_INLIERS, pivot=pivot),
                guess=g, params2=kw2, T2=T2, info2=info2)


def test_scenes_converge_with_margin(street):
    """(a) no sample of any system within 1e-6 of a threshold; (b) OK, and the truth recovered.  Each record carries 1 cm of
    noise; the direction along the street is held by the ~250 samples on the three box faces alone, each against a cell mean of a
    few records: 1 cm * sqrt(2 / 250) ~ 1 mm, so 5 mm is five sigma, and 5 mm over the 20 m half length is 0.015 degrees."""
    info = street["info"]
    print(info["status"], info["iterations"], info["counts"], info["margin"], tr.pose_error(street["T"], street["truth"]))
    assert info["margin"] >= 1e-6
    assert info["status"] == "OK" and all(1 <= i < 20 for i in info["iterations"])
    dt, dr = tr.pose_error(street["T"], street["truth"])
    assert dt < 0.005 and dr < 0.015
    assert tr.pose_error(np.eye(4), street["truth"])[0] > 0.4                     # (the start is half a metre and 1.6 degrees off)


def test_run_from_a_guess_converges_with_margin(street):
    """(a) and (b) for the second run test_gpu_run_matches_the_restatement compares: from a guess, strided, on two levels"""
    info = street["info2"]
    print(info["status"], info["iterations"], info["counts"], info["margin"], tr.pose_error(street["T2"], street["truth"]))
    assert info["margin"] >= 1e-6
    assert info["status"] == "OK" and info["stride"] == GUESS_KW["stride"] and all(1 <= i < 20 for i in info["iterations"])
    assert info["inliers"] >= 2 * GUESS_KW["min_inliers"]
    dt, dr = tr.pose_error(street["T2"], street["truth"])
    assert dt < 0.01 and dr < 0.03                    # (a fifth of the samples: sqrt(5) of test_scenes_converge_with_margin's sigma)


def test_pinned_poses_have_margin(base):
    """(a) at every pose at which a GPU test pins sm_register_debug's system, for the sets of each of them: no sample within 1e-6
    of a threshold -- and the same for every system of the run with loose records"""
    pe, found = base["pe"].astype(F64), {}

    def note(what, pb, levels):
        for l in levels:
            found[f"{what}, level {l}"] = min(pb.rows(pe, l)[3].values())
    for n, level in REDUCTIONS:
        note(f"{n} samples", _reduction_problem(base, n)[1], [level])
    note("order and split", rr.Problem(base["src"], base["tgt"], **base["params"]), range(3))
    note("wrap-around", _wrap_problem(base)[1], [0])
    src, tgt, pb = _loose_problem(base)
    note("loose", pb, range(3))
    run = rr.register(src, tgt, **base["params"])[1]
    found["loose, the run"] = run["margin"]
    for what, m in found.items():
        print(f"{what}: {m:.3g}")
    assert run["status"] == "OK" and min(found.values()) >= 1e-6, min(found, key=found.get)


def test_lone_plane_is_degenerate_in_the_restatement():
    s, t = sc.plane_pair()
    T, info = rr.register(s, t, min_inliers=100)
    assert info["status"] == "DEGENERATE" and np.array_equal(T, np.eye(4))


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _ctx(rows=None, cap=80):
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, preprocess=0, stereo_border=0.0, max_sqrt_vertices=cap))
    if rows is not None and len(rows):
        m.upload_model(rows)
    return m


def _write(folder, name, rows):
    path = str(folder / name)
    cr.write_map(path, np.ascontiguousarray(rows, F32).reshape(-1, 12), 1, 2)
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("n,level", REDUCTIONS,
                         ids=["one-workgroup", "3-parts-l0", "3-parts-l1", "3-parts-l2", "8-parts", "tail-loop", "clamp"])
def test_gpu_system_is_the_exact_sum(base, tmp_path, n, level):
    """k_register_reduce has ceil(n / 1024) workgroups, at most 1024: 200 samples are one workgroup with idle waves, 3000 give
    3 partials (fewer than track_sum_parts' eight lanes per value), 8000 exactly 8, 40960 give 40 (its unrolled loop and its
    tail), 1.1 M clamp the grid so that lanes take several samples"""
    src, pb = _reduction_problem(base, n)
    terms = pb.terms(base["pe"].astype(F64), level)
    assert len(terms) >= min(n, 3000) // 2
    m = _ctx()
    got, ns = m.register_debug([_write(tmp_path, "s.bin", src)], [_write(tmp_path, "t.bin", base["tgt"])], base["pe"], level, **base["params"])
    st = m.register_stats()
    m.close()
    assert ns == n and st["source_records"] == n and st["target_records"] == len(base["tgt"])
    tr.assert_system(got, terms, f"n = {n}, level {level}")


@pytest.mark.gpu
def test_gpu_smallest_table_with_wrap_around(base, tmp_path):
    """max_cells = the keys of the coarsest level leaves the smallest table the rule allows (the power of two >= 2 * max_cells);
    the origin is one at which a run of occupied slots crosses its end, so that a probe walks from the last slot to slot 0"""
    tgt, pb = _wrap_problem(base)
    origin = WRAP["origin"]
    size = 1024
    while size < 2 * pb.cells[0]:
        size <<= 1
    carried = tb.wraps(pb.levels[0]["keys"].tolist(), size - 1)
    assert size == 2048 and carried >= 1
    print(f"origin {origin}: {pb.cells[0]} keys in {size} slots, {carried} carried past the end")
    terms = pb.terms(base["pe"].astype(F64), 0)
    m = _ctx()
    got, _ = m.register_debug([_write(tmp_path, "s.bin", base["src"])], [_write(tmp_path, "t.bin", tgt)], base["pe"], 0, max_cells=pb.cells[0],
                              **WRAP, **base["params"])
    m.close()
    tr.assert_system(got, terms, f"table of {size} slots, {pb.cells[0]} keys")


@pytest.mark.gpu
def test_gpu_sums_do_not_depend_on_order_or_split(base, tmp_path, monkeypatch):
    """the table is a function of the multiset of target records and the samples of the source concatenation: shuffled target
    rows, five target files (one empty, one of a single row) plus a live remainder, another split of the source and the combine
    step off give the same 29 doubles bit for bit, at one pose per level"""
    src, tgt, pe, kw = base["src"], base["tgt"], base["pe"], base["params"]
    m = _ctx()
    s1, t1 = [_write(tmp_path, "s.bin", src)], [_write(tmp_path, "t.bin", tgt)]
    want = [m.register_debug(s1, t1, pe, l, **kw)[0] for l in range(3)]
    pb = rr.Problem(src, tgt, **kw)
    for l in range(3):
        tr.assert_system(want[l], pb.terms(pe.astype(F64), l), f"level {l}")

    def same(what, sp, tp, **more):
        for l in range(3):
            got = m.register_debug(sp, tp, pe, l, **kw, **more)[0]
            assert np.array_equal(got.view(np.uint64), want[l].view(np.uint64)), (what, l, got - want[l])
    perm = np.random.RandomState(7).permutation(len(tgt))
    same("shuffled", s1, [_write(tmp_path, "tp.bin", tgt[perm])])
    parts = np.split(tgt, [5000, 5000, 5001, 12000, 17000])                       # five files and 3000 live rows
    m.upload_model(parts[5])
    same("split", s1, [_write(tmp_path, f"t{i}.bin", parts[i]) for i in range(5)], target_model=True)
    same("source split", [_write(tmp_path, f"s{i}.bin", p) for i, p in enumerate(np.split(src, [1, 1, 1700]))], t1)
    m.upload_model(src[2000:])
    same("source model", [_write(tmp_path, "sh.bin", src[:2000])], t1, source_model=True)
    for v in ("0", "1"):
        monkeypatch.setenv("SM_SIMPLIFY_NO_COMBINE", v)
        same("combine " + v, s1, t1)
    m.close()


@pytest.mark.gpu
def test_gpu_loose_records_in_both_sets(base, tmp_path):
    src, tgt, pb = _loose_problem(base)
    m = _ctx()
    sp, tp = [_write(tmp_path, "s.bin", src)], [_write(tmp_path, "t.bin", tgt)]
    for l in range(3):
        got, ns = m.register_debug(sp, tp, base["pe"], l, **base["params"])
        assert ns == len(src)
        tr.assert_system(got, pb.terms(base["pe"].astype(F64), l), f"loose, level {l}")
    _, info = m.register_maps(sp, tp, **base["params"])
    m.close()
    assert info["cells"] == pb.cells and info["samples"] == int(pb.regular.sum()) == len(src) - 20


def _assert_pose(got, want, what):
    """every entry equal to, or a neighbouring float32 of, the restatement's double pose rounded to float32 (the tolerance of
    tests/test_track_pin.py; the step about the pivot adds three double operations per entry to the trackers', far below it)"""
    got, w32 = np.asarray(got, F32), np.asarray(want, F64).astype(F32)
    diff = np.abs(got.astype(F64) - w32.astype(F64))
    tol = 2.0 ** -23 * np.maximum(1.0, np.abs(w32.astype(F64)))
    assert (diff <= tol).all(), f"{what}: pose entries off by up to {(diff / tol).max():.3g} of the bound\n{got}\n{w32}"


@pytest.mark.gpu
def test_gpu_run_matches_the_restatement(street, tmp_path):
    want = street["info"]
    m = _ctx()
    sp, tp = [_write(tmp_path, "s.bin", street["src"])], [_write(tmp_path, "t.bin", street["tgt"])]
    pose, info = m.register_maps(sp, tp, **street["params"])
    st = m.register_stats()
    print(info, st)
    assert (info["status"], info["iterations"], info["inliers"]) == (want["status"], want["iterations"], want["inliers"])
    assert (info["cells"], info["samples"], info["stride"]) == (want["cells"], want["samples"], want["stride"])
    _assert_pose(pose, street["T"], "run")
    assert abs(info["rmse"] - want["rmse"]) <= 1e-6 * want["rmse"] and abs(info["pivot_ratio"] - want["pivot_ratio"]) <= 1e-6 * want["pivot_ratio"]
    assert st["launches"] == 3 * 1 + 3 + 1 + 2 * 60 and st["chunks"] == 2 and st["iterate_ms"] > 0.0 and st["table_ms"] > 0.0
    # a guess and a stride (test_run_from_a_guess_converges_with_margin has the restatement's margin)
    want2 = street["info2"]
    pose2, info2 = m.register_maps(sp, tp, guess=street["guess"], **street["params2"])
    m.close()
    assert (info2["status"], info2["iterations"], info2["inliers"]) == ("OK", want2["iterations"], want2["inliers"])
    assert (info2["cells"], info2["samples"], info2["stride"]) == (want2["cells"], want2["samples"], GUESS_KW["stride"])
    _assert_pose(pose2, street["T2"], "run from a guess")


@pytest.mark.gpu
def test_gpu_statuses_return_the_guess(base, tmp_path):
    from surfelmapping_amd import capi
    m = _ctx()
    sp, tp = [_write(tmp_path, "s.bin", base["src"])], [_write(tmp_path, "t.bin", base["tgt"])]
    empty = [_write(tmp_path, "e.bin", np.zeros((0, 12), F32))]
    g = _pose_near(base["truth"], 0.3)
    plane_s, plane_t = sc.plane_pair()
    pp = [_write(tmp_path, "ps.bin", plane_s)], [_write(tmp_path, "pt.bin", plane_t)]
    cases = (("LOST", sp, tp, dict(base["params"], min_inliers=2900)),
             ("DEGENERATE", pp[0], pp[1], dict(min_inliers=100)),
             ("NO_TARGET", sp, empty, base["params"]),
             ("NO_SOURCE", empty, tp, base["params"]))
    for status, a, b, kw in cases:
        for guess, back in ((None, np.eye(4, dtype=F32)), (g, g)):
            pose, info = m.register_maps(a, b, guess=guess, **kw)
            assert info["status"] == status, (status, info)
            assert np.array_equal(pose, back), status
    assert rr.register(base["src"], base["tgt"], **dict(base["params"], min_inliers=2900))[1]["status"] == "LOST"
    # SM_E_CAPACITY: fewer cells allowed than a level holds
    with pytest.raises(capi.SurfelMapError) as e:
        m.register_maps(sp, tp, max_cells=1000, **base["params"])
    assert e.value.rc == capi.SM_E_CAPACITY and "max_cells" in str(e.value)
    # SM_E_ARG: a path in both sets, a bad file named before anything runs, parameters out of range
    for bad in (lambda: m.register_maps(sp, sp + tp), lambda: m.register_maps(sp, [str(tmp_path / "none.bin")]),
                lambda: m.register_maps(sp, tp, levels=5), lambda: m.register_maps(sp, tp, angle_thresh=90.0),
                lambda: m.register_maps(sp, tp, stride=1, max_samples=100), lambda: m.register_debug(sp, tp, g, 3)):
        with pytest.raises(capi.SurfelMapError) as e:
            bad()
        assert e.value.rc == capi.SM_E_ARG
    m.close()


@pytest.mark.gpu
def test_gpu_nothing_is_touched(base, tmp_path):
    """the files' bytes, the model's rows, counts() -- the tick is one of them -- and the stored poses with their codes and times"""
    m = _ctx(base["tgt"][:3000])
    m.set_tick(7)
    m.set_ferns()
    words = m.fern_keyframes()["codes"].shape[1]
    for k, pose in enumerate((base["truth"], base["pe"])):
        assert m.fern_add(np.full(words, 0x01234567 * (k + 1), np.uint32), pose, 3 + k) == k
    sp, tp = [_write(tmp_path, "s.bin", base["src"])], [_write(tmp_path, "t.bin", base["tgt"][3000:])]

    def state():
        return [open(p, "rb").read() for p in sp + tp], m.download_model().copy(), m.counts(), m.fern_keyframes()
    before = state()
    assert before[2]["tick"] == 7 and len(before[3]["times"]) == 2
    _, info = m.register_maps(sp, tp, target_model=True, **base["params"])
    assert info["status"] == "OK"
    after = state()
    m.close()
    assert before[0] == after[0] and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32)) and before[2] == after[2]
    for k in ("codes", "poses", "times"):
        assert np.array_equal(before[3][k].view(np.uint32), after[3][k].view(np.uint32)), k
    assert sorted(os.listdir(tmp_path)) == ["s.bin", "t.bin"]


@pytest.mark.gpu
def test_gpu_register_warp_simplify(street, tmp_path):
    """register_maps(apply=True), then simplify_maps over both sets: the record count of the restatement's pipeline, and every
    warped source position within the registration's own error of the truth.  The bound: the largest distance between the
    restatement's pose and the truth applied to a source position, plus float32 rounding -- the pose's 12 entries rounded to
    float32 and the warp's three products and three sums per coordinate, each at most half an ulp of a value below 64 m (2^-19
    m): 16 * 2^-19 m covers the sixteen of them."""
    src, tgt, truth, T = street["src"], street["tgt"], street["truth"], street["T"]
    p = src[:, 0:3].astype(F64)
    want_pos = p @ truth[:3, :3].T + truth[:3, 3]
    bound = np.linalg.norm(p @ T[:3, :3].T + T[:3, 3] - want_pos, axis=1).max() + 16 * 2.0 ** -19
    assert bound < 0.01
    m = _ctx()
    sp, tp = [_write(tmp_path, "s.bin", src)], [_write(tmp_path, "t.bin", tgt)]
    pose, info = m.register_maps(sp, tp, apply=True, **street["params"])
    assert info["status"] == "OK" and info["applied"]
    moved = ret.read_map(sp[0])[0]
    err = np.linalg.norm(moved[:, 0:3].astype(F64) - want_pos, axis=1)
    print(f"largest error of a warped source position {err.max():.6f} m, bound {bound:.6f} m")
    assert err.max() <= bound
    out = str(tmp_path / "both.bin")
    st = m.simplify_maps(tp + sp, out, voxel_mm=200)
    m.close()
    # the restatement's pipeline: its own float32 pose through the warp's float32 arithmetic, then the simplification
    P = np.asarray(T, F64).astype(F32)
    ref = src.copy()
    for k, (a, b) in enumerate(((0, 3), (8, 11))):
        v = src[:, a:b]
        ref[:, a:b] = np.stack([(P[r, 0] * v[:, 0] + P[r, 1] * v[:, 1]) + P[r, 2] * v[:, 2] + (P[r, 3] if k == 0 else F32(0)) for r in range(3)], axis=1)
    want_rows, want_st = sr.simplify_set([tgt, ref], voxel_mm=200)
    near = abs(st["records_out"] - want_st["records_out"])
    print(f"records out {st['records_out']}, the restatement's pipeline {want_st['records_out']}")
    assert st["records_in"] == len(src) + len(tgt) and near == 0
