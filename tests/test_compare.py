"""Change detection between two map sets (sm_compare_maps; include/sm_c_api.h "change detection").  Without a GPU: the symbols,
defaults, layouts and argument errors, and the restatement (tests/compare_ref.py) against labels derived by hand.  With one:
labels, counts, table sizes and the written file against the restatement, bit for bit -- the feature has no tolerance."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import compare_ref as cf
import recall_ref as cr
import register_scenes as sc
import retire_ref as ret
import table_ref as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sm_default_compare_params", "sm_compare_maps", "sm_compare_stats")
F32, F64 = np.float32, np.float64
W, H, F = 96, 64, 60.0
S, CH, OUT, LO = cf.SUPPORTED, cf.CHANGED, cf.OUTSIDE, cf.LOOSE
# The hand-derived scene: voxel_mm = 125 gives V0 = 8192 (cells of 1/8 m) and V1 = 65536 (cover cells of 1 m); the reach is
# 1.25 * 1/8 = 0.15625 m, the plane gate 125 / 1000 = 0.125 m -- all exact in binary.
HAND = dict(voxel_mm=125, cover_shift=3, reach_cells=1.25, plane_mm=125, angle_thresh=30.0)
# ... and its pose, query world -> reference world: a quarter turn about z and a shift, entries 0, 1, -1 and dyadic fractions, so
# that moving a record costs no rounding
HAND_POSE = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 0.5], [0.0, 0.0, 0.0, 1.0]])
# The street (test_gpu_street_matches_the_restatement): cells of 1 m -- the 5 000 reference records are 7 to the square metre, so
# a cell a surface crosses is all but never empty --, cover cells of 2 m, the other parameters the defaults
STREET = dict(voxel_mm=1000, cover_shift=1)
# The smallest tables (test_gpu_smallest_tables_with_wrap_around): cells of 1/8 m, cover cells of 1/4 m -- at cover_shift 3 a
# thousand records have too few cover keys for one of them to be carried past the end of 2048 slots at any origin of the grid
WRAP = dict(voxel_mm=125, cover_shift=1, reach_cells=0.5, origin=(0.0, 0.21 * 19, 0.0))
WRAP_REF_ROWS = 1000
U = 2.0 ** -16


def row(x, y, z, n=(0.0, 0.0, 1.0), conf=1.0, sem=3):
    s = np.zeros(12, F32)
    s[0:3] = (x, y, z); s[3] = conf
    s[4:5].view(np.uint32)[0] = (sem << 24) | 0x102030
    s[6], s[7] = 1.0, 1.0
    s[8:11] = n; s[11] = 0.01
    return s


def _cos_neighbours(deg):
    """the two neighbouring float32 values around cos(deg): (the smallest >= it, the largest < it)"""
    c = math.cos(float(F32(deg)) * (math.pi / 180.0))
    hi = F32(c)
    if float(hi) < c:
        hi = np.nextafter(hi, F32(2))
    return float(hi), float(np.nextafter(hi, F32(0)))


def hand_scene():
    """Three reference records and seventeen query records, each given here where the pose puts it (the query file holds it
    moved back by the pose's inverse, exactly).  Cells are 1/8 m, cover cells 1 m, reach 0.15625, plane gate 0.125, 30 degrees.
      reference  R0 ground (0.34375, 0.3125, 0.09375) n +z: cell (2, 2, 0), alone under its key, so it is its representative
                 R1 ground (2.3125, 0.3125, 0.0625) n +z: cover cell (2, 0, 0)
                 R2 wall (0.3125, 1.0625, 0.5625) n -y: cell (2, 8, 4), face 3, cover cell (0, 1, 0)
      query  0 at R0                                                  d = 0, r = 0                               SUPPORTED
             1 (0.1875, 0.3125, 0.09375): cell x 1, off = V/2, so the neighbour is 2; d = 0.15625 = reach         SUPPORTED
             2 as 1 with y + 2^-16: d = sqrt(0.15625^2 + 2^-32) > reach; cover cell (0, 0, 0) is held             CHANGED
             3 (0.34375, 0.3125, -0.03125): cell z -1, off 0.09375 >= V/2, neighbour 0; r = -0.125 = the gate     SUPPORTED
             4 as 3 with z - 2^-16: |r| = 0.125 + 2^-16, d still inside the reach; cover neighbour z 0            CHANGED
             5 at R0, n = (0, 0.5, c+), c+ the smallest float32 >= cos 30: the dot product is c+                  SUPPORTED
             6 at R0, n = (0, 0.5, c-), c- the float32 below c+                                                   CHANGED
             7 (0.2421875, 0.3125, 0.09375): cell x 1; its own cell is empty, the neighbour towards it holds R0   SUPPORTED
             8 (0.5, 0.3125, 0.09375): d = 0.15625 as well, but cell x 4 with off 0 looks at 3, never at 2        CHANGED
             9 (0.3125, 1.09375, 0.5625) n -y: R2's cell, r = -0.03125                                            SUPPORTED
            10 as 9 with n +y: face 2, which the wall's cell does not hold; cover cell (0, 1, 0)                  CHANGED
            11 (5.3125, 5.3125, 0.0625): cover cells 4..5 or 5..6, none held                                      OUTSIDE
            12 (0.8125, 0.3125, 0.0625): no fine cell near, cover cell (0, 0, 0)                                  CHANGED
            13 (1.25, 0.3125, 0.0625): cover cell x 1, off 0.25, neighbour 0: (0, 0, 0) is held                   CHANGED
            14 (70000, 0.3125, 0.0625): fine cell 560000 is past 65535                                            OUTSIDE
            15 a NaN coordinate                                                                                   LOOSE
            16 a zero normal                                                                                      LOOSE
    With the identity in place of the pose record 0 lies elsewhere and is not SUPPORTED."""
    Rinv, t = HAND_POSE[:3, :3].T, HAND_POSE[:3, 3]

    def place(p, n=(0.0, 0.0, 1.0), **kw):
        pq, nq = Rinv @ (np.asarray(p, F64) - t), Rinv @ np.asarray(n, F64)
        assert np.array_equal(pq.astype(F32).astype(F64), pq) and np.array_equal(nq.astype(F32).astype(F64), nq)
        return row(*pq, n=nq, **kw)
    c_hi, c_lo = _cos_neighbours(30.0)
    r0 = (0.34375, 0.3125, 0.09375)
    ref = np.array([row(*r0), row(2.3125, 0.3125, 0.0625, sem=5), row(0.3125, 1.0625, 0.5625, n=(0.0, -1.0, 0.0), sem=7)])
    qry = [place(r0), place((0.1875, 0.3125, 0.09375)), place((0.1875, 0.3125 + U, 0.09375)), place((0.34375, 0.3125, -0.03125)),
           place((0.34375, 0.3125, -0.03125 - U)), place(r0, (0.0, 0.5, c_hi)), place(r0, (0.0, 0.5, c_lo)),
           place((0.2421875, 0.3125, 0.09375)), place((0.5, 0.3125, 0.09375)), place((0.3125, 1.09375, 0.5625), (0.0, -1.0, 0.0)),
           place((0.3125, 1.09375, 0.5625), (0.0, 1.0, 0.0)), place((5.3125, 5.3125, 0.0625)), place((0.8125, 0.3125, 0.0625)),
           place((1.25, 0.3125, 0.0625)), place((70000.0, 0.3125, 0.0625)), place(r0), place(r0)]
    qry = np.array(qry)
    qry[15, 1] = np.nan
    qry[16, 8:11] = 0.0
    want = np.array([S, S, CH, S, CH, S, CH, S, CH, S, CH, OUT, CH, CH, OUT, LO, LO], np.uint8)
    return qry, ref, HAND_POSE.astype(F32), want


def wall_pair():
    """a wall at yaw 44 degrees in the reference, the same wall seen at 46 degrees in the query: the normals are 2 degrees apart
    and on either side of the tie of the x and y faces"""
    def wall(yaw):
        n = (math.cos(math.radians(yaw)), math.sin(math.radians(yaw)), 0.0)
        return np.array([row(0.3125, 0.3125, 0.0625 + 0.125 * k, n=n) for k in range(5)])
    return wall(46.0), wall(44.0)


def street_case():
    """The street of tests/register_scenes.py without noise.  reference: 4 920 records of it and 80 in one cell of the ground;
    query, in a world of its own (`pose` brings it back): 2 790 records of another sampling with the box in the middle moved by
    1 m along the street, 80 in that one cell, 100 on the ground 6 .. 16 m beyond the street's end, 30 of loose_rows (ten with a NaN,
    ten with a zero normal, ten 20 km out).  Returns dict(query, ref, pose, untouched, box, stretch, dense, loose: index arrays)."""
    length, yaw, centre = 40.0, 20.0, (3.0, -2.0, 0.5)
    rng = np.random.default_rng(77)
    Wm = sc.rigid(rz_deg=yaw, t=centre)
    R, t = Wm[:3, :3], Wm[:3, 3]
    up = np.array([0.0, 0.0, 1.0])

    def dense(n):                                          # the ground's cell (3, -2, 0) of the 1 m grid
        return np.stack([rng.uniform(3.2, 3.8, n), rng.uniform(-1.8, -1.2, n), np.full(n, 0.5)], axis=1), np.tile(up, (n, 1))
    rp, rn = sc.street_points(4920, 3, length=length, yaw_deg=yaw, noise=0.0, centre=centre)
    dp, dn = dense(80)
    ref = sc.records(np.concatenate([rp[:2000], dp, rp[2000:]]), np.concatenate([rn[:2000], dn, rn[2000:]]), rng)

    qp, qn = sc.street_points(2790, 1003, length=length, yaw_deg=yaw, noise=0.0, centre=centre)
    qs = (qp - t) @ R                                     # in the street's own frame
    box = (np.abs(qs[:, 0] - 0.5) < 1e-6) & (qn @ (R @ np.array([-1.0, 0.0, 0.0])) > 0.99)
    qp[box] += R @ np.array([1.0, 0.0, 0.0])
    n_st = 100
    st = np.stack([rng.uniform(length / 2 + 6.0, length / 2 + 16.0, n_st), rng.uniform(-4.0, 4.0, n_st), np.zeros(n_st)], axis=1) @ R.T + t
    dq, dqn = dense(80)
    pos = np.concatenate([qp[:1500], dq, qp[1500:], st])
    nrm = np.concatenate([qn[:1500], dqn, qn[1500:], np.tile(up, (n_st, 1))])
    kind = np.concatenate([np.where(box[:1500], 1, 0), np.full(80, 3), np.where(box[1500:], 1, 0), np.full(n_st, 2)])
    truth = sc.rigid(rx_deg=0.4, ry_deg=-0.3, rz_deg=1.5, t=(0.35, -0.3, 0.1), about=(3.0, -2.0, 1.5))
    inv = np.linalg.inv(truth)
    rows = sc.records(pos @ inv[:3, :3].T + inv[:3, 3], nrm @ inv[:3, :3].T, rng)
    loose = sc.loose_rows(rng, 30)
    query = np.concatenate([rows[:700], loose[:15], rows[700:], loose[15:]])
    kind = np.concatenate([kind[:700], np.full(15, 4), kind[700:], np.full(15, 4)])
    assert len(query) == 3000 and len(ref) == 5000
    names = ("untouched", "box", "stretch", "dense", "loose")
    return dict(query=query, ref=ref, pose=truth.astype(F32), **{k: np.nonzero(kind == i)[0] for i, k in enumerate(names)})


@pytest.fixture(scope="module", autouse=True)
def entry_points():
    """every test of this file is about sm_compare_maps, the restatement's included: a library without it passes none of them"""
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name


@pytest.fixture(scope="module")
def street():
    case = street_case()
    case["want"] = {mask: cf.compare(case["query"], case["ref"], case["pose"], write_mask=mask, **STREET) for mask in (1, 2, 6, 15)}
    return case


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_defaults():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ENTRY_POINTS:
        assert name in capi.SYMBOLS and hasattr(L, name), name
    p = capi.default_compare_params()
    d = cf.DEFAULTS
    assert all(getattr(p, k) == d[k] for k in d if k != "origin") and list(p.origin) == list(d["origin"])
    assert (p.voxel_mm, p.cover_shift, p.reach_cells, p.plane_mm, p.angle_thresh) == (100, 3, 2.0, 50, 30.0)
    assert (p.match_class, p.write_mask, p.max_cells) == (0, 2, 1 << 24)
    assert capi.compare_params(voxel_mm=125, origin=(1, 2, 3)).origin[2] == 3.0
    with pytest.raises(KeyError):
        capi.compare_params(bad=1)
    assert [capi.COMPARE_LABEL[i] for i in range(4)] == list(cf.NAMES)
    assert L.sm_api_version() == 4


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "sm_c_api.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    assert "#define SM_API_VERSION 4 " in text


def test_arguments_without_a_device(tmp_path):
    """every rule that is checked before a context is looked at: SM_E_ARG, and nothing appears at out_path"""
    from surfelmapping_amd import capi
    L = capi.load()
    out = tmp_path / "out.bin"
    p, src, info = capi.default_compare_params(), capi.map_source([], include_model=False), capi.SmCompareInfo()
    st = capi.SmCompareStats()
    path = os.fsencode(str(out))
    assert L.sm_default_compare_params(None) == capi.SM_E_ARG
    assert L.sm_compare_maps(None, C.byref(src), C.byref(src), None, C.byref(p), None, path, C.byref(info)) == capi.SM_E_ARG
    assert b"sm_compare_maps" in L.sm_last_error()
    assert L.sm_compare_stats(None, C.byref(st)) == capi.SM_E_ARG and L.sm_compare_stats(None, None) == capi.SM_E_ARG
    assert b"sm_compare_stats" in L.sm_last_error()
    assert not out.exists() and os.listdir(tmp_path) == []


def test_ref_hand_derived_labels():
    qry, ref, pose, want = hand_scene()
    got = cf.compare(qry, ref, pose, **HAND)
    assert got["labels"].tolist() == want.tolist()
    assert got["counts"] == [6, 7, 2, 2] and got["cells_fine"] == 3 and got["cells_cover"] == 3
    assert np.array_equal(got["written"].view(np.uint32), qry[want == CH].view(np.uint32))
    # what the table holds: R0 alone under its key is its own representative
    t = cf.fine_table(ref, 8192, (0.0, 0.0, 0.0), 0)
    assert int(t["keys"][0]) == ((65538 << 34 | 65538 << 17 | 65536) << 11) | (4 << 8)
    assert t["pos"][0].tolist() == [0.34375, 0.3125, 0.09375] and t["nrm"][0].tolist() == [0.0, 0.0, 1.0]
    assert cf.cover_table(ref, 65536, (0.0, 0.0, 0.0)).tolist() == [((65536 << 34 | 65536 << 17 | 65536) << 11),
                                                                     ((65536 << 34 | 65537 << 17 | 65536) << 11),
                                                                     ((65538 << 34 | 65536 << 17 | 65536) << 11)]
    # the pose is what puts record 0 in place
    assert cf.compare(qry, ref, None, **HAND)["labels"][0] != S
    # the other masks write what their bits say, in set order
    for mask in (1, 6, 15):
        keep = ((mask >> want.astype(int)) & 1).astype(bool)
        assert np.array_equal(cf.compare(qry, ref, pose, write_mask=mask, **HAND)["written"].view(np.uint32), qry[keep].view(np.uint32))
    with pytest.raises(cf.Capacity):
        cf.compare(qry, ref, pose, max_cells=2, **HAND)


def test_ref_match_class_in_the_hand_scene():
    """R0 has class 3, R2 class 7: with match_class a query record of another class finds no key"""
    qry, ref, pose, want = hand_scene()
    qry = qry.copy()
    qry[9, 4:5].view(np.uint32)[0] = (7 << 24) | 0x102030          # the wall's record takes the wall's class
    want1 = want.copy()
    assert cf.compare(qry, ref, pose, match_class=1, **HAND)["labels"].tolist() == want1.tolist()
    qry[0, 4:5].view(np.uint32)[0] = (4 << 24) | 0x102030
    want1[0] = CH
    assert cf.compare(qry, ref, pose, match_class=1, **HAND)["labels"].tolist() == want1.tolist()
    assert cf.compare(qry, ref, pose, match_class=0, **HAND)["labels"].tolist() == want.tolist()


def test_ref_wall_at_45_degrees_needs_the_second_face():
    qry, ref = wall_pair()
    assert cf.compare(qry, ref, None, **HAND)["labels"].tolist() == [S] * 5
    assert cf.compare(qry, ref, None, primary_only=True, **HAND)["labels"].tolist() == [CH] * 5


def test_ref_street_is_what_the_scene_says(street):
    want = street["want"][2]
    lab = want["labels"]
    print({k: np.bincount(lab[street[k]], minlength=4).tolist() for k in ("untouched", "box", "stretch", "dense", "loose")},
          want["counts"], want["cells_fine"], want["cells_cover"])
    assert len(street["box"]) >= 50 and len(street["untouched"]) >= 2500
    assert (lab[street["untouched"]] == S).all() and (lab[street["dense"]] == S).all()
    assert (lab[street["stretch"]] == OUT).all() and (lab[street["box"]] == CH).all()
    assert all(c > 0 for c in want["counts"]) and want["counts"][LO] == 20
    assert len(want["written"]) == want["counts"][CH]
    assert len(street["want"][15]["written"]) == 3000 and len(street["want"][6]["written"]) == want["counts"][CH] + want["counts"][OUT]


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _ctx(rows=None, cap=80):
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(W, H, F, F, W / 2 - 0.5, H / 2 - 0.5, preprocess=0, stereo_border=0.0, max_sqrt_vertices=cap))
    if rows is not None and len(rows):
        m.upload_model(rows)
    return m


def _write(folder, name, rows, a=1, b=2):
    path = str(folder / name)
    cr.write_map(path, np.ascontiguousarray(rows, F32).reshape(-1, 12), a, b)
    return path


def _same(got_labels, info, out, want, what):
    """labels, counts, table sizes and the written file against the restatement's, bit for bit"""
    assert np.array_equal(got_labels, want["labels"]), (what, np.nonzero(got_labels != want["labels"])[0][:10])
    assert info["counts_by_code"] == want["counts"], what
    assert (info["cells_fine"], info["cells_cover"]) == (want["cells_fine"], want["cells_cover"]), what
    rows = ret.read_map(out)[0]
    assert info["written"] == len(rows) == len(want["written"]), what
    assert np.array_equal(rows.view(np.uint32), want["written"].view(np.uint32)), what


@pytest.mark.gpu
def test_gpu_hand_derived_scene(tmp_path):
    from surfelmapping_amd import capi
    qry, ref, pose, want = hand_scene()
    m = _ctx()
    qp, rp, out = [_write(tmp_path, "q.bin", qry, 3, 9)], [_write(tmp_path, "r.bin", ref)], str(tmp_path / "out.bin")
    lab, info = m.compare_maps(qp, rp, pose=pose, out_path=out, **HAND)
    st = m.compare_stats()
    assert lab.tolist() == want.tolist()
    assert info["counts"] == dict(SUPPORTED=6, CHANGED=7, OUTSIDE=2, LOOSE=2) and info["counts_by_code"] == [6, 7, 2, 2]
    assert (info["query_records"], info["reference_records"], info["cells_fine"], info["cells_cover"], info["written"]) == (17, 3, 3, 3, 7)
    rows, a, b = ret.read_map(out)
    assert np.array_equal(rows.view(np.uint32), qry[want == CH].view(np.uint32)) and (a, b) == (3, 9)
    assert st["chunks"] == 2 and st["launches"] == 1 + 1 + 3 and st["table_ms"] > 0.0 and st["classify_ms"] > 0.0
    assert sorted(os.listdir(tmp_path)) == ["out.bin", "q.bin", "r.bin"]
    # no labels asked for, no file asked for
    none, info2 = m.compare_maps(qp, rp, pose=pose, labels=False, **HAND)
    assert none is None and info2["counts_by_code"] == [6, 7, 2, 2] and info2["written"] == 0 and m.compare_stats()["launches"] == 3
    # the argument rules that need a context
    L, h = m._L, m._h
    src_q, src_r = capi.map_source(qp, include_model=False), capi.map_source(rp, include_model=False)
    ci, good = capi.SmCompareInfo(), capi.compare_params(**HAND)
    gone = str(tmp_path / "none.bin")

    def rc(q=src_q, r=src_r, pose16=None, p=good, path=gone):
        g = None if pose16 is None else np.ascontiguousarray(pose16, F32)
        return L.sm_compare_maps(h, C.byref(q), C.byref(r), None if g is None else g.ctypes.data, C.byref(p), None,
                                 None if path is None else os.fsencode(path), C.byref(ci))
    bad = [dict(voxel_mm=9), dict(voxel_mm=10001), dict(cover_shift=0), dict(cover_shift=7), dict(reach_cells=0.0), dict(reach_cells=float("inf")),
           dict(plane_mm=0), dict(plane_mm=10001), dict(angle_thresh=0.0), dict(angle_thresh=90.0), dict(match_class=2), dict(write_mask=0),
           dict(write_mask=16), dict(max_cells=0), dict(origin=(0.0, float("nan"), 0.0))]
    for kw in bad:
        assert rc(p=capi.compare_params(**kw)) == capi.SM_E_ARG, kw
    assert rc(p=capi.compare_params(write_mask=0), path=None) == capi.SM_OK          # (read only if out_path is given)
    nan_pose = np.eye(4, dtype=F32).ravel()
    nan_pose[3] = np.inf
    assert rc(pose16=nan_pose) == capi.SM_E_ARG
    assert rc(r=src_q) == capi.SM_E_ARG and b"both sets" in L.sm_last_error()
    assert rc(path=qp[0]) == capi.SM_E_ARG and rc(path=rp[0]) == capi.SM_E_ARG
    assert rc(q=capi.map_source([gone], include_model=False)) == capi.SM_E_ARG
    assert L.sm_compare_maps(h, C.byref(src_q), C.byref(src_r), None, C.byref(good), None, None, None) == capi.SM_E_ARG
    assert sorted(os.listdir(tmp_path)) == ["out.bin", "q.bin", "r.bin"]
    fresh = _ctx()
    with pytest.raises(capi.SurfelMapError) as e:
        fresh.compare_stats()
    assert e.value.rc == capi.SM_E_ARG
    fresh.close()
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mask", (1, 2, 6, 15))
def test_gpu_street_matches_the_restatement(street, tmp_path, mask):
    m = _ctx()
    out = str(tmp_path / "out.bin")
    lab, info = m.compare_maps([_write(tmp_path, "q.bin", street["query"])], [_write(tmp_path, "r.bin", street["ref"])], pose=street["pose"],
                               out_path=out, write_mask=mask, **STREET)
    m.close()
    print(info)
    _same(lab, info, out, street["want"][mask], f"write_mask {mask}")


@pytest.mark.gpu
def test_gpu_labels_do_not_depend_on_order_or_split(street, tmp_path, monkeypatch):
    """the reference shuffled and split over three files, one of them empty, plus the live model; the query split over two files
    plus the model: the same labels by global id and the same file, with the in-wave combination on and off"""
    ref, qry, pose = street["ref"], street["query"], street["pose"]
    live = ref[4500:]
    q_full = np.concatenate([qry, live])
    want = cf.compare(q_full, ref, pose, write_mask=6, **STREET)
    m = _ctx(live)
    out = str(tmp_path / "out.bin")
    kw = dict(pose=pose, out_path=out, write_mask=6, **STREET)
    lab, info = m.compare_maps([_write(tmp_path, "q.bin", q_full)], [_write(tmp_path, "r.bin", ref)], **kw)
    _same(lab, info, out, want, "one file each")
    one = open(out, "rb").read()
    perm = np.random.RandomState(5).permutation(4500)
    parts = np.split(ref[:4500][perm], [1700, 1700])
    rp = [_write(tmp_path, f"r{i}.bin", part) for i, part in enumerate(parts)]
    qp = [_write(tmp_path, "q0.bin", qry[:1100]), _write(tmp_path, "q1.bin", qry[1100:])]
    for v in ("0", "1"):
        monkeypatch.setenv("SM_SIMPLIFY_NO_COMBINE", v)
        lab, info = m.compare_maps(qp, rp, query_model=True, reference_model=True, **kw)
        _same(lab, info, out, want, "split, combine " + v)
        assert open(out, "rb").read() == one and (info["query_records"], info["reference_records"]) == (3500, 5000)
    m.close()


def _one_class(rows, sem):
    rows = rows.copy()
    rows[:, 4] = np.full(len(rows), (sem << 24) | 0x808080, np.uint32).view(F32)
    return rows


@pytest.mark.gpu
def test_gpu_match_class(street, tmp_path):
    """both sets of one class, but for the query's 80 records in the ground's one cell: with match_class they go from SUPPORTED
    to CHANGED and every other label stays"""
    ref, qry = _one_class(street["ref"], 3), _one_class(street["query"], 3)
    patch = street["dense"]
    qry[patch] = _one_class(qry[patch], 7)
    want = [cf.compare(qry, ref, street["pose"], match_class=mc, **STREET) for mc in (0, 1)]
    others = np.setdiff1d(np.arange(len(qry)), patch)
    assert (want[0]["labels"][patch] == S).all() and (want[1]["labels"][patch] == CH).all()
    assert np.array_equal(want[0]["labels"][others], want[1]["labels"][others])
    m = _ctx()
    qp, rp, out = [_write(tmp_path, "q.bin", qry)], [_write(tmp_path, "r.bin", ref)], str(tmp_path / "out.bin")
    for mc in (0, 1):
        lab, info = m.compare_maps(qp, rp, pose=street["pose"], out_path=out, match_class=mc, **STREET)
        _same(lab, info, out, want[mc], f"match_class {mc}")
    m.close()


@pytest.mark.gpu
def test_gpu_wall_at_45_degrees(tmp_path):
    qry, ref = wall_pair()
    m = _ctx()
    lab, info = m.compare_maps([_write(tmp_path, "q.bin", qry)], [_write(tmp_path, "r.bin", ref)], **HAND)
    m.close()
    assert lab.tolist() == [S] * 5 and info["counts_by_code"] == [5, 0, 0, 0]


@pytest.mark.gpu
def test_gpu_more_than_a_chunk(street, tmp_path):
    """2^20 + 450 query records -- the street's 3 000 over and over: a record's label depends on the record and the reference
    alone, so the restatement's labels repeat with them -- go through in two chunks, and the second chunk's ranks go on from the
    first's"""
    n = (1 << 20) + 450
    reps = -(-n // 3000)
    qry = np.tile(street["query"], (reps, 1))[:n]
    base = street["want"][2]
    labels = np.tile(base["labels"], reps)[:n]
    want = dict(labels=labels, counts=np.bincount(labels, minlength=4).tolist(), cells_fine=base["cells_fine"], cells_cover=base["cells_cover"],
                written=qry[labels == CH])
    assert (labels[:1 << 20] == CH).any() and (labels[1 << 20:] == CH).any()
    m = _ctx()
    out = str(tmp_path / "out.bin")
    lab, info = m.compare_maps([_write(tmp_path, "q.bin", qry)], [_write(tmp_path, "r.bin", street["ref"])], pose=street["pose"], out_path=out, **STREET)
    st = m.compare_stats()
    m.close()
    _same(lab, info, out, want, "two chunks")
    assert st["chunks"] == 3 and st["launches"] == 1 + 1 + 2 * 3


def _wrap_case(street):
    """The first 1 000 reference records of the street -- 7 to the square metre, so with cells of 1/8 m nearly every record has a
    fine cell and, at cover_shift 1, a cover cell of its own: about as many cover keys as fine keys, both tables half full.  The
    query: 1 000 records of the street's query and the reference's own records moved back by the inverse pose, which look for
    the cell they came from; the reach of half a cell leaves most of them no other."""
    ref, pose = street["ref"][:WRAP_REF_ROWS], street["pose"]
    inv = np.linalg.inv(pose.astype(F64))
    back = ref.copy()
    back[:, 0:3] = (ref[:, 0:3].astype(F64) @ inv[:3, :3].T + inv[:3, 3]).astype(F32)
    back[:, 8:11] = (ref[:, 8:11].astype(F64) @ inv[:3, :3].T).astype(F32)
    return np.concatenate([street["query"][:1000], back]), ref, pose


def wrap_tables(ref, params):
    """what the smallest tables of `ref` hold at params' grid: dict(fine, cover: the keys; size: the slots of either; carried:
    how many fine and cover keys go past the last slot; at_the_end: table_ref.end_run of the fine keys; key_of: per record of
    ref its fine key, valid where ok)"""
    origin = params["origin"]
    V0 = cf.rr.cell_edge(params["voxel_mm"])
    ok = cf.rr.fields_ok(ref)
    in_grid, cell, _ = cf.rr.grid(ref[:, 0:3].astype(F64), V0, origin)
    ok &= in_grid
    key_of = cf.rr.pack(np.where(ok[:, None], cell, 0), cf.rr.face_of(ref[:, 8:11]))
    fine = sorted(set(key_of[ok].tolist()))
    cover = cf.cover_table(ref, cf.rr.cell_edge(params["voxel_mm"] << params["cover_shift"]), origin).tolist()
    size = 1024
    while size < 2 * len(fine):
        size <<= 1
    return dict(fine=fine, cover=cover, size=size, carried=(tb.wraps(fine, size - 1), tb.wraps(cover, size - 1)),
                at_the_end=tb.end_run(fine, size - 1), ok=ok, key_of=key_of)


def not_the_only_support(qry, ref, pose, params, t, labels):
    """the keys of t["at_the_end"] without which no SUPPORTED label of `labels` changes"""
    return [k for k in t["at_the_end"]
            if not ((labels == S) & (cf.compare(qry, ref[~(t["ok"] & (t["key_of"] == np.uint64(k)))], pose, **params)["labels"] != S)).any()]


@pytest.mark.gpu
def test_gpu_smallest_tables_with_wrap_around(street, tmp_path):
    """max_cells = the fine keys leaves the smallest tables the rule allows (the power of two >= 2 * max_cells); the origin is one
    at which a run of occupied slots crosses the end of the fine table and one that of the cover table, so that probes walk
    from the last slot to slot 0.  tools/compare_wrap_origin.py found it, with the functions above, as the first of the grid
    (0.37 i, 0.21 j, 0), i, j < 40, that meets what is asserted here, and found none in that grid at cover_shift 3.
    Which keys of such a run the device carries past the end depends on the order it inserts them in, but they are keys whose
    home slot lies in the run (table_ref.end_run): each of those is the only support of some query record, so whichever is
    carried, a label depends on the lookup that follows it"""
    qry, ref, pose = _wrap_case(street)
    t = wrap_tables(ref, WRAP)
    fine, size = t["fine"], t["size"]
    assert fine == cf.fine_table(ref, cf.rr.cell_edge(WRAP["voxel_mm"]), WRAP["origin"], 0)["keys"].tolist()
    assert size == 2048 and t["carried"][0] >= 1 and t["carried"][1] >= 1
    want = cf.compare(qry, ref, pose, write_mask=3, **WRAP)
    assert not_the_only_support(qry, ref, pose, WRAP, t, want["labels"]) == []
    print(f"origin {WRAP['origin']}: {len(fine)} fine and {len(t['cover'])} cover keys in {size} slots, {t['carried'][0]} and "
          f"{t['carried'][1]} carried past the end, {len(t['at_the_end'])} fine keys in the run at the end; labels {want['counts']}")
    assert all(c > 0 for c in want["counts"])
    m = _ctx()
    out = str(tmp_path / "out.bin")
    lab, info = m.compare_maps([_write(tmp_path, "q.bin", qry)], [_write(tmp_path, "r.bin", ref)], pose=pose, out_path=out, write_mask=3,
                               max_cells=len(fine), **WRAP)
    m.close()
    _same(lab, info, out, want, f"tables of {size} slots")


@pytest.mark.gpu
def test_gpu_empty_sets_capacity_and_contexts(street, tmp_path):
    from surfelmapping_amd import capi
    m = _ctx()
    qp, rp = [_write(tmp_path, "q.bin", street["query"])], [_write(tmp_path, "r.bin", street["ref"])]
    empty, out = [_write(tmp_path, "e.bin", np.zeros((0, 12), F32), 4, 6)], str(tmp_path / "out.bin")
    base = street["want"][2]
    # an empty reference: nothing is near anything
    lab, info = m.compare_maps(qp, empty, pose=street["pose"], out_path=out, write_mask=4, **STREET)
    want = np.where(base["labels"] == LO, LO, OUT)
    assert np.array_equal(lab, want) and info["counts_by_code"] == [0, 0, 2980, 20] and (info["cells_fine"], info["cells_cover"]) == (0, 0)
    assert np.array_equal(ret.read_map(out)[0].view(np.uint32), street["query"][want == OUT].view(np.uint32))
    # an empty query: a valid empty file with the query files' frame range
    lab, info = m.compare_maps(empty, rp, out_path=out, **STREET)
    rows, a, b = ret.read_map(out)
    assert len(lab) == 0 and info["counts_by_code"] == [0] * 4 and info["written"] == 0 and len(rows) == 0 and (a, b) == (4, 6)
    assert info["cells_fine"] == base["cells_fine"] and info["reference_records"] == 5000
    # no record with a label of the mask: a valid empty file as well
    far = [_write(tmp_path, "far.bin", street["query"][street["stretch"]], 8, 8)]
    lab, info = m.compare_maps(far, rp, pose=street["pose"], out_path=out, **STREET)
    rows, a, b = ret.read_map(out)
    assert (lab == OUT).all() and info["counts_by_code"] == [0, 0, 100, 0] and info["written"] == 0 and len(rows) == 0 and (a, b) == (8, 8)
    os.remove(out)
    # one key fewer than the fine table holds: no label, no file
    keep = np.full(3000, 9, np.uint8)
    p, ci = capi.compare_params(max_cells=base["cells_fine"] - 1, **STREET), capi.SmCompareInfo()
    src_q, src_r = capi.map_source(qp, include_model=False), capi.map_source(rp, include_model=False)
    with pytest.raises(capi.SurfelMapError) as e:
        m._chk(m._L.sm_compare_maps(m._h, C.byref(src_q), C.byref(src_r), None, C.byref(p), keep.ctypes.data, os.fsencode(out), C.byref(ci)),
               "sm_compare_maps")
    assert e.value.rc == capi.SM_E_CAPACITY and "max_cells" in str(e.value)
    assert (keep == 9).all() and not os.path.exists(out) and not os.path.exists(out + ".compare.tmp")
    assert base["cells_cover"] < base["cells_fine"]
    lab, info = m.compare_maps(qp, rp, pose=street["pose"], max_cells=base["cells_fine"], **STREET)
    assert np.array_equal(lab, base["labels"])
    m.close()
    for configure in ("shard_stream_configure", "rig_configure"):
        part = _ctx()
        getattr(part, configure)(0, 1)
        with pytest.raises(capi.SurfelMapError) as e:
            part.compare_maps(qp, rp, out_path=out, **STREET)
        assert e.value.rc == capi.SM_E_UNSUPPORTED and not os.path.exists(out)
        part.close()


@pytest.mark.gpu
def test_gpu_nothing_else_moves(street, tmp_path):
    """the files' bytes, the model's rows, counts() -- the tick is one of them -- and the stored poses with their codes and times"""
    m = _ctx(street["ref"][:3000])
    m.set_tick(7)
    m.set_ferns()
    words = m.fern_keyframes()["codes"].shape[1]
    assert m.fern_add(np.full(words, 0x01234567, np.uint32), street["pose"], 3) == 0
    qp, rp = [_write(tmp_path, "q.bin", street["query"])], [_write(tmp_path, "r.bin", street["ref"][3000:])]
    out = str(tmp_path / "out.bin")

    def state():
        return [open(p, "rb").read() for p in qp + rp], m.download_model().copy(), m.counts(), m.fern_keyframes()
    before = state()
    assert before[2]["tick"] == 7 and len(before[3]["times"]) == 1
    lab, info = m.compare_maps(qp, rp, pose=street["pose"], reference_model=True, out_path=out, **STREET)
    assert np.array_equal(lab, street["want"][2]["labels"])
    after = state()
    m.close()
    assert before[0] == after[0] and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32)) and before[2] == after[2]
    for k in ("codes", "poses", "times"):
        assert np.array_equal(before[3][k].view(np.uint32), after[3][k].view(np.uint32)), k
    assert sorted(os.listdir(tmp_path)) == ["out.bin", "q.bin", "r.bin"]
