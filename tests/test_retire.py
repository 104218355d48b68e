"""Retirement (sm_retire / sm_retire_device / sm_set_auto_retire, SurfelMap.retire / set_auto_retire; DESIGN.md "4e.
Retirement").  The definition is the numpy mask of tests/retire_ref.py; the CPU oracle has the equivalent without touching it:
download_model() -> mask -> upload_model(kept), which changes neither its tick nor its images."""
import ctypes as C
import os

import numpy as np
import pytest

import retire_ref as rr
from backends import assert_models_equal

CAM, OVER = rr.CAM, rr.OVER
PARAMS = dict(min_age=rr.MIN_AGE, min_distance=rr.MIN_DISTANCE)
IDENT = np.eye(4, dtype=np.float32).T.reshape(16).copy()


@pytest.fixture(scope="module")
def seq():
    return rr.sequence()


@pytest.fixture(scope="module")
def oracle_rows(seq):
    """both rows of the scenario on the oracle alone: without and with lockstep retirement"""
    return {pp: dict(plain=rr.oracle_run(seq, pp, False), retired=rr.oracle_run(seq, pp, True)) for pp in (1, 0)}


def _gpu(pp=0, cap=None, **over):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=pp, max_sqrt_vertices=cap or rr.CAPACITY[pp], **over))


def _cpu(pp=0, cap=None):
    import oracle_lib as ol
    return ol.Oracle(ol.make_config(**CAM, **OVER, preprocess=pp, max_sqrt_vertices=cap or rr.CAPACITY[pp]))


def _same_counts(g, o, what=""):
    cg, co = g.counts(), o.counts()
    assert all(cg[k] == co[k] for k in co), (what, cg, co)


def _rows(n, t, pos=(0.0, 0.0, 0.0)):
    """n hand-made surfels: position `pos`, last update `t` (scalars or arrays), row number in the creation time"""
    m = np.zeros((n, 12), np.float32)
    m[:, 0:3] = np.asarray(pos, np.float32)
    m[:, 3] = 5.0
    m[:, 4] = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) | np.uint32(0x03000000)).view(np.float32)
    m[:, 6] = np.arange(n) % 4096
    m[:, 7] = t
    m[:, 10] = -1.0
    m[:, 11] = 0.05
    return m


# ---------------------------------------------------------------------------------------------------------------------
# 1. the definition, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pp", [0, 1])
@pytest.mark.parametrize("cp", [1, 24])
def test_definition_bit_for_bit(seq, cp, pp):
    g, o = _gpu(pp, compact_period=cp), _cpu(pp)
    for fr in seq[:30]:
        g.process_frame(*fr)
        o.process_frame(*fr)
    log = g.read_frame_log(1)
    pending = int(log["n_slots"][-1]) - int(log["n_before"][-1])
    print(f"compact_period {cp} preprocess {pp}: {pending} dead slots pending at the retirement")
    if cp == 24:
        assert pending > 0            # the retirement meets dead slots: it cannot pass on a model that was compact anyway
    tick = g.counts()["tick"]
    assert tick == o.counts()["tick"] == 30
    m = o.download_model()
    r = rr.mask(m, tick, seq[29][3], **PARAMS)
    assert 1000 < r.sum() < len(m) - 1000, (int(r.sum()), len(m))
    got = g.retire(pose=seq[29][3], **PARAMS)
    assert_models_equal(got, m[r], "retired records")
    assert_models_equal(g.download_model(), m[~r], "kept model")
    o.upload_model(m[~r])
    _same_counts(g, o, "after the retirement")
    assert g.counts()["count"] == g.counts()["offset"] == int((~r).sum()) and g.counts()["tick"] == tick
    for k, fr in enumerate(seq[30:50]):
        g.process_frame(*fr)
        o.process_frame(*fr)
        _same_counts(g, o, f"frame {30 + k}")
    assert_models_equal(g.download_model(), o.download_model(), "20 frames later")


# ---------------------------------------------------------------------------------------------------------------------
# 2. a dry run and a buffer that is too small change nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dry_run_and_small_buffer_leave_no_trace(seq):
    from surfelmapping_amd import capi
    a, b, o = _gpu(0, compact_period=24), _gpu(0, compact_period=24), _cpu(0)
    for fr in seq[:30]:
        a.process_frame(*fr)
        b.process_frame(*fr)
        o.process_frame(*fr)
    want = int(rr.mask(o.download_model(), 30, seq[29][3], **PARAMS).sum())
    assert a.retire(pose=seq[29][3], dry_run=True, **PARAMS) == want > 0
    p = capi.retire_params(a.cfg, **PARAMS)
    n = C.c_uint32()
    buf = np.full((want, 12), 7.0, np.float32)
    rc = a._L.sm_retire(a._h, seq[29][3].ctypes.data_as(C.c_void_p), C.byref(p), buf.ctypes.data_as(C.c_void_p), want - 1, C.byref(n))
    assert rc == capi.SM_E_CAPACITY and n.value == want and (buf == 7.0).all()
    assert a.counts() == b.counts()
    assert np.array_equal(a.read_frame_log(), b.read_frame_log())
    for fr in seq[30:35]:
        a.process_frame(*fr)
        b.process_frame(*fr)
        o.process_frame(*fr)
        assert a.counts() == b.counts()
    assert np.array_equal(a.read_frame_log(), b.read_frame_log())
    ma = a.download_model()
    assert_models_equal(ma, b.download_model(), "after a dry run")
    assert_models_equal(ma, o.download_model(), "against the oracle")


# ---------------------------------------------------------------------------------------------------------------------
# 3. edges, hand-made
# ---------------------------------------------------------------------------------------------------------------------
def _retire_uploaded(m, tick, pose=IDENT, **params):
    """upload m, set the tick, retire: (records, model afterwards, counts)"""
    g = _gpu(0)
    g.upload_model(m)
    g.set_tick(tick)
    got = g.retire(pose=pose, **params)
    return got, g.download_model(), g.counts()


@pytest.mark.gpu
def test_edges_age_and_distance():
    # age: tick - t == min_age stays, min_age + 1 goes (the distance gate off)
    m = _rows(4, [100 - 8, 100 - 9, 100.0, 100 - 300])
    got, kept, c = _retire_uploaded(m, 100, min_age=8, min_distance=0.0)
    assert_models_equal(got, m[[1, 3]])
    assert_models_equal(kept, m[[0, 2]])
    assert c["count"] == c["offset"] == 2 and c["tick"] == 100
    # distance: d2 == min_distance^2 stays, one ulp above goes; the centre is the pose's translation
    pose = IDENT.copy()
    pose[12:15] = (0.5, -2.0, 7.0)
    up = np.nextafter(np.float32(3.0), np.float32(4.0))
    m = _rows(5, 0.0)
    m[0, 0:3] = (3.5, 2.0, 7.0)                    # (3, 4, 0) from the centre: d2 = 25 exactly
    m[1, 0:3] = (np.float32(0.5) + up, 2.0, 7.0)   # one ulp of 25 above
    m[2, 0:3] = (0.5, -2.0, 7.0)                   # at the centre
    m[3, 0:3] = (0.5, -2.0, 107.0)                 # far
    m[4, 0:3] = (0.5, -2.0, 107.0)
    m[4, 7] = 99.0                                 # as far, but young
    d = m[:, 0:3] - pose[12:15]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2[0] == np.float32(25.0) and d2[1] == np.nextafter(np.float32(25.0), np.float32(26.0))
    want = rr.mask(m, 100, pose, 8, 5.0)
    assert want.tolist() == [False, True, False, True, False]
    got, kept, _ = _retire_uploaded(m, 100, pose=pose, min_age=8, min_distance=5.0)
    assert_models_equal(got, m[want])
    assert_models_equal(kept, m[~want])
    # the same rows, the age gate alone: everything old goes, wherever it is
    got, kept, _ = _retire_uploaded(m, 100, pose=pose, min_age=8, min_distance=0.0)
    assert_models_equal(got, m[:4])
    assert_models_equal(kept, m[4:])


@pytest.mark.gpu
def test_edges_nan_empty_and_null_pose(seq):
    # a NaN position fails the distance test, a NaN time the age test: both stay
    m = _rows(4, 0.0, pos=(0.0, 0.0, 50.0))
    m[1, 1] = np.nan
    m[2, 7] = np.nan
    want = rr.mask(m, 100, IDENT, 8, 5.0)
    assert want.tolist() == [True, False, False, True]
    got, kept, _ = _retire_uploaded(m, 100, min_age=8, min_distance=5.0)
    assert_models_equal(got, m[want])
    assert_models_equal(kept, m[~want])
    # an empty model
    got, kept, c = _retire_uploaded(np.zeros((0, 12), np.float32), 100, min_age=0, min_distance=0.0)
    assert got.shape == (0, 12) and kept.shape == (0, 12) and c["count"] == 0
    # no pose given: the pose of the last processed frame
    g, o = _gpu(0), _cpu(0)
    for fr in seq[:14]:
        g.process_frame(*fr)
        o.process_frame(*fr)
    mo = o.download_model()
    want = rr.mask(mo, 14, seq[13][3], 3, 12.0)
    assert want.sum() > 100 and (want != rr.mask(mo, 14, seq[0][3], 3, 12.0)).sum() > 100      # the pose matters here
    assert g.retire(dry_run=True, min_age=3, min_distance=12.0) == want.sum()
    assert_models_equal(g.retire(min_age=3, min_distance=12.0), mo[want])
    assert_models_equal(g.download_model(), mo[~want])


@pytest.mark.gpu
def test_edges_everything_retires_then_frames_go_on(seq):
    g, o = _gpu(0), _cpu(0)
    for fr in seq[:5]:
        g.process_frame(*fr)
        o.process_frame(*fr)
    mo = o.download_model()
    assert len(mo) > 1000
    got = g.retire(min_age=0, min_distance=0.0)            # every surfel is at least one tick old
    assert_models_equal(got, mo)
    assert g.counts()["count"] == 0 and g.download_model().shape == (0, 12)
    o.upload_model(mo[:0])
    _same_counts(g, o)
    for k, fr in enumerate(seq[5:9]):
        g.process_frame(*fr)
        o.process_frame(*fr)
        _same_counts(g, o, f"frame {5 + k}")
    assert g.counts()["count"] > 1000
    assert_models_equal(g.download_model(), o.download_model())


def _pattern(n, per_tile):
    """bool[n]: per 1024-slot tile either a number of retired surfels (spread evenly) or a list of 16 per-word numbers"""
    r = np.zeros(n, bool)
    for t, spec in enumerate(per_tile):
        words = spec if isinstance(spec, (list, tuple)) else None
        if words is None:
            idx = (np.arange(spec) * 1024) // max(spec, 1)
            idx = t * 1024 + idx
            r[idx[idx < n]] = True
        else:
            for w, c in enumerate(words):
                lanes = (np.arange(c) * 64) // max(c, 1) if c not in (63,) else np.delete(np.arange(64), 5)
                idx = t * 1024 + w * 64 + lanes
                r[idx[idx < n]] = True
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("n,per_tile", [
    (3000, [1024, [0, 1, 63, 64] + [0] * 12, [64, 0, 63, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 64]]),
    (7000, [1024, 0, 1, 63, 64, [1] * 16, [63, 64, 0, 1] * 4]),
    (2048 + 5, [0, 1024, [5]]),
])
def test_edges_tiles_waves_and_workgroups(n, per_tile):
    """tiles, waves and workgroups that hold 0, 1, 63, 64 and 1024 retired surfels: all found, order kept"""
    r = _pattern(n, per_tile)
    m = _rows(n, np.where(r, 10.0, 95.0))
    m[:, 0] = np.arange(n) * 0.01
    assert (rr.mask(m, 100, IDENT, 8, 0.0) == r).all() and 0 < r.sum() < n
    counts = [int(r[t * 1024:(t + 1) * 1024].sum()) for t in range((n + 1023) // 1024)]
    print("retired per tile:", counts)
    got, kept, c = _retire_uploaded(m, 100, min_age=8, min_distance=0.0)
    assert_models_equal(got, m[r])
    assert_models_equal(kept, m[~r])
    assert c["count"] == int((~r).sum())


# ---------------------------------------------------------------------------------------------------------------------
# 4. errors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors(seq, tmp_path):
    from surfelmapping_amd import capi
    L = capi.load()
    g = _gpu(0)
    for fr in seq[:3]:
        g.process_frame(*fr)
    before = g.counts()
    n = C.c_uint32()
    buf = np.zeros((before["count"], 12), np.float32)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    def call(fn, h, pose, p, dst=buf, out=n):
        return getattr(L, fn)(h, None if pose is None else ptr(pose), None if p is None else C.byref(p),
                              None if dst is None else ptr(dst), len(buf), None if out is None else C.byref(out))

    ok = capi.retire_params(g.cfg)
    assert (ok.min_age, ok.min_distance) == (g.cfg.time_delta, np.float32(1.5) * np.float32(g.cfg.far_clip))
    assert L.sm_default_retire_params(None, C.byref(ok)) == capi.SM_E_ARG
    bad_pose = IDENT.copy()
    bad_pose[13] = np.inf
    for fn in ("sm_retire", "sm_retire_device"):
        dst = None if fn == "sm_retire_device" else buf          # (argument checks come before anything touches the destination)
        assert call(fn, None, None, ok, dst) == capi.SM_E_ARG
        assert call(fn, g._h, None, ok, dst, out=None) == capi.SM_E_ARG
        assert call(fn, g._h, None, capi.retire_params(g.cfg, min_age=-1), dst) == capi.SM_E_ARG
        assert call(fn, g._h, None, capi.retire_params(g.cfg, min_distance=float("nan")), dst) == capi.SM_E_ARG
        assert call(fn, g._h, None, capi.retire_params(g.cfg, min_distance=float("inf")), dst) == capi.SM_E_ARG
        assert call(fn, g._h, bad_pose, ok, dst) == capi.SM_E_ARG
    assert L.sm_set_auto_retire(None, None, 10, b"x") == capi.SM_E_ARG
    assert L.sm_set_auto_retire(g._h, C.byref(capi.retire_params(g.cfg, min_age=-1)), 10, b"x") == capi.SM_E_ARG
    assert L.sm_auto_retire_stats(None, None, None) == capi.SM_E_ARG
    # between the conflict test and the cull
    g.stage_conflict(seq[2][3], 1.0, 30.0)
    assert call("sm_retire", g._h, None, ok) == capi.SM_E_ARG
    assert call("sm_retire_device", g._h, None, ok, None) == capi.SM_E_ARG
    g.stage_cull()
    # a sharded context and a rig context hold only their own surfels
    for configure in ("shard_stream_configure", "rig_configure"):
        s = _gpu(0)
        getattr(s, configure)(0, 1)
        assert call("sm_retire", s._h, None, ok) == capi.SM_E_UNSUPPORTED
        assert call("sm_retire_device", s._h, None, ok, None) == capi.SM_E_UNSUPPORTED
        assert L.sm_set_auto_retire(s._h, None, 10, os.fsencode(str(tmp_path / "x"))) == capi.SM_E_UNSUPPORTED
    assert g.auto_retire_stats() == (0, 0) and not list(tmp_path.iterdir())


@pytest.mark.gpu
def test_retire_device_writes_the_same_records(seq):
    """sm_retire_device into a buffer of the context's GPU: the records and the model of sm_retire"""
    from surfelmapping_amd import capi
    a, b = _gpu(0, compact_period=24), _gpu(0, compact_period=24)
    for fr in seq[:30]:
        a.process_frame(*fr)
        b.process_frame(*fr)
    want = a.retire(pose=seq[29][3], **PARAMS)
    cap = b.counts()["count"]
    d = b.device_alloc(cap * 48)
    p, n = capi.retire_params(b.cfg, **PARAMS), C.c_uint32()
    pose = seq[29][3]
    assert b._L.sm_retire_device(b._h, pose.ctypes.data_as(C.c_void_p), C.byref(p), d, cap, C.byref(n)) == 0
    assert n.value == len(want) > 0
    assert_models_equal(b.device_download(d, n.value * 48, np.float32).reshape(-1, 12), want)
    assert a.counts() == b.counts()
    assert_models_equal(a.download_model(), b.download_model())


# ---------------------------------------------------------------------------------------------------------------------
# 5. the long run
# ---------------------------------------------------------------------------------------------------------------------
def _run_policy(seq, pp, prefix, how):
    g = _gpu(pp)
    g.set_auto_retire(rr.EVERY, prefix, **PARAMS)
    if how == "device":
        P = g.P
        d_rgb, d_dep, d_sem = g.device_alloc(P * 3), g.device_alloc(P * 2), g.device_alloc(P)
    rcs = []
    for rgb, dep, sem, pose in seq:
        if how == "sync":
            rcs.append(g.process_frame(rgb, dep, sem, pose, allow=(0, -1, -2)))
        elif how == "async":
            rcs.append(g.process_frame_async(np.ascontiguousarray(rgb, np.uint8), np.ascontiguousarray(dep, np.uint16),
                                             np.ascontiguousarray(sem, np.uint8), pose))
        else:
            g.device_upload(d_rgb, np.ascontiguousarray(rgb, np.uint8))
            g.device_upload(d_dep, np.ascontiguousarray(dep, np.uint16))
            g.device_upload(d_sem, np.ascontiguousarray(sem, np.uint8))
            rcs.append(g.process_frame_device(d_rgb, d_dep, d_sem, pose))
    rcs.append(g.sync(allow=(0, -1, -2)))
    return g, rcs


@pytest.mark.gpu
@pytest.mark.parametrize("pp", [1, 0])
def test_long_run(seq, oracle_rows, pp, tmp_path):
    from surfelmapping_amd import capi
    row = oracle_rows[pp]
    # without the policy the product overflows on the frame the oracle does
    g = _gpu(pp)
    fail = next((k for k, fr in enumerate(seq) if g.process_frame(*fr, allow=(0, capi.SM_E_CAPACITY)) != 0), None)
    print(f"preprocess {pp}: first SM_E_CAPACITY at frame {fail} (oracle {row['plain']['first_fail']})")
    assert fail is not None and fail == row["plain"]["first_fail"]
    g.close()
    # with it every frame is fused, and the files are the oracle-lockstep retired sets
    want = row["retired"]
    g, rcs = _run_policy(seq, pp, str(tmp_path / "sync"), "sync")
    assert rcs == [0] * (len(seq) + 1)
    files = sorted(p for p in os.listdir(tmp_path) if p.startswith("sync_"))
    assert files == [f"sync_{i:06d}.bin" for i in range(len(want["files"]))] and len(files) > 10
    other = _gpu(pp)
    for name, (rec, a, b) in zip(files, want["files"]):
        got, ga, gb = rr.read_map(tmp_path / name)
        assert (ga, gb) == (a, b), name
        assert_models_equal(got, rec, name)
        assert other.load_map(str(tmp_path / name)) == (a, b)
        assert_models_equal(other.download_model(), rec, name + " loaded")
    assert_models_equal(g.download_model(), want["model"], "final model")
    _same_counts(g, _Counts(want["counts"]), "final counts")
    total = sum(len(f[0]) for f in want["files"])
    assert g.auto_retire_stats() == (len(files), total)
    print(f"preprocess {pp}: {len(files)} files, {total} surfels retired, {g.counts()['count']} left")
    # the asynchronous entry points (held-back association, two-launch frame) write the same bytes
    for how in ("device", "async"):
        h, rcs = _run_policy(seq, pp, str(tmp_path / how), how)
        assert rcs == [0] * (len(seq) + 1), how
        for name in files:
            twin = name.replace("sync", how)
            assert (tmp_path / twin).read_bytes() == (tmp_path / name).read_bytes(), twin
        assert len([p for p in os.listdir(tmp_path) if p.startswith(how + "_")]) == len(files)
        assert_models_equal(h.download_model(), want["model"], how)
        assert h.auto_retire_stats() == (len(files), total)
        h.close()


class _Counts:
    def __init__(self, c):
        self._c = c

    def counts(self):
        return self._c


@pytest.mark.gpu
def test_long_run_file_cannot_be_written(seq, oracle_rows, tmp_path):
    from surfelmapping_amd import capi
    g = _gpu(0)
    g.set_auto_retire(rr.EVERY, str(tmp_path / "no_such_directory" / "map"), **PARAMS)
    rcs = [g.process_frame(*fr, allow=(0, capi.SM_E_ARG)) for fr in seq[:rr.EVERY]]
    assert rcs == [0] * (rr.EVERY - 1) + [capi.SM_E_ARG]
    assert "no_such_directory" in g._L.sm_last_error().decode()
    assert g.counts()["tick"] == rr.EVERY and g.auto_retire_stats() == (0, 0)
    assert_models_equal(g.download_model(), oracle_rows[0]["retired"]["models"][rr.EVERY], "the model as the frame left it")
    assert not list(tmp_path.iterdir())
    # switched off again: frames go on
    g.set_auto_retire(0, None)
    for fr in seq[rr.EVERY:2 * rr.EVERY + 1]:
        g.process_frame(*fr)
    assert g.counts()["tick"] == 2 * rr.EVERY + 1


# ---------------------------------------------------------------------------------------------------------------------
# 6. other readers after a retirement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_render_and_track_after_retirement(seq):
    import model_view_ref as ref
    a, b = _gpu(0, compact_period=24), _gpu(0, compact_period=24)
    for fr in seq[:30]:
        a.process_frame(*fr)
        b.process_frame(*fr)
    a.retire(pose=seq[29][3], **PARAMS)
    m = b.download_model()
    r = rr.mask(m, 30, seq[29][3], **PARAMS)
    assert 1000 < r.sum() < len(m) - 1000
    b.upload_model(m[~r])
    w, h = 160, 96
    P = ref.projection(w, h, 420.0 * w / 640, 420.0 * h / 480, 320.0 * w / 640, 240.0 * h / 480, 0.1, 1000.0)
    z = float(seq[29][3][14])
    for look in (ref.look_at(0, -6, z - 10, 0, 0, z + 20, 0, -1, 0), ref.look_at(-6, -2, z - 20, 3, 1, z, 0, -1, 0)):
        mvp, inv = ref.view_mats(P, look)
        ra = a.render_model(mvp, inv, w, h, color_type=2, depth=True, ids=True)
        rb = b.render_model(mvp, inv, w, h, color_type=2, depth=True, ids=True)
        assert (ra[2] >= 0).mean() > 0.05
        for x, y, name in zip(ra, rb, ("rgba", "depth", "ids")):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    guess = seq[30][3].reshape(4, 4).T.copy()
    guess[:3, 3] += (0.05, -0.02, 0.08)
    pa, ia = a.track(seq[30][1], guess=guess)
    pb, ib = b.track(seq[30][1], guess=guess)
    assert ia["iterations"] >= 1 and ia["inliers"] > 1000, ia
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    assert {k: v for k, v in ia.items() if k != "guess"} == {k: v for k, v in ib.items() if k != "guess"}
    assert np.array_equal(ia["guess"], ib["guess"])


# ---------------------------------------------------------------------------------------------------------------------
# 7. without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_binding_resolves_the_new_symbols():
    from surfelmapping_amd import capi
    L = capi.load()
    for name in ("sm_default_retire_params", "sm_retire", "sm_retire_device", "sm_set_auto_retire", "sm_auto_retire_stats"):
        assert name in capi.SYMBOLS and getattr(L, name)
    assert C.sizeof(capi.SmRetireParams) == 8
    cfg = capi.make_config(**CAM, **OVER)
    p = capi.retire_params(cfg)
    assert p.min_age == cfg.time_delta == 8 and p.min_distance == np.float32(1.5) * np.float32(cfg.far_clip)
    assert capi.retire_params(cfg, min_distance=2.5).min_distance == 2.5
    with pytest.raises(KeyError):
        capi.retire_params(cfg, max_age=1)


def test_mask_on_hand_made_rows():
    m = _rows(6, [92.0, 91.0, 91.0, 91.0, np.nan, 0.0])
    m[2, 0:3] = (3.0, 4.0, 0.0)
    m[3, 0:3] = (np.nextafter(np.float32(3.0), np.float32(4.0)), 4.0, 0.0)
    m[4, 0:3] = (100.0, 0.0, 0.0)
    m[5, 0:3] = (np.nan, 0.0, 100.0)
    assert rr.mask(m, 100, IDENT, 8, 0.0).tolist() == [False, True, True, True, False, True]
    assert rr.mask(m, 100, IDENT, 8, 5.0).tolist() == [False, False, False, True, False, False]
    assert rr.mask(m, 100, IDENT, 8, -1.0).tolist() == rr.mask(m, 100, IDENT, 8, 0.0).tolist()
    pose = IDENT.copy()
    pose[12:15] = (-3.0, -4.0, 0.0)
    assert rr.mask(m, 100, pose, 8, 5.0).tolist() == [False, False, True, True, False, False]
    assert rr.mask(m[:0], 100, IDENT, 8, 5.0).shape == (0,)


@pytest.mark.parametrize("pp", [1, 0])
def test_scenario_overflows_without_and_fits_with_retirement(oracle_rows, pp):
    """guards the scenario, not the feature: on the oracle alone the sequence overflows the capacity well inside its 140
    frames, and with lockstep retirement every 10 ticks it never does, with more than 10 000 surfels to spare"""
    row, rec = oracle_rows[pp], rr.RECORD[pp]
    cap = rr.CAPACITY[pp] ** 2
    got = dict(first_fail=row["plain"]["first_fail"], peak=row["retired"]["peak"],
               retired=sum(len(f[0]) for f in row["retired"]["files"]), final=row["retired"]["counts"]["count"])
    print(f"preprocess {pp}, capacity {cap}: {got}")
    assert row["plain"]["first_fail"] is not None and 20 < row["plain"]["first_fail"] < rr.N_FRAMES - 20
    assert row["retired"]["first_fail"] is None
    assert row["retired"]["peak"] <= cap - 10000
    assert got == rec
