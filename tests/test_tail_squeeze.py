"""Tail squeeze (DESIGN.md 4 "Tail squeeze"): on an asynchronous plain stream the frame whose compaction only the period asked
for keeps the regular two-launch form -- the slots that are dead ALREADY are squeezed out between its preparation launch and its
pass, from the first tile that holds at least TAIL_DEAD_THRESH dead slots on; the few dead slots below that tile stay where they are.
Nothing the caller can see may depend on it: every variant is compared with the CPU oracle, which compacts at every cull, bit for bit.
SM_TAIL_THRESH moves the threshold (read when the context is created), SM_TAIL_SQUEEZE=0 selects the compacting frame."""
import functools
import math

import numpy as np
import pytest

from backends import assert_models_equal, make
from surfelmapping_amd import synth

pytestmark = pytest.mark.gpu

CAM = dict(width=160, height=120, fx=90.0, fy=90.0, cx=79.5, cy=59.5)        # a few 1024-slot tiles per frame's new surfels
TINY = dict(width=48, height=32, fx=40.0, fy=40.0, cx=23.5, cy=15.5)
IDENT = np.eye(4, dtype=np.float32).T.reshape(16).copy()
COUNT_KEYS = ("count", "offset", "data_count", "conflict_count", "unstable_count", "fused_count", "visible_count", "tick")
LOG_KEYS = ("unstable_count", "fused_count", "conflict_count", "visible_count")
N_FRAMES = 41                                                              # the reference frame + 40 fusing ones


def args(cam):
    return tuple(cam[k] for k in ("width", "height", "fx", "fy", "cx", "cy"))


def wavy(n):
    return [synth.pose_matrix(0.15 * math.sin(0.7 * k), 0.0, 0.35 * k, 0.25 * math.sin(0.5 * k)) for k in range(n)]


@functools.lru_cache(maxsize=None)
def stream(n=N_FRAMES, seed=41):
    return synth.make_sequence(CAM, wavy(n), seed=seed, noise_mm=6.0)


@functools.lru_cache(maxsize=None)
def reference(max_sqrt=700):
    """the oracle over the shared stream, once: (counts after every frame, the final model, the final index-map ids)"""
    o = make("oracle", *args(CAM), preprocess=0, stereo_border=20.0, max_sqrt_vertices=max_sqrt)
    ref = []
    for fr in stream():
        o.process_frame(*fr)
        ref.append(o.counts())
    return ref, o.download_model(), o.download_index_map()[0]


def hip(cam=CAM, **over):
    over.setdefault("preprocess", 0)
    return make("hip", *args(cam), **over)


def enqueue(h, frames, cam=CAM):
    """the frames as device buffers, enqueued without a host wait in between"""
    P = cam["width"] * cam["height"]
    bufs = []
    for rgb, d, s, p in frames:
        dr, dd, ds = h.device_alloc(P * 3), h.device_alloc(P * 2), h.device_alloc(P)
        h.device_upload(dr, rgb); h.device_upload(dd, d); h.device_upload(ds, s)
        bufs.append((dr, dd, ds, p))
    for b in bufs:
        h.process_frame_device(*b)


def same_counts(c, h, what):
    ch = h.counts()
    assert {k: c[k] for k in COUNT_KEYS} == {k: ch[k] for k in COUNT_KEYS}, what


def check_log(log, ref, what):
    """every fusing frame's counters as the device logged them against the oracle's after the same frame"""
    assert len(log) == len(ref) - 1, what
    for k, (e, before, after) in enumerate(zip(log, ref[:-1], ref[1:])):
        assert int(e["n_before"]) == before["count"], f"{what}: frame {k + 1} n_before"
        assert int(e["n_after_cull"]) == after["offset"], f"{what}: frame {k + 1} n_after_cull"
        assert tuple(int(e[x]) for x in LOG_KEYS) == tuple(after[x] for x in LOG_KEYS), f"{what}: frame {k + 1}"


@pytest.mark.parametrize("period", [2, 3, 5])
@pytest.mark.parametrize("thresh", [None, 1])
def test_periodic_squeezes_give_the_oracle_model(period, thresh, monkeypatch):
    """thresh None: the default threshold -- at least one squeeze must have kept a boundary above tile 0 with dead slots below it.
    thresh 1: the first tile with ONE dead slot is the first dead slot's tile, nothing stays behind: the full form, every time."""
    if thresh is not None:
        monkeypatch.setenv("SM_TAIL_THRESH", str(thresh))
    ref, model, ids = reference()
    h = hip(stereo_border=20.0, max_sqrt_vertices=700, compact_period=period)
    enqueue(h, stream())
    h.sync()
    same_counts(ref[-1], h, f"period={period}")
    log = h.read_frame_log(64)
    check_log(log, ref, f"period={period} thresh={thresh}")
    tail, full = h.debug_squeezes()
    moved = log["n_static"] < log["n_slots"]
    carried = log["n_slots"].astype(np.int64) - log["n_before"].astype(np.int64)     # dead slots a frame's cull found in place
    print(f"period={period} thresh={thresh}: squeezes tail={tail} full={full}, frames that moved surfels {int(moved.sum())}, "
          f"dead slots carried into squeezing frames {carried[moved].tolist()}")
    assert tail + full == (N_FRAMES - 1) // period, "every period-th fusing frame squeezes"
    assert moved.sum() >= tail + full - 1 and log["n_kill"].sum() > 2000, "the stream must cull, the squeezes must move surfels"
    if thresh is None:
        assert tail >= 1, "no squeeze left dead slots below its boundary: the tail rule was never exercised"
        assert (carried[moved] > 0).any(), "a tail squeeze leaves its garbage in the frame's log"
    else:
        assert tail == 0 and full >= 1
        assert (carried[moved] == 0).all()
    assert_models_equal(model, h.download_model(), f"period={period} thresh={thresh}")
    np.testing.assert_array_equal(ids, h.download_index_map()[0])


def test_switch_off_gives_the_same_model_and_counts(monkeypatch):
    """SM_TAIL_SQUEEZE=0 (the seven-launch compacting frame, full compaction) and =1 over the same stream"""
    out = []
    for sw in ("0", "1"):
        monkeypatch.setenv("SM_TAIL_SQUEEZE", sw)
        h = hip(stereo_border=20.0, max_sqrt_vertices=700, compact_period=3)
        enqueue(h, stream())
        h.sync()
        log = h.read_frame_log(64)
        out.append((h.counts(), {k: log[k].copy() for k in LOG_KEYS + ("n_before", "n_after_cull", "n_kill")}, h.debug_squeezes(), h.download_model()))
    (c0, l0, s0, m0), (c1, l1, s1, m1) = out
    assert s0 == (0, 0) and sum(s1) == (N_FRAMES - 1) // 3
    assert {k: c0[k] for k in COUNT_KEYS} == {k: c1[k] for k in COUNT_KEYS}
    for k in l0:
        np.testing.assert_array_equal(l0[k], l1[k], err_msg=k)
    assert_models_equal(m0, m1, "SM_TAIL_SQUEEZE=0 against =1")
    assert_models_equal(reference()[1], m1, "SM_TAIL_SQUEEZE=1 against the oracle")


def test_sync_download_and_reset_in_the_middle_of_a_squeezing_stream():
    """a sync + download between two squeezes runs the dense compaction on a model that holds a tail squeeze's garbage; reset()
    discards such a model; the stream goes on after either"""
    seq = stream()
    o = make("oracle", *args(CAM), preprocess=0, stereo_border=20.0, max_sqrt_vertices=700)
    h = hip(stereo_border=20.0, max_sqrt_vertices=700, compact_period=3)
    for fr in seq[:14]:
        o.process_frame(*fr)
    enqueue(h, seq[:14])                               # squeezes in the fusing frames 3, 6, 9, 12: one frame of garbage on top
    h.sync()
    same_counts(o.counts(), h, "before the download")
    assert sum(h.debug_squeezes()) == 4
    assert_models_equal(o.download_model(), h.download_model(), "in the middle")
    np.testing.assert_array_equal(o.download_index_map()[0], h.download_index_map()[0])
    for fr in seq[14:24]:
        o.process_frame(*fr)
    enqueue(h, seq[14:24])
    h.sync()
    same_counts(o.counts(), h, "after the download")
    o.reset(); h.reset()
    for fr in seq[24:34]:
        o.process_frame(*fr)
    enqueue(h, seq[24:34])
    h.sync()
    same_counts(o.counts(), h, "after reset")
    a, b = o.download_model(), h.download_model()
    assert a.shape == b.shape
    ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))     # raw-cloud normals: NaN payloads differ
    assert ok.all()


def old_model(n, seed, rng):
    m = synth.seeded_model(n, tick=1, seed=seed)
    m[:, 0] = rng.uniform(-1.5, 1.5, n)
    m[:, 1] = rng.uniform(-1.0, 1.0, n)
    m[:, 2] = rng.uniform(3.0, 6.0, n)
    return m


def run_tiny(h, o, frames, rgb, sem):
    P = TINY["width"] * TINY["height"]
    bufs = []
    for d in frames:
        dr, dd, ds = h.device_alloc(P * 3), h.device_alloc(P * 2), h.device_alloc(P)
        h.device_upload(dr, rgb); h.device_upload(dd, d); h.device_upload(ds, sem)
        bufs.append((dr, dd, ds))
    for d in frames:
        o.process_frame(rgb, d, sem, IDENT)
    for b in bufs:
        h.process_frame_device(*b, IDENT)
    h.sync()


def test_surfels_below_the_boundary_die_after_a_tail_squeeze_and_id_zero_keeps_its_slot():
    """The K-test that kills id 0 (test_id_zero_dies_in_asynchronous_frames), repeated across squeezes.  Tiles 0..2 hold confident
    surfels and a handful of weak ones (20 per tile die in the first frames: fewer than the threshold), tiles 3..5 weak ones (hundreds
    die per frame): every squeeze starts at tile 3 and leaves the dead of tiles 0..2 -- slot 0 and the 40 behind it among them --
    where they are.  The surfel the reference addresses as id 0 is exempt from the conflict test, so it can only die on arrival
    (conf <= 0, an uploaded model): slots 0..39 do, in the first pass -- in which the exemption is still slot 0's, so slot 40
    (conf 0.7) conflicts like any other surfel and dies with them.  From then on `first_live` is 41 and cannot die; it must survive
    every squeeze as slot 41 (a tile below the boundary always holds a live surfel, so the first live one lies below it), and
    surfels below the boundary keep dying after the squeezes."""
    rng = np.random.default_rng(29)
    n = 6000
    m = old_model(n, 4, rng)
    m[:3072, 3] = rng.uniform(20.5, 30.5, 3072)          # tiles 0..2: never die here ...
    for t in range(3):
        m[t * 1024 + 100:t * 1024 + 120, 3] = rng.uniform(0.5, 4.5, 20)     # ... but for 20 each, one to four conflicts away
    m[3072:, 3] = rng.uniform(0.5, 4.5, n - 3072)        # tiles 3..5: a quarter of them dies per frame
    m[:40, 3] = 0.0                                      # id 0 and the 39 slots behind it are dead already
    m[40, 3] = 0.7                                       # the first live one dies at its first conflict (slot 0 holds the exemption in that pass)
    o = make("oracle", *args(TINY), preprocess=0, stereo_border=0.0, conflict_cap=0, max_sqrt_vertices=200, fuse_thresh=0.05)
    h = hip(TINY, stereo_border=0.0, conflict_cap=0, max_sqrt_vertices=200, fuse_thresh=0.05, compact_period=2)
    o.upload_model(m); h.upload_model(m)
    rgb = rng.integers(0, 255, (32, 48, 3), dtype=np.uint8)
    sem = np.zeros((32, 48), np.uint8)
    far = np.full((32, 48), 20000, np.uint16)
    mid = np.full((32, 48), 4500, np.uint16)
    run_tiny(h, o, [far, far, far, mid, far, far, far], rgb, sem)          # the reference frame + 6 fusing ones: squeezes in 2, 4, 6
    same_counts(o.counts(), h, "id 0 dies, squeezes")
    tail, full = h.debug_squeezes()
    log = h.read_frame_log(16)
    print(f"squeezes tail={tail} full={full}; n_kill {log['n_kill'].tolist()}; n_static {log['n_static'].tolist()} of {log['n_slots'].tolist()}")
    assert tail >= 2, "the squeezes must leave tiles 0..2 and their dead slots alone"
    assert (log["n_kill"][2:] > 0).all(), "surfels keep dying after the first squeeze"
    assert_models_equal(o.download_model(), h.download_model(), "id 0 dies, squeezes")
    np.testing.assert_array_equal(o.download_index_map()[0], h.download_index_map()[0])


def test_conflict_cap_binds_in_the_squeezing_frame_and_the_one_after():
    """20 000 surfels in view of 1 536 pixels: the W*H cap binds in most frames, the squeezing ones and their successors included"""
    rng = np.random.default_rng(11)
    n = 20000
    m = old_model(n, 5, rng)
    m[:, 3] = rng.uniform(0.5, 4.5, n).astype(np.float32)
    m[::5, 3] = np.float32(16777218.0)                   # conf - 1 is not representable: only the undo plane restores it
    m[3::11, 3] = 0.0
    o = make("oracle", *args(TINY), preprocess=0, stereo_border=0.0, conflict_cap=1, max_sqrt_vertices=200)
    h = hip(TINY, stereo_border=0.0, conflict_cap=1, max_sqrt_vertices=200, compact_period=2)
    o.upload_model(m); h.upload_model(m)
    rgb = rng.integers(0, 255, (32, 48, 3), dtype=np.uint8)
    sem = np.zeros((32, 48), np.uint8)
    far = np.full((32, 48), 20000, np.uint16)
    mid = np.full((32, 48), 4500, np.uint16)
    run_tiny(h, o, [far, far, mid, far, far, mid, far, far, far], rgb, sem)          # squeezes in the fusing frames 2, 4, 6, 8
    same_counts(o.counts(), h, "cap binding across squeezes")
    log = h.read_frame_log(16)
    P = 48 * 32
    assert sum(h.debug_squeezes()) == 4
    binds = log["conflict_count"] == P
    print("cap binds in fusing frames", (np.nonzero(binds)[0] + 1).tolist())
    assert (binds[1::2]).any() and (binds[2::2]).any(), "the cap must bind in a squeezing frame (2, 4, ..) and in one right after (3, 5, ..)"
    assert_models_equal(o.download_model(), h.download_model(), "cap binding across squeezes")
    np.testing.assert_array_equal(o.download_index_map()[0], h.download_index_map()[0])


def test_sparse_deaths_everywhere_fall_back_to_the_full_form(monkeypatch):
    """an old model whose surfels die sparsely in every tile, and a threshold no tile can reach: the dead slots that would stay
    behind are all of them, far more than 1/32 of the slots -- every squeeze runs the full form"""
    monkeypatch.setenv("SM_TAIL_THRESH", "2000")
    rng = np.random.default_rng(17)
    n = 20000
    m = old_model(n, 9, rng)
    m[:, 3] = rng.uniform(10.5, 20.5, n)
    # ~340 weak ones per tile, one to three conflicts away: 1 100 (conf <= 1) die in the first frame, 2 200 in each of the next
    # two -- every squeeze finds more than n / 32 = 625 dead slots, spread over all tiles
    weak = rng.choice(n, n // 3, replace=False)
    m[weak, 3] = rng.uniform(0.5, 3.5, len(weak))
    o = make("oracle", *args(TINY), preprocess=0, stereo_border=0.0, conflict_cap=0, max_sqrt_vertices=200)
    h = hip(TINY, stereo_border=0.0, conflict_cap=0, max_sqrt_vertices=200, compact_period=2)
    o.upload_model(m); h.upload_model(m)
    rgb = rng.integers(0, 255, (32, 48, 3), dtype=np.uint8)
    sem = np.zeros((32, 48), np.uint8)
    far = np.full((32, 48), 20000, np.uint16)
    run_tiny(h, o, [far] * 6, rgb, sem)
    same_counts(o.counts(), h, "sparse deaths")
    log = h.read_frame_log(16)
    assert h.debug_squeezes() == (0, 2), "squeezes in the fusing frames 2 and 4, both full"
    carried = log["n_slots"].astype(np.int64) - log["n_before"].astype(np.int64)
    assert carried[1] == 0 and carried[3] == 0 and carried[2] > n // 32, carried
    assert_models_equal(o.download_model(), h.download_model(), "sparse deaths")


def test_capacity_pressure_after_tail_squeezes_and_the_error_arrives_with_the_oracles():
    """36 100 slots, at most P / 2 = 9 600 new surfels per frame.  While live surfels + garbage + 9 600 fit, every second frame
    squeezes (tail squeezes among them: garbage stays behind).  Once the live surfels alone no longer leave room for a frame's
    candidates -- the oracle's count before the frame + 9 600 > 36 100, frame 17 on this stream -- the capacity rule asks for every
    compaction: those run the compacting frame (no dead slot left, dense append), on a model that holds a tail squeeze's garbage, and
    no further squeeze runs.  SM_E_CAPACITY (-2) arrives in exactly the frames in which the oracle's count overflows (first: 24)."""
    seq = stream()[:32]
    cap, new_max = 190 * 190, CAM["width"] * CAM["height"] // 2
    o = make("oracle", *args(CAM), preprocess=0, stereo_border=20.0, max_sqrt_vertices=190)
    h = hip(stereo_border=20.0, max_sqrt_vertices=190, compact_period=2)
    P = CAM["width"] * CAM["height"]
    rcs, sq, before = [], [], []
    for k, (rgb, d, s, p) in enumerate(seq):
        before.append(o.counts()["count"])
        ro = o.process_frame(rgb, d, s, p, allow=(0, -2))
        dr, dd, ds = h.device_alloc(P * 3), h.device_alloc(P * 2), h.device_alloc(P)
        h.device_upload(dr, rgb); h.device_upload(dd, d); h.device_upload(ds, s)
        h.process_frame_device(dr, dd, ds, p)
        rh = h.sync(allow=(0, -2))
        assert ro == rh, f"frame {k}"
        rcs.append(rh)
        sq.append(h.debug_squeezes())
        same_counts(o.counts(), h, f"frame {k}")
    pressure = next(k for k, c in enumerate(before) if c + new_max > cap)        # from here on the live surfels alone force it
    print("return codes", rcs, "squeezes (tail, full) after each frame", sq, "pressure from frame", pressure)
    assert pressure >= 8, "a few periods must squeeze before the pressure starts"
    assert sq[pressure - 1][0] >= 1, "a tail squeeze must have left garbage behind before the pressure starts"
    assert sq[-1] == sq[pressure - 1], "a compaction the capacity rule asks for is never a squeeze"
    assert -2 in rcs[pressure:] and 0 in rcs[rcs.index(-2):], "the stream must overflow, and go on after it"
    log = h.read_frame_log(64)
    carried = log["n_slots"].astype(np.int64) - log["n_before"].astype(np.int64)
    assert (carried[pressure:] == 0).all(), "under pressure every frame compacts fully: no dead slot is carried into the next one"
    assert_models_equal(o.download_model(), h.download_model(), "capacity pressure")
