#!/usr/bin/env python3
"""What closing loops unasked costs per tracked frame, on one GPU, in one process; every figure the median of 5
after 2 warm-ups.

  census   synth.seeded_model(n) uploaded (HD camera, times spread over 300 ticks), the camera at the origin: k_loop_census between
           two events (SM_TRACK_TIMING=1) with none, half and all of the surfels old, the whole sm_old_in_view call on the host
           clock, and next to them the tracker's "prediction" interval (key fill, splat, resolve) of sm_track_debug on the same
           model, as tools/track_probe.py measures it.
  attempt  the scene of tests/test_loop.py (KITTI camera, 10 frames of old world paged back in, 6 young frames at true poses): the
           host-clock time of the young-window track, of the census and of one sm_close_loop that ends SM_LOOP_NONE -- what a
           frame pays when the policy looks and finds nothing to correct.

Writes one text file (--out)."""
import argparse
import os
import sys
import tempfile
import time

os.environ.setdefault("SM_TRACK_TIMING", "1")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from surfelmapping_amd import capi, synth  # noqa: E402

WARM, REPS = 2, 5
TICK, SPAN = 1000, 300
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    return float(np.median(xs))


def probe_census(sm, n):
    cam = synth.HD
    m = synth.seeded_model(n, TICK)
    sm.upload_model(m)
    sm.set_tick(TICK + 1)
    pose = np.eye(4, dtype=np.float32)
    depth = np.zeros((cam["height"], cam["width"]), np.uint16)
    pred = []
    for rep in range(WARM + REPS):
        sm.track_debug(depth, pose)
        if rep >= WARM:
            pred.append(sm.track_stats()[0])
    say(f"  n {n}: prediction interval of sm_track_debug {med(pred):.3f} ms")
    for name, mt in (("none", TICK - SPAN - 1), ("half", TICK - SPAN // 2), ("all", TICK)):
        dev, call, got = [], [], 0
        for rep in range(WARM + REPS):
            t = time.perf_counter()
            got = sm.old_in_view(pose, mt)
            dt = (time.perf_counter() - t) * 1e3
            if rep >= WARM:
                dev.append(sm.census_ms())
                call.append(dt)
        old = int((m[:, 7] <= np.float32(mt)).sum())
        gb = (4.0 * n + n / 8.0 + 16.0 * old) / 1e9
        say(f"  n {n} census, {name} old ({old / n:.3f}): {got} in view  k_loop_census {med(dev):.3f} ms ({gb / (med(dev) * 1e-3):.0f} GB/s)  "
            f"call {med(call):.3f} ms  = {med(dev) / med(pred):.2f} of the prediction interval")


def write_map(path, rows, a, b):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes())
        f.write(np.array([a, b], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, np.float32).tobytes())


def probe_attempt(tmp):
    cam = dict(synth.KITTI)
    poses = synth.kitti_trajectory(11)
    (seq,) = synth.make_sequences_parallel([(cam, poses, 0, 0.0, dict(seed=0, n_boxes=40))], workers=11)
    old = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    for fr in seq[:10]:
        old.process_frame(*fr)
    rows = old.download_model()
    old.close()
    f_path, n_path = os.path.join(tmp, "F.bin"), os.path.join(tmp, "N.bin")
    write_map(f_path, rows, 0, 9)
    g = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    g.set_tick(400)
    for fr in seq[4:10]:
        g.process_frame(*fr)
    g.save_map(n_path, 400, 405)
    g.recall([f_path], pose=seq[9][3], mode="copy", radius=500.0)
    split = 406 - 1 - g.cfg.time_delta
    depth, guess = seq[10][1], poses[10].astype(np.float32)
    t_track, t_census, t_attempt, status, n_old = [], [], [], "", 0
    for rep in range(WARM + REPS):
        t0 = time.perf_counter()
        pose, info = g.track_window(depth, split, 2 ** 31 - 1, guess=guess, dist_thresh=0.5)
        t1 = time.perf_counter()
        n_old = g.old_in_view(pose, split)
        t2 = time.perf_counter()
        _, li = g.close_loop(depth, pose, paths=[n_path], dist_thresh=0.5)
        t3 = time.perf_counter()
        status = li["status"]
        if rep >= WARM:
            t_track.append((t1 - t0) * 1e3); t_census.append((t2 - t1) * 1e3); t_attempt.append((t3 - t2) * 1e3)
    say(f"  kitti, {g.counts()['count']} surfels ({len(rows)} old, {n_old} of them in view): young-window track {med(t_track):.3f} ms ({info['status']}), "
        f"census call {med(t_census):.3f} ms, one attempt ending {status} {med(t_attempt):.3f} ms (SM_TRACK_TIMING=1: events around every kernel)")
    g.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="6000000,20000000")
    ap.add_argument("--no-attempt", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auto_loop_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    sm = capi.SurfelMap(capi.make_config(**synth.HD))
    z = np.zeros((synth.HD["height"], synth.HD["width"]), np.uint16)
    # (one empty frame at the identity: the prediction's pose)
    sm.process_frame(np.zeros(z.shape + (3,), np.uint8), z, np.zeros(z.shape, np.uint8), np.eye(4, dtype=np.float32).reshape(16))
    for n in [int(x) for x in a.sizes.split(",") if x]:
        probe_census(sm, n)
    sm.close()
    if not a.no_attempt:
        with tempfile.TemporaryDirectory(prefix="auto_loop_probe_") as tmp:
            probe_attempt(tmp)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
