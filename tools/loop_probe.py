#!/usr/bin/env python3
"""What warping the map by surfel time costs, on one GPU, in one process; every figure the median of 5 after 2
warm-ups.

  model   synth.seeded_model(n) uploaded (times spread over 300 ticks), sm_warp_by_time of the live model alone with a table that
          selects about half of it and with one that selects all of it: device_ms (k_warp_model between two events) and the whole
          call (with the rebuild of the tile boxes).  Next to it sm_retire's device times (SM_RETIRE_TIMING=1) on the same model
          for a retirement that takes the older half out: mark, scan, gather, clear + compaction, publication.
  files   the same rows sorted by time and cut into 16 map files of a few hundred MB together; sm_warp_by_time of the files alone
          with the split of sm_warp_stats, with the file index (the files whose rows all end before t0 stay unopened) and without.
          The files have just been written: every read is served by the page cache.

Writes one text file (--out)."""
import argparse
import os
import sys
import tempfile
import time

os.environ.setdefault("SM_RETIRE_TIMING", "1")

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


def write_map(path, rows):
    with open(path, "wb") as f:
        f.write(np.array([len(rows), 0, 0], np.uint32).tobytes())
        f.write(rows.tobytes())


def table(n):
    """n small rigid steps of a ramp"""
    D = np.eye(4, dtype=np.float32)
    a = np.radians(0.3)
    D[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    D[:3, 3] = (0.2, 0.0, 0.1)
    return capi.loop_spread(D, 0, n - 1)


def probe_model(sm, m):
    n = len(m)
    for name, t0 in (("half", TICK - SPAN // 2), ("all", TICK - SPAN - 1)):
        tab = table(TICK - t0 + 1)
        dev, tot, moved = [], [], 0
        for rep in range(WARM + REPS):
            sm.upload_model(m)
            t = time.perf_counter()
            sm.warp_by_time([], t0, tab)
            dt = (time.perf_counter() - t) * 1e3
            st = sm.warp_stats()
            moved = st["model_moved"]
            if rep >= WARM:
                dev.append(st["device_ms"])
                tot.append(dt)
        gb = (4.0 * n + 80.0 * moved) / 1e9              # the time plane of every slot; 32 B in, 32 B out and a 48-byte table row (cached) per selected
        say(f"  n {n} warp {name}: selected {moved} ({moved / n:.3f})  k_warp_model {med(dev):.3f} ms ({gb / (med(dev) * 1e-3):.0f} GB/s of planes)  "
            f"call {med(tot):.3f} ms")
    ret = []
    for rep in range(WARM + REPS):
        sm.upload_model(m)
        sm.set_tick(TICK + 1)
        got = sm.retire(min_age=SPAN // 2, min_distance=0.0)
        if rep >= WARM:
            ret.append(sm.retire_stats())
    if ret[0] is None:
        say("  sm_retire: not timed (SM_RETIRE_TIMING was off when the context retired first)")
    else:
        s = {k: med([r[k] for r in ret]) for k in ret[0]}
        say(f"  n {n} sm_retire of the older half ({len(got)} rows): mark {s['mark']:.3f} scan {s['scan']:.3f} gather (with its copies to the host) {s['gather']:.3f} "
            f"clear + compaction {s['compact']:.3f} publication {s['bounds']:.3f} ms")


def probe_files(sm, m, tmp, nf=16):
    n = len(m)
    m = m[np.argsort(m[:, 7], kind="stable")]
    cuts = [n * i // nf for i in range(nf + 1)]
    paths = [os.path.join(tmp, f"w{n}_{i}.bin") for i in range(nf)]
    t0 = TICK - SPAN // 4                                # the newest quarter of the drive moves
    tab = table(TICK - t0 + 1)
    for index in (True, False):
        os.environ["SM_RECALL_NO_INDEX"] = "0" if index else "1"
        ts, stats = [], []
        for rep in range(WARM + REPS):
            for i, p in enumerate(paths):
                write_map(p, m[cuts[i]:cuts[i + 1]])
            if index:                                    # the index knows the files: a warp that selects nothing has read them once
                sm.warp_by_time(paths, 10 * TICK, tab, include_model=False)
            t = time.perf_counter()
            sm.warp_by_time(paths, t0, tab, include_model=False)
            dt = (time.perf_counter() - t) * 1e3
            if rep >= WARM:
                ts.append(dt)
                stats.append(sm.warp_stats())
        s = {x: med([q[x] for q in stats]) for x in ("read_ms", "copy_ms", "device_ms", "write_ms", "total_ms")}
        q = stats[-1]
        say(f"  n {n} in {nf} files ({n * 48 / 1e6:.0f} MB), index {'on ' if index else 'off'}: sm_warp_by_time {med(ts):8.2f} ms  (read {s['read_ms']:.2f} copy "
            f"{s['copy_ms']:.2f} device {s['device_ms']:.2f} write {s['write_ms']:.2f}; kernels {100 * s['device_ms'] / s['total_ms']:.2f} % of the call; files read "
            f"{q['files_read']} skipped {q['files_skipped']} rewritten {q['files_rewritten']} chunks {q['chunks']} records read {q['records_read']} moved {q['records_moved']})")
    os.environ.pop("SM_RECALL_NO_INDEX", None)
    for p in paths:
        os.remove(p)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="6000000,20000000")
    ap.add_argument("--file-rows", type=int, default=8000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    sm = capi.SurfelMap(capi.make_config(**synth.HD))
    with tempfile.TemporaryDirectory(prefix="loop_probe_") as tmp:
        for n in [int(x) for x in a.sizes.split(",") if x]:
            probe_model(sm, synth.seeded_model(n, TICK))
        if a.file_rows:
            probe_files(sm, synth.seeded_model(a.file_rows, TICK), tmp)
    sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
