#!/usr/bin/env python3
"""How old are the surfels a frame's cull kills?  (DESIGN.md 4 "Tail squeeze": the rule that starts a periodic squeeze at the first
DENSE tile rests on this.)  Runs the CPU oracle -- which compacts at every cull, so the model after a frame's cull is a
subsequence of the model before it -- over the bench's own KITTI frames (seed 1, 15 mm noise) and records, for every frame, which
surfels of the previous model are gone and their age `tick - init_time`.  CPU only; a few minutes for the default 110 frames.

    python tools/kill_age_study.py [frames] [--save kills.npy]

Recorded with 110 frames (10 warm-up frames left out): 102.7 k kills per frame;
    age at death (frames)   <=1     <=2     <=3     <=5     <=8      <=12     <=24
    share of all kills      0.619   0.821   0.913   0.974   0.9944   0.9990   0.99999
a cohort of 157 k new surfels thins out to 93 k / 73 k / 63 k / 57 k / 55 k / 54 k after age 1 / 2 / 3 / 5 / 8 / 12.

The key that matches a surfel before and after a cull (position bits and creation time) is neither fully invariant -- a fuse moves a
surfel -- nor unique: per frame a handful of survivors (1-16 of several million) are not found again and are counted as kills at
whatever age they have.  Against ~100 k kills per frame that is noise; the script prints the largest mismatch and names every frame where
it exceeds 1 in 1 000 kills."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
import oracle_lib as ol  # noqa: E402
from surfelmapping_amd import synth  # noqa: E402


def keys(m):
    """a 64-bit key per surfel from what a cull leaves alone: position bits and the creation time"""
    b = np.ascontiguousarray(m[:, :3]).view(np.uint32).astype(np.uint64)
    t = np.ascontiguousarray(m[:, 6]).view(np.uint32).astype(np.uint64)
    return b[:, 0] ^ (b[:, 1] << np.uint64(21)) ^ (b[:, 2] << np.uint64(42)) ^ (t << np.uint64(7))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("frames", nargs="?", type=int, default=110)
    ap.add_argument("--skip", type=int, default=10, help="frames left out of the summary (the bench's warm-up)")
    ap.add_argument("--save", help="write the per-frame records (frame, tick, model size, kills, first killed index, creation times, indices) here")
    a = ap.parse_args()
    ol.build()
    cam = synth.KITTI
    t0 = time.time()
    frames = bench.make_frames(cam, a.frames, 1, 15.0, 16)
    print(f"{a.frames} frames generated in {time.time() - t0:.1f} s", flush=True)
    o = ol.Oracle(ol.make_config(**cam, preprocess=0, conflict_cap=1, max_sqrt_vertices=5000))
    prev, rec, worst = None, [], 0
    for k in range(a.frames):
        o.process_frame(*frames[k])
        c = o.counts()
        m = o.download_model()
        if prev is not None and len(prev):
            gone = np.nonzero(~np.isin(keys(prev), keys(m[:c["offset"]])))[0]
            miss = (len(prev) - len(gone)) - c["offset"]          # survivors the keys did not find again (counted as kills)
            if abs(miss) > max(16, len(gone) // 1000):
                print(f"frame {k}: the key match is off by {miss} survivors ({len(gone)} kills): treat this frame's ages with care", flush=True)
            worst = max(worst, abs(miss))
            rec.append((k, c["tick"], len(prev), len(gone), int(gone.min()) if len(gone) else -1, prev[gone, 6].copy(), gone.copy()))
            if k % 10 == 0:
                print(f"frame {k}: {len(gone)} of {len(prev)} killed, first at index {rec[-1][4]}", flush=True)
        prev = m
    if a.save:
        np.save(a.save, np.array(rec, dtype=object), allow_pickle=True)
    rec = rec[a.skip:]
    ages = np.concatenate([(r[1] - 1) - r[5] for r in rec])
    print(f"kills {len(ages)}, per frame {len(ages) / len(rec):.0f}")
    print(f"largest per-frame mismatch between the key match and the oracle's survivor count: {worst}")
    for age in (0, 1, 2, 3, 5, 8, 12, 24, 48):
        print(f"age <= {age:2d}: {float((ages <= age).mean()):.5f}")
    first = np.array([r[4] for r in rec if r[3]], np.float64) / np.array([r[2] for r in rec if r[3]], np.float64)
    print(f"first killed index / model size: min {first.min():.3f} median {np.median(first):.3f}")


if __name__ == "__main__":
    main()
