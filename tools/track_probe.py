#!/usr/bin/env python3
"""track_probe.py -- cost of a tracked frame (sm_track_frame, DESIGN.md "4d. Tracking") on the MI355X.

Per camera (KITTI 1242x375, HD 1920x1080): a map fused by the core from --frames ground-truth frames of
synth.kitti_trajectory through Scene(n_boxes=40), then --reps calls of track() on the next frame from the constant-velocity
guess (default parameters).  Reports the wall clock per tracked frame (depth upload, prediction, iterations, the one host
wait), the device split from events (SM_TRACK_TIMING=1): prediction (key fill + splat + resolve), vertex stage, the
reductions and solves of the iterations that did work and of the no-op launches after convergence, the iterations used, the
error against the true pose and the live surfels.  Writes $OUT_DIR/track_mi355x.txt.

    OUT_DIR=<folder> python tools/track_probe.py [--frames 40] [--reps 20]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import track_ref as tr  # noqa: E402
from surfelmapping_amd import capi, synth  # noqa: E402


def probe(name, cam, n_frames, reps, out):
    poses = synth.kitti_trajectory(n_frames + 1)
    (seq,) = synth.make_sequences_parallel([(cam, poses, 0, 0.0, dict(seed=0, n_boxes=40))], workers=12)
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=5000))
    for fr in seq[:-1]:
        m.process_frame(*fr)
    m.sync()
    live = m.counts()["count"]
    depth = seq[-1][1]
    for _ in range(3):
        m.track(depth)
    t0 = time.perf_counter()
    for _ in range(reps):
        pose, info = m.track(depth)
    wall = (time.perf_counter() - t0) / reps * 1e3
    os.environ["SM_TRACK_TIMING"] = "1"
    splits = []
    for _ in range(reps):
        m.track(depth)
        splits.append(m.track_stats())
    del os.environ["SM_TRACK_TIMING"]
    ms = np.median(np.array(splits), axis=0)
    it = info["iterations"]
    red, sol = ms[2::2], ms[3::2]
    et, er = tr.pose_error(pose, poses[-1])
    out(f"== {name}: {cam['width']}x{cam['height']}, {live} live surfels after {n_frames} frames, {reps} tracked calls "
        f"(median of the device split)")
    out(f"wall ms/frame {wall:.3f}   device: prediction {ms[0]:.3f}  vertex {ms[1]:.3f}  "
        f"reduce {red[:it].sum():.3f} ({red[:it].mean():.4f}/iter)  solve {sol[:it].sum():.3f} ({sol[:it].mean():.4f}/iter)  "
        f"no-op launches {red[it:].sum() + sol[it:].sum():.3f}  total {ms.sum():.3f}")
    out(f"status {info['status']}  iterations {it} of {len(red)}  inliers {info['inliers']}  rmse {info['rmse'] * 1e3:.3f} mm  "
        f"error {et * 1e3:.3f} mm {er:.4f} deg")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out_dir = os.environ.get("OUT_DIR")
    if not out_dir:
        sys.exit("set OUT_DIR to the folder the results go to")
    os.makedirs(out_dir, exist_ok=True)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out(f"# python tools/track_probe.py --frames {a.frames} --reps {a.reps} on one MI355X (gfx950)")
    for name, cam in (("kitti", dict(synth.KITTI)), ("hd", dict(synth.HD))):
        probe(name, cam, a.frames, a.reps, out)
    with open(os.path.join(out_dir, "track_mi355x.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
