#!/usr/bin/env python3
"""track_rgb_probe.py -- cost of a frame tracked with the colour term (sm_track_frame_rgb, DESIGN.md "4d. Tracking", "colour
term") against sm_track_frame on the same map and frame, on the MI355X.

Per case (KITTI 1242x375 and HD 1920x1080 through Scene(n_boxes=40); KITTI through the corridor Scene(n_boxes=0)): a map fused
by the core from --frames ground-truth frames of synth.kitti_trajectory, then, after 3 warm-up calls each and alternating
between the two, --reps calls of track() and of track_rgb() on the next frame from the constant-velocity guess (default
parameters).  Reports the median wall clock per call (uploads, every launch, the one host wait) and, from a second set of
--reps calls under SM_TRACK_TIMING=1 (events around every kernel: profiled calls are not the timed ones), the median device
split: prediction, vertex stages, luminance pyramid, gather, and per level the geometric reductions, photometric reductions
and solves that did work, with the launches that were no-ops after their level ended.  Writes $OUT_DIR/track_rgb_mi355x.txt.

    OUT_DIR=<folder> python tools/track_rgb_probe.py [--frames 40] [--reps 20]
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


def probe(name, cam, scene, n_frames, reps, out):
    poses = synth.kitti_trajectory(n_frames + 1)
    (seq,) = synth.make_sequences_parallel([(cam, poses, 0, 0.0, scene)], workers=12)
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=5000))
    for fr in seq[:-1]:
        m.process_frame(*fr)
    m.sync()
    live = m.counts()["count"]
    rgb, depth = seq[-1][0], seq[-1][1]
    calls = {"track": lambda: m.track(depth), "track_rgb": lambda: m.track_rgb(rgb, depth)}
    for f in calls.values():
        for _ in range(3):
            f()
    wall = {k: [] for k in calls}
    res = {}
    for _ in range(reps):
        for k, f in calls.items():
            t0 = time.perf_counter()
            res[k] = f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    os.environ["SM_TRACK_TIMING"] = "1"
    icp_split, rgb_split = [], []
    for _ in range(reps):
        m.track(depth)
        icp_split.append(m.track_stats())
        m.track_rgb(rgb, depth)
        rgb_split.append(m.track_rgb_stats())
    del os.environ["SM_TRACK_TIMING"]
    out(f"== {name}: {cam['width']}x{cam['height']}, {live} live surfels after {n_frames} frames, {reps} calls each, alternating "
        f"(medians)")
    # sm_track_frame
    pose, info = res["track"]
    ms = np.median(np.array(icp_split), axis=0)
    it = info["iterations"]
    red, sol = ms[2::2], ms[3::2]
    et, er = tr.pose_error(pose, poses[-1])
    w_icp = float(np.median(wall["track"]))
    out(f"track      wall ms/frame {w_icp:.3f} (min {min(wall['track']):.3f} max {max(wall['track']):.3f})   device: prediction "
        f"{ms[0]:.3f}  vertex {ms[1]:.3f}  reduce {red[:it].sum():.3f} ({red[:it].mean():.4f}/iter)  solve {sol[:it].sum():.3f} "
        f"({sol[:it].mean():.4f}/iter)  no-op launches {red[it:].sum() + sol[it:].sum():.3f}  total {ms.sum():.3f}")
    out(f"           status {info['status']}  iterations {it} of {len(red)}  inliers {info['inliers']}  error {et * 1e3:.3f} mm "
        f"{er:.4f} deg")
    # sm_track_frame_rgb
    pose, info = res["track_rgb"]
    kinds = [(k, l) for k, l, _ in rgb_split[0]]
    ms = np.median(np.array([[x[2] for x in s] for s in rgb_split]), axis=0)
    et, er = tr.pose_error(pose, poses[-1])
    w_rgb = float(np.median(wall["track_rgb"]))

    def total(kind, level=None, first=None, last=None):
        v = [ms[i] for i, (k, l) in enumerate(kinds) if k == kind and (level is None or l == level)]
        return float(np.sum(v[first:last]))
    out(f"track_rgb  wall ms/frame {w_rgb:.3f} (min {min(wall['track_rgb']):.3f} max {max(wall['track_rgb']):.3f})   device: "
        f"prediction {total('prediction'):.3f}  vertex {total('vertex'):.3f}  pyramid {total('pyramid'):.3f}  gather "
        f"{total('gather'):.3f}  level vertex stages {total('level_vertex'):.3f}  total {ms.sum():.3f}")
    noop = 0.0
    for level in range(2, -1, -1):
        n = info["level_iterations"][level]
        launched = sum(1 for k, l in kinds if k == "solve" and l == level)
        parts = {k: total(k, level, 0, n) for k in ("icp", "photo", "solve")}
        noop += sum(total(k, level, n, None) for k in ("icp", "photo", "solve"))
        out(f"           level {level} (stride {1 << level}): {n} of {launched} iterations   icp {parts['icp']:.3f} "
            f"({parts['icp'] / max(n, 1):.4f}/iter)  photo {parts['photo']:.3f} ({parts['photo'] / max(n, 1):.4f}/iter)  solve "
            f"{parts['solve']:.3f} ({parts['solve'] / max(n, 1):.4f}/iter)")
    out(f"           no-op launches {noop:.3f}   status {info['status']}  inliers {info['inliers']}  rgb inliers "
        f"{info['rgb_inliers']}  pivot ratio {info['pivot_ratio']:.3g}  error {et * 1e3:.3f} mm {er:.4f} deg")
    out(f"           wall ratio track_rgb / track {w_rgb / w_icp:.2f}")


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
    out(f"# python tools/track_rgb_probe.py --frames {a.frames} --reps {a.reps} on one MI355X (gfx950)")
    boxes, corridor = dict(seed=0, n_boxes=40), dict(seed=0, n_boxes=0)
    for name, cam, scene in (("kitti", dict(synth.KITTI), boxes), ("hd", dict(synth.HD), boxes),
                             ("kitti corridor", dict(synth.KITTI), corridor)):
        probe(name, cam, scene, a.frames, a.reps, out)
    with open(os.path.join(out_dir, "track_rgb_mi355x.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
