#!/usr/bin/env python3
"""What stereo depth costs, on one GPU, in one process; every figure the median of 5 after 2 warm-ups.

  Per kernel: the time between two events (SM_STEREO_TIMING=1), the bytes the design moves through it (computed from the sizes:
  what it must read and write once, caches ignored) and the rate those give, next to the HBM roof of 8 TB/s.
    census   reads two images (3 B / pixel), writes two planes of codes (8 B / pixel)
    cost     reads the two planes, writes the u8 cost volume (D B / pixel)
    path     per direction: reads the costs (D B / pixel) and, but for the first direction, S (2 D B / pixel); writes S
    select   reads S once per view (2 x 2 D B / pixel), writes depth and disparity
  The yardstick of the issue -- two passes over the W*H*D*2-byte volume per direction and one per view -- is printed beside the
  sum.  Then the whole sm_stereo_depth call with its upload and read-back on the host clock.
  Pairs: synth.stereo_pair of the street scene at 1242 x 375 (D 128, 4 and 8 paths) and 1920 x 1080 (D 128, 8 paths).

Writes one text file (--out)."""
import argparse
import os
import sys
import time

os.environ.setdefault("SM_STEREO_TIMING", "1")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from surfelmapping_amd import capi, synth  # noqa: E402

WARM, REPS = 2, 5
ROOF = 8.0e12
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    return float(np.median(xs))


def line(name, ms, nbytes):
    rate = nbytes / (ms * 1e-3)
    say(f"    {name:<18} {ms * 1e3:9.1f} us  {nbytes / 1e6:9.1f} MB  {rate / 1e9:7.0f} GB/s  {100.0 * rate / ROOF:5.1f} % of the roof")


def probe(cam, D, paths):
    w, h = cam["width"], cam["height"]
    P = w * h
    left, right, depth, _ = synth.stereo_pair(synth.Scene(0), synth.Camera(**cam), synth.pose_matrix(0.3, 0.0, 2.0, 3.0), 0.54)
    sm = capi.SurfelMap(capi.make_config(**cam, max_sqrt_vertices=64))
    sm.set_stereo(max_disp=D, paths=paths)
    ms, call, got = [], [], None
    for rep in range(WARM + REPS):
        t = time.perf_counter()
        got = sm.stereo_depth(left, right)
        dt = (time.perf_counter() - t) * 1e3
        if rep >= WARM:
            ms.append(sm.stereo_ms())
            call.append(dt)
    sm.close()
    say(f"  {w} x {h}, D {D}, {paths} paths: volume {P * D * 2 / 1e6:.0f} MB, cost volume {P * D / 1e6:.0f} MB; "
        f"{100.0 * (got[0] > 0).mean():.1f} % of the pixels get a depth ({100.0 * (depth > 0).mean():.1f} % have one)")
    line("k_stereo_census", med([m["census"] for m in ms]), 2 * P * (3 + 8))
    line("k_stereo_cost", med([m["cost"] for m in ms]), P * (16 + D))
    total_ms, total_b = 0.0, 0
    for r in range(paths):
        t, b = med([m["paths"][r] for m in ms]), P * D * (1 + (2 if r else 0) + 2)
        line(f"k_stereo_path {synth_dir(r)}", t, b)
        total_ms, total_b = total_ms + t, total_b + b
    line("  all directions", total_ms, total_b)
    sel = med([m["select"] for m in ms])
    line("k_stereo_select", sel, 2 * P * D * 2 + P * 4)
    whole = med([m["census"] + m["cost"] + sum(m["paths"]) + m["select"] for m in ms])
    moved = 2 * P * 11 + P * (16 + D) + total_b + 2 * P * D * 2 + P * 4
    yard = (2 * paths + 2) * P * D * 2
    say(f"    all kernels {whole:.3f} ms for {moved / 1e9:.2f} GB ({moved / (whole * 1e-3) / 1e9:.0f} GB/s, {100.0 * moved / (whole * 1e-3) / ROOF:.1f} % of the roof); "
        f"the yardstick (2 passes over the volume per direction, 1 per view) is {yard / 1e9:.2f} GB = {yard / ROOF * 1e3:.3f} ms at the roof")
    say(f"    the call with its upload and read-back {med(call):.3f} ms")


def synth_dir(r):
    return "(%+d,%+d)" % ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))[r]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    probe(synth.KITTI, 128, 4)
    probe(synth.KITTI, 128, 8)
    probe(synth.HD, 128, 8)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
