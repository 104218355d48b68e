#!/usr/bin/env python3
"""What the hole filling of novel views costs, on one GPU, in one process; every figure the median of 5 after 2
warm-ups.

  Views of synth.seeded_model(2 M surfels) held as the live model, drawn by one render_image_maps(fill=..., depth=True) call per
  batch (no files: the live model is the whole set), at 1242 x 375 and 1920 x 1080, levels 3 and 5, batches of 1 and 16 views.
  Per row: the completion's device time (events around the stage, fill_stats), the render's own device time for the same views
  (render_maps_stats, events around the live model's kernels), the stage's launches, the share of pixels it found empty and
  filled, and the bytes the stage must move once -- per image of P pixels with P_l cells at level l: the three planes read
  (6 P), the validity plane written and read (2 P), every record written by the pull and read as a tap (16 P_l), read again as
  the level the push fills (8 P_l, l < levels), and the filled pixels written (6 each) -- next to the time those bytes take at
  the HBM roof of 8 TB/s.  The stage's time over its launches is the figure to hold against a launch boundary.

Writes one text file (--out)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from surfelmapping_amd import capi, synth  # noqa: E402

WARM, REPS = 2, 5
ROOF = 8.0e12
N_SURFELS = 2_000_000
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    return float(np.median(xs))


def poses(V):
    """V cameras through the seeded volume (x -60..60, z -50..250), every fourth looking back"""
    ps = []
    for k in range(V):
        z = -40.0 + 280.0 * k / max(V, 2)
        ps.append(synth.pose_to_colmajor(synth.pose_matrix(10.0 * np.sin(k), 0.0, z, (180.0 if k % 4 == 3 else 0.0) + 5.0 * np.cos(k))))
    return np.stack(ps)


def stage_bytes(w, h, levels, n, filled):
    P, total = w * h, 0
    total += 8 * P * n
    lw, lh = w, h
    for l in range(1, levels + 1):
        lw, lh = (lw + 1) // 2, (lh + 1) // 2
        total += (16 + (8 if l < levels else 0)) * lw * lh * n
    return total + 6 * filled


def probe(model, w, h):
    cam = dict(width=w, height=h, fx=0.58 * w, fy=0.58 * w, cx=w / 2 - 0.5, cy=h / 2 - 0.5)
    sm = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=int(np.ceil(np.sqrt(len(model)))) + 1))
    sm.upload_model(model)
    say(f"  {w} x {h}")
    for V in (1, 16):
        views = poses(16)[3:3 + V] if V == 1 else poses(V)
        for levels in (3, 5):
            fill_ms, render_ms, st = [], [], None
            for rep in range(WARM + REPS):
                sm.render_image_maps([], views, w, h, cam["fx"], cam["fy"], cam["cx"], cam["cy"], fill=dict(levels=levels), depth=True)
                if rep >= WARM:
                    st = sm.fill_stats()
                    fill_ms.append(st["device_ms"])
                    render_ms.append(sm.render_maps_stats()["device_ms"])
            P = w * h * V
            nbytes = stage_bytes(w, h, levels, V, st["filled"])
            t = med(fill_ms)
            say(f"    {V:2d} view(s), levels {levels}: completion {t * 1e3:8.1f} us in {st['launches']} launches ({t * 1e3 / st['launches']:6.1f} us each)"
                f" | render {med(render_ms) * 1e3:9.1f} us | {nbytes / 1e6:7.1f} MB = {nbytes / ROOF * 1e6:6.1f} us at the roof, {100.0 * nbytes / ROOF / (t * 1e-3):4.1f} % of it"
                f" | empty {100.0 * (P - st['valid']) / P:4.1f} %, seen through {st['seen_through']}, filled {100.0 * st['filled'] / P:4.1f} %, left {100.0 * st['left_empty'] / P:4.1f} %")
    sm.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    model = synth.seeded_model(N_SURFELS, 50, seed=2)
    probe(model, 1242, 375)
    probe(model, 1920, 1080)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
