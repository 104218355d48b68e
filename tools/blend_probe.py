#!/usr/bin/env python3
"""What blending the visible layer of a novel view costs, on one GPU, in one process; every time the median of 5
after 2 warm-ups.

  Two models at 1242 x 375: six frames of the synthetic street fused by the pipeline itself (a fused map: discs overlap
  everywhere; its last view is from 0.45 m above the road, where single discs cover thousands of pixels), and
  synth.seeded_model(2 M surfels) (random discs in a volume: many layers behind the front).  Per view: the wall time of
  render_image(depth=True) -- sm_render_image_ex -- and of the same call with blend= (the defaults, then falloff 0 and a
  band of 255 / 256), host copies included in both; the stage's own device time (blend_stats: the accumulate pass and the
  normalisation, events); contributions / drawn -- the fragments that pass the band test per drawn pixel, i.e. the atomics issued
  are four times that -- and changed / drawn, the share of drawn pixels whose colour is not the nearest disc's.

Writes one text file (--out)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from surfelmapping_amd import capi, synth  # noqa: E402

WARM, REPS = 2, 5
W, H = 1242, 375
CAM = dict(width=W, height=H, fx=0.58 * W, fy=0.58 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(call):
    ts = []
    for rep in range(WARM + REPS):
        t0 = time.perf_counter()
        call()
        if rep >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def probe(sm, name, views):
    say(f"  {name}: {sm.counts()['count']} surfels")
    cam = (W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])
    for k, v in enumerate(views):
        plain = timed(lambda: sm.render_image(v, *cam, depth=True))
        for p in (dict(), dict(falloff=0, depth_tol_256=255)):
            dev = []

            def call():
                sm.render_image(v, *cam, depth=True, blend=p)
                dev.append(sm.blend_stats()["device_ms"])
            t = timed(call)
            st = sm.blend_stats()
            d = max(st["drawn"], 1)
            bp = capi.blend_params(**p)
            say(f"    view {k}, tol {bp.depth_tol_256:3d} falloff {bp.falloff}: plain {plain * 1e3:8.1f} us | blended {t * 1e3:8.1f} us = {t / plain:4.2f} x"
                f" | stage {float(np.median(dev[WARM:])) * 1e3:8.1f} us in {st['launches']} launches | drawn {100.0 * st['drawn'] / (W * H):4.1f} %"
                f" | contributions / drawn {st['contributions'] / d:5.2f} | changed / drawn {100.0 * st['changed'] / d:4.1f} %")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blend_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    say(f"  {W} x {H}")
    poses = synth.kitti_trajectory(6)
    sm = capi.SurfelMap(capi.make_config(**CAM))
    for frame in synth.make_sequence(CAM, poses, seed=3):
        sm.process_frame(*frame)
    street = (poses[5], synth.pose_matrix(0.5, 0.0, 4.0), synth.pose_matrix(0.0, -1.0, 2.0, 8.0), synth.pose_matrix(0.0, 1.2, 4.0))
    probe(sm, "fused street, 6 frames", [synth.pose_to_colmajor(m) for m in street])
    sm.close()
    model = synth.seeded_model(2_000_000, 50, seed=2)
    sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=int(np.ceil(np.sqrt(len(model)))) + 1))
    sm.upload_model(model)
    probe(sm, "seeded volume", [synth.pose_to_colmajor(synth.pose_matrix(10.0 * np.sin(k), 0.0, -40.0 + 17.5 * k, 5.0 * np.cos(k))) for k in (3, 8)])
    sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
