#!/usr/bin/env python3
"""What registering one map set against another costs and how well it lands, on one GPU, in one process; every
time the median of 3 after 1 warm-up.

  Two drives of the synthetic KITTI-shaped street at 1242 x 375, --frames (60) frames each, fused by the pipeline itself with
  5 mm of depth noise (different noise per drive), the second 0.3 m to the side of the first.  The second drive's poses are
  given in a world of its own -- the first's moved by the inverse of --offset (metres along x and z) and --yaw (degrees about
  the vertical) -- so registering its map (the source) onto the first's (the target) must return that motion.  Reported: the
  pose error against it, the iterations per level, register_stats, and per iteration the device time next to an estimate of
  the bytes it moves: per sample 32 bytes of position and normal, streamed, and eight probes of one 32-byte record each (a
  lower bound: a probe that walks on reads more), which fall on the occupied records of the level's table and the empty slots
  its missing neighbours hash to -- how few those are says whether the probes come from cache.
File reads come from the page cache.  Writes one text file (--out)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from surfelmapping_amd import capi, synth  # noqa: E402

WARM, REPS = 1, 3
W, H = 1242, 375
CAM = dict(width=W, height=H, fx=0.58 * W, fy=0.58 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def drive(poses_true, poses_given, seed, path):
    """the map of one drive: frames rendered at poses_true of the street, fused at poses_given"""
    sm = capi.SurfelMap(capi.make_config(**CAM))
    scene = synth.Scene(3)
    for (rgb, depth, sem, _), given in zip(synth.make_sequence(CAM, poses_true, seed=seed, noise_mm=5.0, scene=scene), poses_given):
        sm.process_frame(rgb, depth, sem, synth.pose_to_colmajor(given))
    n = sm.counts()["count"]
    sm.save_map(path, 0, len(poses_true))
    sm.close()
    return n


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--offset", type=float, nargs=2, default=[0.4, -0.3])
    ap.add_argument("--yaw", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    first = synth.kitti_trajectory(a.frames)
    second = [p @ synth.pose_matrix(0.3, 0.0, 0.0) for p in first]
    pivot = (0.0, 0.0, float(first[a.frames // 2][2, 3]))
    back = np.eye(4)
    back[:3, 3] = pivot
    truth = back @ synth.pose_matrix(a.offset[0], 0.0, a.offset[1], a.yaw) @ np.linalg.inv(back)       # about the pivot
    with tempfile.TemporaryDirectory() as tmp:
        tgt, src = os.path.join(tmp, "first.bin"), os.path.join(tmp, "second.bin")
        n_t = drive(first, first, 1, tgt)
        n_s = drive(second, [np.linalg.inv(truth) @ p for p in second], 2, src)
        say(f"  {a.frames} frames per drive at {W} x {H}: target {n_t} surfels, source {n_s}; truth {a.offset[0]} m, {a.offset[1]} m, {a.yaw} deg about {pivot}")
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        for levels in (3, 2):
            ts, out = [], None
            for rep in range(WARM + REPS):
                t0 = time.perf_counter()
                out = sm.register_maps([src], [tgt], pivot=pivot, levels=levels)
                if rep >= WARM:
                    ts.append((time.perf_counter() - t0) * 1e3)
            pose, info = out
            st = sm.register_stats()
            d = np.linalg.inv(truth) @ pose.astype(np.float64)
            rot = np.degrees(np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1)))
            iters = sum(info["iterations"])
            say(f"  levels {levels}: status {info['status']}, iterations {info['iterations']} (level 0 first), inliers {info['inliers']} of {info['samples']}"
                f" samples (stride {info['stride']}), rmse {info['rmse']:.4f} m, pivot ratio {info['pivot_ratio']:.3f}, cells {info['cells']}")
            say(f"    pose error {np.linalg.norm(pose[:3, 3] - truth[:3, 3]):.4f} m, {rot:.4f} deg | call {np.median(ts):8.1f} ms: read {st['read_ms']:.1f},"
                f" tables and samples {st['table_ms']:.2f}, iterations {st['iterate_ms']:.2f} ms in {st['launches']} launches, {st['chunks']} chunks")
            if iters:
                us = 1e3 * st["iterate_ms"] / iters
                stream, probes, occupied = info["samples"] * 32 / 1e6, info["samples"] * 8 * 32 / 1e6, max(info["cells"]) * 32 / 1e6
                say(f"    per iteration {us:8.1f} us (the {levels * 20 - iters} launch pairs after the end included): {stream:.1f} MB of samples streamed"
                    f" = {stream / us * 1e3:.0f} GB/s, and >= {probes:.1f} MB of probe reads that fall on at most {max(info['cells'])} occupied records"
                    f" ({occupied:.1f} MB) and the empty slots beside them")
        sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
