#!/usr/bin/env python3
"""What a lidar sweep costs, on one GPU, in one process; every figure the median of 5 after 2 warm-ups.

  resident  synth.seeded_model(n) uploaded, one sweep of a 2048 x 64 sensor (step 360/2048 degrees, el -24.8 .. 2) from the middle
            of the volume: device_ms of the stats, the exact tests per surfel, the share of surfels that went to a whole wave;
            next to it sm_render_image at 1242 x 375 of the same model from the same pose (host clock around the synchronous
            call: the nearest existing kernel of the same shape -- one lane per surfel, footprint loop, 64-bit atomicMin).
  maps      the same model cut into 16 map files, swept from 4 poses in one call with a small context: the split read / copy /
            device of the stats, next to sm_render_image_maps' for the same files and poses.
File reads come from the page cache (the files are written just before they are read).  Writes a text file (--out)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 2, 5
W, H = 1242, 375


def med(xs):
    return float(np.median(xs))


def repeat(fn, read):
    """medians of what read() returns (a dict of numbers) after each timed call, plus the host clock"""
    rows = []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t0) * 1e3
        if k >= WARM:
            rows.append(dict(read(), host_ms=ms))
    return {k: med([r[k] for r in rows]) for k in rows[0]}


def write_map(path, rows):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([0, 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, np.float32).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[6_000_000, 20_000_000])
    ap.add_argument("--files", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_probe.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from surfelmapping_amd import capi, synth
    sensor = capi.lidar_sensor(n_az=2048, az0_deg=-180.0, az_step_deg=360.0 / 2048, el_deg=np.linspace(-24.8, 2.0, 64), max_range=120.0)
    cam = dict(width=W, height=H, fx=0.58 * W, fy=0.58 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
    poses = np.stack([synth.pose_to_colmajor(synth.pose_matrix(5.0 * k, 0.0, 40.0 + 50.0 * k, 10.0 * k)) for k in range(4)])
    lines = [f"lidar_probe: medians of {REPS} after {WARM} warm-ups; sensor 2048 x 64, 1..120 m; render_image {W} x {H}"]
    for n in args.sizes:
        model = synth.seeded_model(n, 50, seed=2)
        side = int(np.ceil(np.sqrt(n))) + 1
        sm = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=side))
        sm.upload_model(model)
        sweep = repeat(lambda: sm.lidar_sweep(poses[1], sensor), sm.lidar_stats)
        out = sm.lidar_sweep(poses[1], sensor)
        render = repeat(lambda: sm.render_image(poses[1], W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"]), dict)
        row = dict(n=n, sweep_device_ms=sweep["device_ms"], sweep_total_ms=sweep["total_ms"], sweep_host_ms=sweep["host_ms"],
                   tests_per_surfel=sweep["tests"] / n, wide_share=sweep["wide"] / n, returns=int((out["id"] >= 0).sum()),
                   render_image_host_ms=render["host_ms"], sweep_over_render=sweep["host_ms"] / render["host_ms"])
        lines.append("resident " + json.dumps(row))
        print(lines[-1], flush=True)
        sm.close()
        with tempfile.TemporaryDirectory() as tmp:
            cuts = np.linspace(0, n, args.files + 1).astype(np.int64)
            paths = []
            for i in range(args.files):
                paths.append(os.path.join(tmp, f"part_{i:02d}.bin"))
                write_map(paths[-1], model[cuts[i]:cuts[i + 1]])
            small = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=10))
            keys = ("read_ms", "copy_ms", "device_ms", "total_ms")
            lid = repeat(lambda: small.lidar_sweep_maps(paths, poses, sensor, include_model=False), small.lidar_stats)
            img = repeat(lambda: small.render_image_maps(paths, poses, W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], include_model=False),
                         small.render_maps_stats)
            row = dict(n=n, files=args.files, sweeps=len(poses), lidar={k: lid[k] for k in keys}, lidar_blocks_skipped=lid["blocks_skipped"],
                       lidar_tests_per_surfel_sweep=lid["tests"] / (n * len(poses)), render_image_maps={k: img[k] for k in keys})
            lines.append("maps " + json.dumps(row))
            print(lines[-1], flush=True)
            small.close()
        del model
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
