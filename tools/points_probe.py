#!/usr/bin/env python3
"""What a point query into a map set costs, on one GPU; every figure the median of 3 after 1 warm-up call per shape.

  The map of the other probes: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the pipeline
  itself, saved as ONE map file.  16 poses along the drive and the 64 x 2048 beams of the lidar probe's sensor.
  a         the returns of the 16 sm_lidar_sweep_maps sweeps as points, each moved by a seeded normal jitter of 5 cm per axis, reach
            0.25 m, at cell_mm 250, 100 and 500: total, read, index, walk and device ms of the stats, ns of device time per point,
            probes and exact tests per point, the walks given up, the points that have a disc within reach
  b         as many seeded uniformly random points in the map's box, reach 1 m, at cell_mm 250
  c         SM_POINTS_NO_INDEX=1 on every 256th point of (a), in a child process under its own time limit
  d         sm_cast_rays_maps of as many beams (those that returned), at cell_mm 250
a, b and d run in this process, one after the other; file reads come from the page cache.  Writes a text file (--out)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1242, 375
CAM = dict(width=W, height=H, fx=0.58 * W, fy=0.58 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
WARM, REPS = 1, 3
N_POSES = 16


def repeat(fn, read):
    rows = []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        got = fn()
        ms = (time.perf_counter() - t0) * 1e3
        if k >= WARM:
            rows.append(dict(read(), host_ms=ms))
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}, got


def row_of(st, out, n, unit, device_part):
    return {unit + "s": n, "total_ms": st["total_ms"], "read_ms": st["read_ms"], "copy_ms": st["copy_ms"], "index_ms": st["index_ms"],
            device_part: st[device_part], "device_ms": st["device_ms"], "host_ms": st["host_ms"], "ns_per_" + unit: st["device_ms"] * 1e6 / n,
            "probes_per_" + unit: st["probes"] / n, "tests_per_" + unit: st["tests"] / n, "wide": int(st["wide"]), "pairs": int(st["pairs"]),
            "cells": int(st["cells"]), "records": int(st["records"]), "gave_up": int(st["gave_up"]), "chunks": int(st["chunks"]),
            "answered": int((out["id"] >= 0).sum())}


def query(sm, drive, pts, cell_mm):
    st, out = repeat(lambda: sm.query_points(pts, [drive], include_model=False, cell_mm=cell_mm, planes=()), sm.query_points_stats)
    return dict(row_of(st, out, len(pts), "point", "walk_ms"), cell_mm=cell_mm)


def child(src):
    from surfelmapping_amd import capi
    a = np.load(src)
    sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
    row = query(sm, str(a["drive"]), a["points"], 250)
    sm.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_probe.txt"))
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    from surfelmapping_amd import capi, synth
    lines = [__doc__.split("\n\n")[0]]

    def say(name, row):
        lines.append(f"{name} {json.dumps(row)}")
        print(lines[-1], flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        poses = synth.kitti_trajectory(a.frames)
        sm = capi.SurfelMap(capi.make_config(**CAM))
        for frame in synth.make_sequence(CAM, poses, seed=3):
            sm.process_frame(*frame)
        drive = os.path.join(tmp, "drive.bin")
        sm.save_map(drive, 0, a.frames)
        rows = np.asarray(sm.download_model(), np.float32).reshape(-1, 12)
        sm.close()
        vk = np.linspace(0, a.frames - 1, N_POSES).astype(int)
        p16 = np.stack([synth.pose_to_colmajor(poses[k]) for k in vk]).astype(np.float32)
        sn = capi.lidar_sensor(n_az=2048, az0_deg=-180.0, az_step_deg=360.0 / 2048, el_deg=np.linspace(-24.8, 2.0, 64), max_range=120.0)
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        sweep = sm.lidar_sweep_maps([drive], p16, sn, include_model=False)
        beams = np.concatenate([capi.lidar_rays(sn, p) for p in p16])
        hit = sweep["id"].reshape(-1) >= 0
        beams = np.ascontiguousarray(beams[hit])
        rng = np.random.default_rng(1)
        n = len(beams)
        surface = np.zeros((n, 4), np.float32)
        surface[:, 0:3] = beams[:, 0:3] + sweep["range"].reshape(-1)[hit, None] * beams[:, 4:7] + rng.normal(0.0, 0.05, (n, 3))
        surface[:, 3] = 0.25
        lo, hi = rows[:, 0:3].min(axis=0), rows[:, 0:3].max(axis=0)
        anywhere = np.zeros((n, 4), np.float32)
        anywhere[:, 0:3] = rng.uniform(lo, hi, (n, 3))
        anywhere[:, 3] = 1.0
        say("drive", dict(frames=a.frames, surfels=len(rows), bytes=os.path.getsize(drive), points=n, radius_median=float(np.median(np.abs(rows[:, 11]))),
                          radius_p99=float(np.quantile(np.abs(rows[:, 11]), 0.99))))
        for cell_mm in (250, 100, 500):
            say(f"a:{cell_mm}", query(sm, drive, surface, cell_mm))
        say("b:250", query(sm, drive, anywhere, 250))
        st, out = repeat(lambda: sm.cast_rays(beams, [drive], include_model=False, cell_mm=250), sm.cast_rays_stats)
        say("d:250", dict(row_of(st, out, n, "ray", "cast_ms"), cell_mm=250))
        sm.close()
        src = os.path.join(tmp, "sub.npz")
        np.savez(src, drive=drive, points=np.ascontiguousarray(surface[::256]))
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", src], capture_output=True, text=True,
                           env=dict(os.environ, SM_POINTS_NO_INDEX="1"))
        got = [l for l in r.stdout.splitlines() if l.startswith("ROW ")]
        if r.returncode != 0 or not got:
            lines.append(f"c: ended with status {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            print(lines[-1], flush=True)
        else:
            say("c:250", json.loads(got[-1][4:]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if lines[-1].startswith("c:250") else 1


if __name__ == "__main__":
    sys.exit(main())
