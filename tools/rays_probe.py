#!/usr/bin/env python3
"""What a ray cast into a map set costs, on one GPU; every figure the median of 3 after 1 warm-up.

  The map of the other probes: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the pipeline
  itself, saved as ONE map file.  16 poses along the drive; per pose the 64 x 2048 beams of the lidar probe's sensor as rays
  (capi.lidar_rays: about 2.1 M rays), and as many uniformly random rays in the map's box (unit directions, t in [0, 120]).
  cast      sm_cast_rays_maps of the beams and of the random rays at cell_mm 100 / 250 / 500: total, read, index, cast and device
            ms of the stats, ns of device time per ray, probes and exact tests per ray, the wide records, the rays that return
  no_index  SM_RAYS_NO_INDEX=1 on every 64th ray of each list
  lidar     sm_lidar_sweep_maps over the same 16 poses and sensor (the grid-only way there was), and one plain streamed view
            (sm_render_image_maps of the first pose), next to the beams' cast at cell_mm 250: the ratio of the device times
  bench     bench.py --gpus 1 --steps 20 --warmup 5 (nothing it times calls this code), next to profiles/bench_r03_kitti_s20_w5.json
Every step is a child process under its own time limit; a step that fails or runs out of time ends the probe.  File reads come
from the page cache.  Writes a text file (--out)."""
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


def sensor_of(capi):
    return capi.lidar_sensor(n_az=2048, az0_deg=-180.0, az_step_deg=360.0 / 2048, el_deg=np.linspace(-24.8, 2.0, 64), max_range=120.0)


def repeat(fn, read):
    rows = []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        got = fn()
        ms = (time.perf_counter() - t0) * 1e3
        if k >= WARM:
            rows.append(dict(read(), host_ms=ms))
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}, got


def step_drive(tmp, frames):
    from surfelmapping_amd import capi, synth
    poses = synth.kitti_trajectory(frames)
    sm = capi.SurfelMap(capi.make_config(**CAM))
    for frame in synth.make_sequence(CAM, poses, seed=3):
        sm.process_frame(*frame)
    drive = os.path.join(tmp, "drive.bin")
    sm.save_map(drive, 0, frames)
    rows = np.asarray(sm.download_model(), np.float32).reshape(-1, 12)
    sm.close()
    vk = np.linspace(0, frames - 1, N_POSES).astype(int)
    p16 = np.stack([synth.pose_to_colmajor(poses[k]) for k in vk]).astype(np.float32)
    sn = sensor_of(capi)
    beams = np.concatenate([capi.lidar_rays(sn, p) for p in p16])
    rng = np.random.default_rng(1)
    lo, hi = rows[:, 0:3].min(axis=0), rows[:, 0:3].max(axis=0)
    rnd = np.zeros((len(beams), 8), np.float32)
    rnd[:, 0:3] = rng.uniform(lo, hi, (len(beams), 3))
    d = rng.normal(size=(len(beams), 3))
    rnd[:, 4:7] = d / np.linalg.norm(d, axis=1)[:, None]
    rnd[:, 7] = 120.0
    np.save(os.path.join(tmp, "poses.npy"), p16)
    np.save(os.path.join(tmp, "beams.npy"), beams)
    np.save(os.path.join(tmp, "random.npy"), rnd)
    return dict(frames=frames, surfels=len(rows), bytes=os.path.getsize(drive), rays=len(beams), radius_median=float(np.median(np.abs(rows[:, 11]))),
                radius_p99=float(np.quantile(np.abs(rows[:, 11]), 0.99)))


def step_cast(tmp, kind, cell_mm, no_index):
    from surfelmapping_amd import capi
    rays = np.load(os.path.join(tmp, kind + ".npy"))
    if no_index:
        rays = np.ascontiguousarray(rays[::64])
        os.environ["SM_RAYS_NO_INDEX"] = "1"
    sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
    st, out = repeat(lambda: sm.cast_rays(rays, [os.path.join(tmp, "drive.bin")], include_model=False, cell_mm=cell_mm), sm.cast_rays_stats)
    sm.close()
    n = len(rays)
    return dict(rays=n, cell_mm=cell_mm, no_index=int(no_index), total_ms=st["total_ms"], read_ms=st["read_ms"], copy_ms=st["copy_ms"],
                index_ms=st["index_ms"], cast_ms=st["cast_ms"], device_ms=st["device_ms"], host_ms=st["host_ms"], ns_per_ray=st["device_ms"] * 1e6 / n,
                probes_per_ray=st["probes"] / n, tests_per_ray=st["tests"] / n, wide=int(st["wide"]), pairs=int(st["pairs"]), cells=int(st["cells"]),
                records=int(st["records"]), no_slot=int(st["no_slot"]), gave_up=int(st["gave_up"]), chunks=int(st["chunks"]), returns=int((out["id"] >= 0).sum()))


def step_lidar(tmp):
    from surfelmapping_amd import capi
    p16 = np.load(os.path.join(tmp, "poses.npy"))
    drive = [os.path.join(tmp, "drive.bin")]
    sn = sensor_of(capi)
    sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
    lid, out = repeat(lambda: sm.lidar_sweep_maps(drive, p16, sn, include_model=False), sm.lidar_stats)
    img, _ = repeat(lambda: sm.render_image_maps(drive, p16[:1], W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], include_model=False), sm.render_maps_stats)
    sm.close()
    keys = ("read_ms", "copy_ms", "device_ms", "total_ms", "host_ms")
    return dict(sweeps=len(p16), lidar={k: lid[k] for k in keys}, lidar_tests_per_beam=lid["tests"] / (len(p16) * 64 * 2048),
                lidar_returns=int((out["id"] >= 0).sum()), one_view={k: img[k] for k in keys})


def step_bench():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True, check=True)
    now = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    with open(os.path.join(ROOT, "profiles", "bench_r03_kitti_s20_w5.json")) as f:
        text = f.read()
    before = json.loads(text) if text.lstrip().startswith("{") else json.loads([l for l in text.splitlines() if l.startswith("{")][-1])
    return dict(frames_per_s=now["value"], ms_per_step=now["ms_per_step"], recorded_frames_per_s=before.get("value"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays_probe.txt"))
    ap.add_argument("--step")
    ap.add_argument("--tmp")
    a = ap.parse_args()
    if a.step:                                               # a child: one step, one JSON line
        name, *rest = a.step.split(":")
        row = (step_drive(a.tmp, a.frames) if name == "drive" else step_bench() if name == "bench" else step_lidar(a.tmp) if name == "lidar" else
               step_cast(a.tmp, rest[0], int(rest[1]), name == "no_index"))
        print("ROW " + json.dumps(row), flush=True)
        return 0
    lines = [__doc__.split("\n\n")[0]]
    steps = [("drive", 300)] + [(f"cast:{kind}:{cell}", 240) for kind in ("beams", "random") for cell in (100, 250, 500)]
    steps += [("no_index:beams:250", 240), ("no_index:random:250", 240), ("lidar", 240), ("bench", 300)]
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in steps:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--frames", str(a.frames), "--step", name, "--tmp", tmp]
            r = subprocess.run(cmd, capture_output=True, text=True)
            got = [l for l in r.stdout.splitlines() if l.startswith("ROW ")]
            if r.returncode != 0 or not got:
                lines.append(f"{name}: ended with status {r.returncode}; the probe stops here\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
                print(lines[-1], flush=True)
                break
            rows[name] = json.loads(got[-1][4:])
            lines.append(f"{name} {got[-1][4:]}")
            print(lines[-1], flush=True)
    if "lidar" in rows and "cast:beams:250" in rows:
        c, l = rows["cast:beams:250"], rows["lidar"]["lidar"]
        lines.append(f"ratio: cast of the beams at cell_mm 250, device_ms {c['device_ms']:.3f} (index {c['index_ms']:.3f}, cast {c['cast_ms']:.3f}) against "
                     f"sm_lidar_sweep_maps device_ms {l['device_ms']:.3f}: x {c['device_ms'] / l['device_ms']:.2f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if len(rows) == len(steps) else 1


if __name__ == "__main__":
    sys.exit(main())
