#!/usr/bin/env python3
"""What moving actors cost in views and sweeps of a map set, on one GPU, in one process, warm and alternating.

  The map of the other probes: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the pipeline
  itself, saved as ONE map file.  sm_segment_maps labels it; the numbered component with the most records of the boxes' class is
  cut out, re-centred on the host and saved as the actor file; 8 copies of it drive along the street over 16 views and 16 sweeps
  (2048 x 64 beams).  Every figure is the median of --reps (5) alternating repetitions after one warm-up, with the spread (min ..
  max) behind it.
  (a) the scene call against the only path there was: per view, every actor's file copied, moved by sm_warp_by_time and drawn by
      a one-view sm_render_image_maps_ex with the copies behind the static file;
  (b) the scene call with zero actors against sm_render_image_maps_ex on the same views, next to the spread between two runs of
      the _maps call itself;
  (c) actor_ms per (record, view) against the device time the streamed kernels need per (record, view) for a file of as many
      records: per view, one file of all copies placed at THAT view's poses, drawn as the only file by a one-view call, the
      device_ms of the 16 calls summed (so the streamed kernels see the actors where the scene call sees them);
  (d) the same three for the sweep.
File reads come from the page cache.  Writes a text file (--out)."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from surfelmapping_amd import capi, synth  # noqa: E402

W, H = 1242, 375
CAM = dict(width=W, height=H, fx=0.58 * W, fy=0.58 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
IMG = (W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])
N_ACTORS, N_VIEWS = 8, 16
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def write_map(path, rows):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([0, 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, np.float32).tobytes())
    return path


def alternate(reps, **fns):
    """every fn once as a warm-up, then `reps` rounds in the given order: {name: (host ms per round, what fn returned per round)}"""
    out = {k: ([], []) for k in fns}
    for r in range(reps + 1):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            got = fn()
            ms = (time.perf_counter() - t0) * 1e3
            if r:
                out[k][0].append(ms)
                out[k][1].append(got)
    return out


def fmt(xs):
    return f"{np.median(xs):9.3f} ms ({min(xs):.3f} .. {max(xs):.3f})"


def rigid12(tx, ty, tz, yaw_deg):
    a = np.radians(yaw_deg)
    c, s = np.cos(a), np.sin(a)
    return np.array([c, 0, s, tx, 0, 1, 0, ty, -s, 0, c, tz], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    poses = synth.kitti_trajectory(a.frames)
    sm = capi.SurfelMap(capi.make_config(**CAM))
    for frame in synth.make_sequence(CAM, poses, seed=3):
        sm.process_frame(*frame)
    with tempfile.TemporaryDirectory() as tmp:
        drive = os.path.join(tmp, "drive.bin")
        sm.save_map(drive, 0, a.frames)
        rows = np.asarray(sm.download_model(), np.float32).reshape(-1, 12)
        sm.close()
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        seg = sm.segment_maps([drive])
        lab, cls = seg["labels"], rows[:, 4].view(np.uint32) >> 24
        numbered = lab < seg["info"]["components"]
        votes = np.bincount(lab[numbered & (cls == 13)], minlength=seg["info"]["components"])
        pick = int(np.argmax(votes))
        box = rows[lab == pick].copy()
        centre = box[:, 0:3].astype(np.float64).mean(axis=0)
        box[:, 0:3] = (box[:, 0:3].astype(np.float64) - centre).astype(np.float32)
        actor = write_map(os.path.join(tmp, "actor.bin"), box)
        say(f"  {a.frames} frames at {W} x {H}: {len(rows)} surfels, {os.path.getsize(drive)} bytes; component {pick} of {seg['info']['components']}:"
            f" {len(box)} records ({int(votes[pick])} of the boxes' class), centre {np.round(centre, 2).tolist()}")
        # 16 views along the first part of the drive; actor j drives ahead of the camera in its own lane, turning a little
        vk = np.linspace(0, min(a.frames - 1, 60), N_VIEWS).astype(int)
        views = np.stack([synth.pose_to_colmajor(poses[k]) for k in vk])
        y = float(centre[1])                                 # (re-centred at its mean: it stands on the road as it did)
        ap12 = [np.stack([rigid12(-4.5 + 9.0 * (j % 4) / 3.0, y, float(views[i][14]) + 8.0 + 5.0 * (j // 4) + 0.4 * i, 4.0 * j + i) for i in range(N_VIEWS)])
                for j in range(N_ACTORS)]
        actors = [(actor, p) for p in ap12]
        sensor = capi.lidar_sensor(n_az=2048, az0_deg=-180.0, az_step_deg=360.0 / 2048, el_deg=np.linspace(-24.8, 2.0, 64), max_range=120.0)

        def old_path(draw):
            for i in range(N_VIEWS):
                copies = []
                for j in range(N_ACTORS):
                    c = os.path.join(tmp, f"copy_{j}.bin")
                    shutil.copyfile(actor, c)
                    sm.warp_by_time([c], 0, ap12[j][i].reshape(1, 12), include_model=False)
                    copies.append(c)
                draw([drive] + copies, views[i:i + 1])

        image_old = lambda p, v: sm.render_image_maps(p, v, *IMG, include_model=False, fill=True, depth=True)
        sweep_old = lambda p, v: sm.lidar_sweep_maps(p, v, sensor, include_model=False)
        placed = [write_map(os.path.join(tmp, f"placed_{i}.bin"), np.concatenate([capi.scene_place_rows(p[i], box) for p in ap12])) for i in range(N_VIEWS)]

        for what, scene_call, maps_call, old, stats in (
                ("image", lambda acts: sm.render_scene([drive], acts, views, *IMG, include_model=False, fill=True, depth=True),
                 lambda p: sm.render_image_maps(p, views, *IMG, include_model=False, fill=True, depth=True), image_old, sm.render_maps_stats),
                ("lidar", lambda acts: sm.lidar_sweep_scene([drive], acts, views, sensor, include_model=False),
                 lambda p: sm.lidar_sweep_maps(p, views, sensor, include_model=False), sweep_old, sm.lidar_stats)):
            say(f"  -- {what}: {N_VIEWS} {'views' if what == 'image' else 'sweeps'}, {N_ACTORS} actors of {len(box)} records")
            r = alternate(a.reps, scene=lambda: (scene_call(actors), sm.scene_stats())[1], per_view=lambda: old_path(old))
            sc = r["scene"][1]
            say(f"  (a) scene call              : {fmt(r['scene'][0])}; load_ms {np.median([s['load_ms'] for s in sc]):.3f}, actor_ms {np.median([s['actor_ms'] for s in sc]):.3f},"
                f" pairs tested / skipped {sc[-1]['pairs_tested']} / {sc[-1]['pairs_skipped']}")
            say(f"      copy + warp + one view  : {fmt(r['per_view'][0])}; ratio {np.median(r['per_view'][0]) / np.median(r['scene'][0]):.1f}")
            r = alternate(a.reps, empty=lambda: scene_call([]), maps_1=lambda: maps_call([drive]), maps_2=lambda: maps_call([drive]))
            say(f"  (b) scene call, no actors   : {fmt(r['empty'][0])}")
            say(f"      the _maps call          : {fmt(r['maps_1'][0])}")
            say(f"      the _maps call again    : {fmt(r['maps_2'][0])}")
            r = alternate(a.reps, scene=lambda: (scene_call(actors), sm.scene_stats())[1], file=lambda: sum((old([placed[i]], views[i:i + 1]), stats()["device_ms"])[1] for i in range(N_VIEWS)))
            pairs = float(N_ACTORS * len(box) * N_VIEWS)
            am, dm = np.median([s["actor_ms"] for s in r["scene"][1]]), np.median(r["file"][1])
            say(f"  (c) actor_ms {am:.3f} = {am * 1e6 / pairs:.2f} ns per (record, view); a file of {N_ACTORS * len(box)} records per view through the streamed kernels:"
                f" device_ms {dm:.3f} over the {N_VIEWS} one-view calls = {dm * 1e6 / pairs:.2f} ns per (record, view)")
    sm.close()
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
