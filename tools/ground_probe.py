#!/usr/bin/env python3
"""What turning a map's surfels into a planner's ground map costs and what it gives, on one GPU, in one process; every
time the median of 3 after 1 warm-up.

  The map of tools/simplify_probe.py: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the
  pipeline itself, saved as ONE map file; a small second context streams it.  Per cell_mm (50, 100, 200): ground_maps of the file
  over a window that covers the map's x and z, with the defaults otherwise -- the cells by state, the records by kind, the
  per-phase times of ground_stats -- and the same call with SM_GROUND_NO_COMBINE=1: the ratio is what the in-wave combination
  of runs saves.  Yardsticks, in the same run on the same file: segment_maps of the file, and one plain streamed view.
  --only-ground leaves the yardsticks and the second variant out (for a kernel trace).
File reads come from the page cache (the file is written just before it is read).  Writes one text file (--out)."""
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


def medians(call, stats):
    """(the last result, median wall ms, median of every stats field) of REPS calls after WARM"""
    ts, sts, out = [], [], None
    for rep in range(WARM + REPS):
        t0 = time.perf_counter()
        out = call()
        if rep >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
            sts.append(stats())
    return out, float(np.median(ts)), {k: float(np.median([s[k] for s in sts])) for k in sts[0]}


def line(st):
    return (f"total_ms {st['total_ms']:.2f}: read_ms {st['read_ms']:.2f}, ground_ms {st['ground_ms']:.2f}, fill_ms {st['fill_ms']:.2f}, accumulate_ms"
            f" {st['accumulate_ms']:.2f}, state_ms {st['state_ms']:.2f}, clear_ms {st['clear_ms']:.2f}, copy_ms {st['copy_ms']:.2f} in"
            f" {int(st['launches'])} launches, {int(st['chunks'])} chunks, {int(st['files_skipped'])} files skipped")


def window(rows, cell_mm):
    """a window of cell_mm cells over the records' x and z, a metre to spare, its low corner on whole metres"""
    lo = np.floor(rows[:, [0, 2]].min(axis=0)) - 1.0
    hi = np.ceil(rows[:, [0, 2]].max(axis=0)) + 1.0
    n = np.ceil((hi - lo) * 1000.0 / cell_mm).astype(int)
    return dict(cell_mm=cell_mm, origin=(float(lo[0]), 0.0, float(lo[1])), nu=int(n[0]), nv=int(n[1]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--cells", type=int, nargs="*", default=[50, 100, 200])
    ap.add_argument("--only-ground", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    poses = synth.kitti_trajectory(a.frames)
    sm = capi.SurfelMap(capi.make_config(**CAM))
    for frame in synth.make_sequence(CAM, poses, seed=3):
        sm.process_frame(*frame)
    n = sm.counts()["count"]
    rows = np.asarray(sm.download_model(), np.float32).reshape(-1, 12)
    rows = rows[np.isfinite(rows[:, :3]).all(axis=1)]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "drive.bin")
        sm.save_map(path, 0, a.frames)
        sm.close()
        say(f"  {a.frames} frames at {W} x {H}: {n} surfels, {os.path.getsize(path)} bytes")
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        for mm in a.cells:
            win = window(rows, mm)
            got, t, st = medians(lambda: sm.ground_maps([path], **win), sm.ground_stats)
            info = got["info"]
            say(f"  cell_mm {mm:4d}: {win['nu']} x {win['nv']} cells at origin {win['origin']}: {info['cells']}; {info['records']} records: {info['counts']}")
            free = got["state"] == 1
            say(f"    the road: {int((got['cls'][free] == 0).sum())} of {int(free.sum())} FREE cells are of class 0; the largest clearance of a FREE cell is"
                f" {np.sqrt(float(got['clear2'][free].max())) * mm / 1000.0 if free.any() else 0.0:.2f} m")
            say(f"    every plane back : call {t:8.1f} ms; {line(st)}")
            if a.only_ground:
                continue
            os.environ["SM_GROUND_NO_COMBINE"] = "1"
            try:
                alone, t1, st1 = medians(lambda: sm.ground_maps([path], **win), sm.ground_stats)
            finally:
                os.environ.pop("SM_GROUND_NO_COMBINE", None)
            same = all(np.array_equal(alone[k], got[k]) for k in capi.GROUND_PLANES) and alone["info"] == info
            say(f"    not combined     : call {t1:8.1f} ms; {line(st1)}")
            say(f"    not combined / combined: ground_ms {st1['ground_ms'] / max(st['ground_ms'], 1e-6):.2f}, accumulate_ms"
                f" {st1['accumulate_ms'] / max(st['accumulate_ms'], 1e-6):.2f}; the same planes and info: {same}")
            _, t2, st2 = medians(lambda: sm.ground_maps([path], planes=("state",), **win), sm.ground_stats)
            say(f"    the states alone : call {t2:8.1f} ms; {line(st2)}")
        if not a.only_ground:
            seg, t_seg, st_seg = medians(lambda: sm.segment_maps([path], voxel_mm=100), sm.segment_stats)
            say(f"  yardstick, segment_maps of the file at 100 mm: call {t_seg:.1f} ms = total_ms {st_seg['total_ms']:.2f}: read_ms {st_seg['read_ms']:.2f},"
                f" table_ms {st_seg['table_ms']:.2f}, link_ms {st_seg['link_ms']:.2f}, label_ms {st_seg['label_ms']:.2f}, write_ms {st_seg['write_ms']:.2f}")
            views = np.stack([synth.pose_to_colmajor(poses[a.frames // 2])])
            _, t_view, st_view = medians(lambda: sm.render_image_maps([path], views, W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], include_model=False),
                                         sm.render_maps_stats)
            say(f"  yardstick, one plain streamed view of the file: call {t_view:.1f} ms (read {st_view['read_ms']:.1f}, device {st_view['device_ms']:.2f})")
        sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
