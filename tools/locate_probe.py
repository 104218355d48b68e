#!/usr/bin/env python3
"""What finding one map set in another without a guess costs and what it gives, on one GPU, in one process; every
time the median of 3 after 1 warm-up.

  The map of tools/simplify_probe.py: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the
  pipeline itself, saved as ONE map file: the target.  Two sources, each moved into a world of its own by the inverse of one
  truth (a yaw about the up axis, tens of metres, a height): a copy of the whole drive, and a 10-frame excerpt of it fused on its
  own.  Per cell_mm (250, 500, 1000): locate_maps with the defaults otherwise over a window that covers the target -- what it
  found against the truth, the split of locate_stats -- and the same call with SM_LOCATE_EXHAUSTIVE=1 where its 2^36 lookups admit
  it.  Yardsticks, in the same run on the same files: register_maps from the located pose, and one plain streamed view.
File reads come from the page cache (the files are written just before they are read).  Writes one text file (--out)."""
import argparse
import math
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
YAW_DEG, SHIFT = 143.0, (64.0, 0.75, -38.0)              # the truth: source world -> target world (up is -y: the yaw is about y)
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def medians(call, stats, reps=REPS, warm=WARM):
    ts, sts, out = [], [], None
    for rep in range(warm + reps):
        t0 = time.perf_counter()
        out = call()
        if rep >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
            sts.append(stats())
    return out, float(np.median(ts)), {k: float(np.median([s[k] for s in sts])) for k in sts[0]}


def fuse(poses, frames, seed=3):
    sm = capi.SurfelMap(capi.make_config(**CAM))
    for i, frame in enumerate(synth.make_sequence(CAM, poses, seed=seed)):
        if i in frames:
            sm.process_frame(*frame)
    rows = np.asarray(sm.download_model(), np.float32).reshape(-1, 12).copy()
    sm.close()
    return rows[np.isfinite(rows[:, :3]).all(axis=1)]


def truth():
    """4x4: x' = c x - s z, z' = s x + c z (the rotation sm_locate_maps' rows make for up = 3), then the shift"""
    c, s = math.cos(math.radians(YAW_DEG)), math.sin(math.radians(YAW_DEG))
    T = np.eye(4)
    T[:3, :3] = [[c, 0, -s], [0, 1, 0], [s, 0, c]]
    T[:3, 3] = SHIFT
    return T


def moved(rows, T):
    out = rows.copy()
    out[:, 0:3] = rows[:, 0:3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    out[:, 8:11] = rows[:, 8:11].astype(np.float64) @ T[:3, :3].T
    return out


def write_map(path, rows):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([0, 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, np.float32).tobytes())
    return path


def pose_error(T, want):
    d = np.linalg.inv(want) @ T.astype(np.float64)
    return float(np.linalg.norm(d[:3, 3])), math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0))))


def line(st):
    return (f"total_ms {st['total_ms']:.2f}: read_ms {st['read_ms']:.2f}, raster_ms {st['raster_ms']:.2f}, pyramid_ms {st['pyramid_ms']:.2f}, search_ms"
            f" {st['search_ms']:.2f}; {int(st['rounds'])} rounds, {int(st['nodes'])} nodes, {int(st['leaves'])} leaves, {int(st['levels'])} levels, range"
            f" {int(st['range'])}, {int(st['launches'])} launches")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--cells", type=int, nargs="*", default=[250, 500, 1000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    poses = synth.kitti_trajectory(a.frames)
    drive = fuse(poses, set(range(a.frames)))
    mid = a.frames // 2
    excerpt = fuse(poses, set(range(mid - 5, mid + 5)))
    T = truth()
    inv = np.linalg.inv(T)
    with tempfile.TemporaryDirectory() as tmp:
        target = os.path.join(tmp, "drive.bin")
        write_map(target, drive)
        sources = {}
        for name, rows in (("the drive's copy", drive), ("a 10-frame excerpt", excerpt)):
            sources[name] = (os.path.join(tmp, name.split()[-1] + ".bin"), moved(rows, inv))
            write_map(*sources[name])
        say(f"  {a.frames} frames at {W} x {H}: {len(drive)} surfels in the target, {len(excerpt)} in the excerpt; truth: yaw {YAW_DEG} degrees, shift {SHIFT}")
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        lo = np.floor(drive[:, [0, 2]].min(axis=0)) - 1.0
        hi = np.ceil(drive[:, [0, 2]].max(axis=0)) + 1.0
        pivot = tuple(float(v) for v in np.median(drive[:, :3], axis=0))
        for name, (path, rows) in sources.items():
            so = 0.5 * (rows[:, :3].min(axis=0) + rows[:, :3].max(axis=0))
            for mm in a.cells:
                n = np.ceil((hi - lo) * 1000.0 / mm).astype(int)
                kw = dict(cell_mm=mm, origin=(float(lo[0]), 0.0, float(lo[1])), nu=int(n[0]), nv=int(n[1]), source_origin=(float(round(so[0])), 0.0, float(round(so[2]))))
                got, t, st = medians(lambda: sm.locate_maps([path], [target], **kw), sm.locate_stats)
                i = got["info"]
                dt, dr = pose_error(got["pose"], T)
                say(f"  {name}, cell_mm {mm:4d}: {kw['nu']} x {kw['nv']} cells, n_s {i['n_s']}, {i['target_cells']} occupied: {i['status']}, yaw {i['yaw_deg']:.3f},"
                    f" score {i['score']} (coarse {i['coarse_score']}, runner-up {i['runner_up']}), {i['height_pairs']} height pairs, dh {i['dh'] / 65536.0:.3f} m;"
                    f" off the truth by {dt:.2f} m and {dr:.2f} degrees")
                say(f"    the search       : call {t:8.1f} ms; {line(st)}")
                os.environ["SM_LOCATE_EXHAUSTIVE"] = "1"
                try:
                    every, t1, st1 = medians(lambda: sm.locate_maps([path], [target], **kw), sm.locate_stats, reps=1, warm=0)
                    say(f"    exhaustive (once): call {t1:8.1f} ms; {line(st1)}")
                    say(f"    exhaustive / search: search_ms {st1['search_ms'] / max(st['search_ms'], 1e-6):.1f}; the same result: {every['info'] == i and np.array_equal(every['pose'], got['pose'])}")
                except capi.SurfelMapError as e:
                    say(f"    exhaustive       : refused ({str(e).split(': ')[-1]})")
                finally:
                    os.environ.pop("SM_LOCATE_EXHAUSTIVE", None)
                if i["status"] in ("OK", "AMBIGUOUS"):
                    (pose, info), t2, st2 = medians(lambda: sm.register_maps([path], [target], guess=got["pose"], pivot=pivot), sm.register_stats)
                    dt, dr = pose_error(pose, T)
                    say(f"    register_maps from the located pose: {info['status']}, off the truth by {dt:.3f} m and {dr:.3f} degrees; call {t2:.1f} ms = total_ms"
                        f" {st2['total_ms']:.2f}: read_ms {st2['read_ms']:.2f}, table_ms {st2['table_ms']:.2f}, iterate_ms {st2['iterate_ms']:.2f};"
                        f" locate / register: {t / max(t2, 1e-6):.2f}")
        views = np.stack([synth.pose_to_colmajor(poses[a.frames // 2])])
        _, t_view, st_view = medians(lambda: sm.render_image_maps([target], views, W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], include_model=False),
                                     sm.render_maps_stats)
        say(f"  yardstick, one plain streamed view of the target: call {t_view:.1f} ms (read {st_view['read_ms']:.1f}, device {st_view['device_ms']:.2f})")
        sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
