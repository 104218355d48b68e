#!/usr/bin/env python3
"""What voxel-cell simplification costs and what it leaves, on one GPU, in one process; every time the median of 3
after 1 warm-up.

  The map: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the pipeline itself, saved as ONE
  map file; a small second context streams it.  Yardstick: one plain render_image_maps view of that file -- one streaming read
  of the same bytes.  Per voxel_mm (20, 50, 100): simplify_maps of the file with and without the combine step
  (SM_SIMPLIFY_NO_COMBINE=1) -- records in and out, file bytes before and after, the device time of the two passes together,
  the read and the total time; then one plain and one blended view of the file before and of the file after, from two poses of
  the drive, and what the simplification changed in the plain view: the share of the pixels drawn in both whose label differs,
  the mean absolute colour difference over those pixels, and the pixels drawn in only one of the two.
File reads come from the page cache (the files are written just before they are read).  Writes one text file (--out)."""
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
IMG = (W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(call):
    out, ts = None, []
    for rep in range(WARM + REPS):
        t0 = time.perf_counter()
        out = call()
        if rep >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ts))


def views_of(sm, path, views):
    """(plain images, plain ms per view, blended ms per view) of the file"""
    plain, t_plain = timed(lambda: sm.render_image_maps([path], views, *IMG, include_model=False))
    _, t_blend = timed(lambda: sm.render_image_maps([path], views, *IMG, include_model=False, blend=True))
    return plain, t_plain / len(views), t_blend / len(views)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--voxels", type=int, nargs="*", default=[20, 50, 100])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    poses = synth.kitti_trajectory(a.frames)
    sm = capi.SurfelMap(capi.make_config(**CAM))
    for frame in synth.make_sequence(CAM, poses, seed=3):
        sm.process_frame(*frame)
    n = sm.counts()["count"]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "drive.bin")
        sm.save_map(path, 0, a.frames)
        sm.close()
        say(f"  {a.frames} frames at {W} x {H}: {n} surfels, {n / a.frames:.0f} per frame, {os.path.getsize(path)} bytes")
        views = np.stack([synth.pose_to_colmajor(poses[k]) for k in (a.frames // 2, a.frames - 1)])
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        _, t_yard = timed(lambda: sm.render_image_maps([path], views[:1], *IMG, include_model=False))
        st = sm.render_maps_stats()
        say(f"  yardstick, one plain view of the file: {t_yard:8.1f} ms (read {st['read_ms']:.1f}, copy {st['copy_ms']:.1f}, device {st['device_ms']:.1f},"
            f" {st['chunks']} chunks)")
        before, tb_plain, tb_blend = views_of(sm, path, views)
        say(f"  views of the file before: plain {tb_plain:8.1f} ms per view, blended {tb_blend:8.1f} ms per view")
        for mm in a.voxels:
            out = os.path.join(tmp, f"simplified_{mm}.bin")
            row = {}
            for name, env in (("combine", "0"), ("no combine", "1")):
                os.environ["SM_SIMPLIFY_NO_COMBINE"] = env
                dev = []

                def call():
                    s = sm.simplify_maps([path], out, voxel_mm=mm)
                    dev.append(s["device_ms"])
                    return s
                s, t = timed(call)
                row[name] = (s, t, float(np.median(dev[WARM:])), open(out, "rb").read() if name == "no combine" else None)
                if name == "combine":
                    kept = open(out, "rb").read()
            os.environ.pop("SM_SIMPLIFY_NO_COMBINE", None)
            assert kept == row["no combine"][3], "the combine step changed the result"
            s = row["combine"][0]
            say(f"  voxel_mm {mm:4d}: records {s['records_in']} -> {s['records_out']} ({100.0 * s['records_out'] / max(s['records_in'], 1):5.1f} %), bytes"
                f" {os.path.getsize(path)} -> {os.path.getsize(out)}, cells merged {s['cells_merged']}, largest {s['largest_cell']}, loose {s['loose']}")
            for name in ("combine", "no combine"):
                s, t, d, _ = row[name]
                say(f"    {name:10s}: both passes on the device {d:8.1f} ms in {s['launches']} launches, {s['chunks']} chunks | read {s['read_ms']:8.1f} ms"
                    f" | call {t:8.1f} ms = {t / t_yard:5.2f} x the yardstick")
            after, ta_plain, ta_blend = views_of(sm, out, views)
            say(f"    views of the file after: plain {ta_plain:8.1f} ms per view ({ta_plain / tb_plain:4.2f} x), blended {ta_blend:8.1f} ms per view"
                f" ({ta_blend / tb_blend:4.2f} x)")
            for k in range(len(views)):
                both = (before[1][k] != 0) & (after[1][k] != 0)
                only = int(((before[1][k] != 0) ^ (after[1][k] != 0)).sum())
                lab = float((before[1][k][both] != after[1][k][both]).mean()) if both.any() else 0.0
                col = float(np.abs(before[0][k][both].astype(np.int32) - after[0][k][both].astype(np.int32)).mean()) if both.any() else 0.0
                say(f"      view {k}: drawn in both {int(both.sum())} of {W * H}, in one only {only} | label changed {100.0 * lab:5.2f} % |"
                    f" mean |colour difference| {col:5.2f} of 255")
            os.remove(out)
        sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
