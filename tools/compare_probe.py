#!/usr/bin/env python3
"""What telling the changes between two map sets costs and what it finds, on one GPU, in one process; every time
the median of 3 after 1 warm-up.

  The two drives of tools/register_probe.py -- the synthetic KITTI-shaped street at 1242 x 375, --frames (60) frames each, fused
  by the pipeline itself with 5 mm of depth noise, the second 0.3 m to the side of the first and in a world of its own -- with
  one box more beside the road in the second.  The second map is registered onto the first (register_maps, three levels) and
  then compared against it at the pose found (compare_maps, the CHANGED records written to a file), with the defaults and with
  cover cells of 3.2 m instead of 0.8 m.  Reported: compare_stats, the label counts, the share of the CHANGED records that lie
  on the added box (within 0.1 m of it, moved by the pose) and the labels of the box's records.  Beside them, on the same files: register_stats' table_ms, which builds three levels where this builds one and a
  table of keys, and one plain streamed view of the second map.  The reverse comparison's counts close the report.
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
EXTRA_BOX = (3.0, 0.05, 24.0, 4.8, 1.65, 28.0)            # lo, hi: clear of the scene's own boxes, right of the road
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def drive(scene, poses_true, poses_given, seed, path):
    """the map of one drive: frames rendered at poses_true of the scene, fused at poses_given"""
    sm = capi.SurfelMap(capi.make_config(**CAM))
    for (rgb, depth, sem, _), given in zip(synth.make_sequence(CAM, poses_true, seed=seed, noise_mm=5.0, scene=scene), poses_given):
        sm.process_frame(rgb, depth, sem, synth.pose_to_colmajor(given))
    n = sm.counts()["count"]
    sm.save_map(path, 0, len(poses_true))
    sm.close()
    return n


def read_rows(path):
    raw = np.fromfile(path, np.uint8)
    return raw[12:].view(np.float32).reshape(-1, 12)


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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--offset", type=float, nargs=2, default=[0.4, -0.3])
    ap.add_argument("--yaw", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    first = synth.kitti_trajectory(a.frames)
    second = [p @ synth.pose_matrix(0.3, 0.0, 0.0) for p in first]
    pivot = (0.0, 0.0, float(first[a.frames // 2][2, 3]))
    back = np.eye(4)
    back[:3, 3] = pivot
    truth = back @ synth.pose_matrix(a.offset[0], 0.0, a.offset[1], a.yaw) @ np.linalg.inv(back)       # about the pivot
    before, after = synth.Scene(3), synth.Scene(3)
    after.boxes = np.vstack([after.boxes, np.array(EXTRA_BOX)])
    with tempfile.TemporaryDirectory() as tmp:
        old, new, changed = (os.path.join(tmp, n) for n in ("first.bin", "second.bin", "changed.bin"))
        n_old = drive(before, first, first, 1, old)
        n_new = drive(after, second, [np.linalg.inv(truth) @ p for p in second], 2, new)
        say(f"  {a.frames} frames per drive at {W} x {H}: reference (first drive) {n_old} surfels, query (second drive, one box more) {n_new}")
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        (pose, reg), t_reg, st_reg = medians(lambda: sm.register_maps([new], [old], pivot=pivot), sm.register_stats)
        say(f"  register_maps: status {reg['status']}, pose error {np.linalg.norm(pose[:3, 3] - truth[:3, 3]):.4f} m | call {t_reg:.1f} ms,"
            f" table_ms {st_reg['table_ms']:.2f} (three levels, and the samples), read {st_reg['read_ms']:.1f}")
        rows = read_rows(new)
        P = pose.astype(np.float64)
        moved = rows[:, 0:3].astype(np.float64) @ P[:3, :3].T + P[:3, 3]
        lo, hi = np.array(EXTRA_BOX[:3]) - 0.1, np.array(EXTRA_BOX[3:]) + 0.1
        with np.errstate(invalid="ignore"):
            on_box = ((moved >= lo) & (moved <= hi)).all(axis=1)
        for shift in (3, 5):                             # cover cells of 0.8 m (the default) and of 3.2 m
            (lab, info), t_cmp, st = medians(lambda: sm.compare_maps([new], [old], pose=pose, out_path=changed, cover_shift=shift), sm.compare_stats)
            say(f"  compare_maps at that pose (voxel_mm 100, cover_shift {shift}, reach 2 cells, plane 50 mm, 30 deg): call {t_cmp:.1f} ms = total_ms"
                f" {st['total_ms']:.2f}: read_ms {st['read_ms']:.2f}, table_ms {st['table_ms']:.2f}, classify_ms {st['classify_ms']:.2f}, write_ms"
                f" {st['write_ms']:.2f} in {int(st['launches'])} launches, {int(st['chunks'])} chunks; cells fine {info['cells_fine']}, cover {info['cells_cover']}")
            say(f"    labels: {info['counts']}; written {info['written']} records")
            ch = lab == capi.SM_COMPARE_CHANGED
            box = np.bincount(lab[on_box], minlength=4)
            say(f"    of the {int(ch.sum())} CHANGED records {int((ch & on_box).sum())} lie on the added box ({100.0 * (ch & on_box).sum() / max(1, ch.sum()):.1f} %);"
                f" the box's {int(on_box.sum())} records: " + ", ".join(f"{capi.COMPARE_LABEL[l]} {int(box[l])}" for l in range(4)))
            assert len(read_rows(changed)) == info["written"] == int(ch.sum())
        views = np.stack([synth.pose_to_colmajor(np.linalg.inv(truth) @ second[a.frames // 2])])
        _, t_view, st_view = medians(lambda: sm.render_image_maps([new], views, W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], include_model=False),
                                     sm.render_maps_stats)
        say(f"  one plain streamed view of the query file: call {t_view:.1f} ms (read {st_view['read_ms']:.1f}, device {st_view['device_ms']:.2f})")
        _, rev = sm.compare_maps([old], [new], pose=np.linalg.inv(P).astype(np.float32), labels=False)
        say(f"  the reverse (first drive against second, the defaults): {rev['counts']}")
        say("  k_compare_classify was not traced: classify_ms is the event time around the labels, ranks and kept records of every chunk")
        sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
