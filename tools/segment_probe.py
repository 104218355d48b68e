#!/usr/bin/env python3
"""What grouping a map's surfels into connected voxel components costs and what it finds, on one GPU, in one
process; every time the median of 3 after 1 warm-up.

  The map of tools/simplify_probe.py: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the
  pipeline itself, saved as ONE map file; a small second context streams it.  Per voxel_mm (100, 200, 400): segment_maps of the
  file with labels, with the defaults otherwise -- segment_stats, the counts, the largest components in metres -- and the same
  call with the reduce step's in-wave combination switched off (SM_SEGMENT_NO_COMBINE=1): link_ms covers link, flatten and
  reduce, so its difference is the combination's.  Then min_records 50 with the kept records written to a file.  Yardsticks, in
  the same run on the same file: compare_maps of the file against a copy of it, and one plain streamed view.
File reads come from the page cache (the files are written just before they are read).  Writes one text file (--out)."""
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
    return (f"total_ms {st['total_ms']:.2f}: read_ms {st['read_ms']:.2f}, table_ms {st['table_ms']:.2f}, link_ms {st['link_ms']:.3f}, label_ms"
            f" {st['label_ms']:.2f}, write_ms {st['write_ms']:.2f} in {int(st['launches'])} launches, {int(st['chunks'])} chunks")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--voxels", type=int, nargs="*", default=[100, 200, 400])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    poses = synth.kitti_trajectory(a.frames)
    sm = capi.SurfelMap(capi.make_config(**CAM))
    for frame in synth.make_sequence(CAM, poses, seed=3):
        sm.process_frame(*frame)
    n = sm.counts()["count"]
    with tempfile.TemporaryDirectory() as tmp:
        path, copy, kept = (os.path.join(tmp, f) for f in ("drive.bin", "copy.bin", "kept.bin"))
        sm.save_map(path, 0, a.frames)
        sm.close()
        shutil.copyfile(path, copy)
        say(f"  {a.frames} frames at {W} x {H}: {n} surfels, {os.path.getsize(path)} bytes")
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        for mm in a.voxels:
            row = {}
            for name, env in (("combine", "0"), ("no combine", "1")):
                os.environ["SM_SEGMENT_NO_COMBINE"] = env
                row[name] = medians(lambda: sm.segment_maps([path], voxel_mm=mm), sm.segment_stats)
            os.environ.pop("SM_SEGMENT_NO_COMBINE", None)
            (got, t, st), (alone, t1, st1) = row["combine"], row["no combine"]
            assert np.array_equal(got["labels"], alone["labels"]) and got["components"].tobytes() == alone["components"].tobytes(), "the combination changed the result"
            info = got["info"]
            say(f"  voxel_mm {mm:4d}: {info['records']} records in {info['cells']} cells: {info['components']} components, the largest of {info['largest']}"
                f" records; {info['counts']}")
            say(f"    combine   : call {t:8.1f} ms; {line(st)}")
            say(f"    no combine: call {t1:8.1f} ms; {line(st1)}")
            say(f"    link_ms with the combination / without: {st['link_ms'] / max(st1['link_ms'], 1e-6):.2f}")
            lo, hi, mean = capi.segment_boxes(got["components"], voxel_mm=mm)
            for i in np.argsort(-got["components"]["records"].astype(np.int64))[:3]:
                c = got["components"][i]
                say(f"      component {i}: class {c['cls']}, {c['records']} records in {c['cells']} cells, box {np.round(lo[i], 1).tolist()} .."
                    f" {np.round(hi[i], 1).tolist()} m, centroid {np.round(mean[i], 2).tolist()}")
            specks, t2, st2 = medians(lambda: sm.segment_maps([path], voxel_mm=mm, min_records=50, out_path=kept, labels=False), sm.segment_stats)
            say(f"    min_records 50, the kept records written: {specks['info']['components']} components, {specks['info']['small_components']} specks of"
                f" {specks['info']['counts']['SMALL']} records dropped, {specks['info']['written']} written; call {t2:.1f} ms; {line(st2)}")
        (lab, cmp_info), t_cmp, st_cmp = medians(lambda: sm.compare_maps([path], [copy]), sm.compare_stats)
        say(f"  yardstick, compare_maps of the file against a copy of it: call {t_cmp:.1f} ms = total_ms {st_cmp['total_ms']:.2f}: read_ms {st_cmp['read_ms']:.2f},"
            f" table_ms {st_cmp['table_ms']:.2f}, classify_ms {st_cmp['classify_ms']:.2f}, write_ms {st_cmp['write_ms']:.2f}")
        views = np.stack([synth.pose_to_colmajor(poses[a.frames // 2])])
        _, t_view, st_view = medians(lambda: sm.render_image_maps([path], views, W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], include_model=False),
                                     sm.render_maps_stats)
        say(f"  yardstick, one plain streamed view of the file: call {t_view:.1f} ms (read {st_view['read_ms']:.1f}, device {st_view['device_ms']:.2f})")
        sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
