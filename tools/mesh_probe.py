#!/usr/bin/env python3
"""What turning a map's surfels into a triangle mesh costs and what it gives, on one GPU, in one process; every
time the median of 3 after 1 warm-up.

  The map of tools/simplify_probe.py: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the
  pipeline itself, saved as ONE map file; a small second context streams it.  Per voxel_mm (50, 100, 200): mesh_maps of the file
  with the defaults otherwise, once with the mesh written to a PLY file and no rows brought back, once with nothing brought back
  at all (counts only: what the file and the copies cost is the difference) -- mesh_stats, the counts of cells, lattice points,
  cubes, vertices and faces, the open edges and the area.  Yardsticks, in the same run on the same file: segment_maps of the
  file, and one plain streamed view.  --only-mesh leaves the yardsticks and the second variant out (for a kernel trace).
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
    return (f"total_ms {st['total_ms']:.2f}: read_ms {st['read_ms']:.2f}, table_ms {st['table_ms']:.2f}, field_ms {st['field_ms']:.2f}, sort_ms"
            f" {st['sort_ms']:.2f}, emit_ms {st['emit_ms']:.2f}, write_ms {st['write_ms']:.2f} in {int(st['launches'])} launches, {int(st['chunks'])} chunks")


def shape(vertices, faces):
    """(open edges, area in m^2) of a mesh"""
    f = faces.astype(np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, count = np.unique(e[:, 0] << 32 | e[:, 1], return_counts=True)
    p = vertices["pos"].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]), axis=1).sum()
    return int((count == 1).sum()), float(area)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--voxels", type=int, nargs="*", default=[50, 100, 200])
    ap.add_argument("--only-mesh", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    poses = synth.kitti_trajectory(a.frames)
    sm = capi.SurfelMap(capi.make_config(**CAM))
    for frame in synth.make_sequence(CAM, poses, seed=3):
        sm.process_frame(*frame)
    n = sm.counts()["count"]
    with tempfile.TemporaryDirectory() as tmp:
        path, ply = os.path.join(tmp, "drive.bin"), os.path.join(tmp, "drive.ply")
        sm.save_map(path, 0, a.frames)
        sm.close()
        say(f"  {a.frames} frames at {W} x {H}: {n} surfels, {os.path.getsize(path)} bytes")
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        for mm in a.voxels:
            got, t, st = medians(lambda: sm.mesh_maps([path], voxel_mm=mm, ply_path=ply, max_vertices=0, max_faces=0), sm.mesh_stats)
            info = got["info"]
            say(f"  voxel_mm {mm:4d}: {info['records']} records in {info['cells']} cells, {info['lattice_points']} lattice points, {info['cubes']} cubes:"
                f" {info['vertices']} vertices, {info['faces']} faces; {info['counts']}")
            say(f"    to a PLY file of {os.path.getsize(ply)} bytes: call {t:8.1f} ms; {line(st)}")
            if a.only_mesh:
                continue
            _, t0, st0 = medians(lambda: sm.mesh_maps([path], voxel_mm=mm, max_vertices=0, max_faces=0), sm.mesh_stats)
            say(f"    counts only                      : call {t0:8.1f} ms; {line(st0)}")
            vertices, faces = capi.read_ply(ply)
            holes, area = shape(vertices, faces)
            say(f"    the mesh: {holes} open edges (the map's own border and its gaps), {area:.0f} m^2")
        if not a.only_mesh:
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
