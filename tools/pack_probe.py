#!/usr/bin/env python3
"""What packed map files cost and what they save, on one GPU, in one process; every time the median of 5 after 1 warm-up.

  The map of tools/ground_probe.py: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the pipeline
  itself, saved as ONE map file; a small second context packs it (pack_maps), unpacks it again (unpack_maps) and then makes the
  same calls on the plain file and on the packed one, alternating between the two: render_image_maps with 16 views, ground_maps at
  100 mm over the map's window, segment_maps at 100 mm.  Per call and set: the call's wall time and every time of its stats; the
  ratio packed / plain of the wall times; whether the two answers are the same bytes where the packed file decodes to the plain
  one (they are not expected to be: a packed block is lossy) and against the unpacked twin (expected).
  k_unpack's device time is unpack_ms of unpack_maps' stats, per full chunk of 2^20 records, and as (20 + 48) B x records / time
  against the 8 TB/s roof.
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

WARM, REPS = 1, 5
W, H = 1242, 375
CAM = dict(width=W, height=H, fx=0.58 * W, fy=0.58 * W, cx=W / 2 - 0.5, cy=H / 2 - 0.5)
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def alternating(calls, stats):
    """calls: {name: call}; REPS rounds after WARM, every round makes each call once, in turn.  {name: (last result, median wall
    ms, median of every stats field)}"""
    ts, sts, out = {k: [] for k in calls}, {k: [] for k in calls}, {}
    for rep in range(WARM + REPS):
        for name, call in calls.items():
            t0 = time.perf_counter()
            out[name] = call()
            if rep >= WARM:
                ts[name].append((time.perf_counter() - t0) * 1e3)
                sts[name].append(stats())
    return {k: (out[k], float(np.median(ts[k])), {f: float(np.median([s[f] for s in sts[k]])) for f in sts[k][0]}) for k in calls}


def times(st):
    return ", ".join(f"{k} {v:.2f}" for k, v in st.items() if k.endswith("_ms"))


def window(rows, cell_mm):
    """a window of cell_mm cells over the records' x and z, a metre to spare, its low corner on whole metres"""
    lo = np.floor(rows[:, [0, 2]].min(axis=0)) - 1.0
    hi = np.ceil(rows[:, [0, 2]].max(axis=0)) + 1.0
    n = np.ceil((hi - lo) * 1000.0 / cell_mm).astype(int)
    return dict(cell_mm=cell_mm, origin=(float(lo[0]), 0.0, float(lo[1])), nu=int(n[0]), nv=int(n[1]))


def same(a, b):
    if isinstance(a, dict):
        return all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_probe.txt"))
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
        # ---- packing and unpacking
        got = alternating(dict(pack=lambda: sm.pack_maps([path], os.path.join(tmp, "pk"))), sm.pack_stats)["pack"]
        packed, st = got[0][0], got[2]
        say(f"  pack_maps  : call {got[1]:8.1f} ms; {times(st)}; {int(st['chunks'])} chunks")
        say(f"    {int(st['blocks'])} blocks, raw_blocks {int(st['raw_blocks'])}; {int(st['bytes_in'])} -> {int(st['bytes_out'])} bytes: the packed file is"
            f" {st['bytes_out'] / st['bytes_in']:.4f} of the plain one (plain / packed {st['bytes_in'] / st['bytes_out']:.3f})")
        got = alternating(dict(unpack=lambda: sm.unpack_maps([packed], os.path.join(tmp, "un"))), sm.pack_stats)["unpack"]
        twin, st = got[0][0], got[2]
        say(f"  unpack_maps: call {got[1]:8.1f} ms; {times(st)}; {int(st['chunks'])} chunks")
        full = st["records"] / float(1 << 20)
        per_chunk = st["unpack_ms"] / full
        say(f"    k_unpack: {st['unpack_ms']:.3f} ms for {int(st['records'])} records = {per_chunk:.3f} ms per full chunk of 2^20; (20 + 48) B x records / time ="
            f" {68.0 * st['records'] / (st['unpack_ms'] * 1e-3) / 1e12:.2f} TB/s of the 8 TB/s roof")
        dec = capi.read_packed_map(packed)[0]
        plain_rows = np.fromfile(path, np.float32, offset=12).reshape(-1, 12)
        say(f"    largest position error of the packed file against the plain one: {np.abs(dec[:, :3].astype(np.float64) - plain_rows[:, :3]).max() * 1e3:.4f} mm")
        # ---- the readers, plain and packed alternating
        views = np.stack([synth.pose_to_colmajor(poses[(i * a.frames) // a.views]) for i in range(a.views)])
        win = window(rows, 100)
        cam = (W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])
        readers = (
            (f"render_image_maps, {a.views} views", lambda p: sm.render_image_maps([p], views, *cam, include_model=False), sm.render_maps_stats),
            ("ground_maps at 100 mm", lambda p: sm.ground_maps([p], **win), sm.ground_stats),
            ("segment_maps at 100 mm", lambda p: sm.segment_maps([p], voxel_mm=100), sm.segment_stats),
        )
        for name, call, stats in readers:
            got = alternating(dict(plain=lambda: call(path), packed=lambda: call(packed)), stats)
            for k in ("plain", "packed"):
                say(f"  {name}, {k:6s}: call {got[k][1]:8.1f} ms; {times(got[k][2])}")
            of_twin = call(twin)
            say(f"    packed / plain: call {got['packed'][1] / got['plain'][1]:.3f}, read_ms {got['packed'][2]['read_ms'] / max(got['plain'][2]['read_ms'], 1e-6):.3f};"
                f" the packed file's answer is its unpacked twin's: {same(got['packed'][0], of_twin)}; the plain file's: {same(got['packed'][0], got['plain'][0])}")
        sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
