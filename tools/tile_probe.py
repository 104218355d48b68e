#!/usr/bin/env python3
"""What spatial tiling costs and what it gains, on one GPU, in one process; every time the median of 3 after 1
warm-up.

  The map: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the pipeline itself, saved as ONE
  map file (written in the order of the drive), and the same rows shuffled as a second file; a small second context works on them.
  Yardstick: one plain render_image_maps view of the file -- one streaming read of the same bytes.
  The call: tile_maps of each file (cell_mm 200, tile_shift 7, files of up to --file-records): the whole call and its parts.
  The sort alone: the device time of the radix passes (tile_stats()['sort_ms']) as records per second, against
  rocprim::radix_sort_pairs on the same (u64, u32) pairs in the same order (tools/tile_sort_yardstick.hip, built here if missing).
  The gain: 16 views along the drive of the shuffled file and of its tiling -- (block, view) pairs skipped of those tested and the
  call time; a recall(mode="count") at the middle of the drive on both -- files skipped and the call time.
File reads come from the page cache (the files are written just before they are read).  Writes one text file (--out)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from surfelmapping_amd import capi, synth  # noqa: E402
import tile_ref  # noqa: E402  (the restatement: the keys the yardstick sorts)

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


def write_map(path, rows, start_id, end_id):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes())
        f.write(np.array([start_id, end_id], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, np.float32).tobytes())


def yardstick(keys, tmp):
    exe = os.path.join(ROOT, "tools", "tile_sort_yardstick")
    if not os.path.exists(exe):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-o", exe, exe + ".hip"])
    path = os.path.join(tmp, "keys.bin")
    np.ascontiguousarray(keys, np.uint64).tofile(path)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        return None, (out.stdout + out.stderr).strip()
    return float(out.stdout.split(" ms ")[1].split()[0]), out.stdout.strip()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--file-records", type=int, default=1 << 16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tile_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    poses = synth.kitti_trajectory(a.frames)
    sm = capi.SurfelMap(capi.make_config(**CAM))
    for frame in synth.make_sequence(CAM, poses, seed=3):
        sm.process_frame(*frame)
    rows = sm.download_model()
    sm.close()
    n = len(rows)
    kw = dict(cell_mm=200, tile_shift=7, max_file_records=a.file_records)
    with tempfile.TemporaryDirectory() as tmp:
        drive, shuffled = os.path.join(tmp, "drive.bin"), os.path.join(tmp, "shuffled.bin")
        mixed = rows[np.random.RandomState(1).permutation(n)]
        write_map(drive, rows, 0, a.frames)
        write_map(shuffled, mixed, 0, a.frames)
        say(f"  {a.frames} frames at {W} x {H}: {n} surfels, {n / a.frames:.0f} per frame, {os.path.getsize(drive)} bytes per file")
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        view1 = np.stack([synth.pose_to_colmajor(poses[a.frames // 2])])
        _, t_yard = timed(lambda: sm.render_image_maps([drive], view1, *IMG, include_model=False))
        st = sm.render_maps_stats()
        say(f"  yardstick, one plain view of the file: {t_yard:8.1f} ms (read {st['read_ms']:.1f}, copy {st['copy_ms']:.1f}, device {st['device_ms']:.1f},"
            f" {st['chunks']} chunks)")

        # ---- the call
        sets = {}
        for name, path in (("drive order", drive), ("shuffled", shuffled)):
            parts = []

            def call():
                files = sm.tile_maps([path], os.path.join(tmp, name.split()[0]), **kw)
                parts.append(sm.tile_stats())
                return files
            files, t = timed(call)
            s = {k: float(np.median([p[k] for p in parts[WARM:]])) for k in ("device_ms", "sort_ms", "read_ms", "write_ms")}
            p = parts[-1]
            sets[name] = (files, p, s)
            say(f"  tile_maps, {name:11s}: call {t:8.1f} ms = {t / t_yard:5.2f} x the yardstick | read {s['read_ms']:7.1f} | device {s['device_ms']:7.1f}"
                f" (sort {s['sort_ms']:6.2f}) | write {s['write_ms']:7.1f} ms")
            say(f"    {p['placed']} placed, {p['loose']} loose, {p['tiles']} tiles, largest {p['largest_tile']}, {p['files_written']} files,"
                f" {p['readings']} readings, {p['chunks']} chunks, {p['launches']} launches, {p['sort_passes']} sort passes")
        assert [open(f, "rb").read() for f in sets["drive order"][0]] != [] and len(sets["drive order"][0]) == len(sets["shuffled"][0])

        # ---- the sort alone
        keys, placed = tile_ref.keys(mixed, kw["cell_mm"])
        keys = keys[placed]
        p, s = sets["shuffled"][1], sets["shuffled"][2]
        mine = p["placed"] / (s["sort_ms"] * 1e-3) if s["sort_ms"] > 0 else float("nan")
        say(f"  the sort alone, shuffled: {p['placed']} (u64, u32) pairs in {p['sort_passes']} passes of 8 bits: {s['sort_ms']:7.3f} ms ="
            f" {mine / 1e9:6.3f} G records/s")
        ms, text = yardstick(keys, tmp)
        if ms is None:
            say(f"    rocprim::radix_sort_pairs: NOT MEASURED ({text})")
        else:
            say(f"    rocprim::radix_sort_pairs, bits 0..50, same pairs: {ms:7.3f} ms = {len(keys) / (ms * 1e-3) / 1e9:6.3f} G records/s;"
                f" hand-written / rocprim = {s['sort_ms'] / ms:5.2f} x the time")

        # ---- the gain
        views = np.stack([synth.pose_to_colmajor(poses[k]) for k in np.linspace(0, a.frames - 1, 16).astype(int)])
        tiled = sets["shuffled"][0]
        images = {}
        for name, paths in (("shuffled", [shuffled]), ("tiled", tiled)):
            out, t = timed(lambda: sm.render_image_maps(paths, views, *IMG, include_model=False, depth=True))
            st = sm.render_maps_stats()
            images[name] = out
            say(f"  16 views, {name:8s}: call {t:8.1f} ms | pairs skipped {st['pairs_skipped']} of {st['pairs_tested']} tested"
                f" ({100.0 * st['pairs_skipped'] / max(st['pairs_tested'], 1):5.1f} %) | read {st['read_ms']:.1f}, device {st['device_ms']:.1f} ms")
        say(f"    depth images equal: {bool(np.array_equal(images['shuffled'][2], images['tiled'][2]))}")
        pose = synth.pose_to_colmajor(poses[a.frames // 2])
        for name, paths in (("shuffled", [shuffled]), ("tiled", tiled)):
            got, t = timed(lambda: sm.recall(paths, pose=pose, mode="count", radius=30.0))
            st = sm.recall_stats()
            say(f"  recall(count, radius 30 m), {name:8s}: {got} records | call {t:8.1f} ms | files skipped {st['files_skipped']} of {st['files_listed']},"
                f" read {st['files_read']}")
        sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
