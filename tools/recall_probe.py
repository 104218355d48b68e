#!/usr/bin/env python3
"""What paging in costs, on one GPU, in one process; every figure the median of 3 after 1 warm-up.

  sizes   synth.seeded_model(n) sorted along z and written as 1 and as 20 map files (so that a file is a slab of the map, as the
          files of a drive are); a pose in the middle and a radius chosen from the numpy definition so that about a third comes
          back.  sm_recall end to end (MOVE and COPY) with the split of sm_recall_stats, with the file index and (20 files)
          without it; and the route there is without the call, through the same build, asserted to give the same model and files:
          per file read_map + the numpy predicate, upload_model(concat(download_model(), rows)), the file rewritten from numpy.
          The files have just been written: every read is served by the page cache.
  frames  frames/s of 200 KITTI-shaped frames, device-resident: both policies off (three times: the spread) alternating with both
          on at every = 1000 (never fire), then every = 50 with retirement alone and with both.

Writes one text file (--out)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from surfelmapping_amd import capi, synth  # noqa: E402

WARM, REPS = 1, 3
LIVE = 1001
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def near(rows, c, radius):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = rows[:, 0] - c[0], rows[:, 1] - c[1], rows[:, 2] - c[2]
        return ((dx * dx + dy * dy) + dz * dz) <= np.float32(radius) * np.float32(radius)


def write_map(path, rows):
    with open(path, "wb") as f:
        f.write(np.array([len(rows), 0, 0], np.uint32).tobytes())
        f.write(rows.tobytes())


def read_map(path):
    raw = np.fromfile(path, np.uint8)
    return raw[12:].view(np.float32).reshape(-1, 12)


def med(xs):
    return float(np.median(xs))


def probe_size(sm, n, tmp):
    m = synth.seeded_model(n, 1000)
    m = m[np.argsort(m[:, 2], kind="stable")]
    live = synth.seeded_model(LIVE, 1000, seed=9)
    c = np.array([0.0, 1.0, 100.0], np.float32)
    pose = np.eye(4, dtype=np.float32).reshape(16).copy()
    pose[12:15] = c
    lo, hi = 1.0, 400.0
    for _ in range(30):                                  # the radius at which a third comes back
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if near(m, c, mid).sum() < n / 3 else (lo, mid)
    radius = float(np.float32(hi))
    k = near(m, c, radius)
    want_model = np.concatenate([live, m[k]])
    say(f"n {n}: radius {radius:.2f} m recalls {int(k.sum())} ({k.sum() / n:.3f})")
    for nf in (1, 20):
        cuts = [n * i // nf for i in range(nf + 1)]
        parts = [m[cuts[i]:cuts[i + 1]] for i in range(nf)]
        paths = [os.path.join(tmp, f"p{n}_{nf}_{i}.bin") for i in range(nf)]
        touched = [i for i in range(nf) if near(parts[i], c, radius).any()]

        def restore(which):
            for i in which:
                write_map(paths[i], parts[i])

        restore(range(nf))
        for mode, index in (("move", True), ("copy", True)) + ((("move", False), ("copy", False)) if nf > 1 else ()):
            os.environ["SM_RECALL_NO_INDEX"] = "0" if index else "1"
            ts, stats = [], []
            for rep in range(WARM + REPS):
                sm.upload_model(live)
                if index:                                # the index knows the files: a COUNT from afar has read them once
                    far = pose.copy()
                    far[12] = 1.0e6
                    sm.recall(paths, pose=far, mode="count", radius=1.0)
                t0 = time.perf_counter()
                got = sm.recall(paths, pose=pose, mode=mode, radius=radius)
                dt = (time.perf_counter() - t0) * 1e3
                assert got == int(k.sum())
                if rep == 0:
                    assert np.array_equal(sm.download_model().view(np.uint32), want_model.view(np.uint32)), "model differs"
                    if mode == "move":
                        for i in range(nf):
                            assert np.array_equal(read_map(paths[i]).view(np.uint32), parts[i][~near(parts[i], c, radius)].view(np.uint32)), paths[i]
                if mode == "move":
                    restore(touched)
                if rep >= WARM:
                    ts.append(dt)
                    stats.append(sm.recall_stats())
            s = {x: med([q[x] for q in stats]) for x in ("read_ms", "copy_ms", "device_ms", "write_ms", "total_ms")}
            q = stats[-1]
            say(f"  files {nf:2d} {mode} index {'on ' if index else 'off'}: sm_recall {med(ts):8.2f} ms  (read {s['read_ms']:.2f} copy {s['copy_ms']:.2f} "
                f"device {s['device_ms']:.2f} write {s['write_ms']:.2f} total {s['total_ms']:.2f}; files read {q['files_read']} skipped "
                f"{q['files_skipped']} rewritten {q['files_rewritten']} chunks {q['chunks']} records read {q['records_read']})")
        os.environ.pop("SM_RECALL_NO_INDEX", None)
        # the route without the call
        ts, parts_ms = [], []
        for rep in range(WARM + REPS):
            sm.upload_model(live)
            t0 = time.perf_counter()
            got, keep = [], {}
            for i, p in enumerate(paths):
                rows = read_map(p)
                kk = near(rows, c, radius)
                if kk.any():
                    got.append(rows[kk])
                    keep[i] = rows[~kk]
            t1 = time.perf_counter()
            sm.upload_model(np.concatenate([sm.download_model()] + got))
            t2 = time.perf_counter()
            for i, rows in keep.items():
                write_map(paths[i], rows)
            t3 = time.perf_counter()
            if rep == 0:
                assert np.array_equal(sm.download_model().view(np.uint32), want_model.view(np.uint32))
            restore(touched)
            if rep >= WARM:
                ts.append((t3 - t0) * 1e3)
                parts_ms.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        a, b, w = (med([x[i] for x in parts_ms]) for i in range(3))
        say(f"  files {nf:2d} route without the call (MOVE): {med(ts):8.2f} ms  (read_map + numpy predicate {a:.2f}, download + concat + upload {b:.2f}, "
            f"rewrite {w:.2f}; without the rewrite, as COPY: {a + b:.2f})")
        for p in paths:
            os.remove(p)


def probe_frames(frames, n_frames, tmp):
    import bench
    import retire_probe
    cam = synth.KITTI
    warm = retire_probe.FRAMES_WARM
    out = {}

    def run(name, every, recall=True):
        sm = capi.SurfelMap(capi.make_config(**cam))
        dp = bench.stage_frames(sm, frames, cam["width"] * cam["height"])
        if every:
            sm.set_auto_retire(every, os.path.join(tmp, name), min_age=20)
            if recall:
                sm.set_auto_recall(radius=capi.recall_params(sm.cfg).radius)
        for k in range(warm):
            sm.process_frame_device(*dp[k])
        sm.sync()
        t0 = time.perf_counter()
        for k in range(warm, warm + n_frames):
            sm.process_frame_device(*dp[k])
        sm.sync()
        dt = time.perf_counter() - t0
        out[name] = n_frames / dt
        say(f"  {name}: {n_frames / dt:8.1f} frames/s ({dt / n_frames * 1e6:.1f} us per frame), retirement files {sm.auto_retire_stats()}, "
            f"recalls {sm.auto_recall_stats()}, surfels at the end {sm.counts()['count']}")
        if every and sm.auto_recall_stats()[0]:
            q = sm.recall_stats()
            say(f"    its last recall: {q['total_ms']:.2f} ms (read {q['read_ms']:.2f} copy {q['copy_ms']:.2f} device {q['device_ms']:.2f} write "
                f"{q['write_ms']:.2f}), files listed {q['files_listed']} skipped {q['files_skipped']} read {q['files_read']}, records read {q['records_read']}")
        sm.close()

    run("warm_up_run", 0)
    for i in range(3):
        run(f"off_{i}", 0)
        run(f"every_1000_{i}", 1000)
    run("every_50_retirement_alone", 50, recall=False)
    run("every_50", 50)
    off = [out[f"off_{i}"] for i in range(3)]
    on = [out[f"every_1000_{i}"] for i in range(3)]
    say(f"  both off: median {med(off):.1f} (min {min(off):.1f} max {max(off):.1f}); both on, every 1000: median {med(on):.1f} "
        f"(min {min(on):.1f} max {max(on):.1f}), {(med(on) / med(off) - 1) * 100:+.2f} % against off; every 50: {out['every_50']:.1f} (retirement alone: {out['every_50_retirement_alone']:.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,8000000,20000000")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recall_mi355x.txt"))
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",") if x]
    frames = None
    if a.frames:
        import retire_probe
        frames = retire_probe.render_frames(a.frames, a.workers)
    say(__doc__.split("\n\n")[0])
    with tempfile.TemporaryDirectory(prefix="recall_probe_") as tmp:
        if sizes:
            sm = capi.SurfelMap(capi.make_config(**synth.HD))
            for n in sizes:
                probe_size(sm, n, tmp)
            sm.close()
        if a.frames:
            say(f"frames: {a.frames} KITTI-shaped frames after 5, sm_process_frame_device, frames staged in HBM, one wait at the end; "
                "policies: min_age 20, min_distance = radius = 1.5 * far_clip")
            probe_frames(frames, a.frames, tmp)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
