#!/usr/bin/env python3
"""What the pose search costs, on one GPU, in one process; every figure the median of 5 after 2 warm-ups.

The scene of tests/test_loop.py (KITTI camera, 10 frames of old world paged back in, 6 young frames at true poses).  The search
centre is frame 10's true pose moved 0.9 m sideways, 0.7 m back and 2 degrees about the vertical; the window holds the old world.
Per level: the device time of the scoring kernels (k_search_samples + k_search_score between two events), the candidates, the
packed samples and the pair tests per second; then the whole sm_search_pose on the host clock with its four refinement tracks,
and next to it one young-window track.

Writes one text file (--out)."""
import argparse
import ctypes as C
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from surfelmapping_amd import capi, synth  # noqa: E402

WARM, REPS = 2, 5
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    return float(np.median(xs))


def write_map(path, rows, a, b):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes())
        f.write(np.array([a, b], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, np.float32).tobytes())


def samples(sm):
    f = sm._L.sm_debug_search_samples
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    n = C.c_uint32()
    sm._chk(f(sm._h, C.byref(n)), "sm_debug_search_samples")
    return int(n.value)


def probe(tmp, colour):
    cam = dict(synth.KITTI)
    poses = synth.kitti_trajectory(11)
    (seq,) = synth.make_sequences_parallel([(cam, poses, 0, 0.0, dict(seed=0, n_boxes=40))], workers=11)
    old = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    for fr in seq[:10]:
        old.process_frame(*fr)
    rows = old.download_model()
    old.close()
    f_path = os.path.join(tmp, "F.bin")
    write_map(f_path, rows, 0, 9)
    g = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    g.set_tick(400)
    for fr in seq[4:10]:
        g.process_frame(*fr)
    g.recall([f_path], pose=seq[9][3], mode="copy", radius=500.0)
    split = 406 - 1 - g.cfg.time_delta
    rgb, depth = (seq[10][0] if colour else None), seq[10][1]
    truth = poses[10].astype(np.float64)
    a = math.radians(2.0)
    D = np.eye(4)
    D[:3, :3] = [[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]
    D[:3, 3] = (0.9, 0.0, -0.7)
    centre = (truth @ D).astype(np.float32)
    what = "depth and colour" if colour else "depth alone"
    say(f"  kitti, {g.counts()['count']} surfels ({len(rows)} old), {what}:")
    prev_ms, prev_tests = 0.0, 0
    for levels in (1, 2):
        ms, tot, info, ns = [], [], None, 0
        for rep in range(WARM + REPS):
            pose, info = g.search_pose(depth, centre, rgb=rgb, max_time=split, search=dict(levels=levels), dist_thresh=0.5)
            ns = samples(g)
            if rep >= WARM:
                ms.append(info["score_ms"]); tot.append(info["total_ms"])
        l = levels - 1
        stride = max(1, 8 >> l)
        tests = info["candidates"][l] * ns
        lvl_ms = med(ms) - prev_ms
        et, er = np.linalg.norm(pose[:3, 3] - truth[:3, 3]), 0.0
        say(f"    level {l}: stride {stride}, {info['candidates'][l]} candidates x {ns} samples = {tests / 1e6:.1f} M pair tests, best score "
            f"{info['best_score'][l]}, score_ms {lvl_ms:.3f} ({tests / (lvl_ms * 1e-3) / 1e9:.1f} G pair tests/s)")
        say(f"    search of {levels} level(s): {info['status']}, rank {info['winner_rank']} wins with {info['track']['inliers']} inliers, "
            f"{et * 100:.2f} cm from the truth; score_ms {med(ms):.3f}, total_ms {med(tot):.3f}")
        prev_ms, prev_tests = med(ms), tests
    t_track = []
    for rep in range(WARM + REPS):
        t0 = time.perf_counter()
        if colour:
            _, ti = g.track_rgb_window(rgb, depth, split, 2 ** 31 - 1, guess=poses[10].astype(np.float32), dist_thresh=0.5)
        else:
            _, ti = g.track_window(depth, split, 2 ** 31 - 1, guess=poses[10].astype(np.float32), dist_thresh=0.5)
        if rep >= WARM:
            t_track.append((time.perf_counter() - t0) * 1e3)
    say(f"    one young-window track next to it: {med(t_track):.3f} ms ({ti['status']})")
    g.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    with tempfile.TemporaryDirectory() as tmp:
        probe(tmp, True)
        probe(tmp, False)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
