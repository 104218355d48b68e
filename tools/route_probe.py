#!/usr/bin/env python3
"""What cost-to-go fields and paths over a ground map cost, on one GPU, in one process; every time the median of 5
after 1 warm-up, with the smallest and the largest in brackets.

  Scene 1: the map of tools/ground_probe.py -- --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the
  pipeline itself, saved as ONE map file -- as a ground map at 100 mm (the ground_maps call is timed too, for scale); route_ground
  over its planes with G = 1, 16 and 256 goal sets of one goal each, spread along the road, and one start per field at the road's
  other end; `next` and the paths come back, the costs stay on the device.  Scene 2: a serpentine of 2048 x 2048 cells, walls in
  every 4th column open at alternating ends, one goal in a corner.  Per scene: rounds, tile visits, launches, the device time per
  phase and the call's time; the same with SM_ROUTE_SWEEPS=1 (one sweep per visit: the plain global relaxation) and with SM_ROUTE_TILE 16 and 64.  A run of the
  big serpentine with one sweep per visit is a million launches: it is made once, without warm-up.
Writes one text file (--out)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from surfelmapping_amd import capi, synth  # noqa: E402
from tools.ground_probe import CAM, H, W, window  # noqa: E402

WARM, REPS = 1, 5
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def measured(call, stats, warm=WARM, reps=REPS):
    """(the last result, (median, min, max) wall ms, median of every stats field) of `reps` calls after `warm`"""
    ts, sts, out = [], [], None
    for rep in range(warm + reps):
        t0 = time.perf_counter()
        out = call()
        if rep >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
            sts.append(stats())
    return out, (float(np.median(ts)), min(ts), max(ts)), {k: float(np.median([s[k] for s in sts])) for k in sts[0]}


def line(t, st):
    return (f"call {t[0]:9.2f} ms [{t[1]:.2f} .. {t[2]:.2f}]; total_ms {st['total_ms']:.2f}: prepare_ms {st['prepare_ms']:.2f}, relax_ms {st['relax_ms']:.2f},"
            f" next_ms {st['next_ms']:.2f}, walk_ms {st['walk_ms']:.2f}, copy_ms {st['copy_ms']:.2f}; {int(st['rounds'])} rounds, {int(st['tile_visits'])} tile"
            f" visits, {int(st['launches'])} launches (tile {int(st['tile'])}, sweep cap {int(st['sweep_cap'])})")


def variants(sm, name, ground, goals, starts, slow_once=False, **kw):
    """the default schedule, one sweep per visit, tiles of 16 and of 64: the same bits, different schedules"""
    base = None
    for what, env in (("default (tile 32)", {}), ("SM_ROUTE_SWEEPS=1", dict(SM_ROUTE_SWEEPS="1")), ("SM_ROUTE_TILE=16", dict(SM_ROUTE_TILE="16")),
                      ("SM_ROUTE_TILE=64", dict(SM_ROUTE_TILE="64"))):
        os.environ.update(env)
        try:
            once = slow_once and "SWEEPS" in what
            got, t, st = measured(lambda: capi.route_ground(sm, ground, goals, starts=starts, **kw), lambda: capi.route_stats(sm),
                                  warm=0 if once else WARM, reps=1 if once else REPS)
        finally:
            for k in env:
                os.environ.pop(k, None)
        if base is None:
            base = got
        same = all(np.array_equal(got[k], base[k]) for k in ("next", "path", "path_len", "path_cost")) and got["info"] == base["info"]
        say(f"    {name} {what:18s}: {line(t, st)}; the default's bits: {same}")
    return base


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--fields", type=int, nargs="*", default=[1, 16, 256])
    ap.add_argument("--serpentine", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_probe.txt"))
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
        say(f"  {a.frames} frames at {W} x {H}: {n} surfels")
        sm = capi.SurfelMap(capi.make_config(**CAM, preprocess=0, max_sqrt_vertices=10))
        win = window(rows, 100)
        ground, t, st = measured(lambda: sm.ground_maps([path], planes=("state", "clear2"), **win), sm.ground_stats)
    say(f"  scene 1: {win['nu']} x {win['nv']} cells of 100 mm: {ground['info']['cells']}")
    say(f"    for scale, the ground_maps call that made the planes: call {t[0]:.2f} ms [{t[1]:.2f} .. {t[2]:.2f}], total_ms {st['total_ms']:.2f}")
    kw = dict(body_cells=5, soft_cells=15, near_weight=8, max_steps=4096, max_rounds=1 << 22)
    passable = np.argwhere((ground["state"] == 1) & (ground["clear2"] >= 25))        # [v, u], in row order: along the road
    say(f"    body_cells 5, soft_cells 15, near_weight 8: {len(passable)} passable cells")
    for G in a.fields:
        picks = passable[np.linspace(0, len(passable) - 1, G + 2).astype(int)[1:-1]]
        goals = [[(int(u), int(v))] for v, u in picks]
        ends = (passable[-1], passable[0])                                     # a field's start: the end of the road farther from its goal
        starts = [(f, int(ends[2 * f >= G][1]), int(ends[2 * f >= G][0])) for f in range(G)]
        got = variants(sm, f"G = {G:3d}", ground, goals, starts, planes=("next",), **kw)
        say(f"      reachable cells per field: {min(i['reachable'] for i in got['info'])} .. {max(i['reachable'] for i in got['info'])}; path cells:"
            f" {int(got['path_len'].min())} .. {int(got['path_len'].max())}")
    S = a.serpentine
    state = np.ones((S, S), np.uint8)
    for i, u in enumerate(range(3, S - 1, 4)):
        state[:, u] = 2
        state[S - 1 if i % 2 == 0 else 0, u] = 1
    snake = dict(state=state, clear2=(state == 1).astype(np.uint32))
    say(f"  scene 2: a serpentine of {S} x {S} cells, one goal at (0, 0), one start at the far end")
    got = variants(sm, "serpentine", snake, [[(0, 0)]], [(0, S - 1, 0)], slow_once=True, planes=("next",), max_steps=64, max_rounds=1 << 22)
    say(f"      reachable cells: {got['info'][0]['reachable']}, the largest cost {got['info'][0]['max_cost']}")
    sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
