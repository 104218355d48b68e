#!/usr/bin/env python3
"""What routes a car can follow cost, on one GPU, in one process; every time the median of 5 after 1 warm-up, with
the smallest and the largest in brackets.

  The scene is tools/route_probe.py's first: --frames (100) frames of the synthetic KITTI-shaped street at 1242 x 375 fused by the
  pipeline itself, saved as ONE map file, as a ground map at 100 mm.  route_car over its planes with G = 1, 16 and 40 goal sets of
  one goal of any heading each, spread along the road, and one start per field at the road's other end, with turn_cells 4 and 16;
  `next` and the paths come back, the costs stay on the device.  In the same run, on the same planes and goal cells: route_ground,
  the yardstick, and the ratio of the two calls per field.  Per run: rounds, tile visits, launches, the device time per phase and
  the call's time; the same with SM_CAR_SWEEPS=1 (one sweep per visit) and with SM_CAR_TILE=16 where turn_cells admits it.
Writes one text file (--out)."""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from surfelmapping_amd import capi, synth  # noqa: E402
from tools.ground_probe import CAM, H, W, window  # noqa: E402
from tools.route_probe import LINES, line, measured, say  # noqa: E402


def variants(sm, name, ground, goals, starts, turn_cells, **kw):
    """the default schedule, one sweep per visit, tiles of 16: the same bits, different schedules; -> (the default's result, its time)"""
    base = t_base = None
    for what, env in (("default (tile 32)", {}), ("SM_CAR_SWEEPS=1", dict(SM_CAR_SWEEPS="1")), ("SM_CAR_TILE=16", dict(SM_CAR_TILE="16"))):
        if "TILE" in what and turn_cells > 8:
            continue
        os.environ.update(env)
        try:
            got, t, st = measured(lambda: capi.route_car(sm, ground, goals, starts=starts, turn_cells=turn_cells, **kw), lambda: capi.route_car_stats(sm))
        finally:
            for k in env:
                os.environ.pop(k, None)
        if base is None:
            base, t_base = got, t
        same = all(np.array_equal(got[k], base[k]) for k in ("next", "path", "path_len", "path_cost")) and got["info"] == base["info"]
        say(f"    {name} {what:18s}: {line(t, st)}; the default's bits: {same}")
    return base, t_base


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--fields", type=int, nargs="*", default=[1, 16, 40])
    ap.add_argument("--turn-cells", type=int, nargs="*", default=[4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "car_probe.txt"))
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
        ground = sm.ground_maps([path], planes=("state", "clear2"), **win)
    say(f"  {win['nu']} x {win['nv']} cells of 100 mm: {ground['info']['cells']}")
    cells = dict(body_cells=5, soft_cells=15, near_weight=8, max_rounds=1 << 22)
    passable = np.argwhere((ground["state"] == 1) & (ground["clear2"] >= 25))        # [v, u], in row order: along the road
    say(f"    body_cells 5, soft_cells 15, near_weight 8: {len(passable)} passable cells; turn_cost 0, reverse_weight 0")
    for G in a.fields:
        picks = passable[np.linspace(0, len(passable) - 1, G + 2).astype(int)[1:-1]]
        ends = (passable[-1], passable[0])                                     # a field's start: the end of the road farther from its goal
        far = [ends[2 * f >= G] for f in range(G)]
        got, t_route, st = measured(lambda: capi.route_ground(sm, ground, [[(int(u), int(v))] for v, u in picks],
                                                              starts=[(f, int(far[f][1]), int(far[f][0])) for f in range(G)], planes=("next",), max_steps=4096, **cells),
                                    lambda: capi.route_stats(sm))
        say(f"    G = {G:3d} route_ground, the yardstick: {line(t_route, st)}")
        for tc in a.turn_cells:
            # the start's heading: along the road towards the goal (the road runs along v: heading 2 is +v, 6 is -v)
            starts = [(f, int(far[f][1]), int(far[f][0]), 2 if picks[f][0] > far[f][0] else 6) for f in range(G)]
            goals = [[(int(u), int(v), -1)] for v, u in picks]
            got, t_car = variants(sm, f"G = {G:3d} turn_cells {tc:2d}", ground, goals, starts, tc, planes=("next",),
                                  max_steps=4096, **cells)
            say(f"      reachable states per field: {min(i['reachable_states'] for i in got['info'])} .. {max(i['reachable_states'] for i in got['info'])},"
                f" cells {min(i['reachable_cells'] for i in got['info'])} .. {max(i['reachable_cells'] for i in got['info'])}; path words:"
                f" {int(got['path_len'].min())} .. {int(got['path_len'].max())}; car / route: {t_car[0] / t_route[0]:.1f} (per field {t_car[0] / G:.2f} ms"
                f" against {t_route[0] / G:.2f} ms)")
    sm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
