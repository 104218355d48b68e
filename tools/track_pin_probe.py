#!/usr/bin/env python3
"""How far the colour tracker's pivot ratio moves when the 28 sums of its last system move within their summation bounds
(tests/test_track_pin.py pivot_tolerance; no GPU: the restatement on the CPU oracle's model).  Per solve shape and schedule:
the restatement's pivot ratio, the largest relative change over 32 draws of the signs, and the tolerance the test allows
(16 times that).  Its output is the first table of profiles/track_pin_probe.txt; the second one there is what the GPU test
printed on the MI355X.

    python tools/track_pin_probe.py > profiles/track_pin_probe.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                                                      # noqa: E402

import test_track_pin as tp                                             # noqa: E402
import track_pin_scenes as ps                                           # noqa: E402
import track_ref as tr                                                  # noqa: E402


def main():
    print("pivot ratio of sm_track_frame_rgb's last system under +- the entry bounds of its 28 sums (32 draws of the signs)")
    print("guess: the displaced true pose turned by 2 degrees; min_inliers W*H/16; rgb_weight 0.01")
    print(f"{'shape':>9} {'schedule':>9} {'levels':>12} {'inliers':>8} {'rgb':>7} {'pivot ratio':>13} {'largest bound/|sum|':>20} "
          f"{'spread':>10} {'tolerance':>10}")
    for W, H in ps.SOLVE_SHAPES:
        c = tp.cpu_case(W, H)
        for name, iters in tp.SCHEDULES.items():
            _, info = c.track_rgb(tp._guess(c, 2.0), min_inliers=tp._min_inliers(c), iters=iters)
            bound = tr.entry_bound(info["terms_icp"], info["terms_rgb"], tp.RGB_WEIGHT)
            spread = ps.spread_of_pivot_ratio(info["sys"], bound, np.asarray(c.t_prev, np.float64)[12:15])
            rel = (bound / np.abs(info["sys"][:28])).max()
            print(f"{W:>5}x{H:<3} {name:>9} {str(info['level_iterations'][:3]):>12} {info['inliers']:>8} {info['rgb_inliers']:>7} "
                  f"{info['pivot_ratio']:>13.6e} {rel:>20.3e} {spread:>10.3e} {16 * spread:>10.3e}")


if __name__ == "__main__":
    main()
