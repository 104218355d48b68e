#!/usr/bin/env python3
"""How the origin of tests/test_compare.py's test_gpu_smallest_tables_with_wrap_around was found: a search on the CPU, with the
restatement's keys and the test's own functions, over the grid (0.37 i, 0.21 j, 0), i, j < --grid (40), for origins at which
the smallest tables of the test's reference have a fine key and a cover key carried past the last slot and every fine key of
the run at the end is the only support of some query record.  Prints, per cover_shift (3, then the test's), how many origins
have a carried cover key at all and the first --first (3) origins that meet everything.  Needs no GPU."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import compare_ref as cf  # noqa: E402
import test_compare as tc  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=40)
    ap.add_argument("--first", type=int, default=3)
    a = ap.parse_args()
    qry, ref, pose = tc._wrap_case(tc.street_case())
    for shift in (3, tc.WRAP["cover_shift"]):
        with_cover, found = 0, []
        for i in range(a.grid):
            for j in range(a.grid):
                params = dict(tc.WRAP, cover_shift=shift, origin=(0.37 * i, 0.21 * j, 0.0))
                t = tc.wrap_tables(ref, params)
                with_cover += t["carried"][1] >= 1
                if len(found) >= a.first or t["size"] != 2048 or min(t["carried"]) < 1:
                    continue
                want = cf.compare(qry, ref, pose, **params)
                if not tc.not_the_only_support(qry, ref, pose, params, t, want["labels"]) and all(c > 0 for c in want["counts"]):
                    found.append((i, j))
                    print(f"  cover_shift {shift}: origin (0.37 * {i}, 0.21 * {j}, 0): {len(t['fine'])} fine and {len(t['cover'])} cover keys,"
                          f" carried {t['carried']}, {len(t['at_the_end'])} fine keys in the run at the end, labels {want['counts']}")
        print(f"cover_shift {shift}: {with_cover} of {a.grid ** 2} origins have a cover key carried past the end of the table; {len(found)} shown")
