"""Routes through the drop-in facade (SurfelMapping::routeGround, GlobalModel::routeGround; tests/cpp/route_demo.cpp).  CPU: the
caller compiles with plain g++ against the C-ABI only.  GPU: the fields and paths the demo prints are the restatements' -- ground_ref's
ground map of the same file, then route_ref's routes over it."""
import os
import subprocess

import numpy as np
import pytest

from surfelmapping_amd.capi import SmRouteParams  # noqa: F401  (the binding's symbol: without it nothing here can run)

import ground_ref as gr
import recall_ref as cr
import route_ref as rr
from test_ground import random_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "route_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "route_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def printed(want):
    """what route_demo prints of two fields and their paths"""
    lines = []
    for f, i in enumerate(want["info"]):
        lines.append(f"route {f}: goals {i['goals_used']} dropped {i['goals_dropped']} reachable {i['reachable']} max {i['max_cost']}")
        for k in ("cost", "next"):
            lines += [f"{k} {f} {r}: " + " ".join(str(int(v)) for v in row) for r, row in enumerate(want[k][f])]
    for s in range(len(want["path_len"])):
        cells = want["path"][s, :want["path_len"][s]]
        lines.append(f"path {s}: cost {int(want['path_cost'][s])} cells" + "".join(f" {int(c)}" for c in cells))
    return "\n".join(lines) + "\nmodel: the same\n"


def test_route_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_routes_over_a_ground_map(tmp_path):
    exe = build_demo(tmp_path)
    rows = random_rows(900, 41, span=(2.4, 1.4))
    path = str(tmp_path / "a.bin")
    cr.write_map(path, rows)
    gkw = dict(cell_mm=100, nu=26, nv=16, reach_cells=5)
    ground = gr.ground(rows, **gkw)
    rkw = dict(body_cells=1, soft_cells=3, near_weight=9, unknown_passable=1, max_steps=12)
    m = rr.multiplier(ground["state"], ground["clear2"], **rkw)
    free = np.argwhere(m > 0)
    assert len(free) > 40
    gv, gu = free[0]
    goals = [[(int(gu), int(gv))], [(int(gu), int(gv)), (25, 15)]]
    cost0 = rr.route(ground["state"], ground["clear2"], goals, **rkw)["cost"][0]
    sv, su = np.argwhere(cost0 == cost0[cost0 != rr.NONE].max())[0]           # the start: the cell farthest from the first goal
    want = rr.route(ground["state"], ground["clear2"], goals, starts=[(0, int(su), int(sv)), (1, int(su), int(sv))], **rkw)
    assert want["info"][0]["reachable"] > 20 and want["path_len"].min() >= 5
    r = subprocess.run([exe, "100", "26", "16", "5", "1", "3", "9", str(gu), str(gv), str(su), str(sv), "12", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.startswith(printed(want)), r.stdout
    assert "routeGround: sm_route_ground: a goal outside the window" in r.stdout and "routeGround: no ground map" in r.stdout
