"""Routes for a car through the drop-in facade (SurfelMapping::routeCar, GlobalModel::routeCar; tests/cpp/car_demo.cpp).  CPU: the
caller compiles with plain g++ against the C-ABI only.  GPU: the fields and paths the demo prints are the restatements' -- ground_ref's
ground map of the same file, then car_ref's routes over it."""
import os
import subprocess

import numpy as np
import pytest

from surfelmapping_amd.capi import SmRouteCarParams  # noqa: F401  (the binding's symbol: without it nothing here can run)

import car_ref as cr
import ground_ref as gr
import recall_ref as rc
import route_ref as rr
from test_ground import random_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "car_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "car_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def printed(want):
    """what car_demo prints of two fields and their paths"""
    lines = []
    for f, i in enumerate(want["info"]):
        lines.append(f"car {f}: goals {i['goals_used']} dropped {i['goals_dropped']} states {i['reachable_states']} cells {i['reachable_cells']} max {i['max_cost']}")
        for k in ("cost", "next"):
            for h in range(8):
                lines += [f"{k} {f} {h} {r}: " + " ".join(str(int(v)) for v in row) for r, row in enumerate(want[k][f, h])]
    for s in range(len(want["path_len"])):
        words = want["path"][s, :want["path_len"][s]]
        lines.append(f"path {s}: cost {int(want['path_cost'][s])} words" + "".join(f" {int(w) & 0x3FFFFF}/{int(w) >> 22 & 7}/{int(w) >> 25}" for w in words))
    return "\n".join(lines) + "\nmodel: the same\n"


def test_car_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_routes_a_car_over_a_ground_map(tmp_path):
    exe = build_demo(tmp_path)
    rows = random_rows(900, 41, span=(2.4, 1.4))
    path = str(tmp_path / "a.bin")
    rc.write_map(path, rows)
    gkw = dict(cell_mm=100, nu=34, nv=22, reach_cells=5)     # the set and open (unknown) ground around it, where a car has room
    ground = gr.ground(rows, **gkw)
    ckw = dict(body_cells=1, turn_cells=1, turn_cost=4, reverse_weight=3, unknown_passable=1, max_steps=100)
    m = rr.multiplier(ground["state"], ground["clear2"], **ckw)
    gu, gv = 30, 18
    assert (m > 0).sum() > 400 and m[gv, gu] > 0
    goals = [[(gu, gv, -1)], [(gu, gv, 0)]]
    cost0 = cr.route_car(ground["state"], ground["clear2"], goals, **ckw)["cost"][0]
    sh, sv, su = (int(x) for x in np.argwhere(cost0 == cost0[cost0 != cr.NONE].max())[0])   # the start: the state farthest from the first goal
    want = cr.route_car(ground["state"], ground["clear2"], goals, starts=[(0, su, sv, sh), (1, su, sv, sh)], **ckw)
    assert want["info"][0]["reachable_cells"] > 400 and 5 <= want["path_len"].min() and want["path_len"].max() <= 100
    r = subprocess.run([exe, "100", "34", "22", "5", "1", "1", "4", "3", str(gu), str(gv), str(su), str(sv), str(sh), "100", path], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.startswith(printed(want)), r.stdout
    assert "routeCar: sm_route_car: a goal's heading outside -1..7" in r.stdout and "routeCar: no ground map" in r.stdout
