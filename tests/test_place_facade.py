"""Place recognition through the drop-in facade (SurfelMapping::setAutoPlace / saveKeyframes / loadKeyframes,
tests/cpp/place_demo.cpp): a second drive that starts 18 m and 5 degrees off in a world of its own loads the keyframes of the
drive that mapped the street, recognises the place from one frame without a pose and closes the loop -- the same closure, bit for
bit, as the same calls through the Python binding."""
import os
import struct
import subprocess

import numpy as np
import pytest

import place_ref as pr
import recall_ref as cr
import retire_ref as rr
import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
f32 = np.float32
CAM = pr.CAM
FIRST_TICK, RADIUS, N_OLD = 400, 500.0, 50


def _build_demo(tmp_path):
    exe = str(tmp_path / "place_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "place_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_place_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def _col(m44):
    return tr.colmajor(np.asarray(m44, np.float64).astype(f32))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _hex16(line):
    return np.array([float.fromhex(v) for v in line.split()[1:]], np.float64).astype(f32)


@pytest.mark.gpu
def test_facade_recognises_the_place_and_closes_the_loop(tmp_path):
    from surfelmapping_amd import capi
    frames = pr.drive()
    first = [k for k, f in enumerate(frames) if f["leg"] == "revisit"][0]
    # the first drive: out and away at the true poses; its model as a map file, its frames as keyframes
    over = dict(preprocess=0, max_sqrt_vertices=pr.CAPACITY)
    a = capi.SurfelMap(capi.make_config(**CAM, **over))
    for f in frames[:N_OLD]:
        a.process_frame(f["rgb"], f["depth"], f["sem"], _col(f["true"]))
    old_map, kf_path = str(tmp_path / "old.bin"), str(tmp_path / "keyframes.fern")
    cr.write_map(old_map, a.download_model(), 0, N_OLD - 1)
    p = pr.params()
    tab = pr.table(p, CAM["width"], CAM["height"])
    codes = np.stack([pr.encode(f["rgb"], f["depth"], p, tab) for f in frames[:N_OLD]])
    with open(kf_path, "wb") as fh:
        fh.write(pr.file_bytes(p, CAM["width"], CAM["height"], codes, np.stack([_col(f["true"]) for f in frames[:N_OLD]]), np.arange(N_OLD)))
    # the second drive: the way back, two frames in the old lane, and the frame that has no pose
    young = [f for f in frames[:first] if f["leg"] == "back"] + list(pr.settle_frames()) + [frames[first]]
    dump = str(tmp_path / "frames.bin")
    with open(dump, "wb") as fh:
        fh.write(struct.pack("<III4f", CAM["width"], CAM["height"], len(young), CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]))
        for f in young:
            fh.write(f["rgb"].tobytes() + f["depth"].tobytes() + f["sem"].tobytes() + _col(f["believed"]).tobytes())
    last = young[-1]
    truth = last["true"].astype(f32)
    # through the binding
    m = capi.SurfelMap(capi.make_config(**CAM, **over))
    m.set_tick(FIRST_TICK)
    for f in young[:-1]:
        m.process_frame(f["rgb"], f["depth"], f["sem"], _col(f["believed"]))
    n_old = m.recall([old_map], pose=_col(young[-2]["believed"]), mode="copy", radius=RADIUS)
    m.set_ferns()
    m.set_auto_place(every=1)
    m.fern_load(kf_path)
    pose, info = m.track_rgb(last["rgb"], last["depth"])
    st = m.auto_place_stats()
    et, er = tr.pose_error(pose, truth)
    print(f"binding: track {info['status']}, keyframe {st['last_k']} at {st['last_dis']} ferns, {st['last']['status']}, the pose {et * 100:.2f} cm and {er:.3f} deg from the truth")
    assert info["status"] == "OK" and (st["encoded"], st["matched"], st["attempts"], st["closed"]) == (1, 1, 1, 1), st
    assert abs(st["last_k"] - pr.REVISIT_OF[0]) <= 1 and et < 0.1 and er < 0.3
    m.process_frame(last["rgb"], last["depth"], last["sem"], tr.colmajor(pose))
    kf_out = str(tmp_path / "kf_binding.fern")
    m.fern_save(kf_out)
    # through the facade
    exe = _build_demo(tmp_path)
    out_kf, out_map = str(tmp_path / "kf_facade.fern"), str(tmp_path / "out.bin")
    r = subprocess.run([exe, dump, str(FIRST_TICK), old_map, str(RADIUS), kf_path, out_kf, out_map], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = {l.split()[0]: l for l in r.stdout.splitlines() if l.strip()}
    print(r.stdout)
    assert lines["recalled"].split()[1] == str(n_old)
    assert lines["encoded"].split() == ["encoded", "1", "added", str(st["added"]), "matched", "1", "attempts", "1", "closed", "1", "keyframe",
                                        str(st["last_k"]), "dis", str(st["last_dis"])]
    assert lines["status"].split()[:6] == ["status", "0", "t_a", str(st["last"]["t_a"]), "t_b", str(st["last"]["t_b"])]
    assert np.array_equal(_bits(_hex16(lines["D"])), _bits(tr.colmajor(st["last"]["D"])))
    assert np.array_equal(_bits(_hex16(lines["pose"])), _bits(tr.colmajor(pose)))
    assert open(out_kf, "rb").read() == open(kf_out, "rb").read()
    assert np.array_equal(_bits(rr.read_map(out_map)[0]), _bits(m.download_model()))
