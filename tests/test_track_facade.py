"""SurfelMapping::processFrame with a null gtPose in the drop-in facade (surfelmapping_amd/csrc/facade/SurfelMapping.h) tracks
the camera.  CPU: a caller compiles with plain g++ against the C-ABI only.  GPU: the poses it records equal, bit for bit,
SurfelMap.process_frame_tracked's, with processFrame synchronous and asynchronous (SM_FACADE_ASYNC)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "track_demo.cpp")
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "track_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC,
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_track_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.fixture(scope="module")
def kitti_seq():
    from surfelmapping_amd import synth
    cam = dict(synth.KITTI)
    poses = synth.kitti_trajectory(14)
    (seq,) = synth.make_sequences_parallel([(cam, poses, 1, 0.0, dict(seed=1, n_boxes=40))], workers=12)
    return cam, poses, seq


@pytest.mark.gpu
@pytest.mark.parametrize("facade_async", ["0", "1"])
def test_null_pose_tracks_like_python(tmp_path, facade_async, kitti_seq):
    import track_ref as tr
    from surfelmapping_amd import capi
    cam, poses, seq = kitti_seq
    frames = tmp_path / "frames.bin"
    with open(frames, "wb") as f:
        f.write(np.array([cam["width"], cam["height"], len(seq)], np.uint32).tobytes())
        f.write(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32).tobytes())
        for rgb, d, s, p in seq:
            f.write(rgb.tobytes()); f.write(d.tobytes()); f.write(s.tobytes()); f.write(p.astype(np.float32).tobytes())
    out_poses, out_map = tmp_path / "poses.bin", tmp_path / "map.bin"
    r = subprocess.run([build_demo(tmp_path), str(frames), "2", str(out_poses), str(out_map)], capture_output=True, text=True,
                       env=dict(os.environ, SM_FACADE_ASYNC=facade_async))
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.frombuffer(open(out_poses, "rb").read(), np.float32).reshape(len(seq), 16)
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    want = []
    for k, (rgb, d, s, p) in enumerate(seq):
        if k < 2:
            m.process_frame(rgb, d, s, p)
            want.append(p)
        else:
            pose, info = m.process_frame_tracked(rgb, d, s)
            want.append(tr.colmajor(pose))
    assert np.array_equal(got.view(np.uint32), np.array(want, np.float32).view(np.uint32))
    # the facade mapped the sequence end to end: every frame tracked, every pose near the truth
    for k in range(2, len(seq)):
        et, er = tr.pose_error(got[k].reshape(4, 4).T, poses[k])
        assert et < 0.05 and er < 0.25, (k, et, er, r.stdout)
    assert f"tracked {len(seq) - 2} of {len(seq) - 2}" in r.stdout, r.stdout
