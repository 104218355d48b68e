"""Stereo depth through the drop-in facade (KittiReader with estimateDepth, SurfelMapping::setStereo / processFrameStereo,
tests/cpp/stereo_demo.cpp): a four-frame stereo dataset without depth files is mapped at the given poses, and tracked from the
second frame on -- the same model and the same poses, bit for bit, as the Python binding fed the numpy restatement's depths."""
import os
import subprocess

import numpy as np
import pytest

import kitti_fixture as kf
import retire_ref as rr
import stereo_fixture as sf
import stereo_ref as sr
import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
CAM = dict(width=256, height=96, fx=200.0, fy=200.0, cx=127.7, cy=48.2)
BASELINE, D, N = 0.54, 64, 4


def _build_demo(tmp_path):
    exe = str(tmp_path / "stereo_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "stereo_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-lz", "-Wl,-rpath," + LIBDIR])
    return exe


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def drive():
    """the frames (left, right, sem), the poses before the reader's offset, and the restatement's depth of every frame"""
    from surfelmapping_amd import synth
    scene, cam = synth.Scene(0), synth.Camera(**CAM)
    poses = [synth.pose_matrix(0.3, 0.0, 2.0 + 0.5 * k, 3.0) for k in range(N)]
    frames = []
    for p in poses:
        left, right, _, sem = synth.stereo_pair(scene, cam, p, BASELINE)
        frames.append((left, right, sem))
    depths = [sr.stereo(l, r, CAM["fx"], max_disp=D, baseline=BASELINE)["depth_mm"] for l, r, _ in frames]
    return frames, poses, depths


def test_stereo_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


def test_reader_without_the_right_images_reports_failure(tmp_path, drive):
    frames, poses, _ = drive
    root = str(tmp_path / "mono")
    sf.write_stereo_dataset(root, CAM, frames, poses, with_right=False)
    out = [str(tmp_path / n) for n in ("poses.bin", "depth.bin", "map.bin")]
    r = subprocess.run([_build_demo(tmp_path), root, str(N), str(BASELINE), str(D)] + out, capture_output=True, text=True)
    # the reader fails (good() false or getNext() false) before anything touches a GPU; no crash
    assert r.returncode == 3 and "reader:" in r.stdout and "image_3" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert not os.path.exists(out[2])


@pytest.mark.gpu
@pytest.mark.parametrize("given", [N, 1])
def test_facade_maps_a_stereo_drive_like_python(tmp_path, drive, given):
    from surfelmapping_amd import capi
    frames, poses, depths = drive
    root = str(tmp_path / "stereo")
    sf.write_stereo_dataset(root, CAM, frames, poses)
    assert not os.path.exists(os.path.join(root, "PSMNet"))
    out_poses, out_depth, out_map = (str(tmp_path / n) for n in ("poses.bin", "depth.bin", "map.bin"))
    r = subprocess.run([_build_demo(tmp_path), root, str(given), str(BASELINE), str(D), out_poses, out_depth, out_map],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    print(r.stdout)
    # through the binding: the left image and the restatement's depth, at the reader's poses / tracked
    m = capi.SurfelMap(capi.make_config(**CAM, preprocess=0))
    want = []
    for k, ((left, _, sem), depth) in enumerate(zip(frames, depths)):
        if k < given:
            p16 = kf.reader_pose(poses[k])
            m.process_frame(left, depth, sem, p16)
            want.append(p16)
        else:
            pose, _ = m.process_frame_tracked(left, depth, sem)
            want.append(tr.colmajor(pose))
    got = np.frombuffer(open(out_poses, "rb").read(), np.float32).reshape(N, 16)
    assert np.array_equal(_u32(got), _u32(np.array(want)))
    assert np.array_equal(np.frombuffer(open(out_depth, "rb").read(), np.uint16).reshape(depths[-1].shape), depths[-1])
    model = m.download_model()
    assert len(model) > 100
    assert np.array_equal(_u32(rr.read_map(out_map)[0]), _u32(model))
    assert f"tracked " in r.stdout and f" of {N - given}" in r.stdout
