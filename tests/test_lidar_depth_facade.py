"""Lidar depth through the drop-in facade (KittiReader::setUseLidar, SurfelMapping::setLidarDepth / processFrameLidar,
tests/cpp/lidar_depth_demo.cpp): a three-frame dataset with velodyne scans and no depth files is mapped at the given poses -- the
same model and the same last depth image, bit for bit, as the Python binding fed the numpy restatement's depths."""
import os
import subprocess

import numpy as np
import pytest

import kitti_fixture as kf
import lidar_depth_ref as lr
import retire_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")
CAM = dict(width=256, height=96, fx=200.0, fy=200.0, cx=127.7, cy=48.2)
N, LARGE = 3, 15
f32 = np.float32


def _build_demo(tmp_path):
    exe = str(tmp_path / "lidar_depth_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lidar_depth_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-lz", "-Wl,-rpath," + LIBDIR])
    return exe


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def write_lidar_dataset(root, frames, poses, with_scans=True, with_transform=True):
    """frames: [(rgb, points, sem)]; the KITTI layout without PSMNet/, with velodyne/%06d.bin and velo_to_cam.txt (12 floats)"""
    for d in ("image_2", "semantics", "velodyne"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    with open(os.path.join(root, "calibration.txt"), "w") as f:
        f.write(f"{CAM['fx']} {CAM['fy']} {CAM['cx']} {CAM['cy']}\n{CAM['width']} {CAM['height']}\n")
    with open(os.path.join(root, "times.txt"), "w") as f:
        f.writelines(f"{0.1 * k:.6f}\n" for k in range(len(frames)))
    with open(os.path.join(root, "pose.txt"), "w") as f:
        for p in poses:
            f.write(" ".join(f"{v:.9g}" for v in np.asarray(p, f32)[:3, :].reshape(-1)) + "\n")
    if with_transform:
        with open(os.path.join(root, "velo_to_cam.txt"), "w") as f:
            f.write(" ".join(f"{v:.9g}" for v in lr.T_STREET[:3].reshape(-1)) + "\n")
    for k, (rgb, pts, sem) in enumerate(frames):
        kf.write_png(os.path.join(root, "image_2", f"{k:06d}.png"), rgb)
        kf.write_png(os.path.join(root, "semantics", f"{k:06d}.png"), sem)
        if with_scans:
            np.ascontiguousarray(pts, f32).tofile(os.path.join(root, "velodyne", f"{k:06d}.bin"))


@pytest.fixture(scope="module")
def drive():
    """the frames (rgb, scan, sem) and the poses before the reader's offset; the scan is every 3rd pixel of every 2nd row of the
    synthetic depth image, in a lidar frame that T_STREET maps to the camera's"""
    from surfelmapping_amd import synth
    poses = [synth.pose_matrix(0.3, 0.0, 2.0 + 0.5 * k, 3.0) for k in range(N)]
    frames = []
    for rgb, depth, sem, _ in synth.make_sequence(CAM, poses, seed=0):
        v, u = np.nonzero(depth[::2, ::3])
        v, u = v * 2, u * 3
        Z = depth[v, u].astype(np.float64) / 1000.0
        pc = np.stack([(u - CAM["cx"]) * Z / CAM["fx"], (v - CAM["cy"]) * Z / CAM["fy"], Z], axis=1)
        pts = np.concatenate([pc - lr.T_STREET[:3, 3].astype(np.float64), np.full((len(Z), 1), 0.25)], axis=1).astype(f32)
        frames.append((rgb, pts, sem))
    return frames, poses


def test_lidar_depth_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([_build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.parametrize("missing", ["scans", "transform"])
def test_reader_without_the_lidar_files_reports_failure(tmp_path, drive, missing):
    frames, poses = drive
    root = str(tmp_path / "camera_only")
    write_lidar_dataset(root, frames, poses, with_scans=missing != "scans", with_transform=missing != "transform")
    out = [str(tmp_path / n) for n in ("depth.bin", "map.bin")]
    r = subprocess.run([_build_demo(tmp_path), root, str(LARGE)] + out, capture_output=True, text=True)
    # the reader fails (setUseLidar() false or getNext() false) before anything touches a GPU; no crash
    assert r.returncode == 3 and "reader:" in r.stdout and ("velodyne" if missing == "scans" else "velo_to_cam.txt") in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert not os.path.exists(out[1])


@pytest.mark.parametrize("with_right", [0, 1])
def test_reader_flags_and_empty_scans(tmp_path, drive, with_right):
    """tests/cpp/lidar_reader_check.cpp: the scan instead of the depth image, an empty scan, estimateDepth as well, switching off"""
    frames, poses = drive
    frames = [frames[0], (frames[1][0], np.zeros((0, 4), f32), frames[1][2]), frames[2]]
    root = str(tmp_path / "flags")
    write_lidar_dataset(root, frames, poses)
    if with_right:
        os.makedirs(os.path.join(root, "image_3"))
        for k, (rgb, _, _) in enumerate(frames):
            kf.write_png(os.path.join(root, "image_3", f"{k:06d}.png"), rgb[:, ::-1])
    exe = str(tmp_path / "lidar_reader_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "lidar_reader_check.cpp"), "-lz"])
    r = subprocess.run([exe, root, str(with_right)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    want = [f"frame {k} points {len(p)} first {float(p[0, 0]) if len(p) else 0.0:.9g}" for k, (_, p, _) in enumerate(frames)]
    assert r.stdout.splitlines() == want


@pytest.mark.gpu
def test_facade_maps_a_lidar_drive_like_python(tmp_path, drive):
    from surfelmapping_amd import capi
    frames, poses = drive
    root = str(tmp_path / "lidar")
    write_lidar_dataset(root, frames, poses)
    assert not os.path.exists(os.path.join(root, "PSMNet"))
    out_depth, out_map = (str(tmp_path / n) for n in ("depth.bin", "map.bin"))
    r = subprocess.run([_build_demo(tmp_path), root, str(LARGE), out_depth, out_map], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert f"points {sum(len(p) for _, p, _ in frames)} in {N} frames" in r.stdout
    # through the binding: the restatement's depth at the reader's poses
    m = capi.SurfelMap(capi.make_config(**CAM, preprocess=0))
    for k, (rgb, pts, sem) in enumerate(frames):
        depth = lr.lidar_depth(pts, lr.T_STREET, CAM, large=LARGE)["depth_mm"]
        m.process_frame(rgb, depth, sem, kf.reader_pose(poses[k]))
    assert np.array_equal(np.frombuffer(open(out_depth, "rb").read(), np.uint16).reshape(depth.shape), depth)
    model = m.download_model()
    assert len(model) > 100
    assert np.array_equal(_u32(rr.read_map(out_map)[0]), _u32(model))
