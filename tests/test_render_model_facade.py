"""GlobalModel::renderModelImage of the drop-in facade (surfelmapping_amd/csrc/facade/GlobalModel.h): CPU: a caller compiles
with plain g++ against the C-ABI only.  GPU: its images in six draw modes equal SurfelMap.render_model on the map it built,
with processFrame synchronous and asynchronous (SM_FACADE_ASYNC)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "render_model_demo.cpp")
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "render_model_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC,
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_render_model_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("facade_async", ["0", "1"])
def test_render_model_image_matches_python(tmp_path, facade_async):
    import model_view_ref as ref
    from surfelmapping_amd import capi, synth
    cam = dict(width=320, height=120, fx=180.0, fy=180.0, cx=159.5, cy=59.5)
    seq = synth.make_sequence(cam, synth.kitti_trajectory(5), seed=12)
    frames = tmp_path / "frames.bin"
    with open(frames, "wb") as f:
        f.write(np.array([cam["width"], cam["height"], len(seq)], np.uint32).tobytes())
        f.write(np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32).tobytes())
        for rgb, d, s, p in seq:
            f.write(rgb.tobytes()); f.write(d.tobytes()); f.write(s.tobytes()); f.write(p.astype(np.float32).tobytes())
    w, h = 200, 150
    P = ref.projection(w, h, 420.0 * w / 640, 420.0 * h / 480, 320.0 * w / 640, 240.0 * h / 480, 0.1, 1000.0)
    MV = ref.look_at(0.0, -2.0, -6.0, 0.0, -2.0, 20.0, 0, -1, 0)      # axis-aligned: its inverse is exact in any method
    camf = tmp_path / "camera.bin"
    with open(camf, "wb") as f:
        f.write((P @ MV).T.reshape(16).astype(np.float64).tobytes())
        f.write(MV.T.reshape(16).astype(np.float64).tobytes())
        f.write(np.array([w, h], np.int32).tobytes())
    out_map, out_img = tmp_path / "map.bin", tmp_path / "images.bin"
    r = subprocess.run([build_demo(tmp_path), str(frames), str(camf), str(out_map), str(out_img)], capture_output=True, text=True,
                       env=dict(os.environ, SM_FACADE_ASYNC=facade_async))
    assert r.returncode == 0, r.stdout + r.stderr
    imgs = np.frombuffer(open(out_img, "rb").read(), np.uint8).reshape(6, h, w, 4)
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=1000))
    m.load_map(str(out_map))
    mvp, inv = ref.view_mats(P, MV)
    clear = (51, 102, 153, 255)                                     # floor(0.2 / 0.4 / 0.6 / 1.0 * 255 + 0.5)
    modes = [dict(color_type=0), dict(color_type=1), dict(color_type=2), dict(color_type=3), dict(color_type=0, window=True),
             dict(color_type=2, points=True)]
    for img, kw in zip(imgs, modes):
        want = m.render_model(mvp, inv, w, h, threshold=0.5, unstable=True, time=len(seq), time_delta=1, clear=clear, **kw)
        assert np.array_equal(img, want), kw
        assert (want[..., 3] == 255).mean() > 0.05
    assert f"model {m.counts()['count']}" in r.stdout
