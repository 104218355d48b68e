"""Blended views through the drop-in facade (SurfelMapping::setBlend and both acquireImages overloads; tests/cpp/blend_demo.cpp).
CPU: the caller compiles with plain g++ against the C-ABI only.  GPU: with the switch on, the PNGs in image/ and semantic/ decode to
the binding's blended views and differ from those written with it off, which are, byte for byte, the files of the plain renderers."""
import os
import subprocess

import numpy as np
import pytest

import test_blend as tb
from test_fill_facade import png_bytes, read_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "surfelmapping_amd")


def build_demo(tmp_path):
    exe = str(tmp_path / "blend_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "blend_demo.cpp"),
                           "-L" + LIBDIR, "-lsurfelmapping_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_blend_demo_compiles_against_c_abi_only(tmp_path):
    r = subprocess.run([build_demo(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stdout


@pytest.mark.gpu
def test_facade_dumps_equal_the_binding(tmp_path):
    scene = tb.Scene()
    rows, views = scene.rows, scene.views
    n0, n1 = 600, 1400
    files = [tb.write_map(tmp_path / "a.bin", rows[:n0]), tb.write_map(tmp_path / "b.bin", rows[n0:n1])]
    live = tb.write_map(tmp_path / "live.bin", rows[n1:])
    with open(tmp_path / "views.bin", "wb") as f:
        f.write(np.array([len(views)], np.uint32).tobytes() + views.astype(np.float32).tobytes())
    exe = build_demo(tmp_path)
    tol, falloff = 20, 1

    def run(blend, out):
        r = subprocess.run([exe, live, "64", str(tmp_path / "views.bin")] + [repr(float(x)) if i >= 2 else str(x) for i, x in enumerate(tb.CAM)] +
                           [str(blend), str(tol), str(falloff), str(out)] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout

    m = tb._ctx(rows[n1:])
    p = dict(depth_tol_256=tol, falloff=falloff)
    on, off = tmp_path / "on", tmp_path / "off"
    stdout = run(1, on)
    run(0, off)
    want_live = [m.render_image(v, *tb.CAM, blend=p) for v in views]
    want_set = m.render_image_maps(files, views, *tb.CAM, blend=p)
    st = m.blend_stats()
    assert (f"views {len(views)} drawn {st['drawn']} contributions {st['contributions']} changed {st['changed']} "
            f"launches {st['launches']}\n") in stdout, stdout
    plain_set = m.render_image_maps(files, views, *tb.CAM)
    for k, v in enumerate(views):
        same_as_ref = np.array_equal(want_set[0][k], scene.ref(k, tol, falloff)["bgr"])
        assert same_as_ref, k
        for sub, first, (bgr, sem), plain in (("live", 0, want_live[k], m.render_image(v, *tb.CAM)),
                                              ("set", 5, (want_set[0][k], want_set[1][k]), (plain_set[0][k], plain_set[1][k]))):
            name = f"{first + k:06d}.png"
            assert np.array_equal(read_png(on / sub / "image" / name), bgr[..., ::-1]), (sub, k)
            assert np.array_equal(read_png(on / sub / "semantic" / name)[..., 0], sem), (sub, k)
            assert not (on / sub / "depth").exists()
            # off: the plain renderers' files; the labels are the same, the picture is not
            assert open(off / sub / "image" / name, "rb").read() == png_bytes(np.ascontiguousarray(plain[0][..., ::-1])), (sub, k)
            assert open(off / sub / "semantic" / name, "rb").read() == open(on / sub / "semantic" / name, "rb").read(), (sub, k)
            assert open(off / sub / "image" / name, "rb").read() != open(on / sub / "image" / name, "rb").read(), (sub, k)
    m.close()
