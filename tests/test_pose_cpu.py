"""The rigid-pose arithmetic of the trackers and the loop closure (surfelmapping_amd/csrc/sm_pose.h), without a GPU:
tests/cpp/pose_check.cpp is compiled against the header alone and its rigid inverse, rigid product and orthonormalisation of a
handful of float poses are compared bit for bit with tests/track_ref.py's restatements (the inverse there is what every
prediction of the reference tracker is made with).  The program is built once more with the address and undefined-behaviour
sanitizers and run on the same poses."""
import math
import os
import subprocess

import numpy as np
import pytest

import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "surfelmapping_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "pose_check.cpp")
# no contraction: every product and sum is its own IEEE operation, as in the core's build and in numpy
FLAGS = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC]


def _pose(rx, ry, rz, t, skew=0.0):
    """Rz * Ry * Rx | t in double, rounded to float32 (orthonormal to float rounding only); skew shears column 1 into column 0"""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
         @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    R[:, 1] += skew * R[:, 0]
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return tr.colmajor(m)


POSES = [
    tr.colmajor(np.eye(4)),
    _pose(0.01, -0.02, 0.005, (0.3, -0.05, 1.2)),                     # a frame-to-frame step
    _pose(0.7, -1.9, 2.6, (-152.25, 3.5, 987.125)),                   # far from the origin, large angles
    _pose(-0.3, 0.4, 0.1, (1e-3, -2e-3, 5e-4), skew=1e-3),            # visibly not orthonormal
    _pose(3.0, 0.0, -3.1, (0.0, -0.0, 1e6)),                          # near half turns, a signed zero
]


def _run(exe):
    args = [float(v).hex() for p in POSES for v in p]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=20)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = {}
    for ln in r.stdout.splitlines():
        name, *vals = ln.split()
        out.setdefault(name, []).append(np.array([float.fromhex(v) for v in vals], np.float64))
    return out


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose")
    plain, san = str(d / "pose_check"), str(d / "pose_check_san")
    subprocess.check_call(FLAGS + ["-o", plain, SRC])
    subprocess.check_call(FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, SRC])
    return plain, san


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_pose_arithmetic_equals_the_restatement_bit_for_bit(built):
    got = _run(built[0])
    eye = np.eye(4).reshape(16)
    assert len(got["eye"]) == 2 and all(np.array_equal(_bits(e), _bits(eye)) for e in got["eye"])
    assert len(got["inv"]) == len(got["mul"]) == len(got["ortho"]) == len(POSES)
    for i, a in enumerate(POSES):
        b = POSES[(i + 1) % len(POSES)]
        assert np.array_equal(_bits(got["inv"][i]), _bits(tr.rigid_inv_d(a))), i
        assert np.array_equal(_bits(got["mul"][i]), _bits(tr.mul_rigid_d(a, b))), i
        assert np.array_equal(_bits(got["ortho"][i]), _bits(tr.orthonormalize_d(a))), i


def test_the_restatement_is_a_rigid_inverse_product_and_orthonormalisation():
    """what the bit-for-bit comparison stands on: the restated operations are what their names say, to double rounding"""
    for i, a in enumerate(POSES):
        A = np.asarray(a, np.float64).reshape(4, 4).T
        B = np.asarray(POSES[(i + 1) % len(POSES)], np.float64).reshape(4, 4).T
        scale = max(1.0, float(np.abs(A[:3, 3]).max()), float(np.abs(B[:3, 3]).max()))
        assert np.allclose(tr.mul_rigid_d(a, POSES[(i + 1) % len(POSES)]).reshape(4, 4).T, A @ B, rtol=0, atol=1e-12 * scale)
        Q = tr.orthonormalize_d(a).reshape(4, 4).T
        assert np.allclose(Q[:3, :3].T @ Q[:3, :3], np.eye(3), rtol=0, atol=1e-15 * 8)
        assert np.linalg.det(Q[:3, :3]) > 0 and np.array_equal(Q[:3, 3], A[:3, 3])
        # the inverse is the rigid one: exact on the orthonormalised pose up to double rounding
        I = tr.mul_rigid_d(tr.rigid_inv_d(Q.T.reshape(16)), Q.T.reshape(16)).reshape(4, 4).T
        assert np.allclose(I, np.eye(4), rtol=0, atol=1e-15 * 8 * scale)


def test_sanitized_build_runs_clean_and_says_the_same(built):
    plain, san = _run(built[0]), _run(built[1])
    for name in plain:
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(plain[name], san[name])), name
