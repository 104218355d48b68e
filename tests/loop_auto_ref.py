"""Numpy restatement of the census of old surfels in view (sm_old_in_view; DESIGN.md "4i. Closing loops unasked"): float32,
term by term in the header's order, with the helpers of tests/track_ref.py that restate the tracker's prediction gates."""
import numpy as np

import track_ref as tr

f32 = np.float32
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def in_window(times, min_time, max_time):
    """min_time < t <= max_time, both comparisons false on a NaN; INT32_MIN / INT32_MAX: that end is not compared"""
    t = np.asarray(times, f32)
    ok = np.ones(len(t), bool)
    with np.errstate(invalid="ignore"):
        if min_time != INT32_MIN:
            ok &= t > f32(min_time)
        if max_time != INT32_MAX:
            ok &= t <= f32(max_time)
    return ok


def gates(model, pose16, cam, near=1.0, far=30.0):
    """k_track_splat's gates for the rows of `model` seen from `pose16` (4x4 or float32[16] column-major): bool[n]"""
    tinv = tr.rigid_inv_d(tr.colmajor(pose16)).astype(f32)
    p = np.asarray(model, f32)
    with np.errstate(all="ignore"):
        c = tr._xform(tinv, p[:, 0], p[:, 1], p[:, 2])
        ok = (c[2] > f32(near)) & (c[2] < f32(far))
        _, _, inb = tr._project(cam, c)
    return ok & inb


def census(model, pose16, cam, max_time, near=1.0, far=30.0):
    """how many rows of `model` (the live surfels: sm_download_model_aos) are old and in view"""
    p = np.asarray(model, f32)
    with np.errstate(invalid="ignore"):
        old = p[:, 7] <= f32(max_time)
    return int((gates(p, pose16, cam, near, far) & old).sum())
