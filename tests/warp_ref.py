"""The definitions of closing loops (include/sm_c_api.h "closing loops") restated in numpy: the row rule of
sm_warp_by_time in fp32 without fused multiply-add, the stored-pose rule and sm_loop_spread in double, and the tracker's
constant-velocity guess (sm_c_api.h "camera tracking") in plain double arithmetic."""
import math

import numpy as np

f32 = np.float32


def select(times, t0, n):
    """(sel bool[m], k int64[m]): which records the table moves and by which of its n rows (k is 0 where sel is False)"""
    tau = np.asarray(times, f32)
    t0f = f32(t0)
    with np.errstate(invalid="ignore", over="ignore"):
        sel = tau >= t0f                                       # False on a NaN
        d = tau - t0f
        last = d >= f32(n - 1)                                 # +inf lands here
        k = np.where(last, n - 1, np.where(sel, np.trunc(np.where(sel & ~last, d, 0)), 0)).astype(np.int64)
    return sel, np.where(sel, k, 0)


def warp_rows(rows, t0, corr):
    """the records after sm_warp_by_time(t0, corr): float32[m][12] -> float32[m][12]; everything but the centre and the normal of
    a selected row keeps its bits"""
    m = np.ascontiguousarray(rows, f32).reshape(-1, 12)
    corr = np.ascontiguousarray(corr, f32).reshape(-1, 12)
    sel, k = select(m[:, 7], t0, len(corr))
    C = corr[k]
    out = m.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        x, y, z = m[:, 0], m[:, 1], m[:, 2]
        nx, ny, nz = m[:, 8], m[:, 9], m[:, 10]
        for i in range(3):
            p = ((C[:, 4 * i] * x + C[:, 4 * i + 1] * y) + C[:, 4 * i + 2] * z) + C[:, 4 * i + 3]
            q = (C[:, 4 * i] * nx + C[:, 4 * i + 1] * ny) + C[:, 4 * i + 2] * nz
            out[:, i] = np.where(sel, p, m[:, i])
            out[:, 8 + i] = np.where(sel, q, m[:, 8 + i])
    # np.where on floats keeps the bits of whichever side it takes
    return out


def warp_pose(pose16, tick, t0, corr):
    """a stored camera->world pose (float32[16] column-major) of tick `tick` after the warp: C * P in double from the widened floats,
    each element ((c0*p0 + c1*p1) + c2*p2) + c3*p3, rounded to float once; unselected: unchanged"""
    P = np.asarray(pose16, f32).reshape(16).copy()
    corr = np.ascontiguousarray(corr, f32).reshape(-1, 12)
    sel, k = select(np.array([float(tick)], f32), t0, len(corr))
    if not sel[0]:
        return P
    C = [float(v) for v in corr[k[0]]]
    p = [float(v) for v in P]
    out = P.copy()
    for j in range(4):
        for i in range(3):
            out[i + 4 * j] = f32(((C[4 * i] * p[4 * j] + C[4 * i + 1] * p[4 * j + 1]) + C[4 * i + 2] * p[4 * j + 2]) + C[4 * i + 3] * p[4 * j + 3])
    return out


def loop_spread(D, t_a, t_b):
    """sm_loop_spread: float32[t_b - t_a + 1][12].  D: float32[16] column-major world->world.  Row 0 is the identity, the last row
    D's own 3x4; between them R_k = exp(w_k * log R_D) by Rodrigues and t_k = w_k * t_D, in double, rounded to float once."""
    D = np.asarray(D, f32).reshape(16)
    R = np.array([[float(D[i + 4 * j]) for j in range(3)] for i in range(3)], np.float64)
    t = [float(D[12 + i]) for i in range(3)]
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    nv = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    c = (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0) * 0.5
    angle = math.atan2(nv * 0.5, c)
    a = v / nv if nv > 0.0 else np.zeros(3)
    if not nv > 0.0:
        angle = 0.0
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    K2 = np.array([[(K[i, 0] * K[0, j] + K[i, 1] * K[1, j]) + K[i, 2] * K[2, j] for j in range(3)] for i in range(3)])
    span = int(t_b) - int(t_a)
    out = np.zeros((span + 1, 12), f32)
    for k in range(span + 1):
        if k == 0:
            out[k] = np.eye(3, 4, dtype=f32).reshape(12)
            continue
        if k == span:
            out[k] = np.array([[D[i + 4 * j] for j in range(4)] for i in range(3)], f32).reshape(12)
            continue
        w = k / span
        ak = w * angle
        sn, oc = math.sin(ak), 1.0 - math.cos(ak)
        for i in range(3):
            for j in range(3):
                out[k, 4 * i + j] = f32(((1.0 if i == j else 0.0) + sn * K[i, j]) + oc * K2[i, j])
            out[k, 4 * i + 3] = f32(w * t[i])
    return out


def rigid_table(n, seed=0, angle_deg=3.0, trans=0.5):
    """n distinct non-trivial rigid transforms as a table float32[n][12] (rotations made in double, rounded to float once)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 12), f32)
    for k in range(n):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = math.radians(angle_deg) * (k + 1)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
        out[k] = np.concatenate([R, (rng.normal(size=3) * trans * (k + 1))[:, None]], axis=1).astype(f32).reshape(12)
    return out


def table_of(G):
    """the one-row table of a 4x4 world->world matrix (numpy row/col indexing)"""
    return np.asarray(G, f32)[:3, :4].reshape(1, 12).copy()


# ---- the tracker's constant-velocity guess (sm_track_frame with guess16 NULL), in plain double arithmetic
def _orthonormalize(m):
    a, b, c = m[0:3], m[4:7], m[8:11]
    na = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    a = [x / na for x in a]
    ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    b = [b[k] - ab * a[k] for k in range(3)]
    nb = math.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    b = [x / nb for x in b]
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    return a + [0.0] + b + [0.0] + c + [0.0] + list(m[12:15]) + [1.0]


def _rigid_inv(m):
    o = [0.0] * 16
    for r in range(3):
        for c in range(3):
            o[c * 4 + r] = m[r * 4 + c]
        o[12 + r] = -((m[r * 4 + 0] * m[12] + m[r * 4 + 1] * m[13]) + m[r * 4 + 2] * m[14])
    o[15] = 1.0
    return o


def _mul_rigid(a, b):
    o = [0.0] * 16
    for c in range(4):
        for r in range(3):
            o[c * 4 + r] = ((a[r] * b[c * 4] + a[4 + r] * b[c * 4 + 1]) + a[8 + r] * b[c * 4 + 2]) + (a[12 + r] if c == 3 else 0.0)
    o[15] = 1.0
    return o


def constant_velocity(prev16, prev2_16):
    """T_prev * (T_prev2^-1 * T_prev) of the orthonormalised poses, float32[16] column-major"""
    p = _orthonormalize([float(v) for v in np.asarray(prev16, f32).reshape(16)])
    p2 = _orthonormalize([float(v) for v in np.asarray(prev2_16, f32).reshape(16)])
    return np.array(_mul_rigid(p, _mul_rigid(_rigid_inv(p2), p)), np.float64).astype(f32)
