"""numpy restatement of the pose search (sm_score_poses_window, sm_search_pose; surfelmapping_amd/csrc/sm_k_search.h and
sm_search.hip; DESIGN.md "4j. Pose search") -- the checker of tests/test_search.py.  The score is tests/track_ref.py's inlier test
(every float32 step one IEEE float32 operation of the kernels, in their order) with the colour gate of tests/track_rgb_ref.py's
luminance; the candidate grids are float64 in the host code's order of operations, with libm's sin and cos, so the candidate lists
are equal bit for bit; the ranking and the level scheme follow."""
import math

import numpy as np

import loop_auto_ref as lar
import track_ref as tr
import track_rgb_ref as trr

f32 = np.float32
DEG = math.pi / 180.0
DEFAULT = dict(levels=2, trans_half=(2.0, 0.0, 2.0), trans_step=(0.25, 0.25, 0.25), rot_half_deg=(0.0, 3.0, 0.0),
               rot_step_deg=(0.5, 0.5, 0.5), refine=4, stride0=8, top_k=4, colour_thresh=0.1)
MAX_CANDIDATES = 1 << 20


# ---------------------------------------------------------------------------------------------------------------------
# the score
# ---------------------------------------------------------------------------------------------------------------------
def samples(rgb, depth_mm, cam, stride, stereo_border=80.0):
    """k_search_samples: the valid grid points of `stride` as (v float32[n][3], n float32[n][3], Y_f float32[n]); rgb None: Y_f = 0"""
    W, H = cam["width"], cam["height"]
    vm, nm = tr.vertex_normal(depth_mm, cam, stereo_border=stereo_border, stride=stride)
    ok = vm[:, 3] != 0
    if rgb is None:
        y = np.zeros(len(vm), f32)
    else:
        rgb = np.asarray(rgb, np.uint8).reshape(H, W, 3)
        y = trr.luminance(rgb[..., 0], rgb[..., 1], rgb[..., 2])[0:H:stride, 0:W:stride].reshape(-1)
    return vm[ok, :3], nm[ok, :3], y[ok]


def prediction(model, t_prev16, cam, min_time=lar.INT32_MIN, max_time=lar.INT32_MAX):
    """the windowed prediction and k_search_gather: (p_m float32[P][3], n_m float32[P][3], Y_m float32[P], valid bool[P])"""
    m = np.asarray(model, f32)
    pred = tr.predict(m, t_prev16, cam, live=lar.in_window(m[:, 7], min_time, max_time)).reshape(-1)
    ok = pred >= 0
    row = m[np.where(ok, pred, 0)]
    ym = trr.colour_luminance(np.ascontiguousarray(row[:, 4]).view(np.uint32))
    return row[:, 0:3], row[:, 8:11], ym, ok


def score(cands16, smp, plane, t_prev16, cam, dist=0.3, angle_deg=30.0, colour_thresh=None, batch=64):
    """k_search_score: uint32[n], the samples that pass track_pair's tests under each candidate (float32[n][16] column-major)
    and, with colour_thresh not None, |Y_f - Y_m| <= colour_thresh"""
    W = cam["width"]
    v, n, yf = smp
    pm, nm, ym, valid = plane
    tinv = tr.rigid_inv_d(tr.colmajor(t_prev16)).astype(f32)
    cosa = f32(math.cos(angle_deg * (math.pi / 180.0)))
    c16 = np.ascontiguousarray(cands16, f32).reshape(-1, 16)
    out = np.zeros(len(c16), np.uint32)
    vx, vy, vz = (v[None, :, k] for k in range(3))
    nx, ny, nz = (n[None, :, k] for k in range(3))
    for b0 in range(0, len(c16), batch):
        m = [c16[b0:b0 + batch, e][:, None] for e in range(16)]
        with np.errstate(all="ignore"):
            w = tr._xform(m, vx, vy, vz)
            nw = tr._rot(m, nx, ny, nz)
            c = tr._xform(tinv, w[0], w[1], w[2])
            fu, fv, inb = tr._project(cam, c)
            ok = (c[2] > 0) & inb
            pix = np.where(ok, fv.astype(np.int64) * W + fu.astype(np.int64), 0)
            ok &= valid[pix]
            d = [w[k] - pm[pix, k] for k in range(3)]
            ok &= np.sqrt(tr._dot(d, d)) <= f32(dist)
            ok &= tr._dot(nw, [nm[pix, k] for k in range(3)]) >= cosa
            if colour_thresh is not None:
                ok &= np.abs(yf[None, :] - ym[pix]) <= f32(colour_thresh)
        out[b0:b0 + batch] = ok.sum(axis=1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the candidate grids (float64, the host code's order of operations)
# ---------------------------------------------------------------------------------------------------------------------
def _mul3(A, B):
    return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def delta_rot(a, b, c):
    """Ry(b) * Rx(a) * Rz(c) of angles in degrees: 3x3 of Python floats"""
    ra, rb, rc = a * DEG, b * DEG, c * DEG
    ca, sa, cb, sb, cc, sc = math.cos(ra), math.sin(ra), math.cos(rb), math.sin(rb), math.cos(rc), math.sin(rc)
    Rx = [[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]]
    Ry = [[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]]
    Rz = [[cc, -sc, 0.0], [sc, cc, 0.0], [0.0, 0.0, 1.0]]
    return _mul3(_mul3(Ry, Rx), Rz)


def grid(base16, n, k0, step):
    """the nested loops over (rot x, rot y, rot z, trans x, trans y, trans z), the last fastest, offsets (k + k0[a]) * step[a]:
    base * [R | t] rounded to float32 once, float32[N][16]"""
    a = [float(x) for x in np.asarray(base16, f32).reshape(16)]
    t = [np.array([(k + k0[ax]) * step[ax] for k in range(n[ax])], np.float64) for ax in (3, 4, 5)]
    tx, ty, tz = (g.reshape(-1) for g in np.meshgrid(t[0], t[1], t[2], indexing="ij"))
    blocks = []
    for i in range(n[0]):
        for j in range(n[1]):
            for k in range(n[2]):
                R = delta_rot((i + k0[0]) * step[0], (j + k0[1]) * step[1], (k + k0[2]) * step[2])
                blk = np.zeros((len(tx), 16), f32)
                for c in range(3):
                    for r in range(3):
                        blk[:, c * 4 + r] = f32((a[r] * R[0][c] + a[4 + r] * R[1][c]) + a[8 + r] * R[2][c])
                for r in range(3):
                    blk[:, 12 + r] = (((a[r] * tx + a[4 + r] * ty) + a[8 + r] * tz) + a[12 + r]).astype(f32)
                blk[:, 15] = 1.0
                blocks.append(blk)
    return np.concatenate(blocks)


def axes(sp):
    """per axis (rot x, y, z, trans x, y, z): (active, n, step) of level 0"""
    out = []
    for a in range(6):
        half = float(f32((sp["rot_half_deg"] if a < 3 else sp["trans_half"])[a % 3]))
        step = float(f32((sp["rot_step_deg"] if a < 3 else sp["trans_step"])[a % 3]))
        active = half > 0.0 and step > 0.0
        out.append((active, 2 * int(math.floor(half / step)) + 1 if active else 1, step))
    return out


def level0(centre16, sp=DEFAULT):
    ax = axes(sp)
    n = [x[1] for x in ax]
    return grid(centre16, n, [-float((k - 1) // 2) for k in n], [x[2] for x in ax])


def next_level(kept16, level, sp=DEFAULT):
    """the list of level `level` (>= 1) around the kept candidates of the level before, in rank order"""
    ax = axes(sp)
    r = int(sp["refine"])
    pw = 1.0
    for _ in range(level):
        pw *= float(r)
    n = [2 * r + 1 if x[0] else 1 for x in ax]
    k0 = [-float(r) if x[0] else 0.0 for x in ax]
    return np.concatenate([grid(b, n, k0, [x[2] / pw for x in ax]) for b in kept16])


def rank(scores, stride, min_inliers, top_k):
    """indices: score descending, then index ascending, only scores with score * stride^2 >= min_inliers, the first top_k"""
    s = np.asarray(scores, np.int64)
    idx = np.nonzero(s * stride * stride >= max(int(min_inliers), 0))[0]
    order = idx[np.lexsort((idx, -s[idx]))]
    return order[:top_k]


def search(rgb, depth_mm, model, t_prev16, centre16, cam, sp=DEFAULT, min_time=lar.INT32_MIN, max_time=lar.INT32_MAX, dist=0.3,
           angle_deg=30.0, min_inliers=1000, stereo_border=80.0):
    """sm_search_pose up to the refinement: dict(status "OK" | "LOST" | "NO_MODEL", levels = [dict(cands, scores, kept (indices),
    poses (float32[k][16], rank order))]); the kept poses of the last level are what the trackers start from"""
    plane = prediction(model, t_prev16, cam, min_time, max_time)
    cands = level0(centre16, sp)
    levels = []
    for l in range(int(sp["levels"])):
        assert len(cands) <= MAX_CANDIDATES
        stride = max(1, int(sp["stride0"]) >> l)
        smp = samples(rgb, depth_mm, cam, stride, stereo_border)
        sc = score(cands, smp, plane, t_prev16, cam, dist, angle_deg, None if rgb is None else sp["colour_thresh"])
        if not plane[3].any():
            levels.append(dict(cands=cands, scores=sc, kept=np.zeros(0, np.int64), poses=cands[:0]))
            return dict(status="NO_MODEL", levels=levels)
        kept = rank(sc, stride, min_inliers, int(sp["top_k"]))
        levels.append(dict(cands=cands, scores=sc, kept=kept, poses=cands[kept]))
        if len(kept) == 0:
            return dict(status="LOST", levels=levels)
        if l + 1 < int(sp["levels"]):
            cands = next_level(cands[kept], l + 1, sp)
    return dict(status="OK", levels=levels)


def offset_pose(pose, x, z, yaw_deg):
    """pose (4x4) right-multiplied by [Ry(yaw) | (x, 0, z)]: float32 4x4"""
    D = np.eye(4)
    D[:3, :3] = delta_rot(0.0, yaw_deg, 0.0)
    D[:3, 3] = (x, 0.0, z)
    return (np.asarray(pose, np.float64) @ D).astype(f32)
