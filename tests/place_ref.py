"""Place recognition (include/sm_c_api.h "place recognition") restated in numpy: the fern table (splitmix64 in
Python integers), the code of a frame, the match, the keyframe file and the keyframe-pose rule of sm_warp_by_time; the smooth
texture the scenario needs (a block mean of synth.Scene's hashed colour carries no place information) and the drive the
end-to-end tests share."""
import functools
import math
import struct

import numpy as np

import retire_ref as rr
import warp_ref as wr

f32 = np.float32
M64 = (1 << 64) - 1
MAGIC, VERSION, HEADER_BYTES = 0x4E524653, 1, 48
FERN_DTYPE = np.dtype([(n, np.uint16) for n in ("x", "y", "tr", "tg", "tb", "td")])
DEFAULT = dict(n_ferns=512, cell=8, seed=1, depth_lo_mm=1000, depth_hi_mm=30000)


def params(**over):
    p = dict(DEFAULT, **over)
    assert set(p) == set(DEFAULT)
    return p


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
class SplitMix:
    def __init__(self, seed):
        self.state = int(seed) & M64

    def draw(self, r):
        self.state = (self.state + 0x9E3779B97F4A7C15) & M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        return ((z >> 32) * int(r)) >> 32


def table(p, width, height):
    """sm_fern_table: a structured array (x, y, tr, tg, tb, td)"""
    gw, gh = width // p["cell"], height // p["cell"]
    assert gw >= 1 and gh >= 1
    g = SplitMix(p["seed"])
    out = np.zeros(p["n_ferns"], FERN_DTYPE)
    for f in range(p["n_ferns"]):
        x, y = g.draw(gw), g.draw(gh)
        tr, tg, tb = g.draw(255), g.draw(255), g.draw(255)
        out[f] = (x, y, tr, tg, tb, p["depth_lo_mm"] + g.draw(p["depth_hi_mm"] - p["depth_lo_mm"]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the code
# ---------------------------------------------------------------------------------------------------------------------
def cell_means(rgb, depth_mm, cell):
    """(R, G, B, D) int64[gh][gw]: the integer means of every whole cell; rgb None: the colour means are None"""
    d = np.asarray(depth_mm, np.uint16)
    H, W = d.shape
    gh, gw = H // cell, W // cell
    blk = d[:gh * cell, :gw * cell].astype(np.int64).reshape(gh, cell, gw, cell)
    cnt = (blk != 0).sum(axis=(1, 3))
    D = np.where(cnt > 0, blk.sum(axis=(1, 3)) // np.maximum(cnt, 1), 0)
    if rgb is None:
        return None, None, None, D
    c = np.asarray(rgb, np.uint8).reshape(H, W, 3)[:gh * cell, :gw * cell].astype(np.int64).reshape(gh, cell, gw, cell, 3)
    m = c.sum(axis=(1, 3)) // (cell * cell)
    return m[..., 0], m[..., 1], m[..., 2], D


def nibbles(rgb, depth_mm, p, tab=None):
    """uint32[n_ferns]: every fern's nibble"""
    d = np.asarray(depth_mm, np.uint16)
    tab = table(p, d.shape[1], d.shape[0]) if tab is None else tab
    R, G, B, D = cell_means(rgb, d, p["cell"])
    x, y = tab["x"].astype(np.int64), tab["y"].astype(np.int64)
    nib = (D[y, x] > tab["td"]).astype(np.uint32) << 3
    if rgb is not None:
        nib |= (R[y, x] > tab["tr"]).astype(np.uint32) | ((G[y, x] > tab["tg"]).astype(np.uint32) << 1) | ((B[y, x] > tab["tb"]).astype(np.uint32) << 2)
    return nib


def pack(nib):
    """fern f in bits 4*(f&7) .. 4*(f&7)+3 of word f>>3"""
    n = np.asarray(nib, np.uint32).reshape(-1, 8)
    return np.bitwise_or.reduce(n << (4 * np.arange(8, dtype=np.uint32))[None, :], axis=1).astype(np.uint32)


def unpack(code):
    c = np.asarray(code, np.uint32)
    return ((c[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & np.uint32(15)).reshape(c.shape[:-1] + (-1,))


def encode(rgb, depth_mm, p, tab=None):
    """sm_fern_encode: uint32[n_ferns / 8]"""
    return pack(nibbles(rgb, depth_mm, p, tab))


# ---------------------------------------------------------------------------------------------------------------------
# the match
# ---------------------------------------------------------------------------------------------------------------------
def dis_all(code, codes):
    """uint32[n]: the ferns whose nibbles differ between `code` and each keyframe"""
    codes = np.asarray(codes, np.uint32)
    if len(codes) == 0:
        return np.zeros(0, np.uint32)
    return (unpack(codes) != unpack(code)[None, :]).sum(axis=1).astype(np.uint32)


def match(code, codes, times, min_time, max_time):
    """sm_fern_match: (index or -1, dis or 2^32 - 1, dis of every keyframe)"""
    d = dis_all(code, codes)
    t = np.asarray(times, np.int64)
    idx = np.nonzero((t > int(min_time)) & (t <= int(max_time)))[0]
    if len(idx) == 0:
        return -1, 0xFFFFFFFF, d
    k = idx[np.argmin(d[idx])]                                # the first smallest: the lower index
    return int(k), int(d[k]), d


# ---------------------------------------------------------------------------------------------------------------------
# the keyframe file and the warp
# ---------------------------------------------------------------------------------------------------------------------
def file_bytes(p, width, height, codes, poses, times, count=None):
    """the bytes sm_fern_save writes for these keyframes (count: what the header says, by default how many there are)"""
    codes = np.ascontiguousarray(codes, np.uint32).reshape(len(times), p["n_ferns"] // 8)
    poses = np.ascontiguousarray(poses, f32).reshape(len(times), 16)
    head = struct.pack("<IIiiQiiiiII", MAGIC, VERSION, p["n_ferns"], p["cell"], p["seed"], p["depth_lo_mm"], p["depth_hi_mm"], width, height,
                       len(times) if count is None else count, 0)
    assert len(head) == HEADER_BYTES
    body = b"".join(struct.pack("<i", int(times[k])) + poses[k].tobytes() + codes[k].tobytes() for k in range(len(times)))
    return head + body


def warp_poses(poses, times, t0, corr):
    """the stored keyframe poses (float32[n][16]) after sm_warp_by_time(t0, corr)"""
    return np.stack([wr.warp_pose(P, int(t), t0, corr) for P, t in zip(np.asarray(poses, f32).reshape(-1, 16), times)]) if len(times) else \
        np.zeros((0, 16), f32)


# ---------------------------------------------------------------------------------------------------------------------
# the smooth texture
# ---------------------------------------------------------------------------------------------------------------------
SKY = np.array([135, 206, 235], np.uint8)
_AB = ((1.0, 0.0), (0.63, 1.3), (0.37, 2.1))


def recolour(depth_mm, sem, pose, cam):
    """A synth frame's colour image drawn again with a low-frequency texture of the world point (angles in radians):
    s = 0.9 x + 1.7 y + 0.45 z; channel i = 0.5 + 0.25 sin(a_i s + b_i + 1.9 class) + 0.25 sin(0.21 (i + 1) z + 0.5 x),
    (a, b) = (1, 0), (0.63, 1.3), (0.37, 2.1); pixels without depth are sky-coloured.  pose: 4x4 camera->world.
    To that, the texture of the feature's planning, every channel adds 0.15 sin(2.5 z + 1.3 x + 0.7 y + i), a wave of 2.1 m: a fern's
    cell mean keeps it, and it is what lets a pose search tell places 0.1 m apart along a street of flat ground and flat walls
    (the planned texture's luminance moves by 0.1, the search's colour gate, only over a metre)."""
    d = np.asarray(depth_mm, np.uint16)
    H, W = d.shape
    zc = d.astype(np.float64) / 1000.0
    i, j = np.arange(W) + 0.5, np.arange(H) + 0.5
    pc = np.stack([(i[None, :] - cam["cx"]) / cam["fx"] * zc, (j[:, None] - cam["cy"]) / cam["fy"] * zc, zc], axis=-1)
    T = np.asarray(pose, np.float64)
    pw = pc @ T[:3, :3].T + T[:3, 3]
    x, y, z = pw[..., 0], pw[..., 1], pw[..., 2]
    s = 0.9 * x + 1.7 * y + 0.45 * z
    k = np.asarray(sem, np.float64)
    ch = [0.5 + 0.25 * np.sin(a * s + b + 1.9 * k) + 0.25 * np.sin(0.21 * (n + 1) * z + 0.5 * x) + 0.15 * np.sin(2.5 * z + 1.3 * x + 0.7 * y + n)
          for n, (a, b) in enumerate(_AB)]
    rgb = np.clip(np.rint(np.stack(ch, axis=-1) * 255.0), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.where((d != 0)[..., None], rgb, SKY[None, None, :]))


# ---------------------------------------------------------------------------------------------------------------------
# the drive: out along the street of tests/retire_ref.py, away, and back over the same stretch with a drifted pose
# ---------------------------------------------------------------------------------------------------------------------
CAM, OVER = rr.CAM, rr.OVER
N_OUT, N_AWAY, N_RAMP, N_BACK, N_REVISIT = 30, 20, 20, 18, 5
# what the odometry has gathered by the time the camera is back: 18.4 m and 5 degrees, world->world.  The drifted street lies
# beside the mapped one, so nothing fused on the way back touches the old map and nothing of it is in view of the believed pose.
DRIFT = dict(x=18.0, z=4.0, yaw_deg=5.0)
# the revisit frames: outbound frame 14, 13, ... seen again from this far beside it (camera x, z in metres, yaw in degrees)
REVISIT_OFFSETS = ((0.3, 0.0, 1.0), (-0.3, 0.25, -1.5), (0.3, 0.0, 1.0), (-0.3, 0.25, -1.5), (0.3, 0.0, 1.0))
REVISIT_OF = (22, 21, 20, 19, 18)                         # (a parked car 5 m ahead: the street alone does not fix the place along it)
# the way back is driven in reverse 3.5 m beside the way out: views that far aside are unlike every keyframe (186 ferns or more),
# so nothing is recognised before the camera is back in its old lane
BACK_LANE = 3.5
CAPACITY = 760                                           # max_sqrt_vertices that holds the whole drive without retirement


def _drift(w):
    """the fraction w of DRIFT as a 4x4 world->world matrix: the rotation about the vertical through the origin, then the shift"""
    a = math.radians(DRIFT["yaw_deg"] * w)
    G = np.eye(4)
    G[:3, :3] = [[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]]
    G[:3, 3] = (DRIFT["x"] * w, 0.0, DRIFT["z"] * w)
    return G


def _offset(pose, x, z, yaw_deg):
    a = math.radians(yaw_deg)
    D = np.eye(4)
    D[:3, :3] = [[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]]
    D[:3, 3] = (x, 0.0, z)
    return np.asarray(pose, np.float64) @ D


def drive_poses():
    """[(true 4x4, believed 4x4, leg)]: `out` at the true poses; `away` further down the street; `ramp` further still while the
    drift comes in, a twentieth per frame; `back` in reverse in the lane beside, facing the same way, with all of it; `revisit` within 0.4 m and
    1.5 degrees of outbound views"""
    from surfelmapping_amd import synth
    out = synth.kitti_trajectory(N_OUT + N_AWAY + N_RAMP, step=0.8)
    poses = [(p, p, "out" if k < N_OUT else "away") for k, p in enumerate(out[:N_OUT + N_AWAY])]
    for j, p in enumerate(out[N_OUT + N_AWAY:]):
        poses.append((p, _drift((j + 1) / N_RAMP) @ p, "ramp"))
    G = _drift(1.0)
    z_far, z_near = out[-1][2, 3], out[REVISIT_OF[0] + 1][2, 3]
    for j in range(N_BACK):
        p = synth.pose_matrix(BACK_LANE, 0.0, z_far + (z_near - z_far) * (j + 1) / N_BACK, 0.0)
        poses.append((p, G @ p, "back"))
    for k, off in zip(REVISIT_OF, REVISIT_OFFSETS):
        p = _offset(out[k], *off)
        poses.append((p, G @ p, "revisit"))
    return poses


def render(true, believed, leg):
    """one frame of the street with the smooth texture: dict(rgb, depth, sem, true (4x4), believed (4x4), leg)"""
    from surfelmapping_amd import synth
    _, depth, sem = synth.Scene(3, n_boxes=10, length=150.0).render(synth.Camera(**CAM), true)
    return dict(rgb=recolour(depth, sem, true, CAM), depth=depth, sem=sem, true=true, believed=believed, leg=leg)


@functools.lru_cache(maxsize=None)
def drive():
    """the frames of the drive, rendered once per process and shared: a tuple of render()'s dicts, not to be written to"""
    return tuple(render(*p) for p in drive_poses())


def settle_frames():
    """two frames between the way back and the first revisit frame, in its lane and at its spacing, for a caller whose tracker
    starts from the constant-velocity guess (the facade's processFrame without a pose)"""
    from surfelmapping_amd import synth
    out = synth.kitti_trajectory(N_OUT, step=0.8)
    G = _drift(1.0)
    return tuple(render(p, G @ p, "settle") for p in (_offset(out[REVISIT_OF[0] + 2], *REVISIT_OFFSETS[0]), _offset(out[REVISIT_OF[0] + 1], *REVISIT_OFFSETS[0])))


def keyframe_policy(codes, ok, add_above=0.2, n_ferns=512):
    """which frames sm_set_auto_place makes keyframes when nothing is closed: frame T of `codes` is looked at iff ok[T] (its track
    was SM_TRACK_OK) and added iff the database is empty or float32(dis_any) > add_above * float32(n_ferns).  Returns the list of T."""
    kept = []
    for T, c in enumerate(codes):
        if not ok[T]:
            continue
        if not kept or f32(int(dis_all(c, np.stack([codes[k] for k in kept])).min())) > f32(add_above) * f32(n_ferns):
            kept.append(T)
    return kept
