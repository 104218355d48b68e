"""The shapes of tests/test_track_pin.py and what the restatements (tests/track_ref.py, tests/track_rgb_ref.py) say about them.
Nothing here needs a GPU: a scene's model comes from a `backend` -- the product on the GPU, or the CPU oracle, whose model is
equal bit for bit (tests/backends.py) -- so the choice of scenes and the conditions they must meet are checked on the CPU, and
the GPU tests compare the kernels with the same numbers.

A shape W x H is a camera of KITTI's field of view (fx = fy = 0.58 W, a principal point off the pixel grid), frames 0..2 of a
slow walk into a synth.Scene fused at their poses, and frame 3 evaluated at its true pose displaced by (0.03, -0.02, 0.05) m.
The scene is a room whose size follows the focal length (`room`): with KITTI's field of view on a few dozen pixels, one pixel of
the street scene spans more than the tracker's 0.3 m association gate and next to nothing pairs, so the surfaces come closer as
the image gets smaller (the far wall about 0.11 fx metres away: a pixel spans about 0.1 m there).  The colours are a smooth
function of the world point, so that the photometric term has inliers at every pyramid level.  The one shape beyond the
workgroup clamp is analytic: two tilted planes."""
import math

import numpy as np

import track_ref as tr
import track_rgb_ref as rr

f32 = np.float32
BORDER = 2.0                                  # stereo_border of every shape: narrow images are not blanked
DISPLACE = (0.03, -0.02, 0.05)
TRACK_BLOCK, TRACK_MAX_PARTS = 256, 1024      # sm_k_track.h

# W, H, nb, the branch of track_sum_parts / the reduction it is there for
SHAPES = [
    (24, 10, 1, "n < 256: a wave with no lane in range, n no multiple of 64"),
    (40, 24, 1, "one workgroup, the last grid-stride trip partial"),
    (64, 40, 3, "nb < 8: five of the eight sub-sums have no partial"),
    (96, 80, 8, "exactly one partial per sub-sum"),
    (128, 72, 9, "tail loop only, uneven"),
    (200, 125, 25, "unrolled loop entered for sub 0 only"),
    (264, 128, 33, "unrolled loop plus tail"),
]
BIG = (1448, 725, 1024, "the clamp: lanes of the first workgroups take a fifth trip")
RGB_SHAPES = [(70, 37), (131, 67), (200, 125), (264, 128)]
SOLVE_SHAPES = [(64, 40), (200, 125), (264, 128)]


def nb_of(n):
    """workgroups of the reductions over a grid of n points (sm_track.hip track_params)"""
    return min(TRACK_MAX_PARTS, max(1, (n + TRACK_BLOCK * 4 - 1) // (TRACK_BLOCK * 4)))


def grid_points(W, H, stride=1):
    return ((W + stride - 1) // stride) * ((H + stride - 1) // stride)


def camera(W, H):
    return dict(width=W, height=H, fx=0.58 * W, fy=0.58 * W, cx=0.5 * W - 0.3, cy=0.5 * H + 0.2)


def config_over(W, H):
    """the config fields every context of a shape is made with (besides the camera)"""
    return dict(preprocess=0, stereo_border=BORDER, max_sqrt_vertices=max(64, 2 * int(math.ceil(math.sqrt(W * H)))))


def texture(depth_mm, pose, cam):
    """rgb uint8[H][W][3]: a smooth function of the world point every pixel sees (sky: a constant)"""
    W, H = cam["width"], cam["height"]
    z = np.asarray(depth_mm, np.float64) / 1000.0
    x = (np.arange(W) + 0.5 - cam["cx"]) / cam["fx"]
    y = (np.arange(H) + 0.5 - cam["cy"]) / cam["fy"]
    pc = np.stack([x[None, :] * z, y[:, None] * z, z], axis=-1)
    P = np.asarray(pose, np.float64)
    pw = pc @ P[:3, :3].T + P[:3, 3]
    a = 0.5 + 0.22 * np.sin(pw[..., 0] * 1.3 + 0.4 * pw[..., 2]) + 0.18 * np.cos(pw[..., 2] * 0.9 - 0.7 * pw[..., 1])
    b = 0.5 + 0.3 * np.sin(pw[..., 1] * 2.1 + pw[..., 0] * 0.5)
    c = 0.5 + 0.3 * np.cos(pw[..., 2] * 0.6 + pw[..., 0] * 0.8)
    rgb = np.clip(np.rint(np.stack([a, b, c], axis=-1) * 255.0), 0, 255).astype(np.uint8)
    rgb[np.asarray(depth_mm) == 0] = (135, 206, 235)
    return np.ascontiguousarray(rgb)


_frames = {}


def room(zf):
    """synth.Scene as a room whose far wall is 1.1 zf ahead: ground 0.3 zf below the camera, side walls 0.6 zf away and as high
    as the view, two boxes before the far wall"""
    from surfelmapping_amd import synth
    s = synth.Scene(seed=0, n_boxes=0)
    s.ground_y, s.wall_x, s.wall_top = 0.3 * zf, 0.6 * zf, -100.0
    s.boxes = np.array([[-100.0, -100.0, 1.1 * zf, 100.0, s.ground_y, 1.1 * zf + 1.0],
                        [-0.30 * zf, 0.05 * zf, 0.8 * zf, 0.05 * zf, s.ground_y, 1.1 * zf],
                        [0.25 * zf, -0.25 * zf, 0.9 * zf, 0.6 * zf, s.ground_y, 1.1 * zf]], np.float64)
    return s


def frames(W, H):
    """(cam, poses, seq): frames 0..3 of the shape, seq[k] = (rgb, depth, sem, pose16)"""
    if (W, H) not in _frames:
        from surfelmapping_amd import synth
        cam = camera(W, H)
        zf = max(2.0, min(12.0, 0.1 * cam["fx"]))
        poses = [synth.pose_matrix(0.0, 0.0, 0.05 * zf * k, 5.0 + 0.3 * k) for k in range(4)]
        scene = room(zf)
        seq = []
        for p in poses:
            _, depth, sem = scene.render(synth.Camera(**cam), p)
            seq.append((texture(depth, p, cam), depth, sem, synth.pose_to_colmajor(p)))
        _frames[(W, H)] = (cam, poses, seq)
    return _frames[(W, H)]


def eval_pose(true_pose):
    pe = np.asarray(true_pose, np.float64).copy()
    pe[:3, 3] += DISPLACE
    return pe.astype(f32)


def turned(T, deg, axis=(0.3, 1.0, -0.2)):
    """T (4x4) turned by deg degrees about `axis` through its centre, as float32"""
    ax = np.asarray(axis, np.float64)
    G = np.asarray(T, np.float64).copy()
    G[:3, :3] = tr.se3_exp(np.r_[0.0, 0.0, 0.0, ax / np.linalg.norm(ax) * math.radians(deg)])[:3, :3] @ G[:3, :3]
    return G.astype(f32)


def fused(backend, W, H):
    """the context backend(cam, **config fields) makes -- a SurfelMap or an Oracle -- after frames 0..2"""
    cam, _, seq = frames(W, H)
    m = backend(cam, **config_over(W, H))
    for fr in seq[:3]:
        m.process_frame(*fr)
    return m


class Case:
    """what the restatement says of one synthetic shape, given the fused model (rows = slots)"""

    def __init__(self, W, H, model):
        self.W, self.H = W, H
        self.cam, self.poses, self.seq = frames(W, H)
        self.model = model
        self.t_prev = self.seq[2][3]
        self.rgb, self.depth = self.seq[3][0], self.seq[3][1]
        self.pe = eval_pose(self.poses[3])
        self.pred = tr.predict(model, self.t_prev, self.cam)
        self._terms, self._photo = {}, {}

    def vertex(self, stride=1):
        return tr.vertex_normal(self.depth, self.cam, stereo_border=BORDER, stride=stride)

    def terms(self, level=0, pred=None):
        """the geometric products at the evaluation pose on the grid of stride 2^level"""
        if pred is not None:
            vm, nm = self.vertex(1 << level)
            return tr.system_terms(vm, nm, pred, self.model, self.pe, self.t_prev, self.cam)
        if level not in self._terms:
            vm, nm = self.vertex(1 << level)
            self._terms[level] = tr.system_terms(vm, nm, self.pred, self.model, self.pe, self.t_prev, self.cam)
        return self._terms[level]

    def photo(self, level=0):
        """the photometric products at the evaluation pose at `level`"""
        if level not in self._photo:
            plane = rr.gather(self.pred, self.model)
            pyr = rr.pyramid(self.rgb, level + 1)
            self._photo[level] = rr.photo_terms_products(plane, self.depth, pyr[level], self.pe, self.cam, level=level,
                                                         stride=1 << level, stereo_border=BORDER)
        return self._photo[level]

    def track(self, guess, **kw):
        return tr.track(self.depth, self.model, self.t_prev, guess, self.cam, stereo_border=BORDER, **kw)

    def track_rgb(self, guess, **kw):
        return rr.track(self.rgb, self.depth, self.model, self.t_prev, guess, self.cam, stereo_border=BORDER, **kw)


# ---- the shape beyond the clamp: analytic ----
PLANES = (((0.28, 0.10, 1.0), 8.0), ((-0.24, 0.14, 1.0), 10.0))      # (normal direction, n . p): left and right half


def big_scene():
    """1448 x 725: (cam, depth uint16[H][W] of two tilted planes, model float32[n][12] with one surfel per pixel of odd i + j on
    the ray through (i, j) -- the pixel the prediction's rounding rule gives it without a tie --, positions and normals float32)"""
    W, H = BIG[0], BIG[1]
    cam = camera(W, H)
    fx, fy, cx, cy = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    half = W // 2
    # the depth image: z of the plane of the pixel's half along the ray through the pixel centre
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    dx, dy = (i + 0.5 - float(cx)) / float(fx), (j + 0.5 - float(cy)) / float(fy)
    z = np.zeros((H, W))
    for side, (n, c) in enumerate(PLANES):
        sel = (i < half) == (side == 0)
        z[sel] = (c / (n[0] * dx + n[1] * dy + n[2]))[sel]
    depth = np.rint(z * 1000.0).astype(np.uint16)
    # the model, float32 throughout
    sel = ((i + j) & 1) == 1
    si, sj = i[sel].astype(f32), j[sel].astype(f32)
    rx, ry = (si - cx) / fx, (sj - cy) / fy
    left = i[sel] < half
    nrm = np.where(left[:, None], np.asarray(PLANES[0][0], f32), np.asarray(PLANES[1][0], f32)).astype(f32)
    cc = np.where(left, f32(PLANES[0][1]), f32(PLANES[1][1])).astype(f32)
    zz = (cc / ((nrm[:, 0] * rx + nrm[:, 1] * ry) + nrm[:, 2])).astype(f32)
    ln = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]).astype(f32)
    model = np.zeros((len(zz), 12), f32)
    model[:, 0], model[:, 1], model[:, 2] = rx * zz, ry * zz, zz
    model[:, 3] = 10.0
    model[:, 4] = np.full(len(zz), 0x00808080, np.uint32).view(f32)
    model[:, 8:11] = nrm / ln[:, None]
    model[:, 11] = 0.02
    return cam, depth, model


def spread_of_pivot_ratio(sys29, bound28, centre, draws=32, seed=0):
    """the largest relative change of tr.pivot_ratio when the 28 sums move by +- their entry bounds with random signs"""
    rng = np.random.default_rng(seed)
    base = tr.pivot_ratio(sys29, centre)
    worst = 0.0
    for _ in range(draws):
        s = np.asarray(sys29, np.float64).copy()
        s[:28] += rng.choice((-1.0, 1.0), 28) * bound28
        worst = max(worst, abs(tr.pivot_ratio(s, centre) - base) / base)
    return worst
