"""The frame path at the image shapes the rest of the suite never reaches: HIP against the oracle, bit for bit.

sm_create accepts any width, height > 0, and much of the frame path's bookkeeping follows the shape: the transposed 32 x 32
tiles of the image preparation, the 14 x 30 tiles of the depth filter chain with their halos of 8, 7 and 1, the pixel pairs of
the association (two consecutive column-major pixels per thread, of which the checkerboard one is taken), the association
blocks of 256 pixels, the candidate groups of 4, 8 or 16 blocks and the one or two rounds of their sum.  Every shape of the two
tables below runs one short scenario through every frame form the product has (FORMS) and is compared with the oracle after
every synchronised step: the counters and the three depth textures; mid-sequence and at the end also the model, the index
map predicted from a second pose and the raw feedback cloud; at the very end the model after one cleanPoints.

The scenario (scene()): a smooth depth surface z = 6 - z_cam + 0.3 sin(x / 7) + 0.2 cos(y / 5) that stands still in the world
while the camera advances, seen twice from the same pose (fuses), from 0.2 m further on (new surfels, and with fuseThresh = 0
conflicts wherever the resampled surface comes out a hair behind a surfel) and twice from 0.6 m further away than it is
(conflicts wholesale: on the small shapes more than W*H of them, so the cap binds or, with conflict_cap = 0, does not).
Columns from W / 2 on carry class 3 and, on images of at least 32 x 32, a patch carries the movable class 13 (removeMovings
drops it on the frames where the surface jumps).

What keeps the comparison honest is asserted on the oracle alone (check_honest): the fuse / conflict / append sums of every
shape over its sequence; the figures measured when the test was written stand next to the table.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from backends import assert_models_equal, make
from surfelmapping_amd import synth
from test_gpu_parity import COUNT_KEYS, assert_models_equal_nan_tolerant

pytestmark = pytest.mark.gpu

# ---- the shapes (W, H): one line each, with the reason it is here.  Measured on the oracle, summed over the 8 frames of scene(),
# conflict_cap = 1: (unstable, conflict, fused) with preprocess = 0 | with preprocess = 1.
SMALL_SHAPES = [
    (1, 1),    # (0, 0, 0) | (0, 0, 0)                  P = 1, no checkerboard pixel at all
    (2, 1),    # (7, 3, 0) | (0, 0, 0)                  one candidate; H = 1 wraps a column inside every pair
    (1, 2),    # (7, 3, 0) | (0, 0, 0)                  one candidate; one column: the pair logic never leaves it
    (3, 3),    # (19, 12, 9) | (0, 0, 0)                P odd; the last pair is half empty
    (7, 5),    # (96, 64, 23) | (0, 0, 0)               narrower than the chain's halo of 8
    (5, 63),   # (892, 647, 207) | (0, 0, 0)            P = 315: one full pixel block plus a partial one; one association workgroup
    (63, 5),   # (872, 618, 227) | (0, 0, 0)            the same, H odd and small: many column wraps inside pairs
    (13, 29),  # (985, 728, 331) | (66, 47, 11)         one pixel less than a chain tile both ways
    (15, 31),  # (1220, 900, 404) | (213, 158, 46)      one more than a chain tile: 2 x 2 chain tiles with 1-pixel slivers; smaller than a prep tile
    (33, 33),  # (2958, 1956, 850) | (1379, 978, 259)   one more than a prep tile; P = 1089 odd; 5 pixel blocks (odd: the last workgroup holds one block)
    (31, 65),  # (5682, 3870, 1367) | (3260, 2432, 660) H = 2 * 32 + 1
    (257, 3),  # (2217, 1524, 478) | (0, 0, 0)          a wave's 128 pixels span 43 columns
    (3, 257),  # (2244, 1561, 451) | (0, 0, 0)          ... or a third of one
    (128, 2),  # (727, 498, 169) | (0, 0, 0)            smallest even H
    (64, 8),   # (1415, 1002, 377) | (298, 228, 66)     P = 512 exactly: one workgroup, nothing partial (the control)
]
# ---- the size classes of the candidate groups (sm_create: 4, 8 or 16 association blocks per group): (W, H, blocks, cg, groups)
SIZE_CLASSES = [
    (1024, 512, 2048, 4, 512),     # last size of the first class, exactly one full round of the group sum
    (1024, 513, 2052, 8, 257),     # first size of the middle class; its last group is half full
    (2049, 1024, 8196, 16, 513),   # first size that needs the second round of the group sum
]

N_FRAMES = 8
SYNC_AFTER = (1, 4, 7)             # the asynchronous forms run bursts of 2, 3 and 3 frames
FULL_AFTER = (4, 7)                # model, index map and raw cloud: once mid-sequence, once at the end
FORMS = [                          # (name, how a frame is handed over, compact_period)
    ("sync, every frame compacts", "sync", 1),         # k_associate + k_append_scan
    ("sync, deferred compaction", "sync", 1000),       # direct append
    ("device bursts", "device", 24),                   # the association rides on the next frame's preparation launch
    ("async host buffers", "async", 4),                # the input ring
]
POSE2 = synth.pose_to_colmajor(synth.pose_matrix(0.05, -0.02, 0.1, 2.0))      # the index map's second pose


def camera(W, H):
    f = 0.8 * max(W, 8)
    return W, H, f, f, W / 2 - 0.5, H / 2 - 0.5


def scene(W, H):
    """[(rgb, depth_mm, sem, pose16)] * N_FRAMES -- a function of the shape alone"""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rgb = np.stack([(7 * x + 3 * y) % 256, (5 * x + 11 * y + 40) % 256, (13 * x + y + 90) % 256], axis=-1).astype(np.uint8)
    sem = np.where(x >= W // 2, 3, 0).astype(np.uint8)
    if W >= 32 and H >= 32:
        sem[H // 4:H // 2, W // 8:W // 4] = 13
    #        reference, new,  fuse, far,  step, fuse, step+far, back
    z_cam = (0.0, 0.0, 0.0, 0.0, 0.2, 0.2, 0.4, 0.4)
    far = (0.0, 0.0, 0.0, 0.6, 0.0, 0.0, 0.6, 0.0)
    out = []
    for k in range(N_FRAMES):
        z = 6.0 - z_cam[k] + far[k] + 0.3 * np.sin(x / 7.0) + 0.2 * np.cos(y / 5.0)
        depth = np.rint(z * 1000.0).astype(np.uint16)
        out.append((rgb, depth, sem, synth.pose_to_colmajor(synth.pose_matrix(0.0, 0.0, z_cam[k]))))
    return out


def capacity(W, H):
    """sqrt of the model's capacity: every frame may append its W*H / 2 candidates"""
    return max(64, int(math.ceil(math.sqrt(N_FRAMES * (W * H // 2 + 1)))))


class Form:
    """one HIP context and the way it is given its frames"""

    def __init__(self, name, kind, period, W, H, **over):
        self.name, self.kind = name, kind
        self.h = make("hip", *camera(W, H), compact_period=period, **over)      # (a null context raises: a listed shape never skips)
        self.P = W * H
        if kind == "device":
            self.dev = [tuple(self.h.device_alloc(n * self.P) for n in (3, 2, 1)) for _ in range(3)]
        if kind == "async":
            self.ring = [self.h.host_frame(), None, self.h.host_frame()]
            self.used = [False] * 3

    def frame(self, k, rgb, depth, sem, pose):
        h = self.h
        if self.kind == "sync":
            h.process_frame(rgb, depth, sem, pose)
        elif self.kind == "device":
            bufs = self.dev[k % 3]                     # (a set is written again only after the sync() that ends its burst)
            for dst, src in zip(bufs, (rgb, depth, sem)):
                h.device_upload(dst, src)
            h.process_frame_device(*bufs, pose)
        else:
            bufs = self.ring[k % 3]
            if bufs is None:                           # pageable arrays: staged inside the call
                h.process_frame_async(np.ascontiguousarray(rgb), np.ascontiguousarray(depth), np.ascontiguousarray(sem), pose)
            else:                                      # pinned frame block: read in place
                if self.used[k % 3]:
                    h.inputs_consumed()
                self.used[k % 3] = True
                for dst, src in zip(bufs, (rgb, depth, sem)):
                    np.copyto(dst, src)
                h.process_frame_async(*bufs, pose)

    def settled(self, k):
        if self.kind == "sync":
            return True
        if k in SYNC_AFTER:
            self.h.sync()
            return True
        return False


def check_honest(W, H, pre, sums):
    """the issue's conditions on the inputs, on the oracle alone"""
    need_conflicts = W * H >= 2
    need_fuses = min(W, H) >= 5
    if pre:
        need_conflicts = need_fuses = min(W, H) >= 8      # thinner: nothing passes the 7-of-8 support rule
    if need_conflicts:
        assert sums["unstable_count"] > 0 and sums["conflict_count"] > 0, (W, H, pre, sums)
    if need_fuses:
        assert sums["fused_count"] > 0, (W, H, pre, sums)


def run_shape(W, H, pre, cap):
    over = dict(preprocess=pre, stereo_border=0.0, conflict_cap=cap, max_sqrt_vertices=capacity(W, H))
    o = make("oracle", *camera(W, H), **over)
    forms = [Form(name, kind, period, W, H, **over) for name, kind, period in FORMS]
    seq = scene(W, H)
    sums = dict(unstable_count=0, conflict_count=0, fused_count=0)
    for k, fr in enumerate(seq):
        o.process_frame(*fr)
        co = {key: o.counts()[key] for key in COUNT_KEYS}
        for key in sums:
            sums[key] += co[key]
        tex = [o.download_depth(which) for which in range(3)]
        full = None
        if k in FULL_AFTER:
            model, cloud = o.download_model(), o.download_raw_cloud()
            o.stage_predict_indices(POSE2, k + 1, 30.0, 200)
            full = (model, cloud, o.download_index_map(), o.counts()["visible_count"])
        for f in forms:
            what = f"{W}x{H} preprocess={pre} cap={cap}, {f.name}, frame {k}"
            f.frame(k, *fr)
            if not f.settled(k):
                continue
            ch = f.h.counts()
            assert co == {key: ch[key] for key in COUNT_KEYS}, what
            for which, name in enumerate(("DEPTH_METRIC", "DEPTH_FILTERED", "LAST")):
                got = f.h.download_depth(which)
                assert np.array_equal(tex[which].view(np.uint32), got.view(np.uint32)), \
                    f"{what}: {name} differs in {(tex[which] != got).sum()} pixels"
            if full is None:
                continue
            assert_models_equal(full[0], f.h.download_model(), what)
            assert_models_equal_nan_tolerant(full[1], f.h.download_raw_cloud(), what + ": raw cloud")
            f.h.stage_predict_indices(POSE2, k + 1, 30.0, 200)
            got = f.h.download_index_map()
            assert np.array_equal(full[2][0], got[0]), what + ": index"
            for a, b, name in zip(full[2][1:], got[1:], ("vertConf", "colorTime", "normRad")):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: {name}"
            assert full[3] == f.h.counts()["visible_count"], what + ": visible_count of the second pose"
    check_honest(W, H, pre, sums)
    _, depth, sem, pose = seq[5]
    o.clean_points(depth, sem, pose)
    model = o.download_model()
    for f in forms:
        f.h.clean_points(depth, sem, pose)
        assert_models_equal(model, f.h.download_model(), f"{W}x{H} preprocess={pre} cap={cap}, {f.name}, after cleanPoints")
    return sums


@pytest.mark.parametrize("cap", [1, 0])
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_shapes(shape, pre, cap):
    run_shape(*shape, pre, cap)


@pytest.mark.parametrize("shape,pre", [(s, 0) for s in SIZE_CLASSES] + [(SIZE_CLASSES[1], 1)],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"pre{v}")
def test_size_class_shapes(shape, pre):
    """That 1024 x 513 and 2049 x 1024 come out bit-exact IS the evidence that the 8-block candidate groups and the second round
    of the group sum ran: no new surfel gets its slot number without them."""
    W, H, blocks, cg, groups = shape
    assert (W * H + 255) // 256 == blocks and (blocks + cg - 1) // cg == groups             # the table's own arithmetic
    assert cg == (4 if blocks <= 2048 else 8 if blocks <= 4096 else 16)
    run_shape(W, H, pre, 1)


@pytest.mark.parametrize("shape", SIZE_CLASSES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("env", [{"SM_TWO_LAUNCH": "0"}, {"SM_DEFER_ASSOC": "0"}], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_size_classes_behind_kernel_switches(env, shape):
    """SM_TWO_LAUNCH=0: the candidate counts come from the fixup launch's own workgroups (one template instance per group size)
    instead of the lean loop behind the surfel pass.  SM_DEFER_ASSOC=0: every asynchronous frame launches its own association.
    The switches are read when the library creates a context, so each runs its size-class case in a fresh child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    case = f"tests/test_frame_shapes.py::test_size_class_shapes[{shape[0]}x{shape[1]}-pre0]"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", case], cwd=root, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-1500:]
    assert "\n1 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]        # the case exists and ran
