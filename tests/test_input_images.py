"""One current depth image and one current class image per context, whichever call gave it.

The reference uploads into ONE depth and ONE class texture (src/SurfelMapping.cpp:122-128, 498-499): a null image means "keep
what is in the texture", whichever call put it there.  The HIP core has several ways in (host images waited for, host images
not waited for through a ring of device input sets, images already on the device, cleanPoints, the per-pass set_frame, the
sharded forms); every one of them must make an image it is given current for all the others, and read the current one for a
null.  Every case here is a script of calls played on the oracle and on the HIP core with the same None's; counters after
every synchronising step and the downloaded model must be bit-identical.

The scripts themselves are checked on the CPU alone (test_script_distinguishes_*): played on the oracle with the WRONG image
in place of each null -- the one a home of its own per entry point would supply -- the final model must differ from the right
one in its surfel count or in at least 1 % of its rows.  A script that cannot tell the images apart proves nothing."""
import math
import os

import numpy as np
import pytest

from backends import assert_models_equal, make
from surfelmapping_amd import synth

W, H = 64, 48
CAM = (W, H, 50.0, 50.0, 31.5, 23.5)
IN_RING = 3                                    # sm_ctx::IN_RING, the device input sets of sm_process_frame_async
COUNT_KEYS = ("count", "offset", "data_count", "conflict_count", "unstable_count", "fused_count", "visible_count", "tick")
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# Scenes and poses
# ---------------------------------------------------------------------------------------------------------------------
_scene_cache = {}
CLASSES = np.array([c for c in range(19) if c not in (10, 11, 12)], np.uint8)   # (the depth filters drop classes 10-12 whole)


def scene(k):
    """(rgb, depth_mm, class) of scene k: a wavy surface about 3 m away whose waves differ from scene to scene, so that two
    scenes' surfaces cross (fused where they are within the threshold, conflicts and new surfels elsewhere); class 3 on the
    left half in every scene (fusion needs equal classes), scene-specific classes on the right; random colours.  Different
    scenes, not noise variants of one."""
    if k not in _scene_cache:
        rng = np.random.default_rng(7000 + k)
        yy, xx = np.mgrid[0:H, 0:W]
        d = 3.0 + 0.05 * k + 0.2 * np.sin(xx / (6.0 + k) + k) + 0.12 * np.cos(yy / (5.0 + 0.5 * k) - k)
        depth = np.rint(d * 1000.0).astype(np.uint16)
        depth[rng.random((H, W)) < 0.005] = 0                                  # holes
        sem = np.where(xx < W // 2, np.uint8(3), CLASSES[(2 * (yy // 24) + 5 * k + 1) % len(CLASSES)]).astype(np.uint8)
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for a in (rgb, depth, sem):
            a.setflags(write=False)                                            # shared among the tests: nobody writes to them
        _scene_cache[k] = (rgb, depth, sem)
    return _scene_cache[k]


def pose(k):
    """a camera that moves sideways, forward and turns, slowly enough for a re-read image to fuse with its own surfels"""
    return synth.pose_to_colmajor(synth.pose_matrix(0.02 * k, 0.0, 0.012 * k, 1.0 * math.sin(0.9 * k)))


ZERO_D, ZERO_S = np.zeros((H, W), np.uint16), np.zeros((H, W), np.uint8)
STEREO_SHIFT = 4                                # the right image is the left one seen 4 px further left: 50 * 0.54 / 4 = 6.75 m
STEREO_MM = 6750


def stereo_right(left):
    return np.ascontiguousarray(np.roll(left, -STEREO_SHIFT, axis=1))


# ---------------------------------------------------------------------------------------------------------------------
# Scripts.  A step is (form, scene, depth given?, class given?); its pose is pose(position in the script).
#   forms that take a frame: "sync" (process_frame), "async_block" / "async_pinned" / "async_pageable" (process_frame_async
#   from a pinned frame block, separate pinned arrays, a pageable array), "device" (process_frame_device), "stereo"
#   (process_frame_stereo), "shard" / "shard_device"; others: "clean" (clean_points), "set_sem" (set_frame(sem=...)),
#   "reset", "sync_counts" (sync() and compare the counters), "download" (compare the model).
# ---------------------------------------------------------------------------------------------------------------------
FRAME_FORMS = ("sync", "async_block", "async_pinned", "async_pageable", "device", "stereo", "shard", "shard_device")
KIND = dict(sync="host", clean="host", set_sem="host", shard="host", async_block="ring", async_pinned="ring",
            async_pageable="ring", device="device", stereo="device", shard_device="device")


def images_of(step, stereo_depth=None):
    """(rgb, depth or None, class or None) the step hands over"""
    form, k, gd, gs = step
    rgb, d, s = scene(k)
    if form == "stereo":
        d = np.full((H, W), STEREO_MM, np.uint16) if stereo_depth is None else stereo_depth
    return rgb, (d if gd else None), (s if gs else None)


def resolve(script, policy):
    """The script with every null replaced by an image: policy "right" -> the current one (what the reference reads);
    "host_home" -> the last one a host form that waits gave, else zeros (today's d_depth_raw / d_sem); "ring_home" -> the
    last one the async form gave, else the host home (today's in_last_*); "first" -> the very first frame's.  Returns the
    explicit steps [(form, rgb, depth, class, pose)] and whether any image differs from the right policy's."""
    cur = dict(d=ZERO_D, s=ZERO_S)
    host = dict(d=ZERO_D, s=ZERO_S)
    ring = dict(d=None, s=None)
    first = None
    out, differs = [], False
    for i, step in enumerate(script):
        form = step[0]
        if form in ("reset", "sync_counts", "download"):
            out.append((form, None, None, None, None))
            continue
        rgb, d, s = images_of(step)
        if first is None and form in FRAME_FORMS:
            first = dict(d=d if d is not None else ZERO_D, s=s if s is not None else ZERO_S)
        given = dict(d=d, s=s)
        use = {}
        for key in "ds":
            if given[key] is not None:
                cur[key] = given[key]
                if KIND[form] == "host":
                    host[key] = given[key]
                elif KIND[form] == "ring":
                    ring[key] = given[key]
                use[key] = given[key]
            else:
                wrong = dict(right=cur[key], host_home=host[key], ring_home=ring[key] if ring[key] is not None else host[key],
                             first=first[key] if first else cur[key])[policy]
                differs |= form in FRAME_FORMS and not np.array_equal(wrong, cur[key])
                use[key] = wrong
        out.append((form, rgb, use["d"], use["s"], pose(i)))
    return out, differs


def play_oracle(explicit, pre):
    o = make("oracle", *CAM, **over_of(pre))
    for form, rgb, d, s, p in explicit:
        if form in FRAME_FORMS:
            o.process_frame(rgb, d, s, p)
        elif form == "clean":
            o.clean_points(d, s, p)
        elif form == "set_sem":
            o.set_frame(sem=s)
        elif form == "reset":
            o.reset()
    return o.download_model()


def over_of(pre):
    return dict(preprocess=pre, stereo_border=3.0, max_sqrt_vertices=300, fuse_thresh=0.05)


def rows_differ(a, b):
    """fraction of rows that differ between two models of equal surfel count (1.0 if the counts differ)"""
    if a.shape != b.shape:
        return 1.0
    if a.shape[0] == 0:
        return 0.0
    return float((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).mean())


class Hip:
    """plays the steps of a script on a HIP context; keeps every device buffer it hands over alive and unchanged"""

    def __init__(self, pre, sharded=False, compact_period=3, **over):
        self.h = make("hip", *CAM, compact_period=compact_period, **dict(over_of(pre), **over))
        self.keep = []                         # device buffers handed to a device form: alive until the context goes
        self.block = self.pinned = None
        self.stereo_on = False
        if sharded:
            self.h.shard_stream_configure(0, 1)

    def device_images(self, rgb, d, s):
        h = self.h
        out = []
        for a in (rgb, d, s):
            if a is None:
                out.append(None)
                continue
            p = h.device_alloc(a.nbytes)
            h.device_upload(p, a)
            self.keep.append(p)
            out.append(p)
        return out

    def pinned_images(self, block, rgb, d, s):
        h = self.h
        if self.block is None:
            self.block = h.host_frame()
            self.pinned = (h.host_array((H, W, 3), np.uint8), h.host_array((H, W), np.uint16), h.host_array((H, W), np.uint8))
        bufs = self.block if block else self.pinned
        h.inputs_consumed()                    # before a pinned buffer is rewritten
        for dst, src in zip(bufs, (rgb, d, s)):
            if src is not None:
                np.copyto(dst, src)
        return bufs[0], (None if d is None else bufs[1]), (None if s is None else bufs[2])

    def scribble(self):
        """garbage over every pinned buffer, once the copies out of them are done"""
        self.h.inputs_consumed()
        for b in (self.block or ()) + (self.pinned or ()):
            b[...] = 0xA5 if b.dtype == np.uint8 else 0xA5A5

    def stereo_depth(self, left):
        if not self.stereo_on:
            self.h.set_stereo(max_disp=64)
            self.stereo_on = True
        return self.h.stereo_depth(left, stereo_right(left))[0]

    def step(self, form, rgb, d, s, p):
        h = self.h
        if form == "sync":
            h.process_frame(rgb, d, s, p)
        elif form == "async_block":
            assert d is not None and s is not None
            h.process_frame_async(*self.pinned_images(True, rgb, d, s), p)
        elif form == "async_pinned":
            h.process_frame_async(*self.pinned_images(False, rgb, d, s), p)
        elif form == "async_pageable":
            h.process_frame_async(np.array(rgb), None if d is None else np.array(d), None if s is None else np.array(s), p)
        elif form == "device":
            h.process_frame_device(*self.device_images(rgb, d, s), p)
        elif form == "stereo":
            assert d is not None
            h.process_frame_stereo(rgb, stereo_right(rgb), s, p)
        elif form == "shard":
            h.shard_frame(rgb, d, s, p)
        elif form == "shard_device":
            h.shard_frame_device(*self.device_images(rgb, d, s), p)
            h.sync()
        elif form == "clean":
            h.clean_points(d, s, p)
        elif form == "set_sem":
            h.set_frame(sem=s)
        elif form == "reset":
            h.reset()
        else:
            raise KeyError(form)

    def model(self, sharded=False):
        return self.h.shard_export_dense() if sharded else self.h.download_model()


def counts_equal(o, g, what, keys=COUNT_KEYS):
    co, cg = o.counts(), g.h.counts()
    print(what, {k: (co[k], cg[k]) for k in keys})
    assert {k: co[k] for k in keys} == {k: cg[k] for k in keys}, what


def models_equal(a, b, what, nan_ok=False):
    if nan_ok and a.shape == b.shape:           # a frame after reset() re-initialises with NaN payloads in raw normals
        same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        assert same.all(), what
        return
    assert_models_equal(a, b, what)


def run_pair(script, pre, what, sharded=False, min_surfels=500, scribble_after=None):
    """the script on the oracle and on the HIP core, the same None's to both; counters after every step that waits for the
    device, the model at every "download" and at the end"""
    o = make("oracle", *CAM, **over_of(pre))
    g = Hip(pre, sharded)
    had_reset = False
    for i, step in enumerate(script):
        form = step[0]
        tag = f"{what} pre={pre} step {i} {step}"
        if form == "sync_counts":
            g.h.sync()
            counts_equal(o, g, tag)
            continue
        if form == "download":
            models_equal(o.download_model(), g.model(sharded), tag, had_reset)
            continue
        if form == "reset":
            o.reset(); g.h.reset()
            had_reset = True
            continue
        sd = g.stereo_depth(scene(step[1])[0]) if form == "stereo" else None
        rgb, d, s = images_of(step, sd)
        if form in FRAME_FORMS:
            o.process_frame(rgb, d, s, pose(i))
        elif form == "clean":
            o.clean_points(d, s, pose(i))
        elif form == "set_sem":
            o.set_frame(sem=s)
        g.step(form, rgb, d, s, pose(i))
        if form in ("sync", "shard", "shard_device"):
            counts_equal(o, g, tag)
        elif form == "clean":
            counts_equal(o, g, tag, ("count", "tick"))
        if scribble_after is not None and i == scribble_after:
            g.scribble()
    g.h.sync()
    counts_equal(o, g, f"{what} pre={pre} end", ("count", "tick") if script[-1][0] in ("clean", "set_sem", "reset") else COUNT_KEYS)
    a = o.download_model()
    models_equal(a, g.model(sharded), f"{what} pre={pre} final model", had_reset)
    assert a.shape[0] >= min_surfels, (what, a.shape)
    return o, g


# ---------------------------------------------------------------------------------------------------------------------
# (a) every giver followed by every null reader; (b) depth and class current in different places; (c) the ring
# ---------------------------------------------------------------------------------------------------------------------
GIVERS = ("sync", "async_block", "async_pinned", "async_pageable", "device", "clean", "set_sem", "stereo")
READERS = ("sync", "async_pageable", "device")
NULLS = {"depth": (False, True), "class": (True, False), "both": (False, False)}


def giver_reader_script(giver, reader, nulls):
    gd, gs = NULLS[nulls]
    give = (giver, 1, giver != "set_sem", True)
    return [("sync", 0, True, True), give, (reader, 2, gd, gs), ("download",), (reader, 3, gd, gs)]


def giver_reader_cases():
    for giver in GIVERS:
        for reader in READERS:
            for nulls in NULLS:
                if giver == "stereo" and nulls != "class":
                    continue                   # its depth is an estimate: judged for the class image only
                if giver == "set_sem" and nulls == "depth":
                    continue                   # it gives no depth image: nothing of its own would be read
                yield giver, reader, nulls


NAMED = {
    # the three sequences that read the wrong image while each entry point kept a home of its own
    "async_A_then_sync_B_then_async_null_reads_B":
        [("sync", 0, True, True), ("async_pinned", 1, True, True), ("sync", 2, True, True), ("async_pageable", 3, False, False)],
    "async_A_then_clean_points_B_then_async_null_reads_B":
        [("sync", 0, True, True), ("async_block", 1, True, True), ("clean", 2, True, True), ("async_pinned", 3, False, False)],
    "async_A_then_sync_null_reads_A":
        [("sync", 0, True, True), ("async_pageable", 1, True, True), ("sync", 2, False, False), ("sync", 3, False, True)],
    "device_S_then_sync_null_class_reads_S":
        [("sync", 0, True, True), ("device", 1, True, True), ("sync", 2, True, False), ("sync", 3, False, False)],
    "device_S_then_async_null_class_reads_S":
        [("sync", 0, True, True), ("device", 1, True, True), ("async_pageable", 2, True, False), ("device", 3, False, False)],
}

SPLIT = {
    # depth only from one entry point, class only from another, then both null
    "async_then_sync": [("sync", 0, True, True), ("async_pinned", 1, True, False), ("sync", 2, False, True),
                        ("sync", 3, False, False), ("async_pageable", 3, False, False), ("device", 3, False, False)],
    "sync_then_device": [("sync", 0, True, True), ("sync", 1, True, False), ("device", 2, False, True),
                         ("device", 3, False, False), ("sync", 3, False, False), ("async_pinned", 3, False, False)],
    "device_then_async": [("sync", 0, True, True), ("device", 1, True, False), ("async_pageable", 2, False, True),
                          ("async_pinned", 3, False, False), ("device", 3, False, False), ("sync", 3, False, False)],
    "async_then_device": [("sync", 0, True, True), ("async_pageable", 1, True, False), ("device", 2, False, True),
                          ("sync", 3, False, False), ("async_pinned", 3, False, False)],
}


def ring_script(n_null):
    """one frame block, a run of nulls longer than twice the ring, a depth-only and a class-only frame that land in the ring
    sets around (n_null = 7) or exactly on (n_null = 8: frame 9 is set 0's again) the holder of the other image, two more nulls"""
    frames = [("async_block", 0, True, True)]
    frames += [("async_pinned" if k % 2 == 0 else "async_pageable", 1 + k % 3, False, False) for k in range(n_null)]
    frames += [("async_pinned", 4, True, False), ("async_pageable", 5, False, True),
               ("async_pinned", 1, False, False), ("async_pageable", 2, False, False)]
    s = []
    for k, fr in enumerate(frames):
        s.append(fr)
        if k in (4, 8):
            s.append(("sync_counts",))             # counters after frames 4 and 8, through a sync()
    return s


RING = {f"nulls_{n}": ring_script(n) for n in (2 * IN_RING + 1, 2 * IN_RING + 2)}

SCRIPTS = {f"giver_{g}-reader_{r}-null_{n}": giver_reader_script(g, r, n) for g, r, n in giver_reader_cases()}
SCRIPTS.update({f"named-{k}": v for k, v in NAMED.items()})
SCRIPTS.update({f"split-{k}": v for k, v in SPLIT.items()})
SCRIPTS.update({f"ring-{k}": v for k, v in RING.items()})


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_script_distinguishes_the_right_image_from_each_wrong_one(name):
    """CPU only.  The oracle with the image of each former home in place of the nulls must build another model than with the
    current image: another surfel count, or at least 1 % of the rows."""
    script = SCRIPTS[name]
    for pre in (0, 1):
        right = play_oracle(resolve(script, "right")[0], pre)
        assert right.shape[0] >= 500, (name, pre, right.shape)
        tried = 0
        for policy in ("host_home", "ring_home", "first"):
            explicit, differs = resolve(script, policy)
            if not differs:
                continue                       # this home happens to hold the current image in this script
            tried += 1
            wrong = play_oracle(explicit, pre)
            frac = rows_differ(right, wrong)
            assert frac >= 0.01, f"{name} pre={pre}: the {policy} image gives the same model ({right.shape[0]} vs {wrong.shape[0]} surfels, {frac:.4f} of rows differ)"
        assert tried >= 1, name


@gpu
@pytest.mark.parametrize("giver,reader,nulls", list(giver_reader_cases()))
def test_giver_then_null_reader(giver, reader, nulls):
    for pre in (0, 1):
        run_pair(giver_reader_script(giver, reader, nulls), pre, f"{giver} -> {reader} null {nulls}")


@gpu
@pytest.mark.parametrize("name", list(NAMED))
def test_named_sequence(name):
    for pre in (0, 1):
        run_pair(NAMED[name], pre, name)


@gpu
@pytest.mark.parametrize("name", list(SPLIT))
def test_depth_and_class_current_in_different_places(name):
    for pre in (0, 1):
        run_pair(SPLIT[name], pre, f"split {name}")


@gpu
@pytest.mark.parametrize("name", list(RING))
def test_async_ring_under_runs_of_nulls(name):
    """the block's host memory is overwritten once its copy is done; the nulls wrap the ring more than twice, and every set
    that holds a current image must stay untouched (and unrecycled) however many frames read it"""
    for pre in (0, 1):
        run_pair(RING[name], pre, f"ring {name}", scribble_after=0)


# ---------------------------------------------------------------------------------------------------------------------
# (d) edges
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("reader", READERS)
def test_null_images_on_the_very_first_frame(reader):
    """both sides start from zeroed images: nothing is appended; the frames after it are ordinary"""
    for pre in (0, 1):
        o, g = run_pair([(reader, 0, False, False), ("sync_counts",), ("download",), (reader, 1, False, False), ("sync_counts",),
                         ("sync", 2, True, True), (reader, 3, False, False)], pre, f"first frame null, {reader}", min_surfels=500)
        del o, g
    o = make("oracle", *CAM, **over_of(0))
    o.process_frame(scene(0)[0], None, None, pose(0)); o.process_frame(scene(1)[0], None, None, pose(1))
    assert o.counts()["count"] == 0


@gpu
@pytest.mark.parametrize("reader", READERS)
@pytest.mark.parametrize("giver", ["sync", "async_pinned", "device"])
def test_null_images_directly_after_reset(giver, reader):
    """the reference's reset keeps the textures"""
    for pre in (0, 1):
        run_pair([("sync", 0, True, True), (giver, 1, True, True), ("reset",), (reader, 2, False, False),
                  (reader, 3, False, False), ("download",), ("sync", 3, False, False)], pre, f"reset, {giver} -> {reader}")


@gpu
@pytest.mark.parametrize("giver", ["sync", "async_pageable", "device"])
@pytest.mark.parametrize("how", ["upload_model", "load_map"])
def test_null_images_after_a_model_upload(giver, how, tmp_path):
    """neither upload_model nor load_map touches the images"""
    for pre in (0, 1):
        o = make("oracle", *CAM, **over_of(pre))
        g = Hip(pre)
        for i, step in enumerate([("sync", 0, True, True), (giver, 1, True, True)]):
            rgb, d, s = images_of(step)
            o.process_frame(rgb, d, s, pose(i)); g.step(step[0], rgb, d, s, pose(i))
        if how == "upload_model":
            m = synth.seeded_model(700, tick=2, seed=5)
            o.upload_model(m); g.h.upload_model(m)
        else:
            path = str(tmp_path / f"m{pre}.bin")
            g.h.save_map(path, 0, 0)
            raw = open(path, "rb").read()
            n = int(np.frombuffer(raw[:4], np.uint32)[0])
            g.h.load_map(path)
            o.upload_model(np.frombuffer(raw[12:], np.float32).reshape(n, 12).copy())
        for i, reader in enumerate(READERS):
            o.process_frame(scene(2 + i)[0], None, None, pose(2 + i))
            g.step(reader, scene(2 + i)[0], None, None, pose(2 + i))
        g.h.sync()
        counts_equal(o, g, f"{how} after {giver}, pre={pre}")
        a = o.download_model()
        assert_models_equal(a, g.h.download_model(), f"{how} after {giver}, pre={pre}")
        assert a.shape[0] >= 500


@gpu
@pytest.mark.parametrize("reader", READERS)
@pytest.mark.parametrize("tracker", ["track", "track_rgb"])
def test_tracking_does_not_make_its_image_current(tracker, reader):
    for pre in (0, 1):
        o = make("oracle", *CAM, **over_of(pre))
        g = Hip(pre)
        for i in range(2):
            o.process_frame(*scene(i), pose(i)); g.step("sync", *scene(i), pose(i))
        if tracker == "track":
            g.h.track(scene(4)[1], guess=pose(2))
        else:
            g.h.track_rgb(scene(4)[0], scene(4)[1], guess=pose(2))
        for i in (2, 3):
            o.process_frame(scene(i)[0], None, scene(i)[2], pose(i)); g.step(reader, scene(i)[0], None, scene(i)[2], pose(i))
        g.h.sync()
        counts_equal(o, g, f"{tracker} then {reader}, pre={pre}")
        a = o.download_model()
        assert_models_equal(a, g.h.download_model(), f"{tracker} then {reader}, pre={pre}")
        assert a.shape[0] >= 500


@gpu
@pytest.mark.parametrize("reader", READERS)
def test_clean_points_is_the_only_giver_on_a_fresh_context(reader):
    for pre in (0, 1):
        run_pair([("clean", 1, True, True), (reader, 2, False, False), (reader, 3, False, False), ("download",),
                  ("sync", 0, False, False)], pre, f"clean_points first, then {reader}")


# ---------------------------------------------------------------------------------------------------------------------
# (e) sharded, world 1 (no collective is needed)
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("order", ["host_then_device", "device_then_host"])
def test_sharded_world1_forms_share_the_current_images(order):
    a, b = ("shard", "shard_device") if order == "host_then_device" else ("shard_device", "shard")
    for pre in (0, 1):
        run_pair([("shard", 0, True, True), (a, 1, True, True), (b, 2, False, False), (b, 3, False, True), (a, 2, False, False),
                  (a, 3, True, False), (b, 1, False, False)], pre, f"sharded {order}", sharded=True)


# ---------------------------------------------------------------------------------------------------------------------
# (f) seeded fuzz
# ---------------------------------------------------------------------------------------------------------------------
def draw_script(rng):
    steps = []
    for _ in range(40):
        what = str(rng.choice(["sync"] * 4 + ["async"] * 4 + ["device"] * 4 + ["clean", "reset", "download"]))
        if what == "async":
            what = str(rng.choice(["async_block", "async_pinned", "async_pageable"]))
        k = int(rng.integers(0, 6))
        gd, gs = bool(rng.random() >= 0.3), bool(rng.random() >= 0.3)
        if what in ("clean", "async_block"):
            gd = gs = True
        if what in ("reset", "download"):
            steps.append((what,))
        else:
            steps.append((what, k, gd, gs))
    return steps


def crosses_kinds(script):
    """from the script alone: did a null image follow a giver of another kind (host / ring / device) at least once?"""
    holder = dict(d=None, s=None)
    hit = False
    for step in script:
        if len(step) == 1:
            continue
        form, _, gd, gs = step
        for key, given in (("d", gd), ("s", gs)):
            if given:
                holder[key] = KIND[form]
            elif form != "clean" and holder[key] is not None and holder[key] != KIND[form]:
                hit = True
    return hit


def fuzz_script(seed):
    rng = np.random.default_rng(4000 + seed)
    while True:
        script = draw_script(rng)
        if crosses_kinds(script):
            return script, rng


FUZZ_SEEDS = int(os.environ.get("SM_INPUT_FUZZ_SEEDS", "32"))       # SM_INPUT_FUZZ_SEEDS=1000 for a soak


def test_fuzz_scripts_cross_the_kinds():
    """CPU only: the draw is a function of the seed, and every script has a null that reads another kind's image"""
    for seed in range(FUZZ_SEEDS):
        a, b = fuzz_script(seed)[0], fuzz_script(seed)[0]
        assert a == b and len(a) == 40 and crosses_kinds(a)
    assert not crosses_kinds([("sync", 0, True, True), ("sync", 1, False, False), ("async_pinned", 1, True, True)])
    assert crosses_kinds([("sync", 0, True, True), ("device", 1, False, True)])


@gpu
@pytest.mark.parametrize("seed", list(range(FUZZ_SEEDS)))
def test_random_scripts_with_null_images_match_the_oracle(seed):
    script, rng = fuzz_script(seed)
    pre = int(rng.integers(0, 2))
    o = make("oracle", *CAM, **dict(over_of(pre), max_sqrt_vertices=400))
    g = Hip(pre, compact_period=int(rng.choice([1, 2, 3, 8, 1000])), max_sqrt_vertices=400)
    had_reset = False
    z = 0.0
    for i, step in enumerate(script):
        form = step[0]
        tag = f"seed {seed} pre={pre} step {i} {step}"
        if form == "download":
            models_equal(o.download_model(), g.h.download_model(), tag, had_reset)
            counts_equal(o, g, tag)
            continue
        if form == "reset":
            o.reset(); g.h.reset()
            had_reset = True
            counts_equal(o, g, tag, ("count", "tick"))
            continue
        z += float(rng.uniform(-0.03, 0.12))
        p = synth.pose_to_colmajor(synth.pose_matrix(0.05 * math.sin(i), 0.0, z, float(rng.uniform(-3, 3))))
        rgb, d, s = images_of(step)
        if form == "clean":
            o.clean_points(d, s, p)
        else:
            o.process_frame(rgb, d, s, p)
        g.step(form, rgb, d, s, p)
        if form == "sync":
            counts_equal(o, g, tag)
        elif form == "clean":
            counts_equal(o, g, tag, ("count", "tick"))
    g.h.sync()
    counts_equal(o, g, f"seed {seed} end", ("count", "tick"))
    models_equal(o.download_model(), g.h.download_model(), f"seed {seed} final", had_reset)
