"""Read-only calls as probes (tests/test_call_order.py, tests/test_set_call_frame.py): a probe is a name and a function
(context, the arguments of one size) -> everything the call gave -- every array it returns, every file it writes, its stats -- and
flat() turns that into a dict of bytes and plain values that two contexts can be compared by, key for key.  The module also holds the
data the probes run on (Data: map files of two sizes around a live model, images, rays, points), the walk over every ordered pair of
probes (euler_walk, arcs) and the loop that drives a context through it (drive).  No fixtures here: the tests make their own."""
import math
import os

import numpy as np

# Stats keys a probe leaves out of its result, with the reason.  The keys that end in "_ms" are times and are left out of every
# result (flat()); anything else a probe does not compare stands here: (probe or "*", key) -> why.  Arrays and files are never left out.
_INDEX = ("the context's file index (sm_map_set.h: FileIndex) keeps the box of every file a recall has read, and a later recall leaves a "
          "file out of reach unread: how much is read depends on the calls before by design, what is recalled does not")
_INDEX_GROUND = ("the ground map leaves a file unread whose box in the context's file index misses the window: files_skipped, and with it "
                 "the chunks read and the launches made for them, depend on which recall came before by design, no plane and no count does")
_CLAIMS = ("the slots the walks of the voxel index read: lanes claim its slots by compare-and-swap (sm_d_simplify.h: lean_probe), so where a key "
           "lies along its probe sequence, and how far a walk to it is, depends on which lane won -- it differs between two runs of one call")
STATS_LEFT_OUT = {("recall_count", k): _INDEX for k in ("files_skipped", "files_read", "records_read", "chunks")}
STATS_LEFT_OUT.update({("ground_maps", k): _INDEX_GROUND for k in ("files_skipped", "chunks", "launches")})
STATS_LEFT_OUT.update({(p, "probes"): _CLAIMS for p in ("rays_maps", "points_maps", "rays", "points")})

SIZES = ("small", "big")
KINDS = ("streamed", "analysis", "resident")

# ---------------------------------------------------------------------------------------------------------------------
# results as bytes and plain values
# ---------------------------------------------------------------------------------------------------------------------
def plain(v):
    return v.tobytes() if isinstance(v, np.ndarray) else v


def counts(st):
    """the stats without the times"""
    return {k: v for k, v in st.items() if not k.endswith("_ms")}


def flat(value, probe="*", key="", out=None):
    """{key path: bytes or plain value} of a nested result: an array as its bytes with dtype and shape, a float by its bits (so that
    a NaN equals itself), dict keys that end in _ms and those of STATS_LEFT_OUT dropped"""
    out = {} if out is None else out
    if isinstance(value, dict):
        for k, v in value.items():
            if str(k).endswith("_ms") or (probe, k) in STATS_LEFT_OUT or ("*", k) in STATS_LEFT_OUT:
                continue
            flat(v, probe, f"{key}.{k}" if key else str(k), out)
    elif isinstance(value, (list, tuple)):
        out[key + ".len"] = len(value)
        for i, v in enumerate(value):
            flat(v, probe, f"{key}[{i}]", out)
    elif isinstance(value, np.ndarray):
        out[key] = (str(value.dtype), tuple(value.shape), value.tobytes())
    elif isinstance(value, (float, np.floating)):
        out[key] = ("float", np.float64(value).tobytes())
    elif isinstance(value, (np.integer, np.bool_)):
        out[key] = int(value)
    else:
        assert value is None or isinstance(value, (int, str, bytes, bool)), (key, type(value))
        out[key] = value
    return out


def differences(got, want):
    """the keys (in the order of `want`, then of `got`) at which two flat results differ"""
    return [k for k in want if k not in got or got[k] != want[k]] + [k for k in got if k not in want]


def first_difference(got, want):
    """the first of them; None if the results are equal"""
    keys = differences(got, want)
    return keys[0] if keys else None


# ---------------------------------------------------------------------------------------------------------------------
# the walk: every ordered pair of probes adjacent at least once
# ---------------------------------------------------------------------------------------------------------------------
def euler_walk(n):
    """An Eulerian circuit of the complete digraph with loops on 0..n-1 as its n^2 + 1 vertices, by Hierholzer's algorithm with the
    edges of every vertex taken in ascending order: deterministic.  Every ordered pair (a, b), a = b included, is adjacent once."""
    if n == 0:
        return []
    unused = [list(range(n - 1, -1, -1)) for _ in range(n)]
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def arcs(walk, n_arcs):
    """the walk cut into n_arcs pieces of nearly equal length that overlap by one visit: the last visit of an arc is the first of
    the next, so that every adjacent pair of the walk is adjacent inside one arc"""
    edges = len(walk) - 1
    n_arcs = max(1, min(n_arcs, edges))
    cuts = [edges * i // n_arcs for i in range(n_arcs + 1)]
    return [walk[a:b + 1] for a, b in zip(cuts[:-1], cuts[1:])]


def pairs_of(pieces):
    return {(a, b) for piece in pieces for a, b in zip(piece[:-1], piece[1:])}


class Difference:
    """one comparison that failed: the call before, the call, the first key that differs"""

    def __init__(self, prev, cur, keys):
        self.prev, self.cur, self.key, self.keys = prev, cur, keys[0], keys

    def __repr__(self):
        before = "the context's first call" if self.prev is None else "after %s(%s)" % self.prev
        more = " (and at %d more: %s)" % (len(self.keys) - 1, ", ".join(self.keys[1:6])) if len(self.keys) > 1 else ""
        return "%s(%s) %s differs from a fresh context at %r%s" % (self.cur + (before, self.key, more))


def drive(visits, run, fresh, after_step=None, sizes=SIZES):
    """A used context through `visits` (probe names): every visit is the probe at each of `sizes` in turn, each result held on the spot
    against fresh(name, size).  run(name, size) -> the flat result on the used context; after_step(name, size) is called after every
    comparison.  Returns the Differences, in order."""
    prev, found = None, []
    for name in visits:
        for size in sizes:
            keys = differences(run(name, size), fresh(name, size))
            if keys:
                found.append(Difference(prev, (name, size), keys))
            if after_step is not None:
                after_step(name, size)
            prev = (name, size)
    return found


# ---------------------------------------------------------------------------------------------------------------------
# the data
# ---------------------------------------------------------------------------------------------------------------------
CAM = dict(width=96, height=64, fx=60.0, fy=60.0, cx=47.5, cy=31.5)
CONFIG = dict(preprocess=0, stereo_border=0.0, max_sqrt_vertices=128)
FILE_ROWS = dict(small=(200, 1, 0), big=(300, 700, 513))
LIVE_ROWS = 300
N_VIEWS = dict(small=1, big=3)
N_QUERIES = dict(small=257, big=4096)
MOVED = np.float32(0.03)
ACTOR_CLASS = 7                                                            # (scene_ref.ACTOR_CLASS: a class the street lacks)
MODEL_VIEW_KW = dict(threshold=0.5, unstable=True, color_type=2)
TICK = 9
# the cell of the rays' and points' voxel index: the street's discs are a third of a metre wide, and at 1 m three quarters of them
# are indexed and the others take the wide path (at the default 250 mm all of them would)
INDEX_MM = 1000


def write_map(path, rows, start_id=0, end_id=0):
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 12)
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([start_id, end_id], np.int32).tobytes() + rows.tobytes())
    return str(path)


def _disc(x, y, z, r, n, sem, bgr):
    s = np.zeros(12, np.float32)
    s[0:3] = (x, y, z); s[3] = 1.0
    s[4:5].view(np.uint32)[0] = (sem << 24) | (bgr[2] << 16) | (bgr[1] << 8) | bgr[0]
    s[6] = s[7] = 1.0
    s[8:11] = n; s[11] = r
    return s


def actor_rows(nx, ny, bgr):
    """a small wall of discs in its own frame, facing -z"""
    return np.stack([_disc(0.15 * (i - nx / 2), 0.15 * (j - ny / 2), 0.0, 0.1, (0, 0, -1), ACTOR_CLASS, bgr) for j in range(ny) for i in range(nx)])


def _pose12(tx, ty, tz, yaw_deg=0.0):
    c, s = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    return np.array([c, 0, s, tx, 0, 1, 0, ty, -s, 0, c, tz], np.float32)


class Args:
    """the arguments of one size: the set's files and everything else a probe passes"""

    def __init__(self, data, size):
        self.data, self.size, self.folder = data, size, data.folder
        self.paths, self.plain, self.other = [], [], []

    def out(self):
        return self.data.out()

    def aim(self, frame, look=False):
        """the images, the pose and the guesses of the probes that take a frame: (rgb, depth, sem, pose16) of the context's camera;
        look: the views and sweeps are taken from that frame's pose as well"""
        big = self.size == "big"
        if look:
            self.views = np.tile(np.asarray(frame[3], np.float32).reshape(1, 16), (len(self.views), 1))
        self.rgb, self.depth = np.ascontiguousarray(frame[0]), np.ascontiguousarray(frame[1])
        self.pose = np.asarray(frame[3], np.float32).reshape(4, 4).T.copy()
        self.guess = self.pose.copy()
        self.guess[:3, 3] += np.array((0.03, -0.02, 0.05) if big else (-0.02, 0.01, -0.04), np.float32)
        k = 64 if big else 5
        self.cands = np.tile(self.pose, (k, 1, 1))
        self.cands[:, :3, 3] += np.random.default_rng(k).uniform(-0.3, 0.3, (k, 3)).astype(np.float32)


class Data:
    """Map files of two sizes around one live model, and what the probes ask of them.  rows: the records the files are cut from,
    live: the live model's; cam: the context's camera; frames: (rgb, depth, sem, pose16) of that camera, the last two of which the
    image probes take (big the last, small the one before); views: camera->world 4x4 matrices, at least three.
    big: three plain files (and, once add_packed() has run, the second of them again as a packed file); small: two files and an
    empty one.  `other`: the plain records moved by 3 cm, in two files."""

    def __init__(self, folder, rows, live, cam, frames, views):
        from surfelmapping_amd import capi, synth
        import model_view_ref as mv
        self.folder, self.cam, self.frames, self.live = str(folder), dict(cam), frames, np.ascontiguousarray(live, np.float32)
        self.n_out = 0
        assert len(rows) >= sum(FILE_ROWS["big"]) and len(views) >= 3 and len(frames) >= 3
        self.views = np.stack([synth.pose_to_colmajor(v) for v in views[:3]])
        self.parts, self.sets = {}, {}
        w, h = cam["width"], cam["height"]
        img = dict(small=(w, h, cam["fx"], cam["fy"], cam["cx"], cam["cy"]),
                   big=(w + 64, h + 32, cam["fx"] * 1.5, cam["fy"] * 1.5, (w + 64) / 2 - 0.5, (h + 32) / 2 - 0.5))
        self.actor_files = [write_map(os.path.join(self.folder, "actor%d.bin" % j), r)
                            for j, r in enumerate((actor_rows(8, 6, (40, 60, 220)), actor_rows(5, 7, (200, 220, 30))))]
        rng = np.random.default_rng(11)
        lo, hi = rows[:, 0:3].min(axis=0), rows[:, 0:3].max(axis=0)
        for size in SIZES:
            a = self.sets[size] = Args(self, size)
            cuts = np.cumsum(FILE_ROWS[size])
            self.parts[size] = np.split(rows[:cuts[-1]], cuts[:-1])
            for i, part in enumerate(self.parts[size]):
                a.paths.append(write_map(os.path.join(self.folder, "%s_%06d.bin" % (size, i)), part, 10 + i, 20 + i))
            a.plain = list(a.paths)
            moved = rows[:cuts[-1]].copy()
            moved[:, 0] += MOVED
            for i, part in enumerate(np.split(moved, [len(moved) * 3 // 10])):
                a.other.append(write_map(os.path.join(self.folder, "%s_other%d.bin" % (size, i)), part, 30, 40))
            V = N_VIEWS[size]
            a.views, a.img = self.views[:V], img[size]
            # the model views: from behind and above, from the side, from straight above
            mw, mh = (160, 120) if size == "big" else (96, 64)
            P = mv.projection(mw, mh, 105.0 * mw / 160, 105.0 * mw / 160, mw / 2.0, mh / 2.0, 0.1, 1000.0)
            eyes = [mv.look_at(0, -3, -4, 0, 0, 8, 0, -1, 0), mv.look_at(3, -2, -2, 0, 0, 8, 0, -1, 0), mv.look_at(0, -25, 8, 0, 0, 8.5, 0, 0, 1)]
            a.model_views = [(mvp, inv, mw, mh) for mvp, inv in (mv.view_mats(P, e) for e in eyes[:V])]
            a.sensor = capi.lidar_sensor(n_az=90 if size == "big" else 45, az0_deg=-178.0, az_step_deg=4.0 if size == "big" else 8.0,
                                         el_deg=np.arange(-7, 8, 2 if size == "big" else 4, dtype=np.float32), min_range=1.0, max_range=60.0, min_conf=0.0)
            # two actors: the first in every view, the second absent from the first view
            t = np.arange(V, dtype=np.float32)
            a.actors = [(self.actor_files[0], np.stack([_pose12(-1.0 + 0.5 * k, 0.9, 7.0 + k) for k in t]), None),
                        (self.actor_files[1], np.stack([_pose12(1.5, 0.6, 9.0 - k, 30.0) for k in t]), np.array([0, 1, 1][:V], np.uint8))]
            # rays from around the cameras, most of them forward; points in and around the records' box; one invalid each
            n = N_QUERIES[size]
            rays = np.zeros((n, 8), np.float32)
            rays[:, 0:3] = rng.uniform((-3.0, -1.5, -1.0), (3.0, 0.5, 6.0), (n, 3))
            rays[:, 4:7] = rng.normal(size=(n, 3)) * (1.0, 0.4, 1.0) + (0.0, 0.0, 1.0)
            rays[:, 7] = 30.0
            rays[5, 4:7] = 0.0
            pts = np.zeros((n, 4), np.float32)
            pts[:, 0:3] = rng.uniform(lo - 0.5, hi + 0.5, (n, 3))
            pts[:, 3] = 0.5
            pts[::7, 3] = np.inf
            pts[5, 3] = -1.0
            a.rays, a.points = rays, pts
            # the images of the resident probes
            a.aim(frames[-1] if size == "big" else frames[-2])
            import test_stereo as tst
            import test_fill as tf
            a.pair = tst._shifted_pair(w, h, 7, shift=9) if size == "big" else tst._shifted_pair(w, h, 8, shift=5)
            v, u = np.nonzero(a.depth)
            pick = np.sort(rng.permutation(len(v))[:n]) if len(v) >= n else np.resize(np.arange(len(v)), n)
            Z = a.depth[v[pick], u[pick]].astype(np.float64) / 1000.0
            a.scan = np.stack([(u[pick] - cam["cx"]) * Z / cam["fx"], (v[pick] - cam["cy"]) * Z / cam["fy"], Z, np.zeros(len(Z))], axis=1).astype(np.float32)
            a.holes = tf.random_images(rng, V, img[size][1], img[size][0], 0.4)
        self.packed = None

    def out(self):
        self.n_out += 1
        return os.path.join(self.folder, "out%d" % self.n_out)

    def add_packed(self, ctx):
        """big's second file once more, packed by `ctx` (a context of its own): at least one packed block, none RAW"""
        src = self.sets["big"].plain[1]
        files = ctx.pack_maps([src], os.path.join(self.folder, "big_packed"))
        st = ctx.pack_stats()
        assert st["blocks"] - st["raw_blocks"] >= 1 and st["raw_blocks"] == 0 and st["records"] == FILE_ROWS["big"][1], st
        self.packed = files[0]
        self.sets["big"].paths.append(files[0])

    def set_files(self):
        return [p for s in SIZES for p in self.sets[s].paths + self.sets[s].other] + self.actor_files

    def snapshot(self):
        return [(open(p, "rb").read(), os.stat(p).st_mtime_ns) for p in self.set_files()]

    def records(self, size, decode=None):
        """the rows of the set in id order: the files' (decode(path) gives a packed file's), then the live model's"""
        parts = list(self.parts[size])
        if size == "big" and self.packed is not None:
            parts.append(decode(self.packed))
        return np.concatenate(parts + [self.live])


def street(folder):
    """the data of the ordered pairs: test_simplify.Scene()'s records (about 1.9 k surfels fused by the oracle at 64 x 48), every sixth
    of the first 1800 live, the others in the files; the frames of the same street through the context's camera"""
    import test_simplify as ts
    from surfelmapping_amd import synth
    rows = ts.Scene().rows
    assert len(rows) >= sum(FILE_ROWS["big"]) + LIVE_ROWS
    at = np.arange(0, 6 * LIVE_ROWS, 6)
    poses = synth.kitti_trajectory(4)
    frames = synth.make_sequence(CAM, poses, seed=3)
    views = [poses[3], synth.pose_matrix(0.5, 0.0, 2.4), synth.pose_matrix(-0.5, 0.0, 1.0, 10.0)]
    return Data(folder, np.delete(rows, at, axis=0), rows[at], CAM, frames, views)


def switches(m, data):
    """the switches a probe needs, set once on every context alike: the stereo matcher, the lidar depth stage, the ferns with three
    keyframes of the data's frames"""
    m.set_stereo(max_disp=64)
    m.set_lidar_depth()
    m.set_ferns()
    for k, fr in enumerate(data.frames[:3]):
        m.fern_add(m.fern_encode(fr[1], fr[0]), fr[3], k + 1)


def context(data, model=None, tick=TICK, config=CONFIG):
    """A context ready for any probe: the switches, one frame processed (the trackers draw their prediction at the last frame's pose),
    then the model replaced by `model` (default: the data's live model) and the tick set."""
    from surfelmapping_amd import capi
    m = capi.SurfelMap(capi.make_config(**data.cam, **config))
    switches(m, data)
    m.process_frame(*data.frames[-3])
    m.upload_model(data.live if model is None else model)
    m.set_tick(tick)
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the analysis calls as test_set_call_frame.py runs them
# ---------------------------------------------------------------------------------------------------------------------
def run_analysis(m, call, sets, include_model=True, out=None, **over):
    """One call; (what it gave, everything as bytes or plain values: outputs, info, files written), the records it says it read"""
    import test_simplify as ts
    out = out or sets.out()
    if call == "simplify":
        st = m.simplify_maps(sets.paths, out, include_model=include_model, voxel_mm=ts.BITE_MM, **over)
        return dict(file=open(out, "rb").read(), **{k: st[k] for k in ts.STAT_KEYS}), st["records_in"]
    if call == "tile":
        files = m.tile_maps(sets.paths, out, include_model=include_model, cell_mm=200, tile_shift=1, max_file_records=256, **over)
        st = m.tile_stats()
        got = {k: st[k] for k in ("records_in", "placed", "loose", "tiles", "largest_tile", "files_written")}
        return dict(files=[open(f, "rb").read() for f in files], **got), st["records_in"]
    if call == "register":
        pose, info = m.register_maps(sets.paths, sets.other, source_model=include_model, voxel_mm=200, levels=2, min_inliers=10,
                                     pivot=(0.0, 0.0, 10.0), **over)
        return dict(pose=pose.tobytes(), **info), m.register_stats()["source_records"]
    if call == "compare":
        lab, info = m.compare_maps(sets.paths, sets.other, query_model=include_model, out_path=out, write_mask=15, **over)
        return dict(labels=lab.tobytes(), file=open(out, "rb").read(), **{k: v for k, v in info.items() if k != "counts"}), info["query_records"]
    if call == "segment":
        got = m.segment_maps(sets.paths, include_model=include_model, out_path=out, voxel_mm=200, **over)
        info = {k: v for k, v in got["info"].items() if k != "counts"}
        return dict(labels=got["labels"].tobytes(), components=got["components"].tobytes(), file=open(out, "rb").read(), info=info), info["records"]
    if call == "mesh":
        got = m.mesh_maps(sets.paths, include_model=include_model, ply_path=out, voxel_mm=200, **over)
        info = {k: v for k, v in got["info"].items() if k != "counts"}
        return dict(vertices=got["vertices"].tobytes(), faces=got["faces"].tobytes(), file=open(out, "rb").read(), info=info), info["records"]
    assert call == "ground"
    got = m.ground_maps(sets.paths, include_model=include_model, **{**dict(cell_mm=100, origin=(-12.8, 0.0, 0.0)), **over})
    info = {k: v for k, v in got.pop("info").items() if k not in ("counts", "cells")}
    return dict({k: plain(v) for k, v in got.items()}, info=info), info["records"]


LOCATE = dict(cell_mm=500, origin=(-16.0, 0.0, -8.0), source_origin=(0.0, 0.0, 8.0), nu=64, nv=64, n_yaw=24, refine=2, min_records=1, min_ground=1)


# ---------------------------------------------------------------------------------------------------------------------
# the registry
# ---------------------------------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, name, kind, fn, entry_points):
        self.name, self.kind, self.fn, self.entry_points = name, kind, fn, entry_points


PROBES = {}


def probe(kind, *entry_points):
    """registers fn(m, a) -> nested result under its name; entry_points: the SurfelMap methods it calls on behalf of the registry"""
    assert kind in KINDS

    def add(fn):
        PROBES[fn.__name__] = Probe(fn.__name__, kind, fn, entry_points)
        return fn
    return add


def run(name, m, data, size):
    """the probe `name` at `size` on context m: its flat result"""
    return flat(PROBES[name].fn(m, data.sets[size]), name)


def _files(paths):
    return [open(p, "rb").read() for p in paths]


# ---- streamed, over the set plus the live model
@probe("streamed", "render_image_maps")
def image_maps(m, a):
    bgr, sem = m.render_image_maps(a.paths, a.views, *a.img)
    return dict(bgr=bgr, sem=sem, stats=m.render_maps_stats())


@probe("streamed", "render_image_maps")
def image_maps_filled(m, a):
    bgr, sem, depth = m.render_image_maps(a.paths, a.views, *a.img, fill=True, depth=True)
    return dict(bgr=bgr, sem=sem, depth=depth, stats=m.render_maps_stats(), fill=m.fill_stats())


@probe("streamed", "render_image_maps")
def image_maps_blended(m, a):
    bgr, sem = m.render_image_maps(a.paths, a.views, *a.img, blend=True)
    return dict(bgr=bgr, sem=sem, stats=m.render_maps_stats(), blend=m.blend_stats())


@probe("streamed", "render_model_maps")
def model_maps(m, a):
    from surfelmapping_amd import capi
    views = [capi.model_view(mvp, inv, w, h, **MODEL_VIEW_KW) for mvp, inv, w, h in a.model_views]
    rgba, depth, ids = m.render_model_maps(a.paths, views, depth=True, ids=True)
    return dict(rgba=rgba, depth=depth, ids=ids, stats=m.render_maps_stats())


@probe("streamed", "lidar_sweep_maps")
def sweep_maps(m, a):
    return dict(m.lidar_sweep_maps(a.paths, a.views, a.sensor), stats=m.lidar_stats())


@probe("streamed", "recall")
def recall_count(m, a):
    n = m.recall(a.paths, pose=a.views[0], mode="count", radius=8.0)
    return dict(n=n, stats=m.recall_stats())


@probe("streamed", "render_scene")
def scene_image(m, a):
    bgr, sem, depth = m.render_scene(a.paths, a.actors, a.views, *a.img, fill=True, depth=True)
    return dict(bgr=bgr, sem=sem, depth=depth, stats=m.scene_stats(), maps=m.render_maps_stats())


@probe("streamed", "lidar_sweep_scene")
def scene_sweep(m, a):
    return dict(m.lidar_sweep_scene(a.paths, a.actors, a.views, a.sensor), stats=m.scene_stats(), lidar=m.lidar_stats())


@probe("streamed", "cast_rays")
def rays_maps(m, a):
    return dict(m.cast_rays(a.rays, a.paths, normal=True, cell_mm=INDEX_MM), stats=m.cast_rays_stats())


@probe("streamed", "query_points")
def points_maps(m, a):
    return dict(m.query_points(a.points, a.paths, cell_mm=INDEX_MM), stats=m.query_points_stats())


@probe("streamed", "pack_maps")
def pack(m, a):
    files = m.pack_maps(a.plain, a.out(), include_model=True)
    return dict(files=_files(files), stats=m.pack_stats())


@probe("streamed", "unpack_maps")
def unpack(m, a):
    files = m.unpack_maps(a.paths, a.out())
    return dict(files=_files(files), stats=m.pack_stats())


# ---- map-set analysis
def _analysis(call):
    def fn(m, a):
        got, records = run_analysis(m, call, a)
        return dict(got=got, records=records, stats=getattr(m, call + "_stats")())
    fn.__name__ = call + "_maps"
    return probe("analysis", call + "_maps")(fn)


for _call in ("simplify", "register", "compare", "tile", "segment", "mesh", "ground"):
    _analysis(_call)


@probe("analysis", "locate_maps")
def locate_maps(m, a, **over):
    got = m.locate_maps(a.paths, a.other, source_model=True, **dict(LOCATE, **over))
    return dict(got, stats=m.locate_stats())


# ---- resident, on the live model
@probe("resident", "render_image")
def image(m, a):
    got = [m.render_image(v, *a.img, fill=True, depth=True, blend=True) for v in a.views]
    return dict(views=got, fill=m.fill_stats(), blend=m.blend_stats())


@probe("resident", "render_model")
def model(m, a):
    return dict(views=[m.render_model(mvp, inv, w, h, depth=True, ids=True, **MODEL_VIEW_KW) for mvp, inv, w, h in a.model_views])


@probe("resident", "lidar_sweep")
def sweep(m, a):
    return dict(sweeps=[m.lidar_sweep(v, a.sensor) for v in a.views], stats=m.lidar_stats())


@probe("resident", "cast_rays")
def rays(m, a):
    return dict(m.cast_rays(a.rays, normal=True, cell_mm=INDEX_MM), stats=m.cast_rays_stats())


@probe("resident", "query_points")
def points(m, a):
    return dict(m.query_points(a.points, cell_mm=INDEX_MM), stats=m.query_points_stats())


# (the defaults ask for 1000 inliers; 300 live records give a few hundred)
TRACK = dict(min_inliers=10, dist_thresh=0.5)


@probe("resident", "track", "old_in_view")
def track(m, a):
    pose, info = m.track(a.depth, a.guess, **TRACK)
    return dict(pose=pose, info=info, old=m.old_in_view(a.pose, TICK))


@probe("resident", "track_rgb", "score_poses")
def track_rgb(m, a):
    pose, info = m.track_rgb(a.rgb, a.depth, a.guess, **TRACK)
    return dict(pose=pose, info=info, scores=m.score_poses(a.depth, a.cands, rgb=a.rgb, stride=2), plain=m.score_poses(a.depth, a.cands))


@probe("resident", "search_pose")
def search(m, a):
    pose, info = m.search_pose(a.depth, a.guess, rgb=a.rgb if a.size == "big" else None, **TRACK)
    return dict(pose=pose, info=info)


@probe("resident", "fern_encode", "fern_match")
def ferns(m, a):
    code = m.fern_encode(a.depth, a.rgb if a.size == "big" else None)
    k, d, every = m.fern_match(code, dis_all=True)
    return dict(code=code, k=k, d=d, every=every)


@probe("resident", "stereo_depth")
def stereo(m, a):
    depth, disp = m.stereo_depth(*a.pair)
    return dict(depth=depth, disp=disp)


@probe("resident", "lidar_depth")
def lidar_depth(m, a):
    depth, sparse, index = m.lidar_depth(a.scan, np.eye(4, dtype=np.float32))
    return dict(depth=depth, sparse=sparse, index=index, stats=m.lidar_depth_stats())


@probe("resident", "fill_image")
def fill(m, a):
    bgr, sem, depth = m.fill_image(*a.holes)
    return dict(bgr=bgr, sem=sem, depth=depth, stats=m.fill_stats())


NAMES = tuple(PROBES)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: calls that give up (or come back short) once the set has gone through the staging
# ---------------------------------------------------------------------------------------------------------------------
# name -> (the call of run_analysis or "locate", its overriding arguments, the SM_* code's name).  The first seven are
# test_set_call_frame.BAD; a mesh and a segmentation that may bring back one row come back short with SM_OK.
REFUSALS = dict(
    simplify=("simplify", dict(max_cells=1), "SM_E_CAPACITY"), register=("register", dict(max_cells=1), "SM_E_CAPACITY"),
    compare=("compare", dict(max_cells=1), "SM_E_CAPACITY"), tile=("tile", dict(max_tiles=1), "SM_E_CAPACITY"),
    segment=("segment", dict(max_cells=1), "SM_E_CAPACITY"), mesh=("mesh", dict(max_cells=1), "SM_E_CAPACITY"),
    ground=("ground", dict(cell_mm=9), "SM_E_ARG"),
    mesh_one_vertex=("mesh", dict(max_vertices=1), "SM_OK"), segment_one_component=("segment", dict(max_components=1), "SM_OK"),
    locate=("locate", dict(max_source_cells=1), "SM_E_CAPACITY"))


def refuse(name, m, data, size="big"):
    """the call of REFUSALS[name] at `size`; the SM_* code it came back with"""
    from surfelmapping_amd import capi
    call, over, _ = REFUSALS[name]
    try:
        if call == "locate":
            locate_maps(m, data.sets[size], **over)
        else:
            run_analysis(m, call, data.sets[size], **over)
    except capi.SurfelMapError as e:
        return e.rc
    return capi.SM_OK
