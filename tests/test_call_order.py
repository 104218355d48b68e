"""One context, any call order ("The frame of a map-set call": a call's result is a function of its arguments, the files
and the model).  Every feature's own suite starts from a context that has done nothing else; here the read-only calls of
tests/call_probes.py run on contexts that have a history -- every ordered pair of them adjacent once on a used context, every one
after a refusal of another call, every one in a gap of an asynchronous frame stream -- and each result is held, bit for bit, against
the same call as a fresh context's first.  Without a GPU: the walk's coverage, the harness against a stub that does remember, and the
registry against capi.SurfelMap's methods."""
import math
import os
import time

import numpy as np
import pytest

import call_probes as cp

gpu = pytest.mark.gpu
N = len(cp.NAMES)
WALK = cp.euler_walk(N)
# Chosen by measurement (profiles/call_order_tests.txt): the arcs of the N^2 visits, each a test function of a few seconds.
N_ARCS = 4
ARCS = cp.arcs(WALK, N_ARCS)
# The probes whose answer depends on the frame stream itself (the last frame's pose, the constant-velocity history), which no upload
# gives a fresh context: between asynchronous frames they are held against a context that ran the same frames synchronously.
FRAME_STATE = ("track", "track_rgb", "search")


# ---------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_walk_is_deterministic_and_covers_every_ordered_pair():
    assert N >= 24 and cp.euler_walk(N) == WALK and len(WALK) == N * N + 1 and WALK[0] == WALK[-1]
    assert set(WALK) == set(range(N)), "a probe of the registry is missing from the walk"
    every = {(a, b) for a in range(N) for b in range(N)}
    assert cp.pairs_of([WALK]) == every
    assert cp.pairs_of(ARCS) == every, sorted(every - cp.pairs_of(ARCS))[:4]
    assert len(ARCS) == N_ARCS and all(a[-1] == b[0] for a, b in zip(ARCS[:-1], ARCS[1:]))
    assert sum(len(a) - 1 for a in ARCS) == N * N
    for n in (1, 2, 3, 7):                                                 # (the construction, at sizes one can check by eye)
        w = cp.euler_walk(n)
        assert len(w) == n * n + 1 and cp.pairs_of([w]) == {(a, b) for a in range(n) for b in range(n)}
        for k in (1, 2, n * n, n * n + 5):
            assert cp.pairs_of(cp.arcs(w, k)) == cp.pairs_of([w])


def test_flat_results_compare_by_bits():
    a = cp.flat(dict(x=np.arange(4, dtype=np.int32), st=dict(n=3, total_ms=1.5, r=float("nan")), files=[b"ab", b"c"]))
    assert set(a) == {"x", "st.n", "st.r", "files.len", "files[0]", "files[1]"}
    assert cp.first_difference(a, cp.flat(dict(x=np.arange(4, dtype=np.int32), st=dict(n=3, total_ms=9.0, r=float("nan")), files=[b"ab", b"c"]))) is None
    assert cp.first_difference(a, cp.flat(dict(x=np.arange(4, dtype=np.uint32), st=dict(n=3, r=float("nan")), files=[b"ab", b"c"]))) == "x"
    assert cp.first_difference(a, cp.flat(dict(x=np.arange(4, dtype=np.int32).reshape(2, 2), st=dict(n=3, r=float("nan")), files=[b"ab", b"c"]))) == "x"
    assert cp.first_difference(a, cp.flat(dict(x=np.arange(4, dtype=np.int32), st=dict(n=3, r=float("nan")), files=[b"ab"]))) == "files.len"
    assert cp.first_difference(a, cp.flat(dict(x=np.arange(4, dtype=np.int32), st=dict(n=3, r=-0.0), files=[b"ab", b"c"]))) == "st.r"
    assert cp.first_difference(cp.flat(dict(v=0.0)), cp.flat(dict(v=-0.0))) == "v"
    assert cp.first_difference(a, dict(a, more=1)) == "more"


class Stub:
    """A context in plain Python whose probes are functions of their size alone -- but for `leaky`, which reads its scratch past its
    own count: after a larger call of any probe it returns what that call left behind."""
    names = ("plain", "grower", "leaky", "other")

    def __init__(self):
        self.left = 0                                                      # the extent of the previous call's data in the scratch
        self.calls = []

    def run(self, name, size):
        self.calls.append((name, size))
        n = dict(small=1, big=3)[size]
        behind, self.left = self.left > n, n
        return cp.flat(dict(n=n, behind=behind) if name == "leaky" else dict(n=n, name=name))


def test_harness_flags_the_probe_that_remembers():
    """through the same walk and comparison code: exactly the leaky probe, at small, and only right after a big call"""
    names = Stub.names
    walk = cp.euler_walk(len(names))
    cache = {}

    def fresh(name, size):
        if (name, size) not in cache:
            cache[name, size] = Stub().run(name, size)
        return cache[name, size]
    found, expected = [], []
    for piece in cp.arcs(walk, 3):
        used = Stub()
        visits = [names[i] for i in piece]
        found += cp.drive(visits, used.run, fresh)
        assert used.calls == [(v, size) for v in visits for size in cp.SIZES]
        # a visit is small, then big: leaky(small) meets the big call of the visit before it, whatever probe that was -- but not
        # as an arc's first call, and leaky(big) never has a larger call before it
        expected += [((before, "big"), ("leaky", "small")) for before, v in zip(visits[:-1], visits[1:]) if v == "leaky"]
    assert [(d.prev, d.cur) for d in found] == expected and all(d.key == "behind" for d in found)
    assert {d.prev[0] for d in found} == set(names), "every probe comes right before leaky once, itself included"
    assert "leaky(small) after grower(big)" in [repr(d).split(" differs")[0] for d in found] and "'behind'" in repr(found[0])
    # a harness that never fails would pass a comparison of `found` with nothing: clean probes give no difference
    clean = Stub()
    assert cp.drive(["plain", "other", "plain"], clean.run, fresh) == [] and len(clean.calls) == 6


# every public method of capi.SurfelMap: the probe that calls it, or why it is none
MUTATES, REWRITES, DEBUG = "it mutates the model", "it rewrites files", "it is a debug call"
# (three further reasons, for methods that compute nothing from the model or the files)
RESULT = "it is part of a probe's result or of the harness's check"        # stats getters, counts, download_model
SWITCH = "it sets a switch or manages the context's memory"                # set once in the fixture of every context alike
FORM = "it is another form of a probed call: "                             # the same entry point's device-pointer or window form
NOT_PROBES = dict(
    close=SWITCH, sync=SWITCH, reset=MUTATES, host_array=SWITCH, host_frame=SWITCH, inputs_consumed=SWITCH,
    process_frame=MUTATES, process_frame_device=MUTATES, process_frame_async=MUTATES, process_frame_tracked=MUTATES,
    process_frame_tracked_rgb=MUTATES, process_frame_stereo=MUTATES, process_frame_lidar=MUTATES,
    clean_points=MUTATES, clean_points_slice=MUTATES, upload_model=MUTATES, load_map=MUTATES, append_model_device=MUTATES,
    retire=MUTATES, set_auto_retire=SWITCH, recall_stats=RESULT, retire_stats=DEBUG, auto_retire_stats=RESULT, set_auto_recall=SWITCH,
    auto_recall_stats=RESULT, warp_by_time=REWRITES, warp_stats=RESULT, simplify=MUTATES, save_map=REWRITES,
    close_loop=MUTATES, close_loop_rgb=MUTATES, set_auto_loop=SWITCH, auto_loop_stats=RESULT, set_auto_place=SWITCH, auto_place_stats=RESULT,
    debug_slow_frames=DEBUG, debug_squeezes=DEBUG, track_debug=DEBUG, track_stats=DEBUG, track_rgb_debug=DEBUG, track_rgb_stats=DEBUG,
    track_debug_old=DEBUG, track_debug_window=DEBUG, track_rgb_debug_window=DEBUG, census_ms=DEBUG, place_ms=DEBUG, stereo_debug=DEBUG,
    stereo_ms=DEBUG, register_debug=DEBUG, render_model_stats=DEBUG, timings=DEBUG, read_frame_log=RESULT, gpu_process_count=DEBUG,
    download_index_map=DEBUG, download_raw_cloud=DEBUG, download_depth=DEBUG,
    track_old=FORM + "track", track_window=FORM + "track", track_rgb_window=FORM + "track_rgb",
    render_model_device=FORM + "model", fill_image_device=FORM + "fill", stereo_depth_device=FORM + "stereo",
    lidar_depth_device=FORM + "lidar_depth", fern_encode_device=FORM + "ferns", diff_maps=FORM + "compare_maps",
    export_model_device=FORM + "pack",
    set_ferns=SWITCH, fern_add=SWITCH, fern_count=RESULT, fern_keyframes=RESULT, fern_save=REWRITES, fern_load=SWITCH,
    set_stereo=SWITCH, set_lidar_depth=SWITCH, set_frame=MUTATES, set_tick=SWITCH, stage_conflict=MUTATES, stage_cull=MUTATES,
    stage_splat=MUTATES, stage_associate_fuse=MUTATES, device_alloc=SWITCH, device_free=SWITCH, device_upload=SWITCH, device_download=SWITCH,
    counts=RESULT, download_model=RESULT,
    render_maps_stats=RESULT, lidar_stats=RESULT, cast_rays_stats=RESULT, query_points_stats=RESULT, scene_stats=RESULT, tile_stats=RESULT,
    pack_stats=RESULT, register_stats=RESULT, segment_stats=RESULT, mesh_stats=RESULT, locate_stats=RESULT, ground_stats=RESULT,
    compare_stats=RESULT, simplify_stats=RESULT, fill_stats=RESULT, blend_stats=RESULT, lidar_depth_stats=RESULT,
    shard_stream_configure=SWITCH, shard_set_collective=SWITCH, shard_rccl_init=SWITCH, shard_rccl_nranks=SWITCH, shard_rccl_finalize=SWITCH,
    shard_frame=MUTATES, shard_frame_device=MUTATES, shard_compact=MUTATES, shard_export_dense_device=FORM + "pack",
    shard_export_dense=FORM + "pack", rig_configure=SWITCH, rig_consolidate=MUTATES, rig_consolidate_step=MUTATES)


def test_every_public_method_is_a_probe_or_says_why_not():
    from surfelmapping_amd import capi
    public = {n for n, v in vars(capi.SurfelMap).items() if not n.startswith("_") and callable(v)}
    probed = {}
    for p in cp.PROBES.values():
        assert p.kind in cp.KINDS and p.entry_points, p.name
        for e in p.entry_points:
            probed.setdefault(e, []).append(p.name)
    assert set(probed) <= public, sorted(set(probed) - public)
    assert not set(probed) & set(NOT_PROBES), sorted(set(probed) & set(NOT_PROBES))
    assert public == set(probed) | set(NOT_PROBES), (sorted(public - set(probed) - set(NOT_PROBES)), sorted(set(NOT_PROBES) - public))
    for name, why in NOT_PROBES.items():
        assert why in (MUTATES, REWRITES, DEBUG, RESULT, SWITCH) or (why.startswith(FORM) and why[len(FORM):] in cp.PROBES), (name, why)
    # the entry points the list of this suite names, each with the modes that have state of their own
    for entry, least in dict(render_image_maps=3, render_model_maps=1, lidar_sweep_maps=1, recall=1, render_scene=1, lidar_sweep_scene=1,
                             cast_rays=2, query_points=2, pack_maps=1, unpack_maps=1, simplify_maps=1, register_maps=1, compare_maps=1,
                             tile_maps=1, segment_maps=1, mesh_maps=1, ground_maps=1, locate_maps=1, render_image=1, render_model=1,
                             lidar_sweep=1, track=1, track_rgb=1, score_poses=1, search_pose=1, fern_encode=1, fern_match=1, stereo_depth=1,
                             lidar_depth=1, fill_image=1).items():
        assert len(probed.get(entry, ())) >= least, entry
    # every stats key a probe leaves out is one of a registered probe (or of all) and has its reason
    for (who, key), why in cp.STATS_LEFT_OUT.items():
        assert (who == "*" or who in cp.PROBES) and not key.endswith("_ms") and len(why) > 10, (who, key)
    # the refusals hold test_set_call_frame's seven
    import test_set_call_frame as sf
    for call, over in sf.BAD.items():
        assert cp.REFUSALS[call][:2] == (call, over), call


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU: the data, and every (probe, size) as a fresh context's first call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from surfelmapping_amd import capi
    d = cp.street(tmp_path_factory.mktemp("call_order"))
    packer = capi.SurfelMap(capi.make_config(**cp.CAM, **cp.CONFIG))
    d.add_packed(packer)
    packer.close()
    d.start = d.snapshot()
    return d


class Fresh:
    """the result of every (probe, size) on a context that has made no call before it: made when first asked for, kept unchanged"""

    def __init__(self, data, **ctx):
        self.data, self.ctx, self.raw, self.flat = data, ctx, {}, {}

    def result(self, name, size):
        if (name, size) not in self.raw:
            m = cp.context(self.data, **self.ctx)
            self.raw[name, size] = cp.PROBES[name].fn(m, self.data.sets[size])
            m.close()
            self.flat[name, size] = cp.flat(self.raw[name, size], name)
        return self.raw[name, size]

    def __call__(self, name, size):
        self.result(name, size)
        return self.flat[name, size]


@pytest.fixture(scope="module")
def fresh(data):
    return Fresh(data)


def untouched(m, data):
    """after every step: the model and every file of the sets are what they were"""
    assert m.download_model().tobytes() == data.live.tobytes(), "the model changed"
    now = data.snapshot()
    assert now == data.start, [p for p, a, b in zip(data.set_files(), now, data.start) if a != b]


def _both(v):
    v = np.asarray(v)
    return bool((v >= 0).any() and (v < 0).any())


def _drawn(sem, least=200):
    return int((np.asarray(sem) != 0).sum()) > least


def _labels_present(r):
    from surfelmapping_amd import capi
    by_name = {capi.COMPARE_LABEL[c]: n for c, n in enumerate(r["got"]["counts_by_code"])}
    return all(by_name[k] > 0 for k in ("SUPPORTED", "CHANGED", "OUTSIDE"))


def _cells_present(r):
    from surfelmapping_amd import capi
    by_name = dict(zip(capi.GROUND_STATES, r["got"]["info"]["cells_by_state"]))
    return by_name["FREE"] > 0 and by_name["OBSTACLE"] > 0


# what the big result of a fresh context has to show, so that "equal to fresh" says something.  The resident views see the 300 live
# records alone: a disc is a pixel or a few at these sizes, hence the lower count there.
NOT_TRIVIAL = dict(
    image_maps=lambda r: _drawn(r["sem"]),
    image_maps_filled=lambda r: _drawn(r["sem"]) and r["fill"]["filled"] > 0 and int((r["depth"] != 0).sum()) > 200,
    image_maps_blended=lambda r: _drawn(r["sem"]) and r["blend"]["changed"] > 0,
    model_maps=lambda r: int((r["ids"] >= 0).sum()) > 200 and len(np.unique(r["ids"])) > 100,
    sweep_maps=lambda r: int((r["id"] >= 0).sum()) > 200 and _both(r["id"]),
    recall_count=lambda r: 0 < r["n"] < r["stats"]["records_read"] == sum(cp.FILE_ROWS["big"]) + cp.FILE_ROWS["big"][1],
    scene_image=lambda r: _drawn(r["sem"]) and (r["sem"][1:] == cp.ACTOR_CLASS + 1).any() and r["stats"]["actors"] == 2,
    scene_sweep=lambda r: int((r["id"] >= 0).sum()) > 200 and (r["sem"] == cp.ACTOR_CLASS + 1).any(),
    rays_maps=lambda r: _both(r["id"]) and r["stats"]["bad_rays"] == 1 and 0 < r["stats"]["wide"] < r["stats"]["records"] and r["stats"]["cells"] > 0,
    points_maps=lambda r: _both(r["id"]) and r["stats"]["bad_points"] == 1 and 0 < r["stats"]["wide"] < r["stats"]["records"] and r["stats"]["cells"] > 0,
    pack=lambda r: r["stats"]["blocks"] - r["stats"]["raw_blocks"] > 0 and len(r["files"]) == 4,
    unpack=lambda r: len(r["files"]) == 4 and r["stats"]["records"] == sum(cp.FILE_ROWS["big"]) + cp.FILE_ROWS["big"][1],
    simplify_maps=lambda r: r["got"]["cells_merged"] > 0 and r["got"]["records_out"] < r["got"]["records_in"],
    register_maps=lambda r: r["got"]["inliers"] > 0 and r["got"]["iterations"][0] > 0,
    compare_maps=_labels_present,
    tile_maps=lambda r: r["got"]["tiles"] > 1 and r["got"]["files_written"] > 1,
    segment_maps=lambda r: r["got"]["info"]["components"] >= 2,
    mesh_maps=lambda r: r["got"]["info"]["faces"] > 0 and r["got"]["info"]["vertices"] > 0,
    ground_maps=_cells_present,
    locate_maps=lambda r: r["info"]["n_s"] > 0 and r["info"]["target_cells"] > 0 and r["info"]["score"] > 0,
    image=lambda r: all(_drawn(v[1], 100) for v in r["views"]) and r["fill"]["filled"] > 0,
    model=lambda r: all(int((v[2] >= 0).sum()) > 100 for v in r["views"]),
    sweep=lambda r: all(_both(v["id"]) for v in r["sweeps"]),
    rays=lambda r: _both(r["id"]) and r["stats"]["cells"] > 0,
    points=lambda r: _both(r["id"]) and r["stats"]["cells"] > 0,
    track=lambda r: r["info"]["status"] == "OK" and r["info"]["inliers"] > 100 and r["info"]["iterations"] > 1 and r["old"] > 0,
    track_rgb=lambda r: r["info"]["status"] == "OK" and r["info"]["rgb_inliers"] > 0 and int(r["scores"].max()) > 0 and int(r["plain"].max()) > 0,
    search=lambda r: r["info"]["status"] == "OK" and r["info"]["levels_run"] > 1 and max(r["info"]["best_score"]) > 0,
    ferns=lambda r: r["code"].any() and r["k"] >= 0 and len(r["every"]) == 3,
    stereo=lambda r: int((r["depth"] != 0).sum()) > 200,
    lidar_depth=lambda r: 0 < int((r["sparse"] != 0).sum()) < int((r["depth"] != 0).sum()),
    fill=lambda r: r["stats"]["filled"] > 0)


def test_every_probe_has_its_check():
    assert set(NOT_TRIVIAL) == set(cp.NAMES)


@gpu
@pytest.mark.parametrize("name", cp.NAMES)
def test_fresh_result_is_not_vacuous(name, data, fresh):
    """big and small differ, and the big result shows what the feature is for"""
    big = fresh.result(name, "big")
    assert cp.first_difference(fresh(name, "big"), fresh(name, "small")) is not None
    shown = {k: v for k, v in cp.flat(big, name).items() if not isinstance(v, (tuple, bytes))}
    print(name, shown)
    assert NOT_TRIVIAL[name](big), shown
    now = data.snapshot()
    assert now == data.start, [p for p, a, b in zip(data.set_files(), now, data.start) if a != b]


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


@gpu
def test_fresh_big_results_are_the_restatements(data, fresh):
    """so that the expectation of the pairs does not rest on the library alone: the numpy restatements of tests/ on the big set's
    records (the packed file's as pack_ref decodes them)"""
    import compare_ref
    import ground_ref
    import pack_ref
    import points_ref
    import rays_ref
    import segment_ref
    import simplify_ref
    import test_simplify as ts
    from surfelmapping_amd import capi
    a = data.sets["big"]
    rows = data.records("big", lambda p: pack_ref.decode(open(p, "rb").read())[0])
    n_files = len(rows) - len(data.live)
    # the packed file, and the pack probe's files
    want, raw = pack_ref.encode(data.parts["big"][1], 11, 21)
    assert open(data.packed, "rb").read() == want and not raw.any()
    got = fresh.result("pack", "big")["files"]
    for i, part in enumerate(data.parts["big"]):
        assert got[i] == pack_ref.encode(part, 10 + i, 20 + i)[0], i
    assert pack_ref.decode(got[3])[0].shape == data.live.shape
    un = fresh.result("unpack", "big")["files"]
    assert un[:3] == [open(p, "rb").read() for p in a.plain] and un[3] == pack_ref.plain_bytes(rows[n_files - 700:n_files], 11, 21)
    # rays and points: streamed over the set, and the live model alone
    for name, ref, model in (("rays_maps", rays_ref.cast, rows), ("rays", rays_ref.cast, data.live)):
        r, want = fresh.result(name, "big"), ref(model, a.rays)
        for k in ("t", "id", "rgb", "sem", "normal"):
            _same(r[k], want[k], (name, k))
    for name, model in (("points_maps", rows), ("points", data.live)):
        r, want = fresh.result(name, "big"), points_ref.query(model, a.points)
        for k in ("d2", "id", "centre", "normal", "radius", "rgb", "sem"):
            _same(r[k], want[k], (name, k))
    # the analysis calls
    out, st = simplify_ref.simplify(rows, voxel_mm=ts.BITE_MM)
    r = fresh.result("simplify_maps", "big")["got"]
    assert r["file"][:4] == np.uint32(len(out)).tobytes() and r["file"][12:] == out.tobytes() and {k: r[k] for k in ts.STAT_KEYS} == st
    other = np.concatenate([np.fromfile(p, np.float32, offset=12).reshape(-1, 12) for p in a.other])
    want = compare_ref.compare(rows, other, write_mask=15)
    r = fresh.result("compare_maps", "big")["got"]
    assert r["labels"] == want["labels"].tobytes() and r["counts_by_code"] == want["counts"] and r["file"][12:] == want["written"].tobytes()
    assert (r["cells_fine"], r["cells_cover"]) == (want["cells_fine"], want["cells_cover"])
    want = segment_ref.segment(rows, voxel_mm=200)
    r = fresh.result("segment_maps", "big")["got"]
    assert r["labels"] == want["labels"].tobytes() and r["components"] == want["components"].tobytes()
    assert r["file"][12:] == want["kept"].tobytes() and r["info"] == want["info"]
    want = ground_ref.ground(rows, cell_mm=100, origin=(-12.8, 0.0, 0.0))
    r = fresh.result("ground_maps", "big")["got"]
    for k in capi.GROUND_PLANES:
        assert r[k] == want[k].tobytes(), k
    assert r["info"] == want["info"]


# ---------------------------------------------------------------------------------------------------------------------
# every ordered pair on one used context
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("arc", range(N_ARCS))
def test_every_ordered_pair_equals_fresh(arc, data, fresh):
    """a visit is the probe at small, then at big; an arc is a used context of its own.  A(big) -> B(small) meets B with A's larger
    leftovers behind it, small -> big inside a visit meets the growth paths."""
    visits = [cp.NAMES[i] for i in ARCS[arc]]
    for name in dict.fromkeys(visits):                                     # (fresh contexts first: none is made while `used` lives)
        fresh(name, "small"), fresh(name, "big")
    used = cp.context(data)
    t0 = time.perf_counter()
    found = cp.drive(visits, lambda name, size: cp.run(name, used, data, size), fresh, lambda name, size: untouched(used, data))
    print("arc %d: %d visits, %.2f s on the used context" % (arc, len(visits), time.perf_counter() - t0))
    used.close()
    assert not found, "%d comparisons differ; the first: %s" % (len(found), found[:8])


# ---------------------------------------------------------------------------------------------------------------------
# any probe after a refusal of another call
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("refusal", tuple(cp.REFUSALS))
def test_every_probe_after_a_refusal_equals_fresh(refusal, data, fresh):
    """the refused call at big (the set has gone through the staging when a capacity is found too small), then every probe at small"""
    from surfelmapping_amd import capi
    for name in cp.NAMES:
        fresh(name, "small")
    used = cp.context(data)
    before = sorted(os.listdir(data.folder))
    found = []
    for name in cp.NAMES:
        rc = cp.refuse(refusal, used, data, "big")
        assert rc == getattr(capi, cp.REFUSALS[refusal][2]), (refusal, rc)
        left = [f for f in os.listdir(data.folder) if f.endswith(".tmp")]
        assert not left, left
        if rc != capi.SM_OK:
            assert sorted(os.listdir(data.folder)) == before, "a refused call wrote something"
        untouched(used, data)
        keys = cp.differences(cp.run(name, used, data, "small"), fresh(name, "small"))
        if keys:
            found.append(cp.Difference((refusal + " refused", "big"), (name, "small"), keys))
        untouched(used, data)
        before = sorted(os.listdir(data.folder))
    used.close()
    assert not found, "%d comparisons differ; the first: %s" % (len(found), found[:8])


# ---------------------------------------------------------------------------------------------------------------------
# probes between asynchronous frames
# ---------------------------------------------------------------------------------------------------------------------
SMALL = dict(width=320, height=120, fx=180.0, fy=180.0, cx=159.5, cy=59.5)      # test_deferred_compaction.py's stream
STREAM = dict(preprocess=0, stereo_border=20.0, max_sqrt_vertices=700)
GROUPS = dict(sets=tuple(n for n in cp.NAMES if cp.PROBES[n].kind != "resident"), resident=tuple(n for n in cp.NAMES if cp.PROBES[n].kind == "resident"))


def wavy(n):
    from surfelmapping_amd import synth
    return [synth.pose_matrix(0.15 * math.sin(0.7 * k), 0.0, 0.35 * k, 0.25 * math.sin(0.5 * k)) for k in range(n)]


@gpu
@pytest.mark.parametrize("period", [None, 1000])
@pytest.mark.parametrize("group", tuple(GROUPS))
def test_probes_between_asynchronous_frames(group, period, tmp_path):
    """Frames go through process_frame_async, and after frame k, with no sync(), one probe runs at size small with the live model in
    the set: (a) its result is that of a fresh context that holds the oracle's model after frame k, at the same tick -- which fails if
    the call exports the model before the frame's held-back association has landed, or if its ids are not positions among live
    surfels; (b) every frame's counters and the final model are the oracle's, as with no probe in the stream; (c) the trackers and
    the pose search in the gaps, which read the prediction buffers, are part of (b).  A model that is uploaded has no last frame:
    the three probes of FRAME_STATE draw their prediction at the last frame's pose and extrapolate the stream's motion, so they are
    held against a second HIP context that ran the same frames synchronously and was synced."""
    import test_simplify as ts
    from backends import assert_models_equal, make
    from surfelmapping_amd import synth
    names = GROUPS[group]
    n = len(names) + 2                                                     # the reference frame, a gap per probe, one frame after the last
    poses = wavy(n)
    seq = synth.make_sequence(SMALL, poses, seed=21, noise_mm=6.0)
    rows = ts.Scene().rows
    data = cp.Data(tmp_path, rows, rows[:1], SMALL, seq, poses[:3])
    start = data.snapshot()
    over = dict(STREAM) if period is None else dict(STREAM, compact_period=period)
    args = tuple(SMALL[k] for k in ("width", "height", "fx", "fy", "cx", "cy"))
    o, h = make("oracle", *args, **over), make("hip", *args, **over).m
    cp.switches(h, data)
    a = data.sets["small"]
    ref, found = [], []
    for k, fr in enumerate(seq):
        o.process_frame(*fr)
        ref.append(o.counts())
        h.process_frame_async(*fr)
        if k == 0 or k > len(names):
            continue
        name = names[k - 1]
        a.aim(seq[k + 1], look=True)
        got = cp.run(name, h, data, "small")                               # (no sync before it)
        if name in FRAME_STATE:
            twin = make("hip", *args, **over).m
            cp.switches(twin, data)
            for f in seq[:k + 1]:
                twin.process_frame(*f)
            twin.sync()
        else:
            twin = cp.context(data, model=o.download_model(), tick=ref[k]["tick"], config=over)
        keys = cp.differences(got, cp.run(name, twin, data, "small"))
        twin.close()
        if keys:
            found.append(cp.Difference(("frame %d" % k, "async"), (name, "small"), keys))
        assert data.snapshot() == start, name
    h.sync()
    log = h.read_frame_log(64)
    assert len(log) == len(seq) - 1
    for e, r in zip(log, ref[1:]):
        assert (e["unstable_count"], e["fused_count"], e["conflict_count"]) == (r["unstable_count"], r["fused_count"], r["conflict_count"])
    if period == 1000:
        assert (log["n_slots"].astype(np.int64) > log["n_before"]).any(), "no dead slot was there when a call compacted"
    assert_models_equal(o.download_model(), h.download_model(), "the stream with probes in its gaps")
    h.close()
    o.close()
    assert not found, "%d comparisons differ; the first: %s" % (len(found), found[:8])
