"""Packed map files on the GPU (sm_pack_maps, sm_unpack_maps, k_unpack in the chunk stream): the encoder and the decoder bit for
bit against tests/pack_ref.py, every reader of a map set on packed files against the same call on their unpacked twins, a packed
file of more than a chunk, and the refusals."""
import os

import numpy as np
import pytest

import model_view_ref as ref
import pack_ref as pr
import recall_ref as cr

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 255, 256, 257, 300, 769)
IMG = (160, 60, 90.0, 90.0, 79.5, 29.5)
MW, MH = 160, 120


def _gpu(cap=64):
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**cr.CAM, **cr.OVER, preprocess=0, max_sqrt_vertices=cap))


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _state(paths):
    return [(open(p, "rb").read(), os.stat(p).st_mtime_ns) for p in paths]


def _no_tmp(folder):
    assert not [f for f in os.listdir(folder) if f.endswith(".tmp")], os.listdir(folder)


# ---------------------------------------------------------------------------------------------------------------------
# bit for bit against the reference
# ---------------------------------------------------------------------------------------------------------------------
class Packed:
    """the plain files of fixture A at every size and of fixture B, packed and unpacked by ONE call each on one context"""

    def __init__(self, folder):
        self.folder = str(folder)
        self.rows = [pr.fixture_a(n, seed=20 + i) for i, n in enumerate(SIZES)] + [pr.fixture_b()[0]]
        self.ids = [(i, 2 * i + 1) for i in range(len(self.rows))]
        self.plain = [os.path.join(self.folder, f"src{i}.bin") for i in range(len(self.rows))]
        for p, r, (a, b) in zip(self.plain, self.rows, self.ids):
            cr.write_map(p, r, a, b)
        self.want = [pr.encode(r, a, b) for r, (a, b) in zip(self.rows, self.ids)]            # (bytes, raw flags)
        self.before = _state(self.plain)
        self.g = _gpu()
        self.packed = self.g.pack_maps(self.plain, os.path.join(self.folder, "pk"))
        self.pack_stats = self.g.pack_stats()
        self.unpacked = self.g.unpack_maps(self.packed + [self.plain[5]], os.path.join(self.folder, "un"))
        self.unpack_stats = self.g.pack_stats()


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    return Packed(tmp_path_factory.mktemp("pack"))


def test_reference_packs_fixture_a_whole_and_flags_fixture_b(packed):
    """a fixture that went all-RAW would prove nothing"""
    for n, (_, raw) in zip(SIZES, packed.want):
        assert len(raw) == (n + 255) // 256 and not raw.any(), n
    assert list(np.flatnonzero(packed.want[-1][1])) == list(pr.fixture_b()[1])


def test_pack_maps_writes_the_reference_bytes(packed):
    assert [os.path.basename(p) for p in packed.packed] == ["pk_%06d.smp" % i for i in range(len(packed.rows))]
    for path, (want, _), n in zip(packed.packed, packed.want, list(SIZES) + ["B"]):
        got = open(path, "rb").read()
        assert len(got) == len(want), n
        assert got[:32] == want[:32], (n, "header")
        nb = len(want) and int(np.frombuffer(want, "<u4", 8)[6])
        assert got[32:32 + 32 * nb] == want[32:32 + 32 * nb], (n, "directory", np.frombuffer(got, pr.DIR_DTYPE, nb, 32), np.frombuffer(want, pr.DIR_DTYPE, nb, 32))
        assert got == want, (n, "payload")
    assert _state(packed.plain) == packed.before
    _no_tmp(packed.folder)


def test_unpack_maps_writes_the_reference_decode(packed):
    for i, (path, (want, _), (a, b)) in enumerate(zip(packed.unpacked, packed.want, packed.ids)):
        assert open(path, "rb").read() == pr.plain_bytes(pr.decode(want)[0], a, b), i
    # a plain source is copied through verbatim
    assert open(packed.unpacked[-1], "rb").read() == packed.before[5][0]
    # what a packed block loses it loses once: packing the unpacked files again and unpacking gives the same files
    again = packed.g.unpack_maps(packed.g.pack_maps(packed.unpacked[:-1], os.path.join(packed.folder, "pk2")), os.path.join(packed.folder, "un2"))
    for p, q in zip(again, packed.unpacked):
        assert open(p, "rb").read() == open(q, "rb").read(), p
    _no_tmp(packed.folder)


def test_read_packed_map_is_both(packed):
    from surfelmapping_amd import capi
    import retire_ref as rr
    for path, un, (want, raw), ids in zip(packed.packed, packed.unpacked, packed.want, packed.ids):
        rows, got_ids, got_raw = capi.read_packed_map(path)
        assert got_ids == ids and np.array_equal(got_raw, raw)
        _same(rows, pr.decode(want)[0], path)
        _same(rows, rr.read_map(un)[0].reshape(-1, 12), un)


def test_pack_stats_are_the_reference_counts(packed):
    st, n = packed.pack_stats, sum(len(r) for r in packed.rows)
    raws = [raw for _, raw in packed.want]
    blocks, raw_blocks = sum(len(r) for r in raws), sum(int(r.sum()) for r in raws)
    raw_records = sum(int(np.minimum(256, len(rows) - 256 * np.flatnonzero(raw)).sum()) for rows, raw in zip(packed.rows, raws))
    assert raw_blocks == len(pr.RAW_CAUSES) and raw_records == 256 * raw_blocks
    assert (st["files"], st["records"], st["blocks"], st["raw_blocks"]) == (len(packed.rows), n, blocks, raw_blocks), st
    assert st["bytes_in"] == sum(12 + 48 * len(r) for r in packed.rows)
    assert st["bytes_out"] == 32 * len(packed.rows) + 32 * blocks + 20 * (n - raw_records) + 48 * raw_records == sum(len(w) for w, _ in packed.want)
    assert st["chunks"] == len(SIZES) and st["total_ms"] > 0.0 and st["device_ms"] > 0.0      # (the empty file has no chunk)
    un = packed.unpack_stats
    assert (un["files"], un["records"], un["blocks"], un["raw_blocks"]) == (len(packed.rows) + 1, n + 300, blocks, raw_blocks), un
    assert un["bytes_in"] == st["bytes_out"] + 12 + 48 * 300 and un["bytes_out"] == st["bytes_in"] + 12 + 48 * 300


def test_live_model_is_packed_as_one_more_file(tmp_path):
    rows, live = pr.fixture_a(300, 30), pr.fixture_a(700, 31)
    src = str(tmp_path / "a.bin")
    cr.write_map(src, rows, 4, 5)
    g = _gpu()
    g.upload_model(live)
    out = g.pack_maps([src], str(tmp_path / "pk"), include_model=True, pos_step_log2=-9)
    assert len(out) == 2
    assert open(out[0], "rb").read() == pr.encode(rows, 4, 5, -9)[0]
    assert open(out[1], "rb").read() == pr.encode(live, 0, 0, -9)[0]
    _same(g.download_model(), live, "the model stays")
    st = g.pack_stats()
    assert st["files"] == 2 and st["records"] == 1000 and st["bytes_in"] == 12 + 48 * 300 + 48 * 700
    _no_tmp(tmp_path)


# ---------------------------------------------------------------------------------------------------------------------
# every reader
# ---------------------------------------------------------------------------------------------------------------------
def _visible(m):
    """fixture rows drawn into the box |x| <= 6, -0.9 <= y <= 1.5, 5 <= z <= 35, radii 6 - 30 cm"""
    m = m.copy()
    m[:, 0] *= np.float32(0.4)
    m[:, 1] *= np.float32(0.3)
    m[:, 2] = m[:, 2] * np.float32(0.5) + np.float32(10.0)
    m[:, 11] *= np.float32(3.0)
    return m


def _flat(v, key=""):
    """a call's answer as a list of (name, bytes or plain value), times left out"""
    if isinstance(v, dict):
        return [x for k in sorted(v) if not k.endswith("_ms") for x in _flat(v[k], f"{key}.{k}")]
    if isinstance(v, (tuple, list)):
        return [x for i, e in enumerate(v) for x in _flat(e, f"{key}[{i}]")]
    if isinstance(v, np.ndarray):
        return [(key, v.dtype.str, v.shape, v.tobytes())]
    return [(key, v)]


class Twins:
    """[packed A, plain, packed B] and [unpacked A, plain, unpacked B] beside one context that holds a live model"""

    def __init__(self, folder):
        self.folder = str(folder)
        a, plain = _visible(pr.fixture_a(600, 11)), _visible(pr.fixture_a(300, 12))
        b, self.raw_b = pr.fixture_b(base=_visible(pr.fixture_a(pr.B_ROWS, 13)))
        self.live = _visible(pr.fixture_a(50, 14))
        src = [os.path.join(self.folder, f"{n}.bin") for n in ("a", "plain", "b")]
        for p, r, i in zip(src, (a, plain, b), range(3)):
            cr.write_map(p, r, i, i + 10)
        self.g = _gpu()
        self.g.upload_model(self.live)
        self.g.set_tick(1100)
        pk = self.g.pack_maps([src[0], src[2]], os.path.join(self.folder, "pk"))
        un = self.g.unpack_maps(pk, os.path.join(self.folder, "un"))
        self.packed, self.unpacked = [pk[0], src[1], pk[1]], [un[0], src[1], un[1]]
        raws = [capi_raw(p) for p in pk]
        assert not raws[0].any() and list(np.flatnonzero(raws[1])) == list(self.raw_b)
        self.records = 600 + 300 + pr.B_ROWS
        # a second set for the calls on two sets: the plain file moved by 3 cm; an actor of a scene
        moved = plain.copy()
        moved[:, 0] += np.float32(0.03)
        self.other = [os.path.join(self.folder, "other.bin")]
        cr.write_map(self.other[0], np.concatenate([a, moved]), 30, 40)
        self.actor = os.path.join(self.folder, "actor.bin")
        cr.write_map(self.actor, _visible(pr.fixture_a(200, 15)), 0, 0)
        self.n_out = 0

    def out(self, tag):
        self.n_out += 1
        return os.path.join(self.folder, f"out{self.n_out}_{tag}")

    def both(self, call, filled, what):
        """call(paths, tag) on the packed set and on its twin: the same answer, byte for byte, and not an empty one"""
        before = _state(self.packed + self.unpacked)
        got, want = call(self.packed, "p"), call(self.unpacked, "u")
        fg, fw = _flat(got), _flat(want)
        assert [x[:-1] for x in fg] == [x[:-1] for x in fw], what
        for x, y in zip(fg, fw):
            assert x == y, (what, x[0])
        n = filled(got)
        print(what, "non-empty:", n)
        assert n > 200, (what, n)
        assert _state(self.packed + self.unpacked) == before, what
        return got


def capi_raw(path):
    from surfelmapping_amd import capi
    return capi.read_packed_map(path)[2]


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    return Twins(tmp_path_factory.mktemp("twins"))


def _views():
    from surfelmapping_amd import synth
    return np.stack([synth.pose_to_colmajor(synth.pose_matrix(*a)) for a in ((0, 0, 0), (2, 0, 8, 10.0), (0, 0, 40, 180.0))])


def _files(paths):
    return [open(p, "rb").read() for p in paths]


def test_views_sweeps_rays_and_points(twins):
    from surfelmapping_amd import capi, synth
    g, views = twins.g, _views()
    twins.both(lambda p, t: g.render_image_maps(p, views, *IMG), lambda r: int((r[1] != 0).sum()), "render_image_maps")
    assert g.render_maps_stats()["chunks"] == 3
    twins.both(lambda p, t: g.render_image_maps(p, views, *IMG, fill=True, depth=True), lambda r: int((r[1] != 0).sum()), "render_image_maps fill")
    twins.both(lambda p, t: g.render_image_maps(p, views, *IMG, blend=True), lambda r: int((r[1] != 0).sum()), "render_image_maps blend")
    P = ref.projection(MW, MH, 105.0, 105.0, 80.0, 60.0, 0.1, 1000.0)
    mv = [capi.model_view(mvp, inv, MW, MH, threshold=0.5, unstable=True, color_type=2)
          for mvp, inv in (ref.view_mats(P, m) for m in (ref.look_at(0, -6, -10, 0, 0, 20, 0, -1, 0), ref.look_at(0, -40, 20, 0, 0, 20.5, 0, 0, 1)))]
    got = twins.both(lambda p, t: g.render_model_maps(p, mv, depth=True, ids=True), lambda r: int((r[2] >= 0).sum()), "render_model_maps")
    seen = got[2][got[2] >= 0]
    assert (seen < 600).any() and ((seen >= 900) & (seen < twins.records)).any() and (seen >= twins.records).any()    # A, B and the live model
    sn = capi.lidar_sensor(n_az=90, az0_deg=-178.0, az_step_deg=4.0, el_deg=np.arange(-7, 8, 2, dtype=np.float32), min_range=1.0, max_range=60.0,
                           min_conf=0.0)
    sweeps = np.stack([synth.pose_to_colmajor(synth.pose_matrix(*a)) for a in ((0, 0, 20), (2, 0, 8, 10.0))])
    twins.both(lambda p, t: g.lidar_sweep_maps(p, sweeps, sn), lambda r: int((r["id"] >= 0).sum()), "lidar_sweep_maps")
    rays = capi.lidar_rays(sn, sweeps[0])
    twins.both(lambda p, t: g.cast_rays(rays, p, normal=True), lambda r: int((r["id"] >= 0).sum()), "cast_rays")
    rows = np.concatenate([capi.read_packed_map(twins.packed[0])[0], twins.live])
    pts = np.concatenate([rows[:, 0:3] + np.float32(0.05), np.full((len(rows), 1), 0.5, np.float32)], axis=1)
    twins.both(lambda p, t: g.query_points(pts, p), lambda r: int((r["id"] >= 0).sum()), "query_points")
    # scenes: an actor file beside the set
    poses = np.tile(np.eye(4, dtype=np.float32)[None], (len(views), 1, 1))
    poses[:, 0, 3] = 1.0
    twins.both(lambda p, t: g.render_scene(p, [(twins.actor, poses)], views, *IMG), lambda r: int((r[1] != 0).sum()), "render_scene")
    twins.both(lambda p, t: g.lidar_sweep_scene(p, [(twins.actor, poses[:2])], sweeps, sn), lambda r: int((r["id"] >= 0).sum()), "lidar_sweep_scene")


def test_analysis_calls(twins):
    from surfelmapping_amd import capi
    g = twins.g

    def simplify(p, t):
        out = twins.out(t)
        st = g.simplify_maps(p, out, include_model=True, voxel_mm=250)
        return dict(file=open(out, "rb").read(), **{k: v for k, v in st.items() if k not in ("launches",)})
    twins.both(simplify, lambda r: r["records_out"], "simplify_maps")

    def register(p, t):
        pose, info = g.register_maps(p, twins.other, source_model=True, voxel_mm=200, levels=2, min_inliers=10, pivot=(0.0, 0.0, 20.0))
        return dict(pose=pose, info=info)
    twins.both(register, lambda r: r["info"]["samples"], "register_maps")

    def compare(p, t):
        out = twins.out(t)
        lab, info = g.compare_maps(p, twins.other, query_model=True, out_path=out, write_mask=15)
        return dict(labels=lab, info=info, file=open(out, "rb").read())
    twins.both(compare, lambda r: int((r["labels"] == capi.SM_COMPARE_SUPPORTED).sum()), "compare_maps")

    def tile(p, t):
        files = g.tile_maps(p, twins.out(t), include_model=True, cell_mm=200, tile_shift=4, max_file_records=512)
        st = g.tile_stats()
        return dict(files=_files(files), **{k: st[k] for k in ("records_in", "placed", "loose", "tiles", "largest_tile", "files_written")})
    twins.both(tile, lambda r: r["placed"], "tile_maps")

    def segment(p, t):
        out = twins.out(t)
        got = g.segment_maps(p, include_model=True, out_path=out, voxel_mm=1000)
        return dict(got, file=open(out, "rb").read())
    twins.both(segment, lambda r: int((r["labels"] < capi.SM_SEGMENT_SKIPPED).sum()), "segment_maps")

    def mesh(p, t):
        out = twins.out(t)
        got = g.mesh_maps(p, include_model=True, ply_path=out, voxel_mm=1000)
        return dict(got, file=open(out, "rb").read())
    twins.both(mesh, lambda r: len(r["vertices"]), "mesh_maps")

    def ground(p, t):
        return g.ground_maps(p, include_model=True, cell_mm=250, origin=(-8.0, 0.0, 4.0), nu=64, nv=128)
    twins.both(ground, lambda r: int((r["state"] != 0).sum()), "ground_maps")


def test_recall_counts_and_copies(twins):
    g = twins.g
    pose = np.eye(4, dtype=np.float32).T.reshape(16).copy()
    pose[12:15] = (0.0, 0.0, 20.0)
    twins.both(lambda p, t: g.recall(p, pose=pose, mode="count", radius=12.0), lambda r: r, "recall count")
    assert g.recall_stats()["files_rewritten"] == 0 and g.recall_stats()["records_read"] == twins.records
    _same(g.download_model(), twins.live, "after COUNT")

    def copy(p, t):
        g.upload_model(twins.live)
        n = g.recall(p, pose=pose, mode="copy", radius=12.0)
        return dict(n=n, model=g.download_model())
    got = twins.both(copy, lambda r: r["n"], "recall copy")
    assert len(got["model"]) == len(twins.live) + got["n"]
    g.upload_model(twins.live)
    _no_tmp(twins.folder)


# ---------------------------------------------------------------------------------------------------------------------
# more than a chunk
# ---------------------------------------------------------------------------------------------------------------------
def test_packed_file_of_more_than_a_chunk(tmp_path):
    """2^20 + 450 records: the last block of the first chunk is RAW, the second chunk has a whole block and a short one"""
    from surfelmapping_amd import capi
    n = (1 << 20) + 450
    rows = _visible(pr.fixture_a(n, 40))
    rows[(1 << 20) - 100, 3] = np.float32(-1.0)              # conf -1: block 4095 is RAW
    src = str(tmp_path / "big.bin")
    cr.write_map(src, rows, 1, 2)
    g = _gpu()
    pk = g.pack_maps([src], str(tmp_path / "pk"))
    st = g.pack_stats()
    assert st["chunks"] == 2 and st["blocks"] == 4098 and st["raw_blocks"] == 1 and st["bytes_out"] == 32 + 32 * 4098 + 20 * (n - 256) + 48 * 256, st
    head = np.frombuffer(open(pk[0], "rb").read(32 + 32 * 4098), "<u1")
    d = head[32:].view(pr.DIR_DTYPE)
    assert list(np.flatnonzero(d["flags"])) == [4095]
    un = g.unpack_maps(pk, str(tmp_path / "un"))
    assert g.pack_stats()["chunks"] == 2
    twin = np.fromfile(un[0], np.float32, offset=12).reshape(-1, 12)
    assert len(twin) == n
    # the chunks' first and last blocks and the RAW one against the reference decode of the reference's encoding of those blocks
    for first in (0, (1 << 20) - 256, 1 << 20, (1 << 20) + 256):
        sl = slice(first, min(first + 256, n))
        _same(twin[sl], pr.decode(pr.encode(rows[sl])[0])[0], first)
    _same(twin[(1 << 20) - 256:1 << 20], rows[(1 << 20) - 256:1 << 20], "the RAW block is verbatim")
    views = _views()
    got, want = g.render_image_maps(pk, views, *IMG, include_model=False), None
    chunks = g.render_maps_stats()["chunks"]
    want = g.render_image_maps(un, views, *IMG, include_model=False)
    assert chunks == 2 == g.render_maps_stats()["chunks"]
    for a, b in zip(got, want):
        _same(a, b, "view")
    assert (got[1] != 0).sum() > 200
    pose = np.eye(4, dtype=np.float32).T.reshape(16).copy()
    pose[12:15] = (0.0, 0.0, 20.0)
    near = g.recall(pk, pose=pose, mode="count", radius=3.0)
    assert g.recall_stats()["chunks"] == 2
    assert near == g.recall(un, pose=pose, mode="count", radius=3.0) == int(cr.near(twin, pose, 3.0).sum()) and near > 200
    assert capi._map_records(pk[0]) == n


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(tmp_path):
    from surfelmapping_amd import capi
    rows = _visible(pr.fixture_a(300, 50))
    plain = str(tmp_path / "pk_000000.smp")                 # (a plain file under the name the packing of [it] would write)
    other = str(tmp_path / "other.bin")
    cr.write_map(plain, rows, 1, 2)
    cr.write_map(other, rows, 1, 2)
    g = _gpu()
    g.upload_model(_visible(pr.fixture_a(50, 51)))
    packed = g.pack_maps([other], str(tmp_path / "good"))[0]
    cut, taken = str(tmp_path / "cut.smp"), str(tmp_path / "good_000001.bin")
    open(cut, "wb").write(open(packed, "rb").read()[:-1])
    cr.write_map(taken, rows[:10], 0, 0)                    # (a source under the name the unpacking of two files would write)
    sources = [plain, other, packed, cut, taken]
    before, listing, model = _state(sources), sorted(os.listdir(tmp_path)), g.download_model()

    def refused(rc, names, call):
        with pytest.raises(capi.SurfelMapError) as e:
            call()
        assert e.value.rc == rc, e.value
        for name in names:
            assert name in str(e.value), e.value
        assert _state(sources) == before and sorted(os.listdir(tmp_path)) == listing
        _same(g.download_model(), model, "the model")

    table = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (2, 1))
    pose = np.eye(4, dtype=np.float32).T.reshape(16).copy()
    views = _views()
    poses = np.tile(np.eye(4, dtype=np.float32)[None], (len(views), 1, 1))
    refused(capi.SM_E_UNSUPPORTED, [packed], lambda: g.warp_by_time([other, packed], 0, table))
    refused(capi.SM_E_UNSUPPORTED, [packed], lambda: g.recall([other, packed], pose=pose, mode="move", radius=100.0))
    refused(capi.SM_E_UNSUPPORTED, [packed], lambda: g.render_scene([other], [(packed, poses)], views, *IMG))
    refused(capi.SM_E_ARG, [packed, "sm_unpack_maps makes a plain one"], lambda: g.load_map(packed))
    refused(capi.SM_E_ARG, [plain, "of its own"], lambda: g.pack_maps([plain], str(tmp_path / "pk")))
    refused(capi.SM_E_ARG, ["of its own"], lambda: g.unpack_maps([packed, taken], str(tmp_path / "good")))
    for step in (-15, -5):
        refused(capi.SM_E_ARG, ["pos_step_log2"], lambda: g.pack_maps([other], str(tmp_path / "x"), pos_step_log2=step))
    refused(capi.SM_E_ARG, [cut, "its directory needs"], lambda: g.render_image_maps([other, cut], views, *IMG))
    refused(capi.SM_E_ARG, [cut], lambda: g.unpack_maps([cut], str(tmp_path / "y")))
    refused(capi.SM_E_ARG, [cut], lambda: g.recall([cut], pose=pose, mode="count", radius=100.0))
    # and the packed file is read by what only reads
    assert g.recall([packed], pose=pose, mode="count", radius=100.0) == 300
