"""The four consumers of the shared map-file staging (MapStream over the context's MapStaging; surfelmapping_amd/csrc/sm_map_stream.h)
interleaved on ONE context: the streamed renderers, sm_recall in its modes, the lidar's sweeps of the set, sm_warp_by_time, then the
map-file writer and the lenient reader.  Each consumer is checked in its own suite (test_render_maps.py, test_recall.py,
test_lidar.py, test_warp.py, multi-chunk files included); here every call finds the staging as another consumer left it.  Files of one chunk each: 300 rows, none, 257 (a block with one row)."""
import os

import numpy as np
import pytest

import model_view_ref as ref
import recall_ref as cr
import retire_ref as rr
import warp_ref as wr
from backends import assert_models_equal

CAM, OVER = cr.CAM, cr.OVER
IMG = (160, 60, 90.0, 90.0, 79.5, 29.5)
MW, MH = 160, 120
SIZES, N_LIVE = (300, 0, 257), 50
KW = dict(threshold=0.5, unstable=True, color_type=2)


def _gpu():
    from surfelmapping_amd import capi
    return capi.SurfelMap(capi.make_config(**CAM, **OVER, preprocess=0, max_sqrt_vertices=64))


def _rows(n, seed):
    """n seeded surfels drawn into the box |x| <= 6, -0.9 <= y <= 1.5, 5 <= z <= 35, radii 6 - 30 cm"""
    from surfelmapping_amd import synth
    m = synth.seeded_model(n, 50, seed=seed)
    m[:, 0] *= np.float32(0.1)
    m[:, 1] *= np.float32(0.3)
    m[:, 2] = m[:, 2] * np.float32(0.1) + np.float32(10.0)
    m[:, 11] *= np.float32(3.0)
    return m


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _resident(rows):
    g = _gpu()
    g.upload_model(rows)
    return g


def _image_equal(g, paths, views, whole, what):
    """render_image_maps of the set against the resident renderer on a context that holds its concatenation"""
    bgr, sem = g.render_image_maps(paths, views, *IMG, include_model=True)
    st = g.render_maps_stats()
    assert st["chunks"] == 2 and st["passes"] == 1, st              # (the empty file has no chunk)
    big = _resident(whole)
    for i, v in enumerate(views):
        wb, ws = big.render_image(v, *IMG)
        _same(bgr[i], wb, (what, "bgr", i))
        _same(sem[i], ws, (what, "sem", i))
    assert (sem != 0).sum() > 200, what
    return st


@pytest.mark.gpu
def test_consumers_interleaved_on_one_context(tmp_path):
    from surfelmapping_amd import capi, synth
    files = [_rows(n, 10 + i) for i, n in enumerate(SIZES)]
    ids = [(1, 2), (3, 4), (5, 6)]
    live = _rows(N_LIVE, 20)
    paths = [str(tmp_path / f"m{i}.bin") for i in range(3)]
    for p, f, (a, b) in zip(paths, files, ids):
        cr.write_map(p, f, a, b)
    views = np.stack([synth.pose_to_colmajor(synth.pose_matrix(*a)) for a in ((0, 0, 0), (2, 0, 8, 10.0), (0, 0, 40, 180.0))])
    P = ref.projection(MW, MH, 105.0, 105.0, 80.0, 60.0, 0.1, 1000.0)
    cams = [ref.view_mats(P, m) for m in (ref.look_at(0, -6, -10, 0, 0, 20, 0, -1, 0), ref.look_at(0, -40, 20, 0, 0, 20.5, 0, 0, 1))]
    pose = np.eye(4, dtype=np.float32).T.reshape(16).copy()
    pose[12:15] = (0.0, 0.0, 20.0)
    radius = 8.0
    near = [cr.near(f, pose, radius) for f in files]
    assert all(0 < k.sum() < len(k) for k, n in zip(near, SIZES) if n), [int(k.sum()) for k in near]
    recalled = np.concatenate([f[k] for f, k in zip(files, near)])

    g = _gpu()
    g.upload_model(live)
    g.set_tick(60)
    whole = np.concatenate(files + [live])

    # 1. the novel views
    _image_equal(g, paths, views, whole, "before")

    # 2. a recall that only counts: the figure of the reference, nothing changes
    before = [(open(p, "rb").read(), os.stat(p).st_mtime_ns) for p in paths]
    assert g.recall(paths, pose=pose, mode="count", radius=radius) == len(recalled)
    st = g.recall_stats()
    assert st["chunks"] == 2 and st["records_read"] == sum(SIZES) and st["files_read"] == 3 and st["files_rewritten"] == 0, st
    assert [(open(p, "rb").read(), os.stat(p).st_mtime_ns) for p in paths] == before
    assert_models_equal(g.download_model(), live, "after COUNT")

    # 3. the model views, with depth and ids
    mv = [capi.model_view(mvp, inv, MW, MH, **KW) for mvp, inv in cams]
    got = g.render_model_maps(paths, mv, include_model=True, depth=True, ids=True)
    assert g.render_maps_stats()["chunks"] == 2
    big = _resident(whole)
    for k, (mvp, inv) in enumerate(cams):
        want = big.render_model(mvp, inv, MW, MH, depth=True, ids=True, **KW)
        for a, b, name in zip(got, want, ("rgba", "depth", "ids")):
            _same(a[k], b, (k, name))
    seen = got[2][got[2] >= 0]
    assert len(seen) > 200 and (seen < SIZES[0]).any() and ((seen >= SIZES[0]) & (seen < sum(SIZES))).any() and (seen >= sum(SIZES)).any()

    # 3b. the lidar: two sweeps of the set in one pass, plane for plane the resident sweep of the concatenation
    sn = capi.lidar_sensor(n_az=90, az0_deg=-178.0, az_step_deg=4.0, el_deg=np.arange(-7, 8, 2, dtype=np.float32), min_range=1.0,
                           max_range=60.0, min_conf=0.0)
    sweeps = np.stack([synth.pose_to_colmajor(synth.pose_matrix(*a)) for a in ((0, 0, 20), (2, 0, 8, 10.0))])
    got = g.lidar_sweep_maps(paths, sweeps, sn)
    st = g.lidar_stats()
    assert st["chunks"] == 2 and st["passes"] == 1, st
    for i, sp in enumerate(sweeps):
        want = big.lidar_sweep(sp, sn)
        for name in ("range", "id", "rgb", "sem"):
            _same(got[name][i], want[name], ("lidar", name, i))
    assert (got["id"] >= 0).sum() > 300
    assert [(open(p, "rb").read(), os.stat(p).st_mtime_ns) for p in paths] == before

    # 4. the recall that moves: the reference's rows into the model, the rows that stay in the files
    ref_files = [[f.copy(), a, b] for f, (a, b) in zip(files, ids)]
    R, rewritten = cr.recall_files(ref_files, pose, radius)
    assert_models_equal(R, recalled, "the reference's own two forms")
    assert g.recall(paths, pose=pose, mode="move", radius=radius) == len(recalled)
    assert g.recall_stats()["files_rewritten"] == rewritten == 2
    assert_models_equal(g.download_model(), np.concatenate([live, recalled]), "after MOVE")
    for p, f, k, (a, b), rf in zip(paths, files, near, ids, ref_files):
        rows, a1, b1 = rr.read_map(p)
        assert_models_equal(rows, f[~k], p)
        assert_models_equal(rows, rf[0], p)
        assert (a1, b1) == (a, b)
    assert (open(paths[1], "rb").read(), os.stat(paths[1]).st_mtime_ns) == before[1]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".recall.tmp")]

    # 5. the novel views of what is now in the files and in the model
    _image_equal(g, paths, views, np.concatenate([f[~k] for f, k in zip(files, near)] + [live, recalled]), "after MOVE")

    # 5b. the warp by time of what the MOVE left, files and model: part of each file's rows is selected
    table, t0 = wr.rigid_table(4, seed=5), -100
    left = [f[~k] for f, k in zip(files, near)]
    model = np.concatenate([live, recalled])
    for f in left:
        sel = wr.select(f[:, 7], t0, len(table))[0]
        assert len(f) == 0 or 0 < sel.sum() < len(f), int(sel.sum())
    empty = (open(paths[1], "rb").read(), os.stat(paths[1]).st_mtime_ns)
    g.warp_by_time(paths, t0, table)
    st = g.warp_stats()
    assert st["files_rewritten"] == 2 and st["chunks"] == 2 and st["records_read"] == sum(len(f) for f in left), st
    warped = [wr.warp_rows(f, t0, table) for f in left]
    for p, f, (a, b) in zip(paths, warped, ids):
        rows, a1, b1 = rr.read_map(p)
        _same(rows, f, p)
        assert (a1, b1) == (a, b)
    _same(g.download_model(), wr.warp_rows(model, t0, table), "after the warp")
    assert (open(paths[1], "rb").read(), os.stat(paths[1]).st_mtime_ns) == empty == before[1]
    assert not [f for f in os.listdir(tmp_path) if f.endswith((".warp.tmp", ".recall.tmp"))]

    # 5c. the novel views of the warped set
    _image_equal(g, paths, views, np.concatenate(warped + [wr.warp_rows(model, t0, table)]), "after the warp")

    # 6. the writer and the lenient reader
    out = str(tmp_path / "saved.bin")
    g.save_map(out, 7, 60)
    model = g.download_model()
    assert open(out, "rb").read() == np.array([len(model)], np.uint32).tobytes() + np.array([7, 60], np.int32).tobytes() + model.tobytes()
    h = _gpu()
    assert h.load_map(out) == (7, 60)
    assert_models_equal(h.download_model(), model, "loaded map")
