"""bench.py's plain run on the GPU: one result line for exactly the steps asked for, with `ms_per_step` and nothing of what
`--full` adds, and `--dump-outputs` writing the timed context's model -- bit-identical to the CPU oracle's over the same
seeded frames -- and its counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from backends import assert_models_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_dumps_the_timed_model(tmp_path):
    out = tmp_path / "dump"
    steps, warmup = 6, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=580)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-1500:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(1e3 / d["ms_per_step"])
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["kernels"] is None and d["roofline"] is None and d["cpu_baseline"] is None
    assert not any(k.endswith("_leg") for k in d)

    model, rows, counts = (np.load(out / f"{n}.npy") for n in ("model", "model_rows", "counts"))
    assert model.dtype == np.float32 and rows.dtype == np.float64 and counts.dtype == np.float64
    n = d["config"]["surfels_end"]
    assert counts[0] == n > 0 and model.shape == (n, 12)
    np.testing.assert_array_equal(rows, np.arange(n))

    import bench
    import oracle_lib as ol
    from surfelmapping_amd import synth
    frames = bench.make_frames(synth.KITTI, warmup + steps, 1, 15.0, 1)      # bench.py's defaults: --seed 1, --noise-mm 15
    o = ol.Oracle(ol.make_config(**synth.KITTI, preprocess=0, conflict_cap=1, max_sqrt_vertices=5000))
    for fr in frames:
        o.process_frame(*fr)
    assert_models_equal(model, o.download_model(), "bench --dump-outputs vs oracle")
    oc = o.counts()
    assert [int(c) for c in counts[:7]] == [oc[k] for k in ("count", "offset", "data_count", "conflict_count", "unstable_count",
                                                            "fused_count", "visible_count")]
    o.close()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_run_longer_than_a_drive_restarts_the_map(tmp_path):
    """More frames than one drive (bench.DRIVE_FRAMES): the map is reset at the drive boundary and the same frames are
    driven again, so the run completes whatever --steps is, and after it the model is that of the last drive's frames on an
    emptied map -- the oracle's after frame 0, reset(), then those frames."""
    import bench
    import oracle_lib as ol
    from surfelmapping_amd import synth
    out = tmp_path / "dump"
    warmup, tail = 2, 10
    steps = bench.DRIVE_FRAMES + tail - warmup
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=580)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    assert d["steps"] == steps and d["config"]["drive"] == {"frames": bench.DRIVE_FRAMES, "map_resets_in_timed_frames": 1}

    frames = bench.make_frames(synth.KITTI, tail, 1, 15.0, 1)
    o = ol.Oracle(ol.make_config(**synth.KITTI, preprocess=0, conflict_cap=1, max_sqrt_vertices=5000))
    o.process_frame(*frames[0])
    o.reset()
    for fr in frames:
        o.process_frame(*fr)
    assert_models_equal(np.load(out / "model.npy"), o.download_model(), "after the drive boundary vs oracle")
    assert np.load(out / "counts.npy")[0] == o.counts()["count"] == d["config"]["surfels_end"]
    o.close()
