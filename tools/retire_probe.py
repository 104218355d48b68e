#!/usr/bin/env python3
"""What a retirement costs, on one GPU, in one process; every figure the median of 5 after 2 warm-ups.

  sizes   synth.seeded_model(n, tick) at config HD (update times spread over 300 ticks: min_age = 200, min_distance = 0 retires
          about a third): sm_retire end to end into host memory; its device part per step by HIP events (SM_RETIRE_TIMING, taken
          from sm_retire_device so that the gather carries no copy); and the route there was before, same model, same result:
          download_model + the numpy mask + upload_model.  Algorithmic bytes over kernel time for mark and gather.
  frames  frames/s of 200 KITTI-shaped frames, device-resident (as bench.py's plain leg feeds them): policy off (three times:
          the spread) alternating with on at every = 1000 (never fires), then on with every = 50.

Writes one JSON file (--out)."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SM_RETIRE_TIMING", "1")
from surfelmapping_amd import capi, synth  # noqa: E402

HBM_ROOF = 8.0e12          # bytes/s
TICK, MIN_AGE = 1000, 200
WARM, REPS = 2, 5


def mask(m, tick, min_age):
    """the definition with min_distance = 0 (include/sm_c_api.h): the age gate alone"""
    with np.errstate(invalid="ignore"):
        return (np.float32(tick) - m[:, 7]) > np.float32(min_age)


def med(xs):
    return float(np.median(xs))


def probe_size(sm, n):
    L = sm._L
    m0 = synth.seeded_model(n, TICK)
    r0 = mask(m0, TICK, MIN_AGE)
    n_ret = int(r0.sum())
    p = capi.retire_params(sm.cfg, min_age=MIN_AGE, min_distance=0.0)
    pose = np.eye(4, dtype=np.float32).reshape(16)
    buf = np.zeros((n, 12), np.float32)
    cnt = C.c_uint32()
    d_buf = sm.device_alloc(n * 48)

    def reset():
        sm.upload_model(m0)
        sm.set_tick(TICK)

    def host():
        return L.sm_retire(sm._h, pose.ctypes.data_as(C.c_void_p), C.byref(p), buf.ctypes.data_as(C.c_void_p), n, C.byref(cnt))

    def device():
        return L.sm_retire_device(sm._h, pose.ctypes.data_as(C.c_void_p), C.byref(p), d_buf, n, C.byref(cnt))

    # the result first: records and model equal the definition
    reset()
    assert host() == 0 and cnt.value == n_ret, (cnt.value, n_ret)
    assert np.array_equal(buf[:n_ret].view(np.uint32), m0[r0].view(np.uint32)), "retired records differ"
    assert np.array_equal(sm.download_model().view(np.uint32), m0[~r0].view(np.uint32)), "kept model differs"
    e2e, host_steps, dev_steps, base, base_parts = [], [], [], [], []
    for k in range(WARM + REPS):
        reset()
        t0 = time.perf_counter()
        rc = host()
        dt = time.perf_counter() - t0
        assert rc == 0 and cnt.value == n_ret
        if k >= WARM:
            e2e.append(dt * 1e3)
            host_steps.append(sm.retire_stats())
    for k in range(WARM + REPS):
        reset()
        rc = device()
        assert rc == 0 and cnt.value == n_ret
        if k >= WARM:
            dev_steps.append(sm.retire_stats())
    for k in range(WARM + REPS):
        reset()
        t0 = time.perf_counter()
        m = sm.download_model()
        t1 = time.perf_counter()
        r = mask(m, TICK, MIN_AGE)
        kept = m[~r]
        gone = m[r]
        t2 = time.perf_counter()
        sm.upload_model(kept)
        t3 = time.perf_counter()
        assert len(gone) == n_ret
        if k >= WARM:
            base.append((t3 - t0) * 1e3)
            base_parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        del m, kept, gone
    sm.device_free(d_buf)
    steps = {k: med([s[k] for s in dev_steps]) for k in dev_steps[0]}
    mark_bytes = n * 20 + n // 8                    # 16 B pos_conf + 4 B time + 1 bit alive per live slot
    gather_bytes = n_ret * (24 + 48)                # the other planes in, the record out (it re-reads the 20 B the mark read)
    return dict(
        n=n, retired=n_ret, sm_retire_ms=med(e2e), sm_retire_ms_all=e2e,
        host_gather_with_copies_ms=med([s["gather"] for s in host_steps]),
        device_steps_ms=steps, device_total_ms=sum(steps.values()),
        baseline_ms=med(base), baseline_ms_all=base,
        baseline_parts_ms=dict(zip(("download_model", "numpy_mask_and_split", "upload_model"),
                                   [med([b[i] for b in base_parts]) for i in range(3)])),
        speedup=med(base) / med(e2e),
        mark_algorithmic_bytes=mark_bytes, mark_bytes_per_s=mark_bytes / (steps["mark"] * 1e-3),
        mark_share_of_hbm_roof=mark_bytes / (steps["mark"] * 1e-3) / HBM_ROOF,
        gather_algorithmic_bytes=gather_bytes, gather_bytes_per_s=gather_bytes / (steps["gather"] * 1e-3),
        gather_share_of_hbm_roof=gather_bytes / (steps["gather"] * 1e-3) / HBM_ROOF,
        pcie_bytes_sm_retire=n_ret * 48, pcie_bytes_baseline=n * 48 + (n - n_ret) * 48)


FRAMES_WARM = 5


def render_frames(n_frames, workers):
    """(before the process holds a GPU context: the renderers are forked)"""
    import bench
    return bench.make_frames(synth.KITTI, FRAMES_WARM + n_frames, 1, 15.0, workers)


def probe_frames(frames, n_frames):
    import bench
    cam = synth.KITTI
    warm = FRAMES_WARM
    os.environ["SM_RETIRE_TIMING"] = "0"            # no events around the policy's retirements
    tmp = tempfile.mkdtemp(prefix="retire_probe_")
    out = {}

    def run(name, every, **params):
        sm = capi.SurfelMap(capi.make_config(**cam))
        dp = bench.stage_frames(sm, frames, cam["width"] * cam["height"])
        if every:
            sm.set_auto_retire(every, os.path.join(tmp, name), **params)
        for k in range(warm):
            sm.process_frame_device(*dp[k])
        sm.sync()
        t0 = time.perf_counter()
        for k in range(warm, warm + n_frames):
            sm.process_frame_device(*dp[k])
        sm.sync()
        dt = time.perf_counter() - t0
        files, surfels = sm.auto_retire_stats()
        out[name] = dict(frames_per_s=n_frames / dt, us_per_frame=dt / n_frames * 1e6, files=files, surfels_retired=surfels,
                         surfels_end=sm.counts()["count"])
        sm.close()

    run("warm_up_run", 0)
    for i in range(3):                              # alternating, so that a drift of the machine shows in both
        run(f"off_{i}", 0)
        run(f"every_1000_{i}", 1000, min_age=20)
    run("every_50", 50, min_age=20)
    del out["warm_up_run"]
    off = [out[f"off_{i}"]["frames_per_s"] for i in range(3)]
    on = [out[f"every_1000_{i}"]["frames_per_s"] for i in range(3)]
    out["off_spread"] = dict(min=min(off), max=max(off), median=med(off))
    out["every_1000_spread"] = dict(min=min(on), max=max(on), median=med(on))
    out["every_1000_within_off_spread"] = bool(min(off) <= med(on) <= max(off))
    out["what"] = (f"{n_frames} KITTI-shaped frames after {warm}, sm_process_frame_device, frames staged in HBM, one wait at the end; "
                   "every_*: min_age = 20, min_distance = 1.5 * far_clip")
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,8000000,20000000")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retire_probe.json"))
    a = ap.parse_args()
    res = dict(what=__doc__.split("\n\n")[0], hbm_roof_bytes_per_s=HBM_ROOF, warm_ups=WARM, repeats=REPS, sizes=[], frames=None)
    sizes = [int(x) for x in a.sizes.split(",") if x]
    frames = render_frames(a.frames, a.workers) if a.frames else None
    if sizes:
        sm = capi.SurfelMap(capi.make_config(**synth.HD))
        for n in sizes:
            res["sizes"].append(probe_size(sm, n))
            s = res["sizes"][-1]
            print(f"n {n}: sm_retire {s['sm_retire_ms']:.2f} ms, download+mask+upload {s['baseline_ms']:.2f} ms "
                  f"({s['speedup']:.1f}x), device steps {s['device_steps_ms']}", flush=True)
            assert s["sm_retire_ms"] < s["baseline_ms"], "sm_retire is slower than the route through the host"
        sm.close()
    if a.frames:
        res["frames"] = probe_frames(frames, a.frames)
        print({k: (round(v["frames_per_s"]) if isinstance(v, dict) and "frames_per_s" in v else v) for k, v in res["frames"].items()},
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
