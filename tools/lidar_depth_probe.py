#!/usr/bin/env python3
"""What lidar depth costs, on one GPU, in one process; every figure the median of 20 calls after 3 warm-ups.

  The scan: the 100 frames of the synthetic drive fused at 1242 x 375, swept at the last pose by 64 x 1100 beams (sm_lidar_sweep),
  and turned back into points (capi.sweep_points); T is the identity.
  Two contexts take the same scan in turn, call by call: the default form (4 launches; DILATE, CLOSE and FILL_SMALL in one
  LDS-tiled launch, the column pass of FILL_LARGE, MEDIAN and SMOOTH in another) and the debug form with every step a launch of its
  own through planes in global memory (SM_LIDAR_DEPTH_UNFUSED=1, 12 launches).  Both must equal the numpy restatement.
  Per launch: the time between two events (SM_LIDAR_DEPTH_TIMING=1), the bytes it must move (computed from the sizes: what it has
  to read and write once, caches ignored) and the rate those give.
    project   reads the points (16 B each), one 8-byte atomic per point that lands
    chain     reads the keys (8 B / pixel); writes sparse_mm, index and the v plane (2 + 4 + 2 B / pixel)
    rowmax    reads the v plane, writes the row maxima (2 + 2 B / pixel)
    finish    reads the v plane and the row maxima, writes depth_mm, clears the keys (2 + 2 + 2 + 8 B / pixel)
  Then the stage's device time by events around all launches, sm_lidar_depth_device to its synchronise and sm_lidar_depth with its
  upload and read-back on the host clock, 50 calls of sm_lidar_depth_device enqueued back to back with one synchronise at the end
  (no tally asked for in between: the host must not wait between them), and sm_stereo_depth_device (D 128, 8 paths) on the same context for scale.  Last,
  the quality of the rules on the analytic street, by the restatement (no GPU in it).

Writes one text file (--out)."""
import argparse
import os
import sys
import time

os.environ["SM_LIDAR_DEPTH_TIMING"] = "1"
os.environ.setdefault("SM_STEREO_TIMING", "1")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lidar_depth_ref as lr  # noqa: E402
from surfelmapping_amd import capi, synth  # noqa: E402

WARM, REPS, BURST = 3, 20, 50
LINES = []
FUSED = ("k_ld_project", "k_ld_chain", "k_ld_rowmax", "k_ld_finish")
UNFUSED = ("k_ld_project", "keys to v", "DILATE", "CLOSE max", "CLOSE min", "FILL_SMALL", "EXTEND_TOP", "FILL_LARGE rows", "FILL_LARGE columns",
           "MEDIAN", "SMOOTH", "output")


def say(s):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    return float(np.median(xs))


def context(cam, unfused):
    os.environ["SM_LIDAR_DEPTH_UNFUSED"] = "1" if unfused else "0"
    sm = capi.SurfelMap(capi.make_config(**cam, max_sqrt_vertices=5000 if not unfused else 64))
    sm.set_lidar_depth()
    return sm


def main(frames, out):
    cam = synth.KITTI
    P = cam["width"] * cam["height"]
    seq = synth.make_sequence(cam, synth.kitti_trajectory(frames), seed=0)
    forms = {"fused": context(cam, False), "unfused": context(cam, True)}
    sm = forms["fused"]
    for fr in seq:
        sm.process_frame(*fr)
    sensor = capi.lidar_sensor(n_az=1100, az0_deg=-45.0, az_step_deg=90.0 / 1100, el_deg=np.linspace(-24.8, 2.0, 64))
    sweep = sm.lidar_sweep(seq[-1][3], sensor)
    pts = capi.sweep_points(sweep["range"], sensor)
    T = np.eye(4, dtype=np.float32)
    n = len(pts)
    want = lr.lidar_depth(pts, T, cam)
    st_ref = want["stats"]
    say(f"  {cam['width']} x {cam['height']}, {frames} frames fused, {sensor.n_el} x {sensor.n_az} beams: {n} returns, {st_ref['landed']} land, "
        f"{100.0 * st_ref['measured'] / P:.1f} % of the pixels measured, {100.0 * (1 - st_ref['left_empty'] / P):.1f} % filled "
        f"(FILL_SMALL {st_ref['filled_small']}, EXTEND_TOP {st_ref['filled_top']}, FILL_LARGE {st_ref['filled_large']})")
    d_pts, d_depth = sm.device_alloc(max(pts.nbytes, 16)), sm.device_alloc(P * 2)
    dev = {"fused": (d_pts, d_depth)}
    u = forms["unfused"]
    dev["unfused"] = (u.device_alloc(max(pts.nbytes, 16)), u.device_alloc(P * 2))
    for name, m in forms.items():
        m.device_upload(dev[name][0], pts)
    stats = {k: [] for k in forms}
    wall_dev = {k: [] for k in forms}
    wall_host = {k: [] for k in forms}
    for rep in range(WARM + REPS):
        for name, m in forms.items():                    # the two forms in turn, call by call
            t = time.perf_counter()
            got = m.lidar_depth(pts, T)
            dt_host = (time.perf_counter() - t) * 1e3
            st = m.lidar_depth_stats()
            if rep == 0:
                for key, g in zip(("depth_mm", "sparse_mm", "index"), got):
                    assert np.array_equal(g, want[key]), (name, key)
                assert all(st[k] == st_ref[k] for k in st_ref), (name, st, st_ref)
            m.sync()
            t = time.perf_counter()
            m.lidar_depth_device(dev[name][0], n, T, dev[name][1])
            m.sync()
            dt_dev = (time.perf_counter() - t) * 1e3
            if rep >= WARM:
                stats[name].append(st)
                wall_host[name].append(dt_host)
                wall_dev[name].append(dt_dev)
    say("  both forms equal the restatement: depth_mm, sparse_mm, index and the tally")
    burst, enq = {}, {}
    for name, m in forms.items():
        per, ret = [], []
        for rep in range(1 + 5):
            m.sync()
            t = time.perf_counter()
            for _ in range(BURST):
                m.lidar_depth_device(dev[name][0], n, T, dev[name][1])
            t_enq = time.perf_counter()
            m.sync()
            if rep:
                per.append((time.perf_counter() - t) * 1e3 / BURST)
                ret.append((t_enq - t) * 1e3 / BURST)
        burst[name], enq[name] = med(per), med(ret)
        got = m.device_download(dev[name][1], P * 2, np.uint16).reshape(want["depth_mm"].shape)
        assert np.array_equal(got, want["depth_mm"]), name
    nbytes = {"k_ld_project": n * 16 + st_ref["landed"] * 8, "k_ld_chain": P * 16, "k_ld_rowmax": P * 4, "k_ld_finish": P * 14}
    for name, labels in (("fused", FUSED), ("unfused", UNFUSED)):
        say(f"  {name}: {stats[name][0]['launches']} launches")
        total = 0.0
        for k, label in enumerate(labels):
            ms = med([s["launch_ms"][k] for s in stats[name]])
            total += ms
            if name == "fused":
                b = nbytes[label]
                say(f"    {label:<20} {ms * 1e3:8.1f} us  {b / 1e6:7.2f} MB  {b / (ms * 1e-3) / 1e9:7.0f} GB/s")
            else:
                say(f"    {label:<20} {ms * 1e3:8.1f} us")
        say(f"    launches summed {total * 1e3:.1f} us; device_ms (events around all of them) {med([s['device_ms'] for s in stats[name]]) * 1e3:.1f} us; "
            f"sm_lidar_depth_device to its synchronise {med(wall_dev[name]) * 1e3:.1f} us; sm_lidar_depth with upload and read-back {med(wall_host[name]) * 1e3:.1f} us")
        say(f"    {BURST} device calls back to back, one synchronise: {burst[name] * 1e3:.1f} us per call, of which the host spends {enq[name] * 1e3:.1f} us in the call")
    f_ms, u_ms = med([s["device_ms"] for s in stats["fused"]]), med([s["device_ms"] for s in stats["unfused"]])
    say(f"  fusing the chain: {u_ms * 1e3:.1f} us -> {f_ms * 1e3:.1f} us of device time ({u_ms / f_ms:.2f} x), "
        f"{med(wall_dev['unfused']) * 1e3:.1f} us -> {med(wall_dev['fused']) * 1e3:.1f} us to the synchronise")
    # for scale: the stereo stage on the same context
    left, right, _, _ = synth.stereo_pair(synth.Scene(0), synth.Camera(**cam), synth.pose_matrix(0.3, 0.0, 2.0, 3.0), 0.54)
    sm.set_stereo(max_disp=128, paths=8)
    d_l, d_r = sm.device_alloc(P * 3), sm.device_alloc(P * 3)
    sm.device_upload(d_l, left)
    sm.device_upload(d_r, right)
    ms = []
    for rep in range(WARM + 5):
        sm.stereo_depth_device(d_l, d_r, d_depth)
        m_ = sm.stereo_ms()
        if rep >= WARM:
            ms.append(m_["census"] + m_["cost"] + sum(m_["paths"]) + m_["select"])
    say(f"  for scale, sm_stereo_depth_device (D 128, 8 paths) on the same context: {med(ms):.3f} ms of kernels")
    q = lr.street_quality()
    say(f"  quality of the rules (the restatement on the CPU; the analytic street of tests/lidar_depth_ref.py, {q['points']} beams hit, {q['landed']} land): "
        f"{100.0 * q['measured']:.2f} % of the pixels measured, {100.0 * q['filled']:.1f} % filled, relative error median {q['median']:.5f}, "
        f"90th percentile {q['p90']:.4f}; tests/test_lidar_depth_ref.py bounds the median at twice that, {2 * round(q['median'], 5):.5f}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_depth_probe.txt"))
    ap.add_argument("--frames", type=int, default=100)
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    main(a.frames, a.out)
