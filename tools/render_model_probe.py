#!/usr/bin/env python3
"""render_model_probe.py -- cost of the model view (sm_render_model, GlobalModel::renderModel) on the MI355X.

Two maps at a 1920x1080 viewport: the steady_leg-style KITTI map (bench.py's 1242x375 stream, --frames frames fused by the core)
and synth.seeded_model(20 M) (BASELINE configs[2]).  The camera is the GUI's (gui/GUI.cpp:46-47: ProjectionMatrix(640, 480,
420, 420, 320, 240, 0.1, 1000) restated at the viewport's size, ModelViewLookAt behind and above the trajectory).  Per mode
(shaded, colour, semantic, points, window): ms per view over --reps renders after warm-up (wall clock per call of
sm_render_model_device, which waits for frames in flight and returns once the launches are queued; the stream is drained
at the end), the kernel split from device events (SM_RENDER_MODEL_TIMING=1), the bytes moved (32 B per live surfel +
20 B per pixel: key fill 8, resolve read 8 and write 4) and the splat's fraction of 8 TB/s, and the overflow list's length.
Then the sweep of the lane/overflow footprint threshold (SM_RENDER_MODEL_LANE_PX) on the shaded view, and the facade's
current renderModel host path (a download of the whole model and a host-side gate) on the same map.

    python tools/render_model_probe.py [--maps kitti,seeded] [--reps 50] [--png DIR]
"""
from __future__ import annotations

import argparse
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import model_view_ref as ref  # noqa: E402  (pangolin's camera matrices)
from surfelmapping_amd import capi, synth  # noqa: E402

HBM = 8.0e12
MODES = {"shaded": dict(color_type=0), "colour": dict(color_type=2), "semantic": dict(color_type=3),
         "points": dict(color_type=2, points=True), "window": dict(color_type=0, window=True)}


def write_png(path, rgba):
    """RGBA8 PNG; rows flipped from GL order (row 0 = bottom) to the image's top-down order"""
    img = np.ascontiguousarray(rgba[::-1])
    h, w = img.shape[:2]
    raw = b"".join(b"\x00" + img[j].tobytes() for j in range(h))

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def camera(w, h, eye, target):
    P = ref.projection(w, h, 420.0 * w / 640, 420.0 * h / 480, 320.0 * w / 640, 240.0 * h / 480, 0.1, 1000.0)
    return ref.view_mats(P, ref.look_at(*eye, *target, 0, -1, 0))


def kitti_map(n_frames, workers):
    import bench
    cam = synth.KITTI
    frames = bench.make_frames(cam, n_frames, 0, 0.0, workers)
    m = capi.SurfelMap(capi.make_config(**cam, preprocess=0, conflict_cap=1, max_sqrt_vertices=5000))
    for fr in frames:
        m.process_frame(*fr)
    m.sync()
    return m, n_frames


def seeded_map(n):
    m = capi.SurfelMap(capi.make_config(**synth.HD, preprocess=0, conflict_cap=0, max_sqrt_vertices=10000))
    m.upload_model(synth.seeded_model(n, tick=300))
    m.set_tick(300)
    return m, 300


def time_view(m, mvp, inv, w, h, d_rgba, reps, warm, **kw):
    for _ in range(warm):
        m.render_model_device(mvp, inv, w, h, d_rgba, **kw)
    m.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        m.render_model_device(mvp, inv, w, h, d_rgba, **kw)
    m.sync()
    wall = (time.perf_counter() - t0) * 1e3 / reps
    os.environ["SM_RENDER_MODEL_TIMING"] = "1"
    split = np.zeros(3)
    for _ in range(reps):
        m.render_model_device(mvp, inv, w, h, d_rgba, **kw)
        split += np.array(m.render_model_stats()[1])
    os.environ.pop("SM_RENDER_MODEL_TIMING")
    n_ovf, _ = m.render_model_stats()
    return wall, split / reps, n_ovf


def probe(name, m, tick, eye, target, args):
    w, h = args.width, args.height
    n = m.counts()["count"]
    mvp, inv = camera(w, h, eye, target)
    d_rgba = m.device_alloc(w * h * 4)
    print(f"== {name}: {n} live surfels, {w}x{h}, eye {eye} -> {target}, {args.reps} renders after {args.warmup}")
    print(f"{'mode':9s} {'ms/view':>8s} {'splat':>7s} {'ovf':>7s} {'resolve':>7s} {'ovf_n':>8s} {'MB':>7s} {'all%8TB':>7s} "
          f"{'splat%8TB':>9s} {'covered':>7s}")
    for mode, kw in MODES.items():
        kw = dict(kw, threshold=0.0, unstable=True, time=tick, time_delta=100)
        wall, split, n_ovf = time_view(m, mvp, inv, w, h, d_rgba, args.reps, args.warmup, **kw)
        nbytes = 32.0 * n + 20.0 * w * h
        rgba = m.render_model(mvp, inv, w, h, **kw)
        cov = float((rgba[..., 3] == 255).mean())
        print(f"{mode:9s} {wall:8.3f} {split[0]:7.3f} {split[1]:7.3f} {split[2]:7.3f} {n_ovf:8d} {nbytes / 1e6:7.1f} "
              f"{100 * nbytes / (split.sum() * 1e-3) / HBM:6.1f}% {100 * 32.0 * n / (split[0] * 1e-3) / HBM:8.1f}% {cov:7.3f}")
        if args.png:
            os.makedirs(args.png, exist_ok=True)
            write_png(os.path.join(args.png, f"render_model_{name}_{mode}.png"), rgba)
    print(f"-- lane/overflow footprint threshold sweep (shaded; SM_RENDER_MODEL_LANE_PX, default 64)")
    print(f"{'lane_px':>8s} {'ms/view':>8s} {'splat':>7s} {'ovf':>7s} {'resolve':>7s} {'ovf_n':>8s}")
    for t in (0, 16, 32, 64, 128, 256, 1024, 1 << 24):
        os.environ["SM_RENDER_MODEL_LANE_PX"] = str(t)
        wall, split, n_ovf = time_view(m, mvp, inv, w, h, d_rgba, max(10, args.reps // 2), 3, threshold=0.0, unstable=True)
        print(f"{t:8d} {wall:8.3f} {split[0]:7.3f} {split[1]:7.3f} {split[2]:7.3f} {n_ovf:8d}")
    os.environ.pop("SM_RENDER_MODEL_LANE_PX")
    # the facade's renderModel today (GlobalModel.h): downloadModel() -> host AoS copy, then the confidence gate on the host
    reps = 3
    t0 = time.perf_counter()
    for _ in range(reps):
        a = m.download_model()
        drawn = a[a[:, 3] >= 0.0, :3]
    host_ms = (time.perf_counter() - t0) * 1e3 / reps
    print(f"-- facade renderModel host path (download {a.nbytes / 1e6:.0f} MB + host gate, {drawn.shape[0]} points): {host_ms:.1f} ms "
          f"per call")
    m.device_free(d_rgba)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maps", default="kitti,seeded")
    ap.add_argument("--frames", type=int, default=110, help="KITTI frames fused (steady_leg: 10 + 100)")
    ap.add_argument("--seeded", type=int, default=20_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--png", default=None, help="directory for the images (PNG, top row first)")
    args = ap.parse_args()
    for name in args.maps.split(","):
        if name == "kitti":
            m, tick = kitti_map(args.frames, args.workers)
            probe("kitti", m, tick, (0.0, -12.0, -25.0), (0.0, 0.0, 40.0), args)
        elif name == "seeded":
            m, tick = seeded_map(args.seeded)
            probe("seeded20m", m, tick, (0.0, -20.0, -90.0), (0.0, 0.0, 100.0), args)
        else:
            raise SystemExit(f"unknown map {name}")
        m.close()


if __name__ == "__main__":
    main()
