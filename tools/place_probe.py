#!/usr/bin/env python3
"""What place recognition costs, on one GPU, in one process; every figure the median of 5 after 2 warm-ups.

  encode   k_fern_encode between two events (SM_PLACE_TIMING=1) at 1242 x 375 and 1920 x 1080, 512 and 2048 ferns of cell 8, next
           to the bytes it reads (5 B x cell^2 x n_ferns), and the whole sm_fern_encode call (upload included) on the host clock.
  match    k_fern_match between two events at 1 k, 100 k and 2^20 keyframes of 512 ferns (256 B each), and the whole
           sm_fern_match call on the host clock.
  policy   the scene of tools/auto_loop_probe.py's attempt (KITTI camera, 10 frames of old world paged back in, 6 young frames):
           sm_track_frame_rgb of the next frame on the host clock with the policy off and with it on over 10 k keyframes none of
           which matches (no attempt, no keyframe added), the same context, the same model; the difference is what the policy adds
           per tracked frame, and the two kernels' device times say how much of it is the device's.

Writes one text file (--out)."""
import argparse
import os
import sys
import tempfile
import time

os.environ.setdefault("SM_PLACE_TIMING", "1")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from surfelmapping_amd import capi, synth  # noqa: E402

WARM, REPS = 2, 5
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    return float(np.median(xs))


def keyframe_file(path, p, w, h, n, seed=0):
    """a keyframe file of n random codes (the layout of include/sm_c_api.h), written in pieces"""
    rng = np.random.default_rng(seed)
    words = p.n_ferns // 8
    rec = np.dtype([("time", "<i4"), ("pose", "<f4", 16), ("code", "<u4", words)])
    with open(path, "wb") as f:
        f.write(np.array([0x4E524653, 1], "<u4").tobytes() + np.array([p.n_ferns, p.cell], "<i4").tobytes() + np.array([p.seed], "<u8").tobytes()
                + np.array([p.depth_lo_mm, p.depth_hi_mm, w, h], "<i4").tobytes() + np.array([n, 0], "<u4").tobytes())
        for first in range(0, n, 1 << 16):
            m = min(1 << 16, n - first)
            blk = np.zeros(m, rec)
            blk["time"] = np.arange(first, first + m)
            blk["pose"][:, [0, 5, 10, 15]] = 1.0
            blk["code"] = rng.integers(0, 2 ** 32, (m, words), dtype=np.uint64).astype(np.uint32)
            f.write(blk.tobytes())


def probe_encode():
    for cam in (synth.KITTI, synth.HD):
        w, h = cam["width"], cam["height"]
        sm = capi.SurfelMap(capi.make_config(**cam, max_sqrt_vertices=64))
        rng = np.random.default_rng(1)
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        depth = rng.integers(0, 30000, (h, w)).astype(np.uint16)
        for n in (512, 2048):
            sm.set_ferns(n_ferns=n)
            dev, call = [], []
            for rep in range(WARM + REPS):
                t = time.perf_counter()
                sm.fern_encode(depth, rgb)
                dt = (time.perf_counter() - t) * 1e3
                if rep >= WARM:
                    dev.append(sm.place_ms()[0])
                    call.append(dt)
            kb = 5 * 64 * n / 1e3
            # (no rate beside it: at these sizes the interval between two events is the floor of any small launch, not a transfer time)
            say(f"  {w} x {h}, {n} ferns: k_fern_encode {med(dev) * 1e3:.1f} us for {kb:.0f} KB of {w * h * 5 / 1e6:.1f} MB; "
                f"the call with its upload {med(call):.3f} ms")
        sm.close()


def probe_match(tmp):
    cam = synth.KITTI
    sm = capi.SurfelMap(capi.make_config(**cam, max_sqrt_vertices=64))
    sm.set_ferns()
    rng = np.random.default_rng(2)
    query = rng.integers(0, 2 ** 32, 64, dtype=np.uint64).astype(np.uint32)
    for n in (1000, 100000, 1 << 20):
        path = os.path.join(tmp, "kf.fern")
        keyframe_file(path, sm._fern, cam["width"], cam["height"], n)
        sm.fern_load(path)
        os.remove(path)
        dev, call, got = [], [], None
        for rep in range(WARM + REPS):
            t = time.perf_counter()
            got = sm.fern_match(query)
            dt = (time.perf_counter() - t) * 1e3
            if rep >= WARM:
                dev.append(sm.place_ms()[1])
                call.append(dt)
        mb = n * 260 / 1e6
        say(f"  {n} keyframes of 256 B (+ 4 B of time): k_fern_match {med(dev) * 1e3:.1f} us for {mb:.2f} MB ({mb * 1e6 / (med(dev) * 1e-3) / 1e9:.0f} GB/s); "
            f"the call {med(call):.3f} ms; best {got}")
    sm.close()


def write_map(path, rows, a, b):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes())
        f.write(np.array([a, b], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, np.float32).tobytes())


def probe_policy(tmp):
    cam = dict(synth.KITTI)
    poses = synth.kitti_trajectory(11)
    (seq,) = synth.make_sequences_parallel([(cam, poses, 0, 0.0, dict(seed=0, n_boxes=40))], workers=11)
    old = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    for fr in seq[:10]:
        old.process_frame(*fr)
    rows = old.download_model()
    old.close()
    f_path = os.path.join(tmp, "F.bin")
    write_map(f_path, rows, 0, 9)
    g = capi.SurfelMap(capi.make_config(**cam, preprocess=0))
    g.set_tick(400)
    for fr in seq[4:10]:
        g.process_frame(*fr)
    g.recall([f_path], pose=seq[9][3], mode="copy", radius=500.0)
    g.set_ferns()
    kf = os.path.join(tmp, "kf.fern")
    keyframe_file(kf, g._fern, cam["width"], cam["height"], 10000)
    g.fern_load(kf)
    rgb, depth, guess = seq[10][0], seq[10][1], poses[10].astype(np.float32)
    res = {}
    for name in ("off", "on", "off again"):
        # add_above 1: no frame is unlike enough to become a keyframe, so every repetition sees the same 10 k
        g.set_auto_place(name == "on", **(dict(add_above=1.0) if name == "on" else {}))
        ts, dev = [], []
        for rep in range(WARM + REPS):
            t = time.perf_counter()
            _, info = g.track_rgb(rgb, depth, guess=guess, dist_thresh=0.5)
            dt = (time.perf_counter() - t) * 1e3
            if rep >= WARM:
                ts.append(dt)
                dev.append(g.place_ms())
        res[name] = med(ts)
        extra = ""
        if name == "on":
            st = g.auto_place_stats()
            extra = (f"; k_fern_encode {med([d[0] for d in dev]) * 1e3:.1f} us, k_fern_match {med([d[1] for d in dev]) * 1e3:.1f} us; "
                     f"{st['encoded']} encoded, {st['matched']} matched, {st['attempts']} attempts, {st['added']} added, best old keyframe at {st['last_dis']} ferns")
        say(f"  kitti, {g.counts()['count']} surfels, 10000 keyframes, policy {name}: sm_track_frame_rgb {res[name]:.3f} ms ({info['status']}){extra}")
    say(f"  the policy adds {(res['on'] - 0.5 * (res['off'] + res['off again'])) * 1e3:.0f} us per tracked frame")
    g.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_probe.txt"))
    a = ap.parse_args()
    say(__doc__.split("\n\n")[0])
    with tempfile.TemporaryDirectory(prefix="place_probe_") as tmp:
        probe_encode()
        probe_match(tmp)
        probe_policy(tmp)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", a.out)
