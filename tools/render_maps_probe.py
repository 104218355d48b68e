#!/usr/bin/env python3
"""What a view of a map set costs, on one GPU, in one process; every figure the median of 3 after 1 warm-up.

  routes  a map that fits, synth.seeded_model(n) as ONE file, V views: the route there was before -- load_map + V x render_image
          / render_model -- against one render_image_maps / render_model_maps call on the same file and views, images asserted
          equal.  --route resident runs the first route alone: it uses nothing this feature added, so the same script times it
          on the commit before (--pkg <checkout>), which is where the "resident" rows of profiles/render_maps_mi355x.txt come from.
  overlap the streamed call's split of the stats: total against max(read, copy, device) and against their sum (every row of
          `routes` carries it; a map of 8 M surfels is 8 chunks).
  splat   device time of the batched splat against the resident splat on the same surfels and views.  Run this step alone
          under the kernel profiler, then let the tool read the profiler's table:
              rocprofv3 --kernel-trace --stats -d DIR/resident -- python tools/render_maps_probe.py --only splat --splat-route resident
              (the same with nocull and cull in place of resident)
              python tools/render_maps_probe.py --kernel-stats DIR
          Both routes draw the same n surfels into the same V views the same number of times, so the ratio of the kernels' total
          times is the ratio per (surfel, view).  The streamed calls run with the box test off, then on.
  cull    a drive (retire_ref.sequence with periodic retirement): the share of (block, view) pairs skipped, the time with and
          without the box test.
File reads come from the page cache (the files are written just before they are read).  Writes one JSON file (--out)."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, REPS = 1, 3


def med(xs):
    return float(np.median(xs))


def timed(fn):
    out, ts = None, []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        out = fn()
        if k >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return out, med(ts)


def write_map(path, rows):
    with open(path, "wb") as f:
        f.write(np.array([len(rows)], np.uint32).tobytes() + np.array([0, 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, np.float32).tobytes())


def image_poses(synth, V):
    """V cameras through the seeded volume (x -60..60, z -50..250), every fourth looking back"""
    ps = []
    for k in range(V):
        z = -40.0 + 280.0 * k / max(V, 2)
        ps.append(synth.pose_to_colmajor(synth.pose_matrix(10.0 * np.sin(k), 0.0, z, (180.0 if k % 4 == 3 else 0.0) + 5.0 * np.cos(k))))
    return np.stack(ps)


def model_cams(ref, V, w, h):
    P = ref.projection(w, h, 420.0 * w / 640, 420.0 * h / 480, 320.0 * w / 640, 240.0 * h / 480, 0.1, 1000.0)
    out = []
    for k in range(V):
        z = -60.0 + 280.0 * k / max(V, 2)
        out.append(ref.view_mats(P, ref.look_at(0, -12, z, 0, 0, z + 30.0, 0, -1, 0)))
    return out


def probe_routes(capi, synth, ref, args, tmp):
    rows = []
    for n in args.sizes:
        model = synth.seeded_model(n, 50, seed=2)
        path = os.path.join(tmp, f"seeded_{n}.bin")
        write_map(path, model)
        side = int(np.ceil(np.sqrt(n))) + 1
        for (w, h) in args.res:
            cam = dict(width=w, height=h, fx=0.58 * w, fy=0.58 * w, cx=w / 2 - 0.5, cy=h / 2 - 0.5)
            sm = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=side))
            small = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=10)) if args.route != "resident" else None
            for V in args.views:
                poses = image_poses(synth, V)
                cams = model_cams(ref, V, w, h)
                kw = dict(threshold=0.5, unstable=True, color_type=2)
                row = dict(n=n, w=w, h=h, V=V)

                def res_image():
                    sm.load_map(path)
                    return [sm.render_image(p, w, h, cam["fx"], cam["fy"], cam["cx"], cam["cy"]) for p in poses]

                def res_model():
                    sm.load_map(path)
                    return [sm.render_model(mvp, inv, w, h, **kw) for mvp, inv in cams]

                ri = rm = None
                if args.route != "streamed":
                    ri, row["resident_image_ms"] = timed(res_image)
                    rm, row["resident_model_ms"] = timed(res_model)
                if args.route != "resident":
                    si, row["streamed_image_ms"] = timed(lambda: small.render_image_maps([path], poses, w, h, cam["fx"], cam["fy"], cam["cx"], cam["cy"], include_model=False))
                    row["streamed_image_stats"] = small.render_maps_stats()
                    row["streamed_image_overlap"] = overlap(row["streamed_image_stats"])
                    mv = [capi.model_view(mvp, inv, w, h, **kw) for mvp, inv in cams]
                    smo, row["streamed_model_ms"] = timed(lambda: small.render_model_maps([path], mv, include_model=False))
                    row["streamed_model_stats"] = small.render_maps_stats()
                    row["streamed_model_overlap"] = overlap(row["streamed_model_stats"])
                    os.environ["SM_RENDER_MAPS_NO_CULL"] = "1"
                    _, row["streamed_model_nocull_ms"] = timed(lambda: small.render_model_maps([path], mv, include_model=False))
                    row["streamed_model_nocull_stats"] = small.render_maps_stats()
                    del os.environ["SM_RENDER_MAPS_NO_CULL"]
                    if ri is not None:
                        for k in range(V):
                            assert np.array_equal(si[0][k], ri[k][0]) and np.array_equal(si[1][k], ri[k][1]), ("novel view differs", n, w, h, k)
                            assert np.array_equal(smo[k], rm[k]), ("model view differs", n, w, h, k)
                        row["images_equal"] = True
                    del si, smo
                del ri, rm
                print(json.dumps(row), flush=True)
                rows.append(row)
            sm.close()
            if small is not None:
                small.close()
        os.remove(path)
    return rows


def overlap(st):
    parts = (st["read_ms"], st["copy_ms"], st["device_ms"])
    return dict(total_ms=st["total_ms"], max_ms=max(parts), sum_ms=sum(parts), total_over_max=st["total_ms"] / max(max(parts), 1e-9),
                total_over_sum=st["total_ms"] / max(sum(parts), 1e-9))


SPLAT_N, SPLAT_V, SPLAT_RES, SPLAT_REPS = 8_000_000, 16, (1242, 375), 3


def probe_splat(capi, synth, ref, tmp, which):
    """the kernels to compare, SPLAT_REPS times each, nothing else timed here: the profiler does that.  `which`: resident
    (k_render_splat; k_view_splat + k_view_overflow), nocull / cull (k_maps_splat_image; k_maps_splat_view)."""
    n, V, (w, h) = SPLAT_N, SPLAT_V, SPLAT_RES
    path = os.path.join(tmp, "splat.bin")
    write_map(path, synth.seeded_model(n, 50, seed=2))
    cam = dict(width=w, height=h, fx=0.58 * w, fy=0.58 * w, cx=w / 2 - 0.5, cy=h / 2 - 0.5)
    poses, cams, kw = image_poses(synth, V), model_cams(ref, V, w, h), dict(threshold=0.5, unstable=True, color_type=2)
    if which == "resident":
        sm = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=int(np.ceil(np.sqrt(n))) + 1))
        sm.load_map(path)
        for _ in range(SPLAT_REPS):
            for p in poses:
                sm.render_image(p, w, h, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
            for mvp, inv in cams:
                sm.render_model(mvp, inv, w, h, **kw)
    else:
        if which == "nocull":
            os.environ["SM_RENDER_MAPS_NO_CULL"] = "1"
        sm = capi.SurfelMap(capi.make_config(**cam, preprocess=0, max_sqrt_vertices=10))
        mv = [capi.model_view(mvp, inv, w, h, **kw) for mvp, inv in cams]
        for _ in range(SPLAT_REPS):
            sm.render_image_maps([path], poses, w, h, cam["fx"], cam["fy"], cam["cx"], cam["cy"], include_model=False)
            sm.render_model_maps([path], mv, include_model=False)
    sm.close()
    os.remove(path)


def kernel_stats(root):
    """{which: {kernel: (calls, total ms)}} from the profiler's *kernel_stats.csv files under root/<which>/"""
    import csv
    import glob
    out = {}
    for which in ("resident", "nocull", "cull"):
        tab = {}
        for f in glob.glob(os.path.join(root, which, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                name = r["Name"].split("(")[0].split("::")[-1].replace(".kd", "")
                calls, ns = tab.get(name, (0, 0.0))
                tab[name] = (calls + int(r["Calls"]), ns + float(r["TotalDurationNs"]))
        out[which] = {k: (c, ns / 1e6) for k, (c, ns) in tab.items() if k.startswith(("k_render_", "k_view_", "k_maps_"))}
    ms = lambda which, *names: sum(out[which].get(k, (0, 0.0))[1] for k in names)
    pairs = SPLAT_N * SPLAT_V * SPLAT_REPS
    res_i, res_v = ms("resident", "k_render_splat"), ms("resident", "k_view_splat", "k_view_overflow")
    for which in ("nocull", "cull"):
        si, sv = ms(which, "k_maps_splat_image"), ms(which, "k_maps_splat_view")
        out[which + "_summary"] = dict(
            novel_ps_per_pair=dict(resident=res_i * 1e9 / pairs, streamed=si * 1e9 / pairs), novel_ratio=si / max(res_i, 1e-9),
            model_ps_per_pair=dict(resident=res_v * 1e9 / pairs, streamed=sv * 1e9 / pairs), model_ratio=sv / max(res_v, 1e-9),
            intake_ms=ms(which, "k_maps_intake"), resolve_ms=ms(which, "k_maps_resolve_image", "k_maps_resolve_view"))
    return out


def probe_cull(capi, args, tmp):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import retire_ref as rr
    import model_view_ref as ref
    g = capi.SurfelMap(capi.make_config(**rr.CAM, **rr.OVER, preprocess=0, max_sqrt_vertices=rr.CAPACITY[0]))
    g.set_auto_retire(rr.EVERY, os.path.join(tmp, "d"), min_age=rr.MIN_AGE, min_distance=rr.MIN_DISTANCE)
    seq = rr.sequence(rr.N_FRAMES)
    for fr in seq:
        g.process_frame(*fr)
    nfiles, nsurf = g.auto_retire_stats()
    paths = [os.path.join(tmp, f"d_{i:06d}.bin") for i in range(nfiles)]
    views = np.stack([fr[3] for fr in seq[::9]])
    c = rr.CAM
    out = dict(files=nfiles, surfels_in_files=nsurf, live=g.counts()["count"], views=len(views))
    for name, env in (("cull", None), ("nocull", "1")):
        if env:
            os.environ["SM_RENDER_MAPS_NO_CULL"] = env
        res, ms = timed(lambda: g.render_image_maps(paths, views, c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"]))
        out[name] = dict(ms=ms, stats=g.render_maps_stats())
        os.environ.pop("SM_RENDER_MAPS_NO_CULL", None)
        if name == "cull":
            keep = res
        else:
            assert np.array_equal(keep[0], res[0]) and np.array_equal(keep[1], res[1])
    st = out["cull"]["stats"]
    out["skipped_share"] = st["pairs_skipped"] / max(st["pairs_tested"], 1)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=ROOT, help="checkout whose surfelmapping_amd package is measured")
    ap.add_argument("--route", choices=("both", "resident", "streamed"), default="both")
    ap.add_argument("--sizes", type=int, nargs="*", default=[8_000_000, 20_000_000])
    ap.add_argument("--views", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--res", type=lambda s: tuple(int(x) for x in s.split("x")), nargs="*", default=[(1242, 375), (1920, 1080)])
    ap.add_argument("--no-cull-probe", action="store_true")
    ap.add_argument("--only", choices=("splat",), help="run one step alone (splat: under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--splat-route", choices=("resident", "nocull", "cull"), default="resident")
    ap.add_argument("--kernel-stats", metavar="DIR", help="read the profiler's tables of the splat step (DIR/resident, DIR/nocull, DIR/cull) and print the ratios")
    ap.add_argument("--out", default="render_maps_probe.json")
    args = ap.parse_args()
    if args.kernel_stats:
        print(json.dumps(kernel_stats(args.kernel_stats), indent=1))
        return
    sys.path.insert(0, args.pkg)
    capi = importlib.import_module("surfelmapping_amd.capi")
    synth = importlib.import_module("surfelmapping_amd.synth")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import model_view_ref as ref
    result = dict(pkg=os.path.abspath(args.pkg), route=args.route, warm=WARM, reps=REPS)
    if args.only == "splat":
        with tempfile.TemporaryDirectory() as tmp:
            probe_splat(capi, synth, ref, tmp, args.splat_route)
        return
    with tempfile.TemporaryDirectory() as tmp:
        result["routes"] = probe_routes(capi, synth, ref, args, tmp)
        if args.route != "resident" and not args.no_cull_probe:
            result["cull"] = probe_cull(capi, args, tmp)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
