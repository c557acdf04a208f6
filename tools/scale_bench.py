#!/usr/bin/env python3
"""Room-scale timing of the resident depth maps and of K39 against the route they replace.  The scans have the size of tools/depthfill_bench.py's (--frames scans of
--points points, half-size maps of a 5760 x 2880 panorama, size 4, max_depth 40), the pair list the size of tools/relpose_bench.py's (every frame with its next
--neighbours frames, 70 % of --matches points per pair, a share --large of the pairs with 70 % of --large-matches).  So that the scales mean something, all frames
see ONE static cloud from camera centres --step metres apart along a line, and a pair's triangulated points are a sample of its first frame's scan in the camera
frame divided by the pair's baseline: the maps then hold the depths the points need, up to what the splat's windows and the completion do to them.
  (a) the maps     --route host: ONE pvlm_compute_depth_images call (the maps come to the host); --route resident: ONE pvlm_depthset_compute call (they stay)
  (b) the scales   --route host: relpose_detail::SetScaleOne over the list on one thread (tests/cpp/scale_core_check.cpp: the host step, as upstream's loop effectively
                   is here); --route resident: ONE pvlm_set_translation_scales call
A process runs ONE route (PVLM_LIB may select the library of another commit for --route host): wall clock around each part, the median of --repeat runs after a
warm-up.  Reported: seconds of (a), (b) and a + b, pairs / s and points / s of (b), the shares of the three exits, the bytes of maps that cross the link, the peak
resident host memory of the process.  With --check the resident route also runs the host step and compares every output bit for bit.  One JSON line, appended to --out."""
import argparse
import ctypes as C
import json
import os
import resource
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("host", "resident"), required=True)
    ap.add_argument("--frames", type=int, default=454)
    ap.add_argument("--points", type=int, default=28800)
    ap.add_argument("--rows", type=int, default=2880)
    ap.add_argument("--cols", type=int, default=5760)
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--large", type=float, default=0.01)
    ap.add_argument("--large-matches", type=int, default=1500)
    ap.add_argument("--step", type=float, default=0.01)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k39_scale_bench.jsonl"))
    args = ap.parse_args()
    import panovlm_amd as pv
    from panovlm_amd import api
    from tests import depthfill_ref as ref
    from tests import scale_ref as sr
    F = args.frames
    rows, cols = (args.rows + 1) // 2, (args.cols + 1) // 2
    rng = np.random.default_rng(1)
    world = ref.synthetic_cloud(args.points, 100, radius=(0.8, 30.0)).astype(np.float64)
    T = ref.T_CL.reshape(4, 4)
    axis = np.array([1.0, 0.0, 0.0])                                             # the camera centres move along the LiDAR's x
    clouds = [(world - args.step * f * axis).astype(np.float32) for f in range(F)]
    first = np.zeros(F + 1, np.int64); first[1:] = np.cumsum([len(c) for c in clouds])
    xyz = np.ascontiguousarray(np.concatenate(clouds))
    src, tgt, off, Rs, ts, tri = [], [], [0], [], [], []
    for i in range(F):
        cam = clouds[i].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        for j in range(i + 1, min(i + 1 + args.neighbours, F)):
            n = int(0.7 * (args.large_matches if rng.random() < args.large else args.matches))
            t_ij = T[:3, :3] @ (-args.step * (j - i) * axis)                     # p_j = p_i + t_ij
            s = np.linalg.norm(t_ij)
            pick = rng.integers(0, len(cam), n)
            src.append(i); tgt.append(j); Rs.append(np.eye(3)); ts.append(t_ij / s); tri.append(cam[pick] / s); off.append(off[-1] + n)
    src = np.array(src, np.int32); tgt = np.array(tgt, np.int32); off = np.array(off, np.int64)
    Rs = np.array(Rs); ts = np.array(ts); tri = np.concatenate(tri)
    P = len(src)
    frame_rows = np.full(F, args.rows, np.int32)
    ctx = pv.Context(0)
    line = dict(route=args.route, label=args.label, lib=os.path.basename(api.lib_path()), frames=F, points_per_scan=args.points, map_rows=rows, map_cols=cols, pairs=P,
                points=int(off[-1]), points_per_pair_median=float(np.median(np.diff(off))), points_per_pair_max=int(np.diff(off).max()), map_bytes=int(F * rows * cols * 2))
    start = dict(points_with_depth=np.zeros(P, np.int32), upper_scale=np.full(P, -1.0), lower_scale=np.full(P, -1.0))

    def host_step(maps):
        chk = sr.build_check()
        ptrs = (C.c_void_p * F)(*[maps[f].ctypes.data for f in range(F)])
        mr = np.full(F, rows, np.int32); mc = np.full(F, cols, np.int32)
        t = ts.copy(); X = tri.copy(); ok = np.zeros(P, np.uint8); pwd = start["points_with_depth"].copy(); up = start["upper_scale"].copy(); lo = start["lower_scale"].copy()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        t0 = time.perf_counter()
        chk.chk_scale_list_host(C.c_int(args.rows), C.c_int(args.cols), p(frame_rows), ptrs, p(mr), p(mc), C.c_int(P), p(src), p(tgt), p(off), p(Rs), p(t), p(X), p(ok), p(pwd),
                                p(up), p(lo))
        return time.perf_counter() - t0, dict(t_21=t, triangulated=X, ok=ok, points_with_depth=pwd, upper_scale=up, lower_scale=lo)

    if args.route == "host":
        ctx.compute_depth_images_flat(rows, cols, first[:3], xyz, ref.T_CL, 4, 40.0)                 # warm-up: code object, pool
        a_times, maps, stats = [], None, None
        for _ in range(max(args.repeat, 1)):
            maps = None
            t0 = time.perf_counter(); maps, stats = ctx.compute_depth_images_flat(rows, cols, first, xyz, ref.T_CL, 4, 40.0); a_times.append(time.perf_counter() - t0)
        b_times, res = [], None
        for _ in range(max(args.repeat, 1)):
            dt, res = host_step(maps); b_times.append(dt)
        line.update(map_bytes_over_the_link=line["map_bytes"])
    else:
        api.DepthSet.compute_flat(ctx, rows, cols, first[:3], xyz, ref.T_CL, 4, 40.0).close()        # warm-up
        a_times, ds = [], None
        for _ in range(max(args.repeat, 1)):
            if ds is not None:
                ds.close()
            t0 = time.perf_counter(); ds = api.DepthSet.compute_flat(ctx, rows, cols, first, xyz, ref.T_CL, 4, 40.0); a_times.append(time.perf_counter() - t0)
        stats = ds.stats
        call = lambda: api.set_translation_scales(ctx, ds, args.rows, args.cols, frame_rows, src, tgt, off, Rs, ts, tri, **start)
        call()                                                                                       # warm-up on the timed list
        b_times, res = [], None
        for _ in range(max(args.repeat, 1)):
            t0 = time.perf_counter(); res = call(); b_times.append(time.perf_counter() - t0)
        line.update(map_bytes_over_the_link=0, scale_stats=res["stats"])
        if args.check:
            maps = np.stack([ds.read(f) for f in range(F)])
            _, h = host_step(maps)
            line["equals_host_step"] = bool(all(np.array_equal(np.ascontiguousarray(res[k]).view(np.uint8), np.ascontiguousarray(h[k]).view(np.uint8)) for k in h))
        ds.close()
    a_s, b_s = float(np.median(a_times)), float(np.median(b_times))
    ok = res["ok"].astype(bool); median = ok & (res["upper_scale"] == 0) & (res["lower_scale"] == 0)
    line.update(maps_s=a_s, maps_s_all=a_times, scales_s=b_s, scales_s_all=b_times, chain_s=a_s + b_s, scale_pairs_per_s=P / b_s, scale_points_per_s=int(off[-1]) / b_s,
                exit_share=dict(mean=float((ok & ~median).mean()), median=float(median.mean()), unscaled=float((~ok).mean())),
                device_splat_ms=stats["splat_ms"], device_fill_ms=stats["fill_ms"], batches=stats["batches"],
                peak_host_bytes=int(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss) * 1024)
    ctx.close()
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
