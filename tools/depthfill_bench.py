#!/usr/bin/env python3
"""Room-scale timing of K37: ONE pvlm_compute_depth_images call on --frames synthetic VLP-16 scans (--points points each on 16 rings) into half-size depth maps of a
5760 x 2880 panorama (1440 x 2880), size 4, at Room's max_depth = 5 (near band only) and at max_depth = 40 (all three bands), against the host loop of the same core
(tests/cpp/depthfill_core_check.cpp, what ComputeDepthImageHost runs) on --threads threads over --host-frames of the same scans.  Reported per max_depth: ms per frame
of the call (wall clock, uploads of the points and downloads of the maps included; the median of --repeat calls after a warm-up), the HIP-event time of the splat and
of the three completion kernels from the call's statistics, the share of the splat, the host loop's ms per frame, and the bytes the completion kernels move per pixel
at the algorithmic minimum of the three-phase scheme (8 B splat word in + 4 B s4 out, 4 B in + 4 B out, 4 B in + 2 B out = 26 B) against the HBM peak.  No speed-up is
promised: the line records what was measured.  The host's maps must equal the call's on the frames both computed.  One JSON line, appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (roof, HBM_PEAK_GBPS)

ALGORITHMIC_BYTES_PER_PIXEL = 8 + 4 + 4 + 4 + 4 + 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=454)
    ap.add_argument("--points", type=int, default=28800)
    ap.add_argument("--rows", type=int, default=2880)
    ap.add_argument("--cols", type=int, default=5760)
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k37_depthfill_bench.jsonl"))
    args = ap.parse_args()
    import panovlm_amd as pv
    from tests import depthfill_ref as ref
    rows, cols = (args.rows + 1) // 2, (args.cols + 1) // 2
    clouds = [ref.synthetic_cloud(args.points, 100 + f, radius=(0.8, 30.0)) for f in range(args.frames)]
    first = np.zeros(args.frames + 1, np.int64); first[1:] = np.cumsum([len(c) for c in clouds])
    xyz = np.ascontiguousarray(np.concatenate(clouds))
    ctx = pv.Context(0)
    line = dict(frames=args.frames, points_per_scan=args.points, rows=rows, cols=cols, size=4, host_threads=args.threads, host_frames=args.host_frames,
                algorithmic_bytes_per_pixel=ALGORITHMIC_BYTES_PER_PIXEL)
    for max_depth in (5.0, 40.0):
        ctx.compute_depth_images_flat(rows, cols, first[:3], xyz, ref.T_CL, 4, max_depth)            # warm-up: code object, pool
        times, stats, maps = [], None, None
        for _ in range(max(args.repeat, 1)):
            t0 = time.perf_counter(); maps, stats = ctx.compute_depth_images_flat(rows, cols, first, xyz, ref.T_CL, 4, max_depth); times.append(time.perf_counter() - t0)
        gpu_s = float(np.median(times))
        nh = min(args.host_frames, args.frames)
        t0 = time.perf_counter(); rc, host = ref.host_depth_images(rows, cols, clouds[:nh], ref.T_CL, 4, max_depth, n_threads=args.threads); host_s = time.perf_counter() - t0
        npix = rows * cols * args.frames
        fill_GBps = npix * ALGORITHMIC_BYTES_PER_PIXEL / (stats["fill_ms"] * 1e-3) / 1e9
        line["max_depth_%g" % max_depth] = dict(
            call_s=gpu_s, call_s_all=times, call_ms_per_frame=1e3 * gpu_s / args.frames, batches=stats["batches"], frames_per_batch=-(-args.frames // stats["batches"]),
            splat_ms=stats["splat_ms"], fill_ms=stats["fill_ms"], splat_share_of_device_time=stats["splat_ms"] / (stats["splat_ms"] + stats["fill_ms"]),
            fill_ms_per_frame=stats["fill_ms"] / args.frames, valid_in_share=stats["valid_in"] / npix, valid_out_share=stats["valid_out"] / npix,
            host_rc=int(rc), host_s=host_s, host_ms_per_frame=1e3 * host_s / nh, call_over_host_per_frame=(host_s / nh) / (gpu_s / args.frames),
            host_equals_call=bool(np.array_equal(host, maps[:nh])),
            fill_roof=bench.roof("hbm, %d B per pixel: the minimum of the three-phase scheme" % ALGORITHMIC_BYTES_PER_PIXEL, fill_GBps, "GB/s", algorithmic_peak=bench.HBM_PEAK_GBPS))
    ctx.close()
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
