#!/usr/bin/env python3
"""Room- and Floor-scale timing of K32: pvlm_triangulate_tracks (keypoints input) and pvlm_filter_tracks_far on a vectorised version of the
trajectory scene of tests/sfm_ba_ref.py (F panoramas 0.4 m apart, every point seen by a window of 3 to 9 consecutive frames, keypoints
rounded to pixels), against the same work by the host compile of the per-track cores (tests/cpp/structure_core_check.cpp) on 16 threads.
The device call figures are whole calls: validation, uploads, the kernel, the download.  The kernels alone: for every size the tool starts
itself once more as a child under `rocprofv3 --kernel-trace --stats` (with --child: the same scene and calls, no host loop, nothing written) and
reads the average duration of k_triangulate_tracks and k_filter_tracks_far from the kernel statistics; null when rocprofv3 is not there or
--no-kernels is given.  One JSON line per size, appended to --out."""
import argparse
import ctypes as C
import json
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(rng, F, M, rows, cols, min_track, max_track):
    yaw = 0.02 * np.arange(F)
    R = np.zeros((F, 3, 3)); R[:, 0, 0] = np.cos(yaw); R[:, 0, 2] = np.sin(yaw); R[:, 1, 1] = 1; R[:, 2, 0] = -np.sin(yaw); R[:, 2, 2] = np.cos(yaw)
    t = np.stack([0.4 * np.arange(F), np.zeros(F), 0.1 * np.sin(0.2 * np.arange(F))], 1)
    k = rng.integers(min_track, max_track + 1, size=M)
    first = rng.integers(0, np.maximum(F - k, 1))
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    fid = np.concatenate([np.arange(f, f + kk) for f, kk in zip(first, k)]).astype(np.int32)
    d = rng.normal(size=(M, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    X = t[np.minimum(first + k // 2, F - 1)] + d * rng.uniform(3.0, 12.0, size=(M, 1))
    pt = np.repeat(np.arange(M), k)
    p = np.einsum("nji,nj->ni", R[fid], X[pt] - t[fid])
    lon = np.arctan2(p[:, 0], p[:, 2]); lat = -np.arcsin(p[:, 1] / np.linalg.norm(p, axis=1))
    kp = np.rint(np.stack([cols * (0.5 + lon / (2 * np.pi)), rows * (0.5 - lat / np.pi)], 1)).astype(np.float32)
    T = np.concatenate([np.transpose(R, (0, 2, 1)), -np.einsum("nji,nj->ni", R, t)[:, :, None]], 2)
    return off, fid, kp, np.ascontiguousarray(T), t, X


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def kernel_times_us(F, args):
    """Average kernel durations (us) of a child run of this tool at F frames under rocprofv3, or None."""
    prof = shutil.which("rocprofv3")
    if prof is None or args.no_kernels:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "-d", d, "-o", "k32", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child",
               "--frames", str(F), "--tracks-per-frame", str(args.tracks_per_frame), "--rows", str(args.rows), "--cols", str(args.cols),
               "--min-track", str(args.min_track), "--max-track", str(args.max_track), "--reps", str(args.reps)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        out = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for key in ("k_triangulate_tracks", "k_filter_tracks_far"):
                    if row["Name"].startswith(key):
                        out[key] = dict(avg_us=float(row["AverageNs"]) / 1e3, launches=int(row["Calls"]))
        return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="454,1593", help="comma-separated: Room 454, Floor 1593")
    ap.add_argument("--tracks-per-frame", type=int, default=440)          # Room: 200 k tracks
    ap.add_argument("--rows", type=int, default=2880)
    ap.add_argument("--cols", type=int, default=5760)
    ap.add_argument("--min-track", type=int, default=3)
    ap.add_argument("--max-track", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-kernels", action="store_true", help="skip the child run under rocprofv3")
    ap.add_argument("--child", action="store_true", help="the device calls only (what the rocprofv3 child runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k32_structure_bench.jsonl"))
    args = ap.parse_args()
    frames = [int(x) for x in args.frames.split(",")]
    kernels = {} if args.child else {F: kernel_times_us(F, args) for F in frames}      # before this process opens the GPU itself
    import panovlm_amd as pv
    so = os.path.join(ROOT, "build", "libstructure_check.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "cpp", "structure_core_check.cpp")])
    chk = C.CDLL(so)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx = pv.Context(0)
    for F in frames:
        M = F * args.tracks_per_frame
        off, fid, kp, T, t_wc, X_true = scene(np.random.default_rng(1), F, M, args.rows, args.cols, args.min_track, args.max_track)
        X, st = pv.api.triangulate_tracks(ctx, args.rows, args.cols, off, fid, T, keypoints=kp)
        keep = pv.api.filter_tracks_far(ctx, off, fid, X, t_wc, 8.0)
        tri_ms = median_ms(lambda: pv.api.triangulate_tracks(ctx, args.rows, args.cols, off, fid, T, keypoints=kp), args.reps)
        far_ms = median_ms(lambda: pv.api.filter_tracks_far(ctx, off, fid, X, t_wc, 8.0), args.reps)
        if args.child:
            continue
        # the host compile on `threads` threads: contiguous slices of tracks (ctypes releases the GIL)
        cuts = np.linspace(0, M, args.threads + 1).astype(np.int64)
        Xh = np.zeros((M, 3)); sth = np.zeros(M, np.uint8); keeph = np.zeros(M, np.uint8)

        def tri_slice(j):
            a, b = cuts[j], cuts[j + 1]
            o = np.ascontiguousarray(off[a:b + 1])
            chk.chk_triangulate(C.c_int(args.rows), C.c_int(args.cols), C.c_int(int(b - a)), p(o), p(fid), p(kp), None, p(T), None, p(Xh[a:b]), p(sth[a:b]))

        def far_slice(j):
            a, b = cuts[j], cuts[j + 1]
            o = np.ascontiguousarray(off[a:b + 1])
            chk.chk_filter_far(C.c_int(int(b - a)), p(o), p(fid), p(X[a:b]), p(t_wc), None, C.c_double(8.0), p(keeph[a:b]))

        with ThreadPoolExecutor(args.threads) as pool:
            host_tri_ms = median_ms(lambda: list(pool.map(tri_slice, range(args.threads))), 3)
            host_far_ms = median_ms(lambda: list(pool.map(far_slice, range(args.threads))), 3)
        same = bool(np.array_equal(X.view(np.uint64), Xh.view(np.uint64)) and np.array_equal(st, sth) and np.array_equal(keep, keeph))
        err = np.linalg.norm(X[st == 0] - X_true[st == 0], axis=1)
        line = dict(frames=F, tracks=M, observations=int(off[-1]), rows=args.rows, cols=args.cols, triangulate_call_ms=tri_ms, filter_far_call_ms=far_ms,
                    triangulate_kernel_us=kernels[F] and kernels[F].get("k_triangulate_tracks", {}).get("avg_us"),
                    filter_far_kernel_us=kernels[F] and kernels[F].get("k_filter_tracks_far", {}).get("avg_us"),
                    kernel_launches_traced=kernels[F] and kernels[F].get("k_triangulate_tracks", {}).get("launches"), host_threads=args.threads, host_triangulate_ms=host_tri_ms, host_filter_far_ms=host_far_ms, device_equals_host_bits=same,
                    status_ok=int((st == 0).sum()), kept_far=int(keep.sum()), median_point_error_m=float(np.median(err)))
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
