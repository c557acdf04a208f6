#!/usr/bin/env python3
"""Timing of K45: ONE pvlm_rotavg_least_square (RotationAveragingLeastSquare by shift-and-invert subspace iteration) at two sizes — Room (454 cameras, every frame
with its next 19: 8 436 pairs, K36's pair list) and Campus-Large (8 730 cameras, the same rule: 165 680 pairs).  The scenes are those of tools/rotavg_bench.py
(random rotations, 1 degree of rotation noise per pair) without outlier pairs, since upstream meets this stage behind its triplet filter; the start is the spanning
tree of the pair list from camera 0, as the host mirror makes it.  Reported per size: seconds per call (the median of --repeat calls after a warm-up call on the same
list, wall clock around the ABI call), iterations, solves, info, the last residual, milliseconds split into kernels / camera solve / host (the library's own stage
clocks, PVLM_ROTAVG_PROFILE; every stage ends in a wait for the stream) with the solve's share, and the largest angle to the truth before and after.  The iteration
converges by (lambda_2 + sigma) / (lambda_3 + sigma) per step; on a long band with this much noise that ratio is near one, so --max-iterations defaults to 1000
here (the library's default is 100) and the line records whether the call converged.  At Room size the host compile of the same core (tests/cpp/
rotstart_core_check.cpp: one dense host Cholesky, one thread) and numpy.linalg.eigh of the dense matrix — the baseline upstream's method implies — are timed too;
at Campus-Large the dense route is stated as not run: 72 F^2 bytes = 5.5 GB for the matrix and its eigenvectors, 27 F^3 = 1.8e13 operations.  No speed-up is
promised: the line records what it is.  Each size runs in a process of its own (the profile lines come on its stderr).  One JSON line per size, appended to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"room": 454, "mid": 2000, "campus-large": 8730}


def worker(size, reach, repeat, baseline, max_iterations):
    import panovlm_amd as pv
    from tests import rotavg_ref as rr
    from tests import rotstart_ref as rs
    from tools.rotavg_bench import make_scene
    sc = make_scene(SIZES[size], reach, 1, 0.0)
    ctx = pv.Context(0)

    def gpu():
        return pv.api.rotavg_least_square(ctx, sc["first"], sc["second"], sc["R_21"], sc["R0"], max_iterations=max_iterations)
    t0 = time.perf_counter(); g = gpu(); first_s = time.perf_counter() - t0          # warm-up: the plan of the camera system, the pool
    times = []
    os.environ["PVLM_ROTAVG_PROFILE"] = "1"
    for _ in range(max(repeat, 1)):
        t0 = time.perf_counter(); g = gpu(); times.append(time.perf_counter() - t0)
    del os.environ["PVLM_ROTAVG_PROFILE"]
    ctx.close()
    angle = lambda R: float(np.degrees(max(rr.angle_between(R[c], sc["truth"][c]) for c in range(sc["F"]))))
    F = sc["F"]
    line = dict(size=size, cameras=F, pairs=sc["P"], unknowns=3 * F, max_iterations=max_iterations, gpu_s=float(np.median(times)), gpu_s_all=times, gpu_first_call_s=first_s,
                iterations=int(g["iterations"]), solves=int(g["solves"]), info=int(g["info"]), converged=bool(g["info"] == 0), residual=float(g["residual"]),
                theta=[float(v) for v in g["theta"]], angle_start_deg=angle(sc["R0"]), angle_result_deg=angle(g["rotations"]), guard_intact=bool(g["guard_intact"]),
                dense_bytes=72 * F * F, dense_operations=27 * F ** 3)
    if baseline:
        t0 = time.perf_counter(); h = rs.host_least_square(sc, max_iterations=max_iterations); ht = time.perf_counter() - t0
        t0 = time.perf_counter(); ref = rs.least_square_ref(sc); et = time.perf_counter() - t0
        line.update(host_one_thread_s=ht, host_over_gpu=ht / line["gpu_s"], host_info=h["info"], host_iterations=h["iterations"], dense_eigh_s=et, dense_eigh_over_gpu=et / line["gpu_s"],
                    angle_diff_host_rad=rr.largest_angle(h["rotations"], g["rotations"]), angle_diff_dense_rad=rr.largest_angle(ref["rotations"], g["rotations"]),
                    lambda_2=float(ref["eigenvalues"][2]), lambda_3=float(ref["eigenvalues"][3]))
    else:
        line.update(host_one_thread_s=None, dense_eigh_s=None,
                    dense_note="not run: the dense matrix and its eigenvectors take 72 F^2 = %.1f GB, the decomposition 27 F^3 = %.1e operations" % (72 * F * F / 1e9, 27.0 * F ** 3))
    print("rotstart_bench_result " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="room,campus-large")
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=1000)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per size")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k45_rotstart_bench.jsonl"))
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.neighbours, args.repeat, args.worker == "room", args.max_iterations)
        return
    for size in [s for s in args.sizes.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", size, "--neighbours", str(args.neighbours), "--repeat", str(args.repeat), "--max-iterations", str(args.max_iterations)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            line = dict(size=size, cameras=SIZES[size], failed="no result within %d s" % args.timeout)
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            break                                     # nothing more is started on the device behind a call that did not come back
        got = [ln for ln in res.stdout.splitlines() if ln.startswith("rotstart_bench_result ")]
        if res.returncode != 0 or not got:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("the %s run failed (exit %d)" % (size, res.returncode))
        line = json.loads(got[-1][len("rotstart_bench_result "):])
        prof = [json.loads(ln[len("pvlm_rotavg_profile "):]) for ln in res.stderr.splitlines() if ln.startswith("pvlm_rotavg_profile ")]
        prof = [p for p in prof if p["entry"] == "least_square"]
        if prof:
            med = lambda k: float(np.median([p[k] for p in prof]))
            line.update(ms=dict(total=med("total_ms"), kernels=med("kernels_ms"), solve=med("solve_ms"), host=med("host_ms")), solve_share=med("solve_ms") / med("total_ms"),
                        ms_per_solve=med("solve_ms") / max(int(prof[-1]["solves"]), 1))
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
