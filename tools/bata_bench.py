#!/usr/bin/env python3
"""Timing of K44: ONE pvlm_transavg_bata with upstream's default BATAConfig (10 LUD passes of two solves each, 9 outers of 10 inners: 110 camera solves) at two
sizes — Room (454 cameras, every frame with its next 19: 8 436 pairs, K36's pair list) and Campus-Large (8 730 cameras, the same rule: 165 680 pairs).  Synthetic
centres on a walk through the scene, 1 % direction noise, 10 % outlier pairs (random directions), 30 % of the pairs without a scale (a positive draw as their start).
Reported per size: seconds per call (the median of --repeat calls after a warm-up call on the same list, wall clock around the ABI call), and milliseconds per solve
split into kernels, camera solve and host (the library's own stage clocks, PVLM_BATA_PROFILE; every stage ends in a wait for the stream), and the distance to the
truth after the LUD stage and at the end (in metres, after the common factor and camera 0's shift).  At Room size the host compile of the same core with a dense host
Cholesky (tests/cpp/bata_core_check.cpp), on one thread, is timed as the baseline; Campus-Large is too large for that (a dense 26 187 x 26 187 factorisation per
solve on one thread) and the line says so.  No speed-up is promised: the line records what it is.  Each size runs in a process of its own (the profile line comes on
its stderr).  One JSON line per size, appended to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"room": 454, "campus-large": 8730}


def make_scene(F, reach, seed):
    """centres on a random walk (0.5 m steps); every camera with its next `reach`; the direction of centre[first] - centre[second]"""
    rng = np.random.default_rng(seed)
    first = np.concatenate([np.arange(0, F - k) for k in range(1, reach + 1)]); second = np.concatenate([np.arange(k, F) for k in range(1, reach + 1)])
    order = np.lexsort((second, first)); first, second = first[order].astype(np.int32), second[order].astype(np.int32)
    P = len(first)
    Cw = np.cumsum(rng.normal(size=(F, 3)) * 0.5 / np.sqrt(3), axis=0); Cw -= Cw[0]
    v = Cw[first] - Cw[second]
    n = np.linalg.norm(v, axis=1)
    d = v / n[:, None] + 0.01 * rng.normal(size=(P, 3)) / np.sqrt(3)          # 1 % direction noise
    bad = rng.random(P) < 0.10
    u = rng.normal(size=(P, 3)); d[bad] = u[bad]
    d /= np.linalg.norm(d, axis=1)[:, None]
    free = rng.random(P) < 0.30
    s0 = np.where(free, rng.uniform(0.05, 1.0, P), n)
    return dict(F=F, P=P, n_cameras=F, first=first, second=second, dir=d, s0=s0, centres=Cw)


def worker(size, reach, repeat, baseline):
    import panovlm_amd as pv
    from tests import bata_ref as br
    sc = make_scene(SIZES[size], reach, 1)
    ctx = pv.Context(0)

    def gpu():
        return pv.api.bata_solve(ctx, sc["F"], sc["first"], sc["second"], sc["dir"], sc["s0"])
    t0 = time.perf_counter(); g = gpu(); first_s = time.perf_counter() - t0          # warm-up: the plan of the camera system, the pool
    times = []
    os.environ["PVLM_BATA_PROFILE"] = "1"
    for _ in range(max(repeat, 1)):
        t0 = time.perf_counter(); g = gpu(); times.append(time.perf_counter() - t0)
    del os.environ["PVLM_BATA_PROFILE"]
    ctx.close()
    line = dict(size=size, cameras=sc["F"], pairs=sc["P"], unknowns=3 * (sc["F"] - 1), gpu_s=float(np.median(times)), gpu_s_all=times, gpu_first_call_s=first_s, info=g["info"],
                guard_intact=bool(g["guard_intact"]), dropped_rows=int(np.isinf(g["scales"]).sum()))
    if g["info"] == 0:
        f, truth = br.align(g["centres"], sc["centres"]); fl, truth_l = br.align(g["lud_centres"], sc["centres"])
        line.update(error_lud_m=float(np.linalg.norm(g["lud_centres"] - truth_l, axis=1).max() / fl), error_final_m=float(np.linalg.norm(g["centres"] - truth, axis=1).max() / f))
    if baseline:
        t0 = time.perf_counter(); h = br.host_solve(sc); ht = time.perf_counter() - t0
        line.update(host_one_thread_s=ht, host_over_gpu=ht / line["gpu_s"], host_info=h["info"])
        if g["info"] == 0 and h["info"] == 0:
            line.update(differences_host=br.differences(g, h))
    else:
        line.update(host_one_thread_s=None, host_note="too large for the dense host Cholesky baseline")
    print("bata_bench_result " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="room,campus-large")
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per size")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k44_bata_bench.jsonl"))
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.neighbours, args.repeat, baseline=args.worker == "room" and not args.no_baseline)
        return
    for size in [s for s in args.sizes.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", size, "--neighbours", str(args.neighbours), "--repeat", str(args.repeat)] + (["--no-baseline"] if args.no_baseline else [])
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            line = dict(size=size, cameras=SIZES[size], failed="no result within %d s" % args.timeout)
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            break                                     # nothing more is started on the device behind a call that did not come back
        got = [ln for ln in res.stdout.splitlines() if ln.startswith("bata_bench_result ")]
        if res.returncode != 0 or not got:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("the %s run failed (exit %d)" % (size, res.returncode))
        line = json.loads(got[-1][len("bata_bench_result "):])
        prof = [json.loads(ln[len("pvlm_bata_profile "):]) for ln in res.stderr.splitlines() if ln.startswith("pvlm_bata_profile ")]
        if prof:
            n = max(int(prof[-1]["solves"]), 1)
            med = lambda k: float(np.median([p[k] for p in prof]))
            line.update(ms_per_solve=dict(total=med("total_ms") / n, kernels=med("kernels_ms") / n, solve=med("solve_ms") / n, host=med("host_ms") / n), camera_solves=n)
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
