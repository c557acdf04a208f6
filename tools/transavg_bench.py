#!/usr/bin/env python3
"""Timing of K42: ONE EstimateGlobalTranslation-sized pvlm_transavg_solve at two sizes — Room (454 cameras, every frame with its next 19: 8 436 pairs, K36's pair
list) and Campus-Large (8 730 cameras, the same rule: about 1.6e5 pairs).  Synthetic poses on a walk through the scene, 1 % direction noise, 10 % outlier pairs,
30 % of the pairs without a scale; the start is pvlm_transavg_dlt's solution (camera 0 is the origin), as the reference's configs do.  Reported per size: seconds per
call (the median of --repeat calls after a warm-up call on the same list, wall clock around the ABI call), the LM iterations, and milliseconds per LM iteration split
into kernels, camera solves and host (the library's own stage clocks, PVLM_TRANSAVG_PROFILE; every stage ends in a wait for the stream), the DLT's seconds, and the
distance to the truth before and after.  At Room size the host compile of the same core with a dense host Cholesky (tests/cpp/transavg_core_check.cpp), on one
thread, is timed as the baseline; Campus-Large is too large for that (a dense 26 187 x 26 187 factorisation per iteration on one thread) and the line says so.
No speed-up is promised: the line records what it is.  Each size runs in a process of its own (the profile line comes on its stderr).  One JSON line per size,
appended to --out."""
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
    """cameras on a random walk (0.5 m steps), random rotations; every camera with its next `reach`"""
    from tests import transavg_ref as tr
    rng = np.random.default_rng(seed)
    first = np.concatenate([np.arange(0, F - k) for k in range(1, reach + 1)]); second = np.concatenate([np.arange(k, F) for k in range(1, reach + 1)])
    order = np.lexsort((second, first)); first, second = first[order].astype(np.int32), second[order].astype(np.int32)
    P = len(first)
    w = rng.normal(size=(F, 3)) * 0.6
    Rc = np.array([tr.rodrigues(v) for v in w])
    C = np.cumsum(rng.normal(size=(F, 3)) * 0.5 / np.sqrt(3), axis=0); C -= C[0]
    t = -np.einsum("cij,cj->ci", Rc, C); t[0] = 0
    R21 = np.einsum("pij,pkj->pik", Rc[second], Rc[first])
    v = t[second] - np.einsum("pij,pj->pi", R21, t[first])
    n = np.linalg.norm(v, axis=1)
    d = v / n[:, None] + 0.01 * rng.normal(size=(P, 3)) / np.sqrt(3)          # 1 % direction noise
    bad = rng.random(P) < 0.10
    u = rng.normal(size=(P, 3)); d[bad] = u[bad]
    d /= np.linalg.norm(d, axis=1)[:, None]
    free = rng.random(P) < 0.30
    t21 = np.where(free[:, None], d, d * n[:, None])
    return dict(F=F, P=P, first=first, second=second, R_21=R21, t_21=t21, scales=np.where(free, 1.0, n), origin=0, truth=t)


def worker(size, reach, repeat, max_iterations, baseline):
    import panovlm_amd as pv
    from tests import transavg_ref as tr
    sc = make_scene(SIZES[size], reach, 1)
    ctx = pv.Context(0)
    t0 = time.perf_counter(); dlt = pv.api.transavg_dlt(ctx, sc["F"], sc["first"], sc["second"], sc["R_21"], sc["t_21"]); dlt_first = time.perf_counter() - t0
    t0 = time.perf_counter(); dlt = pv.api.transavg_dlt(ctx, sc["F"], sc["first"], sc["second"], sc["R_21"], sc["t_21"]); dlt_s = time.perf_counter() - t0
    assert dlt["info"] == 0
    start = dlt["translations"]

    def gpu():
        return pv.api.transavg_solve(ctx, sc["first"], sc["second"], sc["R_21"], sc["t_21"], sc["scales"], 0, start, None, 0.01, 1.3, 1.0, max_iterations)
    t0 = time.perf_counter(); g = gpu(); first_s = time.perf_counter() - t0          # warm-up: the plan of the camera system, the pool
    times = []
    os.environ["PVLM_TRANSAVG_PROFILE"] = "1"
    for _ in range(max(repeat, 1)):
        t0 = time.perf_counter(); g = gpu(); times.append(time.perf_counter() - t0)
    del os.environ["PVLM_TRANSAVG_PROFILE"]
    ctx.close()
    its = g["successful_steps"] + g["unsuccessful_steps"]
    line = dict(size=size, cameras=sc["F"], pairs=sc["P"], unknowns_unreduced=3 * (sc["F"] - 1) + sc["P"], unknowns_reduced=3 * (sc["F"] - 1), gpu_s=float(np.median(times)),
                gpu_s_all=times, gpu_first_call_s=first_s, dlt_s=dlt_s, dlt_first_call_s=dlt_first, lm_iterations=int(its), accepted=int(g["successful_steps"]),
                rejected=int(g["unsuccessful_steps"]), termination=pv.api.TRANSAVG_TERMINATIONS[g["termination"]], initial_cost=g["initial_cost"], final_cost=g["final_cost"],
                error_dlt_m=float(np.abs(start - sc["truth"]).max()), error_final_m=float(np.abs(g["translations"] - sc["truth"]).max()), guard_intact=bool(g["guard_intact"]))
    if baseline:
        ht = []
        for _ in range(2):
            t0 = time.perf_counter(); h = tr.host_solve(sc, start, loss_a=0.01, upper_ratio=1.3, lower_ratio=1.0, max_num_iterations=max_iterations); ht.append(time.perf_counter() - t0)
        line.update(host_one_thread_s=min(ht), host_s_all=ht, host_over_gpu=min(ht) / line["gpu_s"], host_lm_iterations=h["successful"] + h["unsuccessful"],
                    same_steps_as_host=bool((h["successful"], h["unsuccessful"], h["termination"]) == (g["successful_steps"], g["unsuccessful_steps"], g["termination"])),
                    final_cost_diff_host=abs(h["final_cost"] - g["final_cost"]))
    else:
        line.update(host_one_thread_s=None, host_note="too large for the dense host Cholesky baseline")
    print("transavg_bench_result " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="room,campus-large")
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per size")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k42_transavg_bench.jsonl"))
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.neighbours, args.repeat, args.max_iterations, baseline=args.worker == "room")
        return
    for size in [s for s in args.sizes.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", size, "--neighbours", str(args.neighbours), "--repeat", str(args.repeat), "--max-iterations",
               str(args.max_iterations)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            line = dict(size=size, cameras=SIZES[size], failed="no result within %d s" % args.timeout)
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            break                                     # nothing more is started on the device behind a call that did not come back
        got = [ln for ln in res.stdout.splitlines() if ln.startswith("transavg_bench_result ")]
        if res.returncode != 0 or not got:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("the %s run failed (exit %d)" % (size, res.returncode))
        line = json.loads(got[-1][len("transavg_bench_result "):])
        prof = [json.loads(ln[len("pvlm_transavg_profile "):]) for ln in res.stderr.splitlines() if ln.startswith("pvlm_transavg_profile ")]
        if prof:
            its = max(line["lm_iterations"], 1)
            med = lambda k: float(np.median([p[k] for p in prof]))
            line.update(ms_per_lm_iteration=dict(total=med("total_ms") / its, kernels=med("kernels_ms") / its, solve=med("solve_ms") / its, host=med("host_ms") / its),
                        camera_solves=int(prof[-1]["solves"]))
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
