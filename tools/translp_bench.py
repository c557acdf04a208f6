#!/usr/bin/env python3
"""Timing of K47: pvlm_transavg_l1 at two sizes — Room (454 cameras, every camera with its next 19: 8 436 pairs) and Campus-Large (8 730 cameras, the same rule: about
1.6e5 pairs) — on the scenes of tools/transavg_bench.py (a random walk, 1 % direction noise, 10 % outlier pairs, 30 % of the pairs of unit length).  Reported per
size: the triplets of the pair list and the rows of the programme (19 per triplet), the interior-point iterations, seconds per call (the median of --repeat calls
after a warm-up call on the same list, wall clock around the ABI call), milliseconds per iteration split into kernels, camera solves and host (the library's own stage
clocks, PVLM_TRANSLP_PROFILE; every stage ends in a wait for the stream), gamma with its dual bound, and K42's solve (pvlm_transavg_solve from the DLT start, as
tools/transavg_bench.py times it) from the same process beside it.  At Room size the host compile of the same core with a dense host Cholesky
(tests/cpp/translp_core_check.cpp), on one thread, is timed as the baseline, and HiGHS on the literal programme (tests/translp_ref.py) is given --highs-timeout
seconds in a process of its own; Campus-Large is too large for either and the line says so.  No speed-up is promised: the line records what it is.  Each size runs
in a process of its own (the profile lines come on its stderr).  One JSON line per size, appended to --out."""
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


def chain_triplets(sc, reach):
    """the triplets of "every camera with its next `reach`", in FindTriplet's order (per pair (a, b) ascending, the common neighbours ascending, the pair then leaving:
    the third camera is past b), and the indices of their pairs in the sorted pair list"""
    F = sc["F"]
    a, k1, k2 = np.meshgrid(np.arange(F), np.arange(1, reach + 1), np.arange(1, reach + 1), indexing="ij")
    keep = (k1 < k2) & (a + k2 < F)
    i, j, k = a[keep], (a + k1)[keep], (a + k2)[keep]
    key = sc["first"].astype(np.int64) * F + sc["second"]
    assert np.all(np.diff(key) > 0)

    def idx(x, y):
        return np.searchsorted(key, x.astype(np.int64) * F + y).astype(np.int32)
    return np.stack([i, j, k], axis=1).astype(np.int32), np.stack([idx(i, j), idx(j, k), idx(i, k)], axis=1)


def make_scene(F, reach, seed):
    from tools import transavg_bench
    sc = transavg_bench.make_scene(F, reach, seed)
    sc["triplets"], sc["triplet_pairs"] = chain_triplets(sc, reach)
    return sc


def highs_worker(size, reach):
    from tests import translp_ref as lp
    sc = make_scene(SIZES[size], reach, 1)
    t0 = time.perf_counter(); r = lp.lp_ref(sc)
    print("translp_highs_result " + json.dumps(dict(seconds=time.perf_counter() - t0, gamma=r["gamma"], status=int(r["status"]))), flush=True)


def worker(size, reach, repeat, baseline):
    import panovlm_amd as pv
    from tests import translp_ref as lp
    sc = make_scene(SIZES[size], reach, 1)
    T = len(sc["triplets"])
    ctx = pv.Context(0)
    zero = np.zeros((sc["F"], 3))

    def gpu():
        return pv.api.transavg_l1(ctx, sc["first"], sc["second"], sc["R_21"], sc["t_21"], sc["triplet_pairs"], 0, zero, want_duals=False)
    t0 = time.perf_counter(); g = gpu(); first_s = time.perf_counter() - t0          # warm-up: the plan of the camera system, the pool
    times = []
    os.environ["PVLM_TRANSLP_PROFILE"] = "1"
    for _ in range(max(repeat, 1)):
        t0 = time.perf_counter(); g = gpu(); times.append(time.perf_counter() - t0)
    del os.environ["PVLM_TRANSLP_PROFILE"]
    line = dict(size=size, cameras=sc["F"], pairs=sc["P"], triplets=T, rows=19 * T, unknowns_reduced=3 * (sc["F"] - 1), gpu_s=float(np.median(times)), gpu_s_all=times,
                gpu_first_call_s=first_s, iterations=int(g["iterations"]), termination=pv.api.TRANSLP_TERMINATIONS[g["termination"]], bumps=int(g["bumps"]),
                gamma=g["gamma"], dual_objective=g["dual_objective"], gap=g["gap"], primal_residual=g["primal_residual"], dual_residual=g["dual_residual"],
                n_components=int(g["n_components"]), n_loose=int(g["n_loose"]), guard_intact=bool(g["guard_intact"]))
    # K42 on the same pair list, as tools/transavg_bench.py runs it
    dlt = pv.api.transavg_dlt(ctx, sc["F"], sc["first"], sc["second"], sc["R_21"], sc["t_21"])
    k42 = lambda: pv.api.transavg_solve(ctx, sc["first"], sc["second"], sc["R_21"], sc["t_21"], sc["scales"], 0, dlt["translations"], None, 0.01, 1.3, 1.0, 50)
    k42()
    kt = []
    for _ in range(max(repeat, 1)):
        t0 = time.perf_counter(); k = k42(); kt.append(time.perf_counter() - t0)
    line.update(k42_gpu_s=float(np.median(kt)), k42_lm_iterations=int(k["successful_steps"] + k["unsuccessful_steps"]))
    ctx.close()
    if baseline:
        t0 = time.perf_counter(); h = lp.host_l1(sc); host_s = time.perf_counter() - t0
        line.update(host_one_thread_s=host_s, host_over_gpu=host_s / line["gpu_s"], host_iterations=h["iterations"], host_gamma=h["gamma"],
                    gamma_diff_host_relative=abs(h["gamma"] - g["gamma"]) / abs(h["gamma"]))
    else:
        line.update(host_one_thread_s=None, host_note="too large for the dense host Cholesky baseline")
    print("translp_bench_result " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="room,campus-large")
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per size")
    ap.add_argument("--highs-timeout", type=int, default=120, help="seconds HiGHS gets at Room size (0: not run)")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--highs-worker", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k47_translp_bench.jsonl"))
    args = ap.parse_args()
    if args.highs_worker:
        highs_worker(args.highs_worker, args.neighbours)
        return
    if args.worker:
        worker(args.worker, args.neighbours, args.repeat, baseline=args.worker == "room")
        return
    for size in [s for s in args.sizes.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", size, "--neighbours", str(args.neighbours), "--repeat", str(args.repeat)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            line = dict(size=size, cameras=SIZES[size], failed="no result within %d s" % args.timeout)
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            break                                     # nothing more is started on the device behind a call that did not come back
        got = [ln for ln in res.stdout.splitlines() if ln.startswith("translp_bench_result ")]
        if res.returncode != 0 or not got:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("the %s run failed (exit %d)" % (size, res.returncode))
        line = json.loads(got[-1][len("translp_bench_result "):])
        prof = [json.loads(ln[len("pvlm_translp_profile "):]) for ln in res.stderr.splitlines() if ln.startswith("pvlm_translp_profile ")][:args.repeat]
        if prof:
            its = max(line["iterations"], 1)
            med = lambda k: float(np.median([p[k] for p in prof]))
            line.update(ms_per_iteration=dict(total=med("total_ms") / its, kernels=med("kernels_ms") / its, solve=med("solve_ms") / its, host=med("host_ms") / its),
                        camera_solves=int(prof[-1]["solves"]))
        # HiGHS on the literal programme: no device, a process of its own under its time limit
        if size == "room" and args.highs_timeout > 0:
            try:
                hres = subprocess.run([sys.executable, os.path.abspath(__file__), "--highs-worker", size, "--neighbours", str(args.neighbours)], capture_output=True, text=True,
                                      timeout=args.highs_timeout)
                hg = [ln for ln in hres.stdout.splitlines() if ln.startswith("translp_highs_result ")]
                line["highs"] = json.loads(hg[-1][len("translp_highs_result "):]) if hg else dict(failed="exit %d" % hres.returncode)
                if hg and line["highs"]["gamma"] > 0:
                    line["highs"]["gamma_diff_relative"] = abs(line["highs"]["gamma"] - line["gamma"]) / line["highs"]["gamma"]
            except subprocess.TimeoutExpired:
                line["highs"] = dict(failed="no result within %d s" % args.highs_timeout)
        else:
            line["highs"] = dict(note="not run at this size")
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
