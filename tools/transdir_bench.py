#!/usr/bin/env python3
"""Timing of K46: pvlm_transavg_chordal and pvlm_transavg_lud at two sizes — Room (454 cameras, every camera with its next 19: 8 436 pairs, K36's pair list) and
Campus-Large (8 730 cameras, the same rule: about 1.6e5 pairs).  Synthetic centres on a walk through the scene, 1 % direction noise; for LUD 10 % outlier pairs and
30 % of the pairs without a scale (chordal runs on the list without the outliers: upstream's chordal formulation does not survive them); the start is the truth plus
0.3 m of normal noise per coordinate.  Reported per size and problem: seconds per call (the median of --repeat calls after a warm-up call on the same list, wall clock
around the ABI call), the LM iterations, milliseconds per LM iteration split into kernels, camera solves and host (the library's own stage clocks,
PVLM_TRANSDIR_PROFILE; every stage ends in a wait for the stream), the distance to the truth before and after, and for LUD the solves TranslationAveragingLUD's loop
runs under its stop rule (at most --lud-solves) with the seconds of the whole loop.  At Room size the host compile of the same core with a dense host Cholesky
(tests/cpp/transdir_core_check.cpp), on one thread, is timed as the baseline; Campus-Large is too large for that and the line says so.  No speed-up is promised: the
line records what it is.  Each size runs in a process of its own (the profile lines come on its stderr).  One JSON line per size, appended to --out."""
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
    """cameras on a random walk (0.5 m steps); every camera with its next `reach`"""
    rng = np.random.default_rng(seed)
    first = np.concatenate([np.arange(0, F - k) for k in range(1, reach + 1)]); second = np.concatenate([np.arange(k, F) for k in range(1, reach + 1)])
    order = np.lexsort((second, first)); first, second = first[order].astype(np.int32), second[order].astype(np.int32)
    P = len(first)
    Cw = np.cumsum(rng.normal(size=(F, 3)) * 0.5 / np.sqrt(3), axis=0); Cw -= Cw[0]
    v = Cw[first] - Cw[second]
    n = np.linalg.norm(v, axis=1)
    clean = v / n[:, None] + 0.01 * rng.normal(size=(P, 3)) / np.sqrt(3)          # 1 % direction noise
    clean /= np.linalg.norm(clean, axis=1)[:, None]
    d = clean.copy()
    bad = rng.random(P) < 0.10
    u = rng.normal(size=(P, 3)); d[bad] = u[bad] / np.linalg.norm(u[bad], axis=1)[:, None]
    free = rng.random(P) < 0.30
    start = Cw + 0.3 * rng.normal(size=(F, 3)); start[0] = 0.0
    return dict(F=F, P=P, first=first, second=second, dir=d, clean_dir=clean, scales=np.where(free, 1.0, n), origin=0, truth=Cw, start=start)


def _error(c, truth, fit=False):
    if fit:
        c = c * float((c * truth).sum() / (c * c).sum())
    return float(np.linalg.norm(c - truth, axis=1).max())


def worker(size, reach, repeat, lud_solves, baseline):
    import panovlm_amd as pv
    from tests import transdir_ref as td
    sc = make_scene(SIZES[size], reach, 1)
    ctx = pv.Context(0)
    calls = dict(chordal=lambda: pv.api.transavg_chordal(ctx, sc["first"], sc["second"], sc["clean_dir"], 0, sc["start"]),
                 lud=lambda: pv.api.transavg_lud(ctx, sc["first"], sc["second"], sc["dir"], sc["scales"], None, 0, sc["start"]))
    line = dict(size=size, cameras=sc["F"], pairs=sc["P"], unknowns_reduced=3 * (sc["F"] - 1))
    for problem, call in calls.items():
        t0 = time.perf_counter(); g = call(); first_s = time.perf_counter() - t0          # warm-up: the plan of the camera system, the pool
        times = []
        os.environ["PVLM_TRANSDIR_PROFILE"] = "1"
        for _ in range(max(repeat, 1)):
            t0 = time.perf_counter(); g = call(); times.append(time.perf_counter() - t0)
        del os.environ["PVLM_TRANSDIR_PROFILE"]
        fit = problem == "chordal"
        r = dict(gpu_s=float(np.median(times)), gpu_s_all=times, gpu_first_call_s=first_s, lm_iterations=int(g["successful_steps"] + g["unsuccessful_steps"]),
                 accepted=int(g["successful_steps"]), rejected=int(g["unsuccessful_steps"]), termination=pv.api.TRANSAVG_TERMINATIONS[g["termination"]],
                 initial_cost=g["initial_cost"], final_cost=g["final_cost"], error_start_m=_error(sc["start"], sc["truth"], fit),
                 error_final_m=_error(g["centres"], sc["truth"], fit), guard_intact=bool(g["guard_intact"]))
        if baseline:
            kw = dict(dir=sc["clean_dir"]) if fit else {}
            t0 = time.perf_counter(); h = td.host_solve(problem, dict(sc, **kw)); host_s = time.perf_counter() - t0
            r.update(host_one_thread_s=host_s, host_over_gpu=host_s / r["gpu_s"], host_lm_iterations=h["successful"] + h["unsuccessful"],
                     same_steps_as_host=bool((h["successful"], h["unsuccessful"], h["termination"]) == (g["successful_steps"], g["unsuccessful_steps"], g["termination"])),
                     final_cost_diff_host=abs(h["final_cost"] - g["final_cost"]))
        else:
            r.update(host_one_thread_s=None, host_note="too large for the dense host Cholesky baseline")
        line[problem] = r
    # TranslationAveragingLUD's loop (:550-652): weights and scales fed back, the stop rule of :628
    t0 = time.perf_counter()
    c, s, w, last, solves, sums = sc["start"], sc["scales"], None, 0.0, 0, []
    for _ in range(lud_solves):
        g = pv.api.transavg_lud(ctx, sc["first"], sc["second"], sc["dir"], s, w, 0, c)
        c, s, w, solves = g["centres"], g["scales"], g["weight"], solves + 1
        sums.append(g["sum_e"])
        if abs(last - g["sum_e"]) / g["sum_e"] < 0.05 or g["sum_e"] < 10:
            break
        last = g["sum_e"]
    line["lud_loop"] = dict(solves=solves, seconds=time.perf_counter() - t0, sum_e=sums, error_final_m=_error(c, sc["truth"]))
    ctx.close()
    print("transdir_bench_result " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="room,campus-large")
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--lud-solves", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=900, help="seconds per size")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k46_transdir_bench.jsonl"))
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.neighbours, args.repeat, args.lud_solves, baseline=args.worker == "room")
        return
    for size in [s for s in args.sizes.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", size, "--neighbours", str(args.neighbours), "--repeat", str(args.repeat), "--lud-solves",
               str(args.lud_solves)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            line = dict(size=size, cameras=SIZES[size], failed="no result within %d s" % args.timeout)
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            break                                     # nothing more is started on the device behind a call that did not come back
        got = [ln for ln in res.stdout.splitlines() if ln.startswith("transdir_bench_result ")]
        if res.returncode != 0 or not got:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("the %s run failed (exit %d)" % (size, res.returncode))
        line = json.loads(got[-1][len("transdir_bench_result "):])
        prof = [json.loads(ln[len("pvlm_transdir_profile "):]) for ln in res.stderr.splitlines() if ln.startswith("pvlm_transdir_profile ")]
        for problem in ("chordal", "lud"):
            mine = [p for p in prof if p["call"] == "pvlm_transavg_" + problem][:args.repeat]
            if mine:
                its = max(line[problem]["lm_iterations"], 1)
                med = lambda k: float(np.median([p[k] for p in mine]))
                line[problem].update(ms_per_lm_iteration=dict(total=med("total_ms") / its, kernels=med("kernels_ms") / its, solve=med("solve_ms") / its, host=med("host_ms") / its),
                                     camera_solves=int(mine[-1]["solves"]))
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
