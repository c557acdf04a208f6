#!/usr/bin/env python3
"""Timing of K40: ONE EstimateGlobalRotation-sized pvlm_rotavg_l1 followed by pvlm_rotavg_l2 at Room size (454 cameras, every frame with its next 19: 8 436 pairs,
K36's pair list) and Campus-Large (8 730 cameras, the same rule: 165 680 pairs); `mid` (2 000 cameras) sits between them.  The synthetic walk of
tools/transavg_bench.py: random rotations, 1 degree of rotation noise per pair, 10 % outlier pairs (random rotations; --outliers); the start is the spanning tree of
the pair list from camera 0, as EstimateGlobalRotation makes it — with outliers in the list most tree paths cross one (upstream meets this stage behind its triplet
filter), so the start and the result are far from the truth and the loops run to their caps: what is timed is the work, not the accuracy.  Reported per size: seconds per call (the median of --repeat calls after a warm-up call on the same list,
wall clock around the ABI call) for both entry points, the iteration counts of the three loops, milliseconds per ADMM iteration (the kernels' stage clock over the
ADMM iterations; every iteration ends in a wait for the stream), the bytes per second of the dense product if ALL of that time were the product's (8 (F - 1)^2
bytes of G per iteration: a lower bound on what the kernel reaches) against the HBM roof, the time to form G = (2 L)^-1, the IRLS / LM solves, and the largest angle
to the truth before and after.  At Room size the host compile of the same core (tests/cpp/rotavg_core_check.cpp: dense host Cholesky, one thread) is timed as the
baseline; the larger sizes are too large for that and the line says so.  No speed-up is promised: the line records what it is.  Each size runs in a process of its
own (the profile lines come on its stderr).  One JSON line per size, appended to --out."""
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
HBM_ROOF = 8.0e12        # bytes per second, MI355X data sheet


def make_scene(F, reach, seed, outliers=0.10):
    """random rotations; every camera with its next `reach`; 1 degree of noise, `outliers` of the pairs random; the spanning-tree start from camera 0"""
    from tests import rotavg_ref as rr
    rng = np.random.default_rng(seed)
    first = np.concatenate([np.arange(0, F - k) for k in range(1, reach + 1)]); second = np.concatenate([np.arange(k, F) for k in range(1, reach + 1)])
    order = np.lexsort((second, first)); first, second = first[order].astype(np.int32), second[order].astype(np.int32)
    P = len(first)
    Rc = np.array([rr.exp_so3(v) for v in rng.normal(size=(F, 3)) * 0.6])
    noise = np.array([rr.exp_so3(v) for v in rng.normal(size=(P, 3)) * np.radians(1.0) / np.sqrt(3)])
    R21 = np.einsum("pij,pjk->pik", noise, np.einsum("pij,pkj->pik", Rc[second], Rc[first]))
    bad = np.flatnonzero(rng.random(P) < outliers)
    for p in bad:
        R21[p] = rr.exp_so3(rng.normal(size=3) * 1.5)
    return dict(F=F, P=P, first=first, second=second, R_21=R21, start=0, truth=np.einsum("cij,kj->cik", Rc, Rc[0]),
                R0=rr.spanning_tree_start(F, first, second, R21, 0))


def worker(size, reach, repeat, baseline, outliers):
    import panovlm_amd as pv
    from tests import rotavg_ref as rr
    sc = make_scene(SIZES[size], reach, 1, outliers)
    ctx = pv.Context(0)

    def l1():
        return pv.api.rotavg_l1(ctx, sc["first"], sc["second"], sc["R_21"], 0, sc["R0"])
    t0 = time.perf_counter(); g1 = l1(); first_s = time.perf_counter() - t0          # warm-up: the pool, the plan of the IRLS system
    g2 = pv.api.rotavg_l2(ctx, sc["first"], sc["second"], sc["R_21"], g1["rotations"])
    t1, t2 = [], []
    os.environ["PVLM_ROTAVG_PROFILE"] = "1"
    for _ in range(max(repeat, 1)):
        t0 = time.perf_counter(); g1 = l1(); t1.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); g2 = pv.api.rotavg_l2(ctx, sc["first"], sc["second"], sc["R_21"], g1["rotations"]); t2.append(time.perf_counter() - t0)
    del os.environ["PVLM_ROTAVG_PROFILE"]
    ctx.close()
    angle = lambda R: float(np.degrees(max(rr.angle_between(R[c], sc["truth"][c]) for c in range(sc["F"]))))
    line = dict(size=size, cameras=sc["F"], pairs=sc["P"], outliers=outliers, l1_s=float(np.median(t1)), l1_s_all=t1, l1_first_call_s=first_s, l2_s=float(np.median(t2)), l2_s_all=t2,
                l1_iterations=int(g1["l1_iterations"]), admm_iterations=int(g1["admm_iterations"]), irls_iterations=int(g1["irls_iterations"]), info=int(g1["info"]),
                l2_accepted=int(g2["successful_steps"]), l2_rejected=int(g2["unsuccessful_steps"]), l2_termination=pv.api.TRANSAVG_TERMINATIONS[g2["termination"]],
                l2_initial_cost=g2["initial_cost"], l2_final_cost=g2["final_cost"], angle_start_deg=angle(sc["R0"]), angle_l1_deg=angle(g1["rotations"]),
                angle_l2_deg=angle(g2["rotations"]), g_bytes=8 * (sc["F"] - 1) ** 2, guard_intact=bool(g1["guard_intact"] and g2["guard_intact"]))
    if baseline:
        t0 = time.perf_counter(); h1 = rr.host_l1(sc); h1_s = time.perf_counter() - t0
        t0 = time.perf_counter(); h2 = rr.host_l2(sc, g1["rotations"]); h2_s = time.perf_counter() - t0
        line.update(host_one_thread_l1_s=h1_s, host_one_thread_l2_s=h2_s, host_over_gpu_l1=h1_s / line["l1_s"], host_over_gpu_l2=h2_s / line["l2_s"],
                    same_counts_as_host=bool(rr.counts_l1(h1) == (g1["l1_iterations"], g1["admm_iterations"], g1["irls_iterations"], g1["info"] > 0) and
                                             rr.counts_l2(h2) == (g2["successful_steps"], g2["unsuccessful_steps"], g2["termination"])),
                    angle_l1_diff_host_rad=rr.largest_angle(h1["rotations"], g1["rotations"]), angle_l2_diff_host_rad=rr.largest_angle(h2["rotations"], g2["rotations"]))
    else:
        line.update(host_one_thread_l1_s=None, host_note="too large for the dense host Cholesky baseline")
    print("rotavg_bench_result " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="room,campus-large")
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--outliers", type=float, default=0.10, help="fraction of the pairs with a random rotation")
    ap.add_argument("--timeout", type=int, default=900, help="seconds per size")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k40_rotavg_bench.jsonl"))
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.neighbours, args.repeat, args.worker == "room", args.outliers)
        return
    for size in [s for s in args.sizes.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", size, "--neighbours", str(args.neighbours), "--repeat", str(args.repeat), "--outliers", str(args.outliers)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            line = dict(size=size, cameras=SIZES[size], failed="no result within %d s" % args.timeout)
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            break                                     # nothing more is started on the device behind a call that did not come back
        got = [ln for ln in res.stdout.splitlines() if ln.startswith("rotavg_bench_result ")]
        if res.returncode != 0 or not got:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("the %s run failed (exit %d)" % (size, res.returncode))
        line = json.loads(got[-1][len("rotavg_bench_result "):])
        prof = [json.loads(ln[len("pvlm_rotavg_profile "):]) for ln in res.stderr.splitlines() if ln.startswith("pvlm_rotavg_profile ")]
        p1 = [p for p in prof if p["entry"] == "l1"]; p2 = [p for p in prof if p["entry"] == "l2"]
        med = lambda ps, k: float(np.median([p[k] for p in ps]))
        if p1:
            its = max(line["admm_iterations"], 1)
            ms = med(p1, "kernels_ms") / its
            line.update(l1_ms=dict(total=med(p1, "total_ms"), kernels=med(p1, "kernels_ms"), irls_solves=med(p1, "solve_ms"), form_g=med(p1, "form_g_ms"), host=med(p1, "host_ms")),
                        ms_per_admm_iteration=ms, product_bytes_per_s_at_least=line["g_bytes"] / (ms * 1e-3), hbm_roof_bytes_per_s=HBM_ROOF,
                        product_fraction_of_roof_at_least=line["g_bytes"] / (ms * 1e-3) / HBM_ROOF, form_g_s=med(p1, "form_g_ms") * 1e-3)
        if p2:
            line.update(l2_ms=dict(total=med(p2, "total_ms"), kernels=med(p2, "kernels_ms"), solves=med(p2, "solve_ms"), host=med(p2, "host_ms")))
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
