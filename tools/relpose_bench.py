#!/usr/bin/env python3
"""Room-scale timing of K36: ONE pvlm_refine_relative_poses call on a synthetic pair list of the size tools/essential_bench.py's scene leaves behind K34 (--frames
frames on a circle, every frame with its next --neighbours frames, 70 % of --matches matches as inliers per pair, a share --large of the pairs with 70 % of
--large-matches; each pair starts 0.5 degrees / 2 degrees off its true pose with the points triangulated there, and a share --planted of its inliers carries a 20-pixel
error) against RefineRelativePosesHost's loop (the host compile of the same core, tests/cpp/relpose_core_check.cpp, on --threads threads) over the same list.  Reported:
pairs per second and LM iterations per second of both, the share of pairs per termination code, the spread of iterations per pair (the load-imbalance figure: a
workgroup lives as long as its pair iterates), and how many pairs take the same steps on both sides.  The GPU figure is the median of --repeat calls after a warm-up
call on the same list, wall clock around the call (the host gather of the observations, uploads and downloads included); the host figure is the faster of two runs
(the window includes the ctypes marshalling and the single-threaded argument check).  What the tree could do before this call existed, one ceres_like::Solve with a
pvlm_baset per pair, is timed by the host mirror's driver (pvlm_relpose_driver solve-route) on --solve-pairs pairs of its own scene (about 280 inliers each) next to
one call on the same pairs; its figures are merged into the line.  No speed-up is promised: the line records what it is.  One JSON line, appended to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def triangulate(R, t, p1, p2):
    """the midpoint of tests/essential_ref.triangulate_2view for all points at once"""
    t12 = -R.T @ t; b2 = p2 @ R
    a11 = (p1 * p1).sum(1); a12 = -(p1 * b2).sum(1); a21 = -a12; a22 = -(b2 * b2).sum(1)
    r1 = p1 @ t12; r2 = b2 @ t12
    det = a11 * a22 - a12 * a21
    l1 = (r1 * a22 - a12 * r2) / det; l2 = (a11 * r2 - a21 * r1) / det
    return (l1[:, None] * p1 + l2[:, None] * b2 + t12) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=454)
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--large", type=float, default=0.01)
    ap.add_argument("--large-matches", type=int, default=1500)
    ap.add_argument("--planted", type=float, default=0.02)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--solve-pairs", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k36_relpose_bench.jsonl"))
    args = ap.parse_args()
    import panovlm_amd as pv
    from tests import essential_ref as er
    from tests import relpose_ref as rr
    rng = np.random.default_rng(1)
    pairs = [(i, j) for i in range(args.frames) for j in range(i + 1, min(i + 1 + args.neighbours, args.frames))]
    scenes = []
    for (i, j) in pairs:
        n = int(0.7 * (args.large_matches if rng.random() < args.large else args.matches))
        step = j - i
        b1, b2, m, _, R, t = er.two_view_scene(rng, n, outlier_fraction=0.0, t=(0.3 * step, 0.05, -0.02 * step), w=(0.01, 0.03 * step, 0.0), shuffle=False)
        kp1 = rr.pixels_of(b1); kp2 = rr.pixels_of(b2)
        bad = rng.permutation(n)[:int(round(args.planted * n))]
        ang = rng.uniform(0, 2 * np.pi, len(bad))
        kp2[bad] += (20.0 * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
        R0, t0 = rr.perturbed(rng, R, t)
        X0 = triangulate(R0, t0, b1.astype(np.float64), b2.astype(np.float64))
        good = np.isfinite(X0).all(1)
        scenes.append(dict(kp1=kp1, kp2=kp2, matches=m, idx=np.flatnonzero(good).astype(np.int32), R0=R0, t0=t0, X0=X0[good], n=int(good.sum())))
    call = rr.assemble(scenes)
    ctx = pv.Context(0)

    def gpu(c):
        return pv.api.refine_relative_poses(ctx, c["keypoints"], c["img_rows"], c["img_cols"], c["src"], c["tgt"], c["match_offsets"], c["matches"], c["inlier_offsets"],
                                            c["inlier_idx"], c["R_21"], c["t_21"], c["triangulated"])
    gpu(call)                                                                                 # warm-up on the timed list: code object, pool
    times = []
    for _ in range(max(args.repeat, 1)):
        t0 = time.perf_counter(); g = gpu(call); times.append(time.perf_counter() - t0)
    gpu_s = float(np.median(times))
    chk = rr.build_check("off")
    host_times = []
    for _ in range(2):
        t0 = time.perf_counter(); rc, h = rr.host_refine(chk, call, "pixel", 50, threads=args.threads); host_times.append(time.perf_counter() - t0)
    host_s = min(host_times)
    ctx.close()
    from panovlm_amd import build
    build.build_host()
    out = subprocess.run([build.RELPOSE_DRIVER, "solve-route", str(args.solve_pairs)], capture_output=True, text=True, timeout=400)
    if out.returncode != 0:
        raise RuntimeError("pvlm_relpose_driver solve-route failed: " + out.stdout + out.stderr)
    solve = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    sg, sh = g["summaries"], h["summaries"]
    iters = (sg["successful_steps"] + sg["unsuccessful_steps"]).astype(np.int64)
    same_steps = (sg["successful_steps"] == sh["successful_steps"]) & (sg["unsuccessful_steps"] == sh["unsuccessful_steps"]) & (sg["termination"] == sh["termination"])
    rel = np.abs(sg["final_cost"] - sh["final_cost"]) / np.maximum(np.abs(sh["final_cost"]), 1e-300)
    n_in = np.diff(call["inlier_offsets"])
    line = dict(solve, frames=args.frames, pairs=int(len(pairs)), inliers=int(n_in.sum()), inliers_per_pair_median=float(np.median(n_in)), inliers_per_pair_max=int(n_in.max()),
                gpu_s=gpu_s, gpu_s_all=times, gpu_pairs_per_s=len(pairs) / gpu_s, gpu_lm_iterations_per_s=float(iters.sum()) / gpu_s, host_threads=args.threads, host_rc=int(rc),
                host_s=host_s, host_s_all=host_times, host_pairs_per_s=len(pairs) / host_s, host_lm_iterations_per_s=float((sh["successful_steps"] + sh["unsuccessful_steps"]).sum()) / host_s,
                gpu_over_host=host_s / gpu_s, termination_share={pv.api.RELPOSE_TERMINATIONS[k]: float((sg["termination"] == k).mean()) for k in np.unique(sg["termination"])},
                iterations_per_pair=dict(min=int(iters.min()), median=float(np.median(iters)), p95=float(np.percentile(iters, 95)), max=int(iters.max()), mean=float(iters.mean())),
                ok_share=float(g["ok"].mean()), pairs_with_the_hosts_steps=float(same_steps.mean()),
                final_cost_rel_diff_median_where_steps_agree=float(np.median(rel[same_steps])) if same_steps.any() else None, guard_intact=bool(g["guard_intact"]))
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
