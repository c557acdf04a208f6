#!/usr/bin/env python3
"""Where does the plane-run form of the fused point-to-plane kernel start to pay?  Uploaded sets of about `--rows` rows whose planes repeat with a forced
mean run length L (1, 1.25, 1.5, 2); the same rows are uploaded under PVLM_PLANE_RUNS=0 and =1 and linearised in alternating rounds; prints one JSON line per
(L, form) with the fused kernel's own time per round (pvlm_profile_*), the median and the spread.  The point columns are the same for every L; the planes, and
with them the residuals, are not.  The threshold beside kPlaneRunsMinMean (csrc/pvlm_plane_runs.hip) is read off this table (profiles/plane_runs_ab.txt).

    python tools/plane_runs_sweep.py [--rows 50000000] [--pairs 32] [--reps 20] [--rounds 3]            # block form (long segments)
    python tools/plane_runs_sweep.py --pairs 12000 --wave-units 1                                      # wave form (4 k rows per pair)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATTERNS = {1.0: [1], 1.25: [1, 1, 1, 2], 1.5: [1, 2], 2.0: [2]}     # run lengths, repeated


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20, help="launches per round")
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per form, the two forms alternating")
    ap.add_argument("--lengths", type=float, nargs="+", default=sorted(PATTERNS), choices=sorted(PATTERNS))
    ap.add_argument("--wave-units", type=int, default=None, help="force the wave-per-chunk (1) or block-per-chunk (0) kernel")
    args = ap.parse_args()
    import panovlm_amd as pv
    from panovlm_amd import synthetic as sy
    F = 8
    rng = np.random.default_rng(3)
    per = args.rows // args.pairs // 16 * 16
    n = per * args.pairs
    off = np.arange(args.pairs + 1, dtype=np.int64) * per
    ref = (np.arange(args.pairs) % F).astype(np.int32); nei = ((ref + 1) % F).astype(np.int32)
    aa, t = (np.array(x) for x in zip(*[sy.pose_params(*sy.estimated_pose(k)) for k in range(F)]))
    rows = np.empty((n, 7))
    rows[:, :3] = rng.normal(size=(n, 3)) * 4.0
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    base = np.concatenate([nrm, (-(nrm * rows[:, :3]).sum(axis=1) + rng.choice([1e-3, 5e-3, 0.05], size=n))[:, None]], axis=1)
    del nrm
    if args.wave_units is not None:
        os.environ["PVLM_WAVE_UNITS"] = str(args.wave_units)
    ctx = pv.Context(0)
    ctx.set_poses(aa, t)
    ui = sorted(set((min(a, b), max(a, b)) for a, b in zip(ref.tolist(), nei.tolist())))
    neq = pv.NormalEq(ctx, F, [u[0] for u in ui], [u[1] for u in ui])
    packed = np.zeros(neq.size)
    def timed(rs):
        ctx.profile_enable(True)
        for _ in range(args.reps):
            neq.accumulate_async(rs, packed, pv.LOSS_HUBER, 2 * np.pi / 180)
        ctx.synchronize()
        ms, launches = ctx.profile_read(0)
        ctx.profile_enable(False)
        return ms / max(launches, 1)

    for L in args.lengths:
        pat = PATTERNS[L]
        lens = np.tile(np.array(pat), per // sum(pat) + 1)
        first = np.repeat(np.cumsum(lens) - lens, lens)[:per]                        # first row of the run of every row of a pair
        rows[:, 3:] = base.reshape(args.pairs, per, 4)[:, first, :].reshape(n, 4)
        sets, info = [], []
        for form in (0, 1):                                                          # both forms of the same rows live side by side
            os.environ["PVLM_PLANE_RUNS"] = str(form)
            m0 = ctx.mem_info()
            rs = pv.ResidualSet.upload(ctx, pv.POINT2PLANE_ANGLE, rows, off, ref, nei, flags=pv.FLAG_NORMALIZE_DISTANCE)
            sets.append(rs); info.append(ctx.mem_info()["in_use"] - m0["in_use"])
            for _ in range(3):
                neq.accumulate_async(rs, packed, pv.LOSS_HUBER, 2 * np.pi / 180)
            ctx.synchronize()
        ms = [[], []]
        sums = [None, None]
        for _ in range(args.rounds):                                                 # alternating: the spread of a form is the spread of its rounds
            for form in (0, 1):
                ms[form].append(timed(sets[form]))
                sums[form] = float(packed.sum())
        for form in (0, 1):
            st = sets[form].plane_runs()
            med = float(np.median(ms[form]))
            print(json.dumps({"forced_L": L, "plane_runs": form, "in_use": st["in_use"], "wave_units": args.wave_units, "pairs": args.pairs, "rows": n,
                              "runs": st["runs"], "fused_kernel_ms_rounds": ms[form], "fused_kernel_ms_median": med,
                              "spread_ms": max(ms[form]) - min(ms[form]), "launches_per_round": args.reps, "G_evals_per_s": n / med / 1e6,
                              "set_bytes": info[form], "packed_sum": sums[form]}), flush=True)
            sets[form].close()
    neq.close(); ctx.close()


if __name__ == "__main__":
    main()
