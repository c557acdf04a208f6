#!/usr/bin/env python3
"""Share of the evaluation slots of a bench-like point-to-plane set (64 scans x 8 neighbours, 4096 columns) whose 64 lanes all lie below a bound on the
angle: a slot is what a wave of k_eval_fused evaluates together, 64 consecutive rows: one half of the 128 consecutive rows of a wave's trip.  The bounds are those of
atan2_pos (pi/8), of two shorter polynomials (tan r <= 1/16, 1/32) and the Huber threshold of the bench (2 degrees: a slot of inliers only).
"pair_share": the same per PAIR of slots, the two halves of one group of 128 rows — what one wave does in one trip of the row loop; which
combination of tiers (short: both below 1/32 ... octant: a row above pi/8) and of Huber paths the two slots of a trip take, and the trips whose second half
is empty ("half tail": a segment end in the first half).  Before the dense half-trips a slot was the rows of equal parity of the 128 (the figures of
profiles/eval_angle_form_ab.txt section 6 and profiles/eval_row_pairs_ab.txt are of that definition).
python tools/angle_tier_share.py   (one JSON line; profiles/eval_half_trips_ab.txt)"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench
from panovlm_amd import synthetic as sy, sharding
F, nb, cols = 64, 8, 4096
ref, nei = sy.pair_list(F, nb)
scans = bench.generate_scans(sorted(set(ref.tolist()) | set(nei.tolist())), cols, 0.2)
import panovlm_amd as pv
ctx = pv.Context(0)
ds = dict(zip(sorted(scans), pv.Scan.upload_batch(ctx, [scans[k] for k in sorted(scans)])))
rs = ctx.assoc_point2plane([ds[int(r)] for r in ref], [ds[int(n)] for n in nei], 0.05, 1.0, kind=pv.POINT2PLANE_ANGLE, flags=pv.FLAG_NORMALIZE_DISTANCE, weight=1.0)
poses = [sy.pose_params(*sy.estimated_pose(k)) for k in range(F)]
ctx.set_poses(np.array([p[0] for p in poses]), np.array([p[1] for p in poses]))
r, _ = rs.eval(jac=False)
off = rs.download()[0]
r = np.abs(np.asarray(r))
bounds = {"pi/8": np.pi / 8, "1/16": np.arctan(1 / 16), "1/32": np.arctan(1 / 32), "huber 2 deg (all inliers)": 2 * np.pi / 180}
slots = 0; ok = {k: 0 for k in bounds}; rows_ok = {k: 0 for k in bounds}
t32, t8, hub = np.arctan(1 / 32), np.pi / 8, 2 * np.pi / 180
trips = 0; pair = {k: 0 for k in ("short/short", "full/full", "short/full", "full/short", "an octant slot", "half tail")}; pair_huber = {"inliers/inliers": 0, "an outlier slot": 0}
for p in range(len(off) - 1):
    seg = r[off[p]:off[p + 1]]
    n = (len(seg) + 63) // 64
    if n:
        pad = np.zeros(n * 64); pad[:len(seg)] = seg
        mx = pad.reshape(n, 64).max(1)
        slots += n
        for k, b in bounds.items():
            ok[k] += int((mx <= b).sum())
    # slot pairs: the groups of 128 rows of the segment; a tail group of at most 64 rows has no second slot
    n = (len(seg) + 127) // 128
    if n:
        pad = np.zeros(n * 128); pad[:len(seg)] = seg
        mx = pad.reshape(n, 2, 64).max(2)              # [group, half]
        tier = np.where(mx <= t32, 0, np.where(mx <= t8, 1, 2))
        odd = np.zeros(n, bool); odd[-1] = 0 < len(seg) % 128 <= 64
        trips += n
        pair["half tail"] += int(odd.sum())
        pair["an octant slot"] += int(((tier.max(1) == 2) & ~odd).sum())
        for name, a, b in (("short/short", 0, 0), ("full/full", 1, 1), ("short/full", 0, 1), ("full/short", 1, 0)):
            pair[name] += int(((tier[:, 0] == a) & (tier[:, 1] == b) & ~odd).sum())
        pair_huber["inliers/inliers"] += int((mx.max(1) <= hub).sum())
        pair_huber["an outlier slot"] += int((mx.max(1) > hub).sum())
for k, b in bounds.items():
    rows_ok[k] = float((r <= b).mean())
out = {"rows": int(len(r)), "slots": slots, "live_rows": float((r > 0).mean()), "slot_share": {k: ok[k] / slots for k in bounds}, "row_share": rows_ok,
       "trips": trips, "pair_share": {k: v / trips for k, v in pair.items()}, "pair_huber_share": {k: v / trips for k, v in pair_huber.items()}}
print(json.dumps(out))
rs.close(); ctx.close()
