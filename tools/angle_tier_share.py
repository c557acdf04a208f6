#!/usr/bin/env python3
"""Share of the evaluation slots of a bench-like point-to-plane set (64 scans x 8 neighbours, 4096 columns) whose 64 lanes all lie below a bound on the
angle: a slot is what a wave of k_eval_fused evaluates together, the rows of equal parity of 128 consecutive rows of a segment.  The bounds are those of
atan2_pos (pi/8), of two shorter polynomials (tan r <= 1/16, 1/32) and the Huber threshold of the bench (2 degrees: a slot of inliers only).
python tools/angle_tier_share.py   (one JSON line; profiles/eval_angle_form_ab.txt section 6)"""
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
for p in range(len(off) - 1):
    seg = r[off[p]:off[p + 1]]
    for h in (0, 1):
        x = seg[h::2]
        if len(x) == 0: continue
        n = (len(x) + 63) // 64
        pad = np.zeros(n * 64); pad[:len(x)] = x
        mx = pad.reshape(n, 64).max(1)
        slots += n
        for k, b in bounds.items():
            ok[k] += int((mx <= b).sum())
for k, b in bounds.items():
    rows_ok[k] = float((r <= b).mean())
out = {"rows": int(len(r)), "slots": slots, "live_rows": float((r > 0).mean()), "slot_share": {k: ok[k] / slots for k in bounds}, "row_share": rows_ok}
print(json.dumps(out))
rs.close(); ctx.close()
