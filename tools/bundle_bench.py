#!/usr/bin/env python3
"""Room-scale timing of the reprojection kernels (K9; --kind angle2 / pixel: the two-row kinds of K31): F cameras on a trajectory, M points each seen by a
window of consecutive cameras (what SIFT tracks look like), N = sum of track lengths observations.
Prints wall times of pvlm_ba_reduce / step / cost (each includes its small host<->device copies).  Several --kind values
run in one process on the same scene, one JSON line each."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=454)          # Room: 454 frames
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--min-track", type=int, default=3)
    ap.add_argument("--max-track", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kind", default="angle1", help="comma-separated: angle1 (PanoramaReprojResidual_1Angle), angle2, pixel")
    ap.add_argument("--rows", type=int, default=3840)
    ap.add_argument("--cols", type=int, default=7680)
    args = ap.parse_args()
    import panovlm_amd as pv
    rng = np.random.default_rng(1)
    F, M = args.cams, args.points
    aa = rng.normal(size=(F, 3)) * 0.05
    t = np.stack([np.zeros(F), np.zeros(F), -0.1 * np.arange(F)], axis=1) + rng.normal(size=(F, 3)) * 0.01
    k = rng.integers(args.min_track, args.max_track + 1, size=M)
    first = rng.integers(0, np.maximum(F - k, 1))
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    cam = np.concatenate([np.arange(f, f + kk) for f, kk in zip(first, k)]).astype(np.int32)
    # points around the cameras that see them; bearings = true directions + noise
    centre = -t[np.minimum(first + k // 2, F - 1)]             # camera centres ~ -t for small rotations
    X = centre + rng.normal(size=(M, 3)) * np.array([2.0, 1.0, 2.0])
    pt = np.repeat(np.arange(M), k)
    pc = X[pt] + t[cam]                                        # R ~ I
    bearing = pc / np.linalg.norm(pc, axis=1, keepdims=True) + rng.normal(size=pc.shape) * 2e-3
    # two-row observations of the same points: keypoint pixels with 0.5 px noise, or the sphere angles of those pixels
    lon = np.arctan2(pc[:, 0], pc[:, 2]); lat = -np.arcsin(pc[:, 1] / np.linalg.norm(pc, axis=1))
    pix = np.stack([args.cols * (0.5 + lon / (2 * np.pi)), args.rows * (0.5 - lat / np.pi)], 1) + rng.normal(size=(len(pc), 2)) * 0.5
    sph = np.stack([(2 * pix[:, 0] / args.cols - 1) * np.pi, (0.5 - pix[:, 1] / args.rows) * np.pi], 1)
    ctx = pv.Context(0)
    ctx.set_poses(aa, t)
    for kind in args.kind.split(","):
        obs, a = {"angle1": (bearing, 4.0 * np.pi / 180.0), "angle2": (sph, 4.0 * np.pi / 180.0), "pixel": (pix, 4.0)}[kind]
        t0 = time.perf_counter()
        bs = pv.BundleSet(ctx, off, cam, obs, X, weight=1.0, kind=kind, rows=args.rows, cols=args.cols)
        t_create = time.perf_counter() - t0
        bs.reduce(pv.LOSS_HUBER, a, init_scale=True)
        res = {}
        for name, fn in (("reduce", lambda: bs.reduce(pv.LOSS_HUBER, a, radius=1e3)),
                         ("step", lambda: bs.step(np.full((bs.n_cams, 6), 1e-4), pv.LOSS_HUBER, a)),
                         ("cost", lambda: bs.cost(pv.LOSS_HUBER, a, candidate=True))):
            fn()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            res[name + "_ms"] = (time.perf_counter() - t0) / args.reps * 1e3
        print(json.dumps(dict(kind=kind, cams=F, points=M, observations=int(len(cam)), covisible_pairs=int(bs.n_upairs), packed_doubles=bs.size,
                              create_s=t_create, **res)), flush=True)
        bs.close()


if __name__ == "__main__":
    main()
