#!/usr/bin/env python3
"""Room-scale timing of K34: pvlm_filter_image_pairs on a synthetic pair list (--frames frames on a circle, every frame with its next --neighbours frames, --matches
matches per pair of which 30 % are gross outliers; a share --large of the pairs gets --large-matches matches, above N_LDS, so that the fall-back runs) with upstream's
40 runs of 300 iterations, against FilterImagePairsHost (the host compile of the core, tests/cpp/essential_core_check.cpp, on --threads threads) on a sample of pairs,
where the two must agree bit for bit.  Hypotheses per second, ms per pair and the share of fall-back chains.  No speed-up is promised: the line records what it is.
One JSON line, appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=454)
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--large", type=float, default=0.01)
    ap.add_argument("--large-matches", type=int, default=1500)
    ap.add_argument("--runs", type=int, default=40)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--threshold", type=int, default=20)
    ap.add_argument("--sample-host", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k34_essential_bench.jsonl"))
    args = ap.parse_args()
    import panovlm_amd as pv
    from tests import essential_ref as er
    rng = np.random.default_rng(1)
    pairs = [(i, j) for i in range(args.frames) for j in range(i + 1, min(i + 1 + args.neighbours, args.frames))]
    src = np.array([p[0] for p in pairs], np.int32); tgt = np.array([p[1] for p in pairs], np.int32)
    # every pair brings its own keypoints: frame f's bearings are the concatenation of what its pairs put there
    per_frame = [[] for _ in range(args.frames)]; rows = np.zeros(args.frames, np.int64); ms = []
    for (i, j) in pairs:
        n = args.large_matches if rng.random() < args.large else args.matches
        step = j - i
        b1, b2, m, _, _, _ = er.two_view_scene(rng, n, t=(0.3 * step, 0.05, -0.02 * step), w=(0.01, 0.03 * step, 0.0), shuffle=False)
        m["query"] += rows[i]; m["train"] += rows[j]
        per_frame[i].append(b1); per_frame[j].append(b2); rows[i] += n; rows[j] += n
        ms.append(m)
    bearings = [np.concatenate(b) if b else np.zeros((0, 3), np.float32) for b in per_frame]
    off = np.concatenate([[0], np.cumsum([len(m) for m in ms])]); m = np.concatenate(ms)
    ctx = pv.Context(0)
    pv.api.filter_image_pairs(ctx, bearings, src[:4], tgt[:4], off[:5], m[:off[4]], args.threshold, 2, 20, 1)              # warm-up
    t0 = time.perf_counter(); g = pv.api.filter_image_pairs(ctx, bearings, src, tgt, off, m, args.threshold, args.runs, args.iterations, 1); gpu_s = time.perf_counter() - t0
    sel = np.unique(np.concatenate([np.arange(min(args.sample_host // 2, len(src))), np.arange(max(len(src) - args.sample_host // 2, 0), len(src))]))
    hm = np.concatenate([ms[p] for p in sel]); hoff = np.concatenate([[0], np.cumsum([len(ms[p]) for p in sel])])
    chk = er.build_check()
    t0 = time.perf_counter(); rc, h = er.host_filter(chk, bearings, src[sel], tgt[sel], hoff, hm, args.threshold, args.runs, args.iterations, 1, threads=args.threads)
    host_s = time.perf_counter() - t0
    same = bool(rc == 0 and np.array_equal(h["keep"], g["keep"][sel]) and h["R_21"].tobytes() == g["R_21"][sel].tobytes() and h["t_21"].tobytes() == g["t_21"][sel].tobytes() and
                h["inlier_idx"].tobytes() == b"".join(g["inlier_idx"][g["offsets"][p]:g["offsets"][p + 1]].tobytes() for p in sel))
    st = g["stats"]
    line = dict(frames=args.frames, pairs=int(len(src)), matches=int(len(m)), runs=args.runs, iterations=args.iterations, gpu_s=gpu_s, gpu_ms_per_pair=1e3 * gpu_s / len(src),
                chains=int(st["chains"]), hypotheses=int(st["hypotheses"]), gpu_hypotheses_per_s=st["hypotheses"] / gpu_s, fallback_chains=int(st["fallback_chains"]),
                fallback_share=st["fallback_chains"] / max(st["chains"], 1), kept_pairs=int(g["keep"].sum()), host_threads=args.threads, host_pairs=int(len(sel)),
                host_ms_per_pair=1e3 * host_s / len(sel), host_hypotheses_per_s=h["hypotheses"] / host_s, host_equals_gpu=same)
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
