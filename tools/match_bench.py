#!/usr/bin/env python3
"""Room-scale timing of K33: pvlm_match_pairs on 454 frames of 8096 SIFT-like descriptors (integer values in 0..255; frame f + 1 repeats a third of frame f's rows
with a few components changed, so neighbouring frames have real matches), the contiguous pair list (every frame with its next --neighbours frames).  Fast mode runs
the whole list; exact mode (PVLM_FLAG_MATCH_EXACT) and the host loop (the host compile of the core, tests/cpp/match_core_check.cpp, 8-wide AVX2 FMA where the CPU has it, on --threads threads) run on a
sample of pairs, half from the head and half from the tail of the list, and must give the same records as fast mode there.  ms per pair, TFLOP/s of the 2 n1 n2 128 FLOP of a pair's distance matrix against the 157.3
fp32 matrix peak, and the fallback rate.  One JSON line, appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames(rng, F, n):
    out = [rng.integers(0, 256, size=(n, 128)).astype(np.float32)]
    for _ in range(1, F):
        d = rng.integers(0, 256, size=(n, 128)).astype(np.float32)
        k = n // 3
        rows = rng.choice(n, k, replace=False)
        d[rows] = out[-1][rng.choice(n, k, replace=False)]
        d[rows[:, None], rng.integers(0, 128, size=(k, 6))] += rng.integers(-20, 21, size=(k, 6)).astype(np.float32)
        out.append(np.clip(d, 0, 255))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=454)
    ap.add_argument("--rows", type=int, default=8096)
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--sample-exact", type=int, default=16)
    ap.add_argument("--sample-host", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--threshold", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k33_match_bench.jsonl"))
    args = ap.parse_args()
    import panovlm_amd as pv
    from tests import match_ref as ref
    rng = np.random.default_rng(1)
    descs = frames(rng, args.frames, args.rows)
    src = np.array([i for i in range(args.frames) for j in range(i + 1, min(i + 1 + args.neighbours, args.frames))], np.int32)
    tgt = np.array([j for i in range(args.frames) for j in range(i + 1, min(i + 1 + args.neighbours, args.frames))], np.int32)
    ctx = pv.Context(0)
    t0 = time.perf_counter(); ds = pv.api.DescSet(ctx, descs); create_s = time.perf_counter() - t0
    pv.api.match_pairs(ctx, ds, src[:8], tgt[:8], args.ratio, args.threshold)                      # warm-up
    t0 = time.perf_counter(); fast = pv.api.match_pairs(ctx, ds, src, tgt, args.ratio, args.threshold); fast_s = time.perf_counter() - t0
    def sample(n):                                                      # half from the head of the list, half from its tail (another batch of the fast run)
        n = min(n, len(src))
        return np.concatenate([np.arange(n // 2), np.arange(len(src) - (n - n // 2), len(src))])

    def fast_records(sel):
        return b"".join(fast["matches"][fast["offsets"][p]:fast["offsets"][p + 1]].tobytes() for p in sel)

    se = sample(args.sample_exact); ne = len(se)
    t0 = time.perf_counter(); exact = pv.api.match_pairs(ctx, ds, src[se], tgt[se], args.ratio, args.threshold, pv.api.FLAG_MATCH_EXACT); exact_s = time.perf_counter() - t0
    same_exact = bool(np.array_equal(exact["keep"], fast["keep"][se]) and exact["matches"].tobytes() == fast_records(se))
    sh = sample(args.sample_host); nh = len(sh)
    chk = ref.build_check()
    t0 = time.perf_counter(); rc, hkeep, hoff, hrec = ref.host_match_pairs(chk, descs, src[sh], tgt[sh], args.ratio, args.threshold, threads=args.threads)
    host_s = time.perf_counter() - t0
    same_host = bool(rc == 0 and np.array_equal(hkeep, fast["keep"][sh]) and hrec.tobytes() == fast_records(sh))
    flop_pair = 2.0 * args.rows * args.rows * 128
    line = dict(frames=args.frames, rows=args.rows, pairs=int(len(src)), descset_create_s=create_s, fast_s=fast_s, fast_ms_per_pair=1e3 * fast_s / len(src),
                fast_tflops=flop_pair * len(src) / fast_s / 1e12, fast_fraction_of_157_3=flop_pair * len(src) / fast_s / 157.3e12,
                queries=int(fast["stats"]["queries"]), fallback_queries=int(fast["stats"]["fallback_queries"]),
                fallback_rate=fast["stats"]["fallback_queries"] / max(fast["stats"]["queries"], 1), batches=int(fast["stats"]["batches"]),
                kept_pairs=int(fast["keep"].sum()), matches=int(fast["needed"]), exact_pairs=int(ne), exact_ms_per_pair=1e3 * exact_s / ne, exact_equals_fast=same_exact,
                host_threads=args.threads, host_pairs=int(nh), host_ms_per_pair=1e3 * host_s / nh, host_equals_fast=same_host)
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    ds.close(); ctx.close()


if __name__ == "__main__":
    main()
