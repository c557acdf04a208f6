#!/usr/bin/env python3
"""Room-scale timing of K35: the VLAD retrieval of SfM::InitImagePairs on 454 frames of 8096 SIFT-like descriptors (tools/match_bench.py's generator): the k-means
codebook over half the frames (128 words, up to 25 passes), the embedding of every frame (type 2) and 15 neighbours per frame, in fast mode and in exact mode
(PVLM_FLAG_MATCH_EXACT), which must give the same bits.  The host loops (the host compile of the core, tests/cpp/vlad_core_check.cpp, on --threads threads) are timed
on a sample: ONE k-means pass over the training rows and the embedding of --sample-frames frames, and must agree with the device there.  ms for the codebook (in all and
per pass), the embedding and the neighbours, and the fast mode's fallback share.  One JSON line, appended to --out."""
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
    ap.add_argument("--rows", type=int, default=8096)
    ap.add_argument("--ratio", type=float, default=0.5)
    ap.add_argument("--book-size", type=int, default=128)
    ap.add_argument("--iterations", type=int, default=25)
    ap.add_argument("--neighbours", type=int, default=15)
    ap.add_argument("--sample-frames", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k35_vlad_bench.jsonl"))
    args = ap.parse_args()
    import panovlm_amd as pv
    from tests import vlad_ref as ref
    from tools.match_bench import frames as make_frames
    rng = np.random.default_rng(1)
    descs = make_frames(rng, args.frames, args.rows)
    train = rng.choice(args.frames, int(args.ratio * args.frames), replace=False).astype(np.int32)
    n_train = int(len(train)) * args.rows
    init = rng.choice(n_train, args.book_size, replace=False).astype(np.int64)
    ctx = pv.Context(0)
    ds = pv.api.DescSet(ctx, descs)
    pv.api.vlad_kmeans(ctx, ds, train[:2], args.book_size, 1, init % (2 * args.rows))                 # warm-up
    res = {}
    for name, flags in (("fast", 0), ("exact", pv.api.FLAG_MATCH_EXACT)):
        t0 = time.perf_counter(); cb, alive, assign, kst = pv.api.vlad_kmeans(ctx, ds, train, args.book_size, args.iterations, init, flags); k_s = time.perf_counter() - t0
        t0 = time.perf_counter(); vs = pv.api.vlad_embed(ctx, ds, cb, alive, 2, flags); e_s = time.perf_counter() - t0
        t0 = time.perf_counter(); nb, _ = pv.api.vlad_neighbors(ctx, vs, args.neighbours); n_s = time.perf_counter() - t0
        res[name] = dict(cb=cb, alive=alive, assign=assign, V=vs.read(), nb=nb, kst=kst, est=vs.stats, k_s=k_s, e_s=e_s, n_s=n_s)
        vs.close()
    f, e = res["fast"], res["exact"]
    same_exact = bool(f["cb"].tobytes() == e["cb"].tobytes() and np.array_equal(f["alive"], e["alive"]) and np.array_equal(f["assign"], e["assign"])
                      and f["V"].tobytes() == e["V"].tobytes() and np.array_equal(f["nb"], e["nb"]))
    # the host loops on a sample: one pass from the initial centres, and the embedding of the first --sample-frames frames with the device's codebook
    chk = ref.build_check()
    cb1, alive1, assign1, _ = pv.api.vlad_kmeans(ctx, ds, train, args.book_size, 1, init)
    t0 = time.perf_counter(); rc, hcb, halive, hassign, _, _ = ref.host_kmeans(chk, descs, train, args.book_size, 1, init, threads=args.threads); hk_s = time.perf_counter() - t0
    same_host = bool(rc == 0 and hcb.tobytes() == cb1.tobytes() and np.array_equal(halive, alive1) and np.array_equal(hassign, assign1))
    ns = min(args.sample_frames, args.frames)
    t0 = time.perf_counter(); rc, hV = ref.host_embed(chk, descs[:ns], f["cb"], f["alive"], 2, threads=args.threads); he_s = time.perf_counter() - t0
    same_host = bool(same_host and rc == 0 and hV.tobytes() == f["V"][:ns].tobytes())
    line = dict(frames=args.frames, rows=args.rows, train_rows=n_train, book_size=args.book_size, neighbours=args.neighbours)
    for name in ("fast", "exact"):
        r = res[name]
        line.update({name + "_codebook_ms": 1e3 * r["k_s"], name + "_iterations": r["kst"]["iterations"], name + "_ms_per_iteration": 1e3 * r["k_s"] / max(r["kst"]["iterations"], 1),
                     name + "_embed_ms": 1e3 * r["e_s"], name + "_neighbours_ms": 1e3 * r["n_s"]})
    line.update(dead_centres=f["kst"]["dead_centres"], kmeans_fallback_share=f["kst"]["fallback_queries"] / max(f["kst"]["queries"], 1),
                embed_fallback_share=f["est"]["fallback_queries"] / max(f["est"]["queries"], 1), exact_equals_fast=same_exact, host_threads=args.threads,
                host_ms_per_iteration=1e3 * hk_s, host_embed_frames=ns, host_embed_ms_per_frame=1e3 * he_s / ns, host_equals_device=same_host)
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as out:
        out.write(json.dumps(line) + "\n")
    ds.close(); ctx.close()
    if not (same_exact and same_host):
        sys.exit(1)


if __name__ == "__main__":
    main()
