#!/usr/bin/env python3
"""Timing of K48: pvlm_triplets_find and pvlm_triplets_filter at two sizes — Room (454 cameras, every camera with its next 19: 8 436 pairs) and Campus-Large (8 730
cameras, the same rule: about 1.6e5 pairs, 1.49 M triplets) — on the scenes of tools/transavg_bench.py.  Reported per size: the triplet count; seconds per call of
either entry (the median of --repeat calls after a warm-up call, wall clock around the ABI call on buffers made beforehand); the library's stage clocks
(PVLM_TRIPLET_PROFILE, one stderr line per call: rank / rows on the host by std::sort, upload, count, scan, emit, copy-out; every stage then ends in a wait, so
the profiled calls are timed apart from the plain ones); the 24 B per triplet written, against the emit kernel's time and against the device-to-host copy; the host
mirror's FindTriplet with TranslationAveragingL1's three `place` lookups per triplet and FilterByTriplet without its LargestBiconnectedGraph, on one thread in the
same run (tests/cpp/pvlm_triplet_driver.cpp, mode `bench`), with the host compile of the K48 core beside them; and n_uncertain.  No speed-up is promised: the line
records what it is.  Each size runs in a process of its own.  One JSON line per size, appended to --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"room": 454, "campus-large": 8730}


def host_walk(sc, threshold):
    """the driver's `bench` mode on the scene: the host mirror's one-thread clocks"""
    from panovlm_amd import build
    if not os.path.exists(build.TRIPLET_DRIVER):
        build.build_host()
    F = sc["F"]
    zero = " ".join(["0"] * 12)
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("%d\n" % F)
        f.write("".join("%d %s\n" % (i, zero) for i in range(F)))
        f.write("%d\n" % sc["P"])
        R = sc["R_21"].reshape(-1, 9)
        for p in range(sc["P"]):
            f.write("%d %d %s 0 0 0 0 0\n" % (sc["first"][p], sc["second"][p], " ".join(repr(float(v)) for v in R[p])))
        path = f.name
    try:
        res = subprocess.run([build.TRIPLET_DRIVER, "bench", "host", path, repr(float(threshold))], capture_output=True, text=True, timeout=600)
    finally:
        os.unlink(path)
    got = [ln for ln in res.stdout.splitlines() if ln.startswith("bench ")]
    if res.returncode != 0 or not got:
        raise SystemExit("the host walk failed (exit %d): %s" % (res.returncode, res.stderr[-2000:]))
    return json.loads(got[-1][len("bench "):])


def worker(size, reach, repeat, threshold):
    import panovlm_amd as pv
    from panovlm_amd import api
    from tools import transavg_bench
    sc = transavg_bench.make_scene(SIZES[size], reach, 1)
    F, P = sc["F"], sc["P"]
    first = np.ascontiguousarray(sc["first"], np.int32); second = np.ascontiguousarray(sc["second"], np.int32)
    R = np.ascontiguousarray(sc["R_21"].reshape(-1, 9))
    ctx = pv.Context(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    sizing = api.triplets_find(ctx, F, first, second, want_triplets=False, want_pairs=False)          # warm-up: the code object, the pool
    T = int(sizing["needed"])
    trip = np.zeros((T + 1, 3), np.int32); tp = np.zeros((T + 1, 3), np.int32); counts = np.zeros(P, np.int64); needed = C.c_longlong(0)
    keep = np.zeros(P, np.uint8); st = api.TripletStats(0, 0, 0, 0)

    def find():
        t0 = time.perf_counter()
        rc = ctx.lib.pvlm_triplets_find(ctx._h, C.c_int(F), C.c_int(P), ptr(first), ptr(second), ptr(trip), ptr(tp), C.c_longlong(T), C.byref(needed), ptr(counts))
        dt = time.perf_counter() - t0
        assert rc == 0 and needed.value == T
        return dt

    def filt():
        t0 = time.perf_counter()
        rc = ctx.lib.pvlm_triplets_filter(ctx._h, C.c_int(F), C.c_int(P), ptr(first), ptr(second), ptr(R), C.c_double(threshold), ptr(keep), C.byref(st))
        dt = time.perf_counter() - t0
        assert rc == 0 and st.n_triplets == T
        return dt
    find(); filt()
    find_s = [find() for _ in range(max(repeat, 1))]
    filter_s = [filt() for _ in range(max(repeat, 1))]
    os.environ["PVLM_TRIPLET_PROFILE"] = "1"
    for _ in range(max(repeat, 1)):
        find(); filt()
    del os.environ["PVLM_TRIPLET_PROFILE"]
    ctx.close()
    line = dict(size=size, cameras=F, pairs=P, triplets=T, threshold_deg=threshold, find_s=float(np.median(find_s)), find_s_all=find_s, filter_s=float(np.median(filter_s)),
                filter_s_all=filter_s, bytes_written=24 * T, n_kept_triplets=int(st.n_kept_triplets), n_uncertain=int(st.n_uncertain), n_kept_pairs=int(st.n_kept_pairs),
                sort="host std::sort in the call's set-up")
    line.update(host_walk(sc, threshold))
    line["host_find_with_place_s"] = line["host_find_triplet_s"] + line["host_place_lookups_s"]
    line["host_find_with_place_over_find"] = line["host_find_with_place_s"] / line["find_s"]
    line["host_filter_over_filter"] = line["host_filter_without_biconnected_s"] / line["filter_s"]
    print("triplet_bench_result " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="room,campus-large")
    ap.add_argument("--neighbours", type=int, default=19)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.1, help="degrees: EstimateGlobalRotation's")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per size")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k48_triplet_bench.jsonl"))
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.neighbours, args.repeat, args.threshold)
        return
    for size in [s for s in args.sizes.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", size, "--neighbours", str(args.neighbours), "--repeat", str(args.repeat), "--threshold", str(args.threshold)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            line = dict(size=size, cameras=SIZES[size], failed="no result within %d s" % args.timeout)
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            break                                     # nothing more is started on the device behind a call that did not come back
        got = [ln for ln in res.stdout.splitlines() if ln.startswith("triplet_bench_result ")]
        if res.returncode != 0 or not got:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("the %s run failed (exit %d)" % (size, res.returncode))
        line = json.loads(got[-1][len("triplet_bench_result "):])
        prof = [json.loads(ln[len("pvlm_triplet_profile "):]) for ln in res.stderr.splitlines() if ln.startswith("pvlm_triplet_profile ")]
        for entry, keys in (("find", ("total_ms", "rows_ms", "upload_ms", "count_ms", "scan_ms", "emit_ms", "copy_out_ms")),
                            ("filter", ("total_ms", "rows_ms", "upload_ms", "filter_ms", "copy_out_ms"))):
            mine = [p for p in prof if p["entry"] == entry]
            if mine:
                line[entry + "_stage_ms"] = {k: float(np.median([p[k] for p in mine])) for k in keys}
                if entry == "filter":
                    line["filter_passes"] = int(mine[-1]["passes"])
        if "find_stage_ms" in line and line["triplets"]:
            s = line["find_stage_ms"]
            line["emit_gb_per_s"] = line["bytes_written"] / (s["emit_ms"] * 1e-3) / 1e9 if s["emit_ms"] > 0 else None
            line["copy_out_gb_per_s"] = line["bytes_written"] / (s["copy_out_ms"] * 1e-3) / 1e9 if s["copy_out_ms"] > 0 else None
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
