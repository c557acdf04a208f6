"""K29 (the fused LiDAR map, LidarOdometry::FuseLidar(skip, 0, max_range)) at Room (454 scans) and Floor (1593 scans) size, skip 4 and skip 0, on synthetic raw
VLP-16 scans (synthetic.raw_vlp16_scan; scan k of a batch is a copy, in memory of its own, of one of 8 generated scans, with its own pose).  Per configuration,
one JSON line:
  host_call      pvlm_fuse_scans from C++ (tests/cpp/pvlm_fuse_driver.cpp `fusebench`): wall per call into a caller buffer reused across calls (best / median) and
                 into a fresh buffer per call, the host-link roof (16 B up per input point + 16 B down per kept point at the measured link rate) and its
                 fraction, the plain C++ restatement of upstream's loop on 1 and on 16 threads and LidarOdometry::FuseLidar of the host mirror (both with a
                 fresh result per call, as upstream returns one)
  dev_call       pvlm_fuse_scans_dev on device tensors: HIP-event time per call (torch events on the call's stream).  The GPU waits while the Python
                 wrapper marshals the descriptors, so this is a call time, not a kernel time: the kernel times come from a trace (below)
The synthetic scans lie within 40 m (every point kept: a dense copy); the *_near configurations (max_range 4 m, ~55 % kept) measure the compaction.
Kernel times and their fraction of HBM: run --dev-only under `rocprofv3 --kernel-trace --output-format csv`, keep its JSON lines, then
  python tools/fuse_bench.py --summarize-trace <..._kernel_trace.csv> --bench-lines <the JSON lines>
which attributes the kernels to the configurations in dispatch order (one warm-up call + --reps calls each) and prints one CSV row per configuration
(profiles/k29_fuse_kernels.csv was made so from profiles/k29_fuse_kernel_trace.csv and profiles/k29_fuse_dev_calls.jsonl).
  python tools/fuse_bench.py [--configs room4,room0,floor4,floor0,floor4_near,floor0_near] [--reps 5] [--dev-only]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LINK_GBPS = 55.7        # host link, measured (bench.py PEAKS)
HBM_GBPS = 8000.0       # MI355X HBM3E spec peak (bench.py HBM_PEAK_GBPS); 6290 GB/s measured with a float4 copy
CONFIGS = {"room4": (454, 4, 40.0), "room0": (454, 0, 40.0), "floor4": (1593, 4, 40.0), "floor0": (1593, 0, 40.0),
           "floor4_near": (1593, 4, 4.0), "floor0_near": (1593, 0, 4.0)}
MIN_RANGE = 0.0


def base_scans(n=8):
    from panovlm_amd import synthetic as sy
    out = []
    for k in range(n):
        R, t = sy.estimated_pose(k % 16)
        out.append(dict(id=k, R_wl=R, t_wl=t, raw=sy.raw_vlp16_scan(k, cols=1800, clutter=40)))
    return out


def host_call(raw_path, n_scans, skip, max_range, reps):
    from tests import fuse_ref
    out = fuse_ref.run("fusebench", raw_path, n_scans, skip, repr(MIN_RANGE), repr(max_range), reps, timeout=1800).stdout
    kv = {}
    for line in out.splitlines():
        k, v = line.split()
        kv[k] = float(v) if "." in v else int(v)
    bytes_ = 16 * kv["points_in"] + 16 * kv["points_kept"]
    roof_ms = bytes_ / (LINK_GBPS * 1e9) * 1e3
    kv["link_roof"] = {"bound": "host link, 16 B up per input point + 16 B down per kept point", "GBps": LINK_GBPS, "ms_at_link_rate": roof_ms,
                       "frac": roof_ms / kv["device_call_best_ms"]}
    kv["host_16_threads_over_device_call"] = kv["host_16_threads_ms"] / kv["device_call_best_ms"]
    return kv


def dev_call(base, n_scans, skip, max_range, reps):
    import torch
    import panovlm_amd as pv
    from panovlm_amd import api
    dev = torch.device("cuda", 0)
    idx = list(range(0, n_scans, skip + 1))
    sizes = [len(base[i % len(base)]["raw"]) for i in idx]
    big = torch.empty((sum(sizes), 4), dtype=torch.float32, device=dev)       # every scan in memory of its own (no cache reuse between copies)
    tens, at = [], 0
    for i, n in zip(idx, sizes):
        v = big[at:at + n]; v.copy_(torch.from_numpy(base[i % len(base)]["raw"])); tens.append(v); at += n
    poses = [(base[i % len(base)]["R_wl"], base[i % len(base)]["t_wl"]) for i in idx]
    ctx = pv.Context(0)
    out = torch.empty_like(big)
    api.fuse_scans_dev(ctx, tens, poses, MIN_RANGE, max_range, out=out)      # warm-up: code objects, pool
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, _, n = api.fuse_scans_dev(ctx, tens, poses, MIN_RANGE, max_range, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    kept = int(n.item())
    ctx.close()
    return {"scans": len(idx), "points_in": int(big.shape[0]), "points_kept": kept, "call_event_ms_best": min(ms), "call_event_ms_median": sorted(ms)[len(ms) // 2],
            "includes": "the Python wrapper's descriptor marshalling (the GPU waits for it), descriptor staging, the three kernels; torch events on the call's stream"}


def summarize_trace(trace_csv, bench_lines):
    """One CSV row per --dev-only configuration: median kernel times of the timed calls and their fraction of HBM (algorithmic: 16 B read per input point +
    16 B written per kept point; moved: the count pass reads every point a second time)."""
    import csv
    runs = [json.loads(l) for l in open(bench_lines) if l.startswith("{") and '"config"' in l]
    calls, cur = [], {}
    for r in csv.DictReader(open(trace_csv)):
        name = r["Kernel_Name"]
        for k in ("k_fuse_count", "k_fuse_scan", "k_fuse_scatter"):
            # the scan is pvlm_compact::k_tile_scan<ScanDesc> (k_fuse_scan in traces recorded before the compaction was shared)
            if k + "(" in name or (k == "k_fuse_scan" and "k_tile_scan<" in name):
                cur[k] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                if k == "k_fuse_scatter":
                    calls.append(cur); cur = {}
    at = 0
    print("config,points_in,points_kept,calls,count_us,scan_us,scatter_us,total_us,frac_hbm_algorithmic,frac_hbm_moved")
    for run in runs:
        d = run["dev_call"]
        n_calls = 1 + int(run.get("reps", 0))
        timed = calls[at + 1:at + n_calls]
        at += n_calls
        med = {k: float(np.median([c[k] for c in timed])) for k in ("k_fuse_count", "k_fuse_scan", "k_fuse_scatter")}
        total = sum(med.values())
        alg, moved = 16 * d["points_in"] + 16 * d["points_kept"], 32 * d["points_in"] + 16 * d["points_kept"]
        print("%s,%d,%d,%d,%.1f,%.1f,%.1f,%.1f,%.3f,%.3f" % (run["config"], d["points_in"], d["points_kept"], len(timed), med["k_fuse_count"], med["k_fuse_scan"],
                                                          med["k_fuse_scatter"], total, alg / (total * 1e-6) / (HBM_GBPS * 1e9), moved / (total * 1e-6) / (HBM_GBPS * 1e9)))
    assert at == len(calls), "the trace holds %d calls, the bench lines account for %d" % (len(calls), at)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dev-only", action="store_true")
    ap.add_argument("--summarize-trace", default=None, help="a rocprofv3 kernel_trace.csv of a --dev-only run")
    ap.add_argument("--bench-lines", default=None, help="the JSON lines that run printed")
    a = ap.parse_args()
    if a.summarize_trace:
        summarize_trace(a.summarize_trace, a.bench_lines)
        return
    t0 = time.time()
    base = base_scans()
    with tempfile.TemporaryDirectory() as d:
        raw = os.path.join(d, "raw.bin")
        if not a.dev_only:
            from tests import host_io
            host_io.write_raw_scans(raw, base)
        for name in a.configs.split(","):
            n_scans, skip, max_range = CONFIGS[name]
            rec = {"config": name, "scans_in_set": n_scans, "skip": skip, "min_range": MIN_RANGE, "max_range": max_range, "reps": a.reps}
            if not a.dev_only:
                rec["host_call"] = host_call(raw, n_scans, skip, max_range, a.reps)
            rec["dev_call"] = dev_call(base, n_scans, skip, max_range, a.reps)
            print(json.dumps(rec), flush=True)
    print(json.dumps({"seconds": time.time() - t0}))


if __name__ == "__main__":
    main()
