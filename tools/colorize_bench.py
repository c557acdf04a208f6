"""K30 (the coloured LiDAR map, Texture::ColorizeLidarPointCloud(1.5, 35)) at Room (454 pairs) and Floor (1593 pairs) size with 5760 x 2880 frames, on synthetic raw
VLP-16 scans (synthetic.raw_vlp16_scan; pair k's cloud is a copy, in memory of its own, of one of 8 generated scans) and frames drawn from a POOL of at most 16
distinct synthetic images (a sky band over the top third, a pattern below) — pair k uses image k % pool.  Per configuration, one JSON line:
  host_call   pvlm_colorize_scans from C++ (tests/cpp/pvlm_texture_driver.cpp `texbench`): wall per call (best / median), its host-link roof (16 B up + 4 B down
              + 4 B up per point, 16 B down per kept point at the measured link rate), the host gather's wall and thread milliseconds (PVLM_COLORIZE_PROFILE),
              and a plain C++ restatement of upstream's per-pair loop on 1 and 16 threads in two forms: HSV of the whole image first (cvtColor, as upstream)
              and HSV at the hit pixels only (the fair comparison).  The whole-image form on 1 thread is timed on 16 pairs and scaled to the set.
  dev_call    pvlm_colorize_scans_dev on device tensors: HIP-event time per call (torch events on the call's stream; the Python marshalling included).
Kernel times and their fraction of HBM: run --dev-only under `rocprofv3 --kernel-trace --output-format csv`, then
  python tools/colorize_bench.py --summarize-trace <..._kernel_trace.csv> --bench-lines <the JSON lines>
(bytes: 16 B read per point, 4 B word written and read again, 16 B read + 16 B written per kept point, and a 128-byte cache line per image read).
  python tools/colorize_bench.py [--configs room,floor] [--reps 3] [--dev-only] [--pool 16]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

LINK_GBPS = 55.7        # host link, measured (bench.py PEAKS)
HBM_GBPS = 8000.0       # MI355X HBM3E spec peak (bench.py HBM_PEAK_GBPS)
LINE = 128              # bytes an image read pulls through L2
CONFIGS = {"room": 454, "floor": 1593}
ROWS, COLS = 2880, 5760
T_CL = np.array([0.9998, -0.0175, 0.0087, 0.12, 0.0174, 0.9998, 0.0052, -0.05, -0.0088, -0.0050, 0.9999, 0.21])


def base_scans(n=8):
    from panovlm_amd import synthetic as sy
    out = []
    for k in range(n):
        R, t = sy.estimated_pose(k % 16)
        out.append(dict(id=k, R_wl=R, t_wl=t, raw=sy.raw_vlp16_scan(k, cols=1800, clutter=40)))
    return out


def pool_images(n):
    """The driver's synthetic frames (texbench), restated for the device run."""
    r = np.arange(ROWS, dtype=np.int64)[:, None]; c = np.arange(COLS, dtype=np.int64)[None, :]
    out = []
    for i in range(n):
        im = np.empty((ROWS, COLS, 3), np.uint8)
        im[..., 0] = (r * 7 + c * 3 + 11 * i) & 255
        im[..., 1] = ((r * 3) ^ (c * 5 + i * 17)) & 255
        im[..., 2] = (c + 2 * r + 31 * i) & 255
        im[: ROWS // 3] = (235, 180, 120)
        out.append(im)
    return out


def host_call(raw_path, n_pairs, pool, reps):
    from panovlm_amd import build
    build.build_host()
    env = dict(os.environ, PVLM_COLORIZE_PROFILE="1")
    p = subprocess.run([build.TEXTURE_DRIVER, "texbench", raw_path, str(n_pairs), str(pool), str(ROWS), str(COLS), str(reps)], capture_output=True, text=True,
                       timeout=3000, env=env)
    if p.returncode != 0:
        raise RuntimeError(p.stderr[-2000:])
    kv = {}
    for line in p.stdout.splitlines():
        k, v = line.split()
        kv[k] = float(v) if "." in v else int(v)
    prof = [l.split() for l in p.stderr.splitlines() if l.startswith("colorize_profile")]
    if prof:
        g = [dict(zip(x[1::2], map(float, x[2::2]))) for x in prof[1:]]      # the timed calls (the first is the warm-up)
        kv["gather_wall_ms_median"] = float(np.median([x["gather_wall_ms"] for x in g]))
        kv["gather_thread_ms_median"] = float(np.median([x["gather_thread_ms"] for x in g]))
        kv["pieces"] = int(g[0]["pieces"])
    bytes_ = 24 * kv["points"] + 16 * kv["kept"]
    roof_ms = bytes_ / (LINK_GBPS * 1e9) * 1e3
    kv["link_roof"] = {"bound": "host link: 16 B up + 4 B down + 4 B up per point, 16 B down per kept point", "GBps": LINK_GBPS, "ms_at_link_rate": roof_ms,
                       "frac": roof_ms / kv["device_call_best_ms"]}
    kv["host_hit_pixels_16_threads_over_device_call"] = kv["host_hit_pixels_16threads_ms"] / kv["device_call_best_ms"]
    kv["host_whole_image_16_threads_over_device_call"] = kv["host_whole_image_16threads_ms"] / kv["device_call_best_ms"]
    return kv


def dev_call(base, n_pairs, pool, reps):
    import torch
    import panovlm_amd as pv
    from panovlm_amd import api
    dev = torch.device("cuda", 0)
    sizes = [len(base[k % len(base)]["raw"]) for k in range(n_pairs)]
    big = torch.empty((sum(sizes), 4), dtype=torch.float32, device=dev)       # every pair's cloud in memory of its own
    tens, at = [], 0
    for k, n in enumerate(sizes):
        v = big[at:at + n]; v.copy_(torch.from_numpy(base[k % len(base)]["raw"])); tens.append(v); at += n
    imgs = [torch.from_numpy(im).to(dev) for im in pool_images(pool)]
    images = [imgs[k % pool] for k in range(n_pairs)]
    Ts = [T_CL] * n_pairs
    ctx = pv.Context(0)
    out = torch.empty_like(big)
    api.colorize_scans_dev(ctx, tens, Ts, images, 1.5, 35.0, out=out)           # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, _, n = api.colorize_scans_dev(ctx, tens, Ts, images, 1.5, 35.0, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    kept = int(n.item())
    ctx.close()
    return {"pairs": n_pairs, "points_in": int(big.shape[0]), "points_kept": kept, "call_event_ms_best": min(ms), "call_event_ms_median": sorted(ms)[len(ms) // 2],
            "includes": "the Python wrapper's descriptor marshalling, descriptor staging, the three kernels; torch events on the call's stream"}


def summarize_trace(trace_csv, bench_lines):
    """One CSV row per --dev-only configuration: median kernel times of the timed calls and their fraction of HBM peak."""
    import csv
    runs = [json.loads(l) for l in open(bench_lines) if l.startswith("{") and '"config"' in l]
    calls, cur = [], {}
    names = ("k_tex_word_dev", "k_tex_scan", "k_tex_scatter")
    for r in csv.DictReader(open(trace_csv)):
        for k in names:
            # the scan is pvlm_compact::k_tile_scan<PairDesc> (k_tex_scan in traces recorded before the compaction was shared)
            if k + "(" in r["Kernel_Name"] or (k == "k_tex_scan" and "k_tile_scan<" in r["Kernel_Name"]):
                cur[k] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                if k == "k_tex_scatter":
                    calls.append(cur); cur = {}
    at = 0
    print("config,points_in,points_kept,calls,word_us,scan_us,scatter_us,total_us,bytes_streams,bytes_with_lines,frac_hbm_streams,frac_hbm_with_lines")
    for run in runs:
        d = run["dev_call"]
        n_calls = 1 + int(run.get("reps", 0))
        timed = calls[at + 1:at + n_calls]
        at += n_calls
        med = {k: float(np.median([c[k] for c in timed])) for k in names}
        total = sum(med.values())
        # streams: the clouds, the words and the records; with lines: plus one 128-byte line per kept point's image read (each read counted as the line it
        # pulls, as if no two points shared one — neighbouring points of a ring hit neighbouring pixels, so above 1 means the lines come from the caches)
        streams = (16 + 4 + 4) * d["points_in"] + (16 + 16) * d["points_kept"]
        lines = streams + LINE * d["points_kept"]
        bw = (total * 1e-6) * (HBM_GBPS * 1e9)
        print("%s,%d,%d,%d,%.1f,%.1f,%.1f,%.1f,%d,%d,%.3f,%.3f" % (run["config"], d["points_in"], d["points_kept"], len(timed), med[names[0]], med[names[1]],
                                                                med[names[2]], total, streams, lines, streams / bw, lines / bw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pool", type=int, default=16)
    ap.add_argument("--dev-only", action="store_true")
    ap.add_argument("--summarize-trace", default=None)
    ap.add_argument("--bench-lines", default=None)
    a = ap.parse_args()
    if a.summarize_trace:
        summarize_trace(a.summarize_trace, a.bench_lines)
        return
    pool = max(1, min(a.pool, 16))
    t0 = time.time()
    base = base_scans()
    print(json.dumps({"note": "synthetic data: %d distinct %d x %d frames drawn in turn by the pairs; 8 distinct raw VLP-16 scans copied per pair" % (pool, COLS, ROWS)}),
          flush=True)
    with tempfile.TemporaryDirectory() as d:
        raw = os.path.join(d, "raw.bin")
        if not a.dev_only:
            from tests import host_io
            host_io.write_raw_scans(raw, base)
        for name in a.configs.split(","):
            n_pairs = CONFIGS[name]
            rec = {"config": name, "pairs": n_pairs, "rows": ROWS, "cols": COLS, "image_pool": pool, "min_dist": 1.5, "max_dist": 35.0, "reps": a.reps}
            if not a.dev_only:
                rec["host_call"] = host_call(raw, n_pairs, pool, a.reps)
            rec["dev_call"] = dev_call(base, n_pairs, pool, a.reps)
            print(json.dumps(rec), flush=True)
    print(json.dumps({"seconds": time.time() - t0}))


if __name__ == "__main__":
    main()
