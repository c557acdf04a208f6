#!/usr/bin/env python3
"""Timing of K49: pvlm_mvs_select_neighbors_sfm at two sizes — Room (454 views) and Campus-Large (8 730 views).

The scene is synthetic.  The views stand a metre apart along a serpentine path (rows of 60, 1.5 m between rows), each with a random rotation.  Every view anchors
--tracks-per-view tracks (default 300, so a view lies in about 1 470 of them: 2.6 M tracks and 6.2e7 contributions at Campus-Large); a track is seen by L views drawn without repetition from the 24 views that follow its
anchor on the path, with the length distribution
    L        3     4     5     6     7     8     9     10
    P(L)   0.30  0.22  0.15  0.11  0.08  0.06  0.05  0.03        (mean 5.0 views, 23.8 contributions a track)
and its point lies 4 to 30 m off the mean of its views' centres in a random direction.  No track repeats a view.

Reported per size: tracks, observations, contributions (additions into the score matrix); seconds per call (the median of --repeat calls after a warm-up call, wall
clock around the ABI call on buffers made beforehand); the library's stage clocks (PVLM_NEIGHBOR_PROFILE, one stderr line per call: the index on the host, upload,
accumulation, selection, copy-out, the host's rows; every stage then ends in a wait, so the profiled calls are timed apart from the plain ones); contributions per
second of the accumulation kernel and of the whole call; the literal host loop on one thread in the same run (the host compile of the K49 core: the dense F x F float
matrix, every track and every (i, j), then every row's walk — what the host mirror's host route runs), once; whether both gave the same neighbour ids; n_uncertain.
No speed-up is promised: the line records what it is.  Each size runs in a process of its own.  One JSON line per size, appended to --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"room": 454, "campus-large": 8730}
LENGTHS = np.arange(3, 11)
LENGTH_P = np.array([0.30, 0.22, 0.15, 0.11, 0.08, 0.06, 0.05, 0.03])
WINDOW = 24


def make_scene(F, tracks_per_view, seed):
    rng = np.random.default_rng(seed)
    k = np.arange(F)
    row, col = k // 60, k % 60
    col = np.where(row % 2 == 1, 59 - col, col)
    centres = np.stack([col * 1.0, row * 1.5, 1.6 + 0.05 * rng.standard_normal(F)], 1) + 0.05 * rng.standard_normal((F, 3))
    q = rng.standard_normal((F, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(F, 3, 3)
    T_wc = np.concatenate([R, centres[:, :, None]], 2)
    T = F * tracks_per_view
    length = rng.choice(LENGTHS, size=T, p=LENGTH_P)
    anchor = rng.integers(0, max(F - WINDOW, 1), size=T)
    order = np.argsort(rng.random((T, WINDOW)), axis=1)                      # a random subset of the window: the first L of a random permutation
    keep = np.arange(WINDOW)[None, :] < length[:, None]
    picks = np.where(keep, order, WINDOW + 1)
    picks.sort(axis=1)
    views = (anchor[:, None] + picks)[picks <= WINDOW].astype(np.int32)
    off = np.zeros(T + 1, np.int64); np.cumsum(length, out=off[1:])
    assert len(views) == off[-1] and views.max() < F
    mean = np.add.reduceat(centres[views], off[:-1], axis=0) / length[:, None]
    d = rng.standard_normal((T, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    points = mean + d * rng.uniform(4.0, 30.0, size=(T, 1))
    return dict(F=F, T=T, T_wc=np.ascontiguousarray(T_wc.reshape(F, 12)), valid=np.ones(F, np.uint8), off=off, views=np.ascontiguousarray(views),
                points=np.ascontiguousarray(points), contributions=int((length * (length - 1)).sum()))


def worker(size, tracks_per_view, repeat, K, threshold, with_host):
    import panovlm_amd as pv
    from panovlm_amd import api, build
    sc = make_scene(SIZES[size], tracks_per_view, 1)
    F, T = sc["F"], sc["T"]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    n = np.zeros(F, np.int32); ids = np.zeros(F * K, np.int32); R = np.zeros(9 * F * K, np.float32); t = np.zeros(3 * F * K, np.float32); s = np.zeros(F * K, np.float32)
    st = api.NeighborSfmStats(0, 0, 0, 0)
    ctx = pv.Context(0)

    def call():
        t0 = time.perf_counter()
        rc = ctx.lib.pvlm_mvs_select_neighbors_sfm(ctx._h, C.c_int(F), ptr(sc["T_wc"]), ptr(sc["valid"]), C.c_int(T), ptr(sc["off"]), ptr(sc["views"]), ptr(sc["points"]),
                                                   C.c_int(K), C.c_double(threshold), ptr(n), ptr(ids), ptr(R), ptr(t), ptr(s), C.byref(st))
        dt = time.perf_counter() - t0
        assert rc == 0, ctx.lib.pvlm_last_error(ctx._h)
        return dt
    call()                                                    # warm-up: the code object, the pool
    call_s = [call() for _ in range(max(repeat, 1))]
    os.environ["PVLM_NEIGHBOR_PROFILE"] = "1"
    for _ in range(max(repeat, 1)):
        call()
    del os.environ["PVLM_NEIGHBOR_PROFILE"]
    ctx.close()
    line = dict(size=size, views=F, tracks=T, observations=int(sc["off"][-1]), contributions=int(st.n_contributions), neighbor_size=K, sq_distance_threshold=threshold,
                call_s=float(np.median(call_s)), call_s_all=call_s, n_candidates=int(st.n_candidates), n_uncertain=int(st.n_uncertain), n_repeat_tracks=int(st.n_repeat_tracks),
                mean_neighbours=float(n.mean()), tile_cols=api.neighbor_sfm_tile_cols())
    assert line["contributions"] == sc["contributions"]
    if with_host:
        lib = C.CDLL(build.build_neighbor_sfm_check())
        hn = np.zeros(F, np.int32); hids = np.zeros(F * K, np.int32); hR = np.zeros(9 * F * K, np.float32); ht = np.zeros(3 * F * K, np.float32); hs = np.zeros(F * K, np.float32)
        hst = np.zeros(4, np.int64)
        t0 = time.perf_counter()
        rc = lib.chk_ns_select(C.c_int(F), ptr(sc["T_wc"]), ptr(sc["valid"]), C.c_int(T), ptr(sc["off"]), ptr(sc["views"]), ptr(sc["points"]), C.c_int(K), C.c_double(threshold),
                               ptr(hn), ptr(hids), ptr(hR), ptr(ht), ptr(hs), ptr(hst))
        line["host_loop_one_thread_s"] = time.perf_counter() - t0
        assert rc == 0
        line["ids_equal_host"] = bool(np.array_equal(hn, n) and np.array_equal(hids, ids))
        line["R_t_equal_host"] = bool(np.array_equal(hR.view(np.uint32), R.view(np.uint32)) and np.array_equal(ht.view(np.uint32), t.view(np.uint32)))
        line["max_rel_score_diff"] = float(np.max(np.abs(hs.astype(np.float64) - s) / np.maximum(hs, 1e-30)))
        line["host_over_call"] = line["host_loop_one_thread_s"] / line["call_s"]
    print("neighbor_bench_result " + json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="room,campus-large")
    ap.add_argument("--tracks-per-view", type=int, default=300)
    ap.add_argument("--neighbor-size", type=int, default=8)
    ap.add_argument("--threshold", type=float, default=0.25, help="sq_distance_threshold: Square(min_distance = 0.5 m)")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread host loop")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per size")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k49_neighbor_bench.jsonl"))
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.tracks_per_view, args.repeat, args.neighbor_size, args.threshold, not args.no_host)
        return
    for size in [s for s in args.sizes.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", size, "--tracks-per-view", str(args.tracks_per_view), "--repeat", str(args.repeat),
               "--neighbor-size", str(args.neighbor_size), "--threshold", str(args.threshold)] + (["--no-host"] if args.no_host else [])
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            line = dict(size=size, views=SIZES[size], failed="no result within %d s" % args.timeout)
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            break                                     # nothing more is started on the device behind a call that did not come back
        got = [ln for ln in res.stdout.splitlines() if ln.startswith("neighbor_bench_result ")]
        if res.returncode != 0 or not got:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit("the %s run failed (exit %d)" % (size, res.returncode))
        line = json.loads(got[-1][len("neighbor_bench_result "):])
        prof = [json.loads(ln[len("pvlm_neighbor_profile "):]) for ln in res.stderr.splitlines() if ln.startswith("pvlm_neighbor_profile ")]
        if prof:
            keys = ("total_ms", "index_ms", "upload_ms", "accumulate_ms", "select_ms", "copy_out_ms", "host_rows_ms")
            line["stage_ms"] = {k: float(np.median([p[k] for p in prof])) for k in keys}
            acc = line["stage_ms"]["accumulate_ms"]
            line["accumulate_contributions_per_s"] = line["contributions"] / (acc * 1e-3) if acc > 0 else None
        line["call_contributions_per_s"] = line["contributions"] / line["call_s"]
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
