#!/usr/bin/env python3
"""Room-scale timing of K41: ONE pvlm_sift_extract call (capacity left open: what api.sift_extract and pvlm::ReadImages do, device_calls in the line) over --images synthetic panoramas of --cols x --rows (5760 x 2880), nfeatures 8096, RootSIFT, against
ExtractSIFTHost (the host compile of csrc/pvlm_sift_core.h, tests/cpp/sift_core_check.cpp) on --threads threads over --host-images of the same images, in the same
run; the host results must equal the call's bit for bit.  The images are seeded blobs (stamped patches of both signs, sigma 1.5 .. 12) plus low-amplitude noise,
shifted copies of one field; the host compile confirms more than nfeatures keypoints before the selection on the first image.
Reported: wall clock of the call (median of --repeat after a warm-up) and per image, the HIP-event time of the parts (a) doubling + first blur, (b) layer blurs +
differences, (c) decimation, (d) extrema + refinement, (e) orientation, (f) descriptors, the host's ms per image and the speed-up, and the roofline of (b): its
compulsory traffic is one float read and one write per Gaussian layer pixel plus one write per difference pixel (layers 1..5 of every octave: 3 x 4 B x 5 layers per
pixel), achieved bytes/s = that over the event time of (b), against the 6.3 TB/s the MI355X sustains.  One JSON line, appended to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 6.3e12


def field(rows, cols, seed, blobs):
    rng = np.random.default_rng(seed)
    f = np.full((rows, cols), 110.0, np.float32)
    for _ in range(blobs):
        s = rng.uniform(1.5, 12.0); a = rng.uniform(30, 110) * rng.choice([-1.0, 1.0])
        h = int(4 * s)
        cy, cx = int(rng.integers(h, rows - h)), int(rng.integers(h, cols - h))
        yy, xx = np.mgrid[-h:h + 1, -h:h + 1].astype(np.float32)
        f[cy - h:cy + h + 1, cx - h:cx + h + 1] += (a * np.exp(-(yy * yy + xx * xx) / (2 * s * s))).astype(np.float32)
    return f, rng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--rows", type=int, default=2880)
    ap.add_argument("--cols", type=int, default=5760)
    ap.add_argument("--nfeatures", type=int, default=8096)
    ap.add_argument("--blobs", type=int, default=60000)
    ap.add_argument("--host-images", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k41_sift_bench.jsonl"))
    args = ap.parse_args()
    import panovlm_amd as pv
    from panovlm_amd import api
    from tests import sift_ref as sr
    f, rng = field(args.rows, args.cols, 41, args.blobs)
    imgs = []
    for i in range(args.images):
        g = np.roll(f, (37 * i, 101 * i), (0, 1)) + rng.integers(0, 3, f.shape).astype(np.float32)
        imgs.append(np.clip(np.rint(g), 0, 255).astype(np.uint8))
    ctx = pv.Context(0)
    flags = api.FLAG_SIFT_ROOT
    api.sift_extract(ctx, imgs, args.nfeatures, flags=flags)                              # warm-up: sizes the pool
    # the route of a caller who leaves the capacity open (api.sift_extract, pvlm::ReadImages): buffers for nfeatures + room for ties per image, ONE device call
    times, res = [], None
    for _ in range(max(args.repeat, 1)):
        t0 = time.perf_counter(); res = api.sift_extract(ctx, imgs, args.nfeatures, flags=flags); times.append(time.perf_counter() - t0)
    call_s = float(np.median(times))
    st = res["stats"]
    sr.build_check()                                                                      # compiled outside the timed loop
    host_s, same, detected = [], True, []
    for i in range(min(args.host_images, args.images)):
        t0 = time.perf_counter(); k, d = sr.host_extract(imgs[i], args.nfeatures, None, True, threads=args.threads, detected=detected); host_s.append(time.perf_counter() - t0)
        a, b = res["offsets"][i], res["offsets"][i + 1]
        same = same and res["keypoints"][a:b].tobytes() == k.tobytes() and res["descriptors"][a:b].tobytes() == d.tobytes()
    host_ms = 1e3 * float(np.mean(host_s)) if host_s else None
    pix = sum(r * c for r, c in sr.octave_sizes(args.rows, args.cols))
    blur_bytes = args.images * pix * 5 * 3 * 4
    b_s = st["part_ms"]["b"] * 1e-3
    line = dict(label=args.label, images=args.images, rows=args.rows, cols=args.cols, nfeatures=args.nfeatures, blobs=args.blobs, root_sift=True,
                date=time.strftime("%Y-%m-%d"), device_calls=res["calls"], keypoints_detected=st["keypoints_detected"], keypoints=st["keypoints"],
                candidates=st["candidates"], call_s=call_s, call_s_all=times, ms_per_image=1e3 * call_s / args.images, part_ms=st["part_ms"],
                part_ms_per_image={k: v / args.images for k, v in st["part_ms"].items()}, host_threads=args.threads, host_images=len(host_s), host_ms_per_image=host_ms,
                speed_up=(host_ms / (1e3 * call_s / args.images)) if host_ms else None, host_equals_device=bool(same),
                blur_compulsory_bytes=blur_bytes, blur_bytes_per_s=blur_bytes / b_s if b_s > 0 else None,
                blur_share_of_peak=(blur_bytes / b_s / PEAK_BYTES_PER_S) if b_s > 0 else None)
    line["host_keypoints_detected"] = detected                                            # before the selection, by the host compile
    ctx.close()
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fo:
        fo.write(json.dumps(line) + "\n")
    if not same:
        sys.exit("the host results differ from the call's")
    if res["calls"] != 1:
        sys.exit("the timed route took %d device calls" % res["calls"])
    if detected and min(detected) <= args.nfeatures:
        sys.exit("not more than nfeatures keypoints before the selection")


if __name__ == "__main__":
    main()
