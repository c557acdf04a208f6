"""K39 test helpers: the scenes of SetTranslationScaleDepthMap (the generator of tests/test_relpose_cpu.py::_depth_scene restated for 96 x 192 images, and crafted
scenes whose scale lists are chosen value by value), a numpy restatement of the survivor list and of the exit the reference takes, and the ctypes wrapper of the host
compile of csrc/pvlm_scale_core.h (tests/cpp/scale_core_check.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import essential_ref as er
from tests import relpose_ref as rr

ROOT = rr.ROOT
ROWS, COLS = 96, 192                         # the image; half-size maps are 48 x 96
START = (3, -1.0, -1.0)                      # points_with_depth, upper, lower a pair holds before the step (3: any value the step would not write)
SIZES = (4, 5, 6, 63, 64, 65, 129, 200, 700)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
def depth_scene(seed, n=60, half=True, true_scale=2.5, noise=None, spread=None, rows=ROWS, cols=COLS, shrink=1.0):
    """_depth_scene of tests/test_relpose_cpu.py: n points in front of both cameras of a pair with |t_21| = 1 and the two depth maps that hold true_scale x depth at the
    pixel each point rounds to.  noise: per-point factors on map 2; spread: per-point factors on both maps.  shrink: the geometry (points and t) multiplied by it, the
    maps unchanged: every scale divided by it."""
    rng = np.random.default_rng(seed)
    R = er.rodrigues((0.02, -0.1, 0.03)); t = np.array([0.8, 0.1, -0.59]); t /= np.linalg.norm(t)
    X = rng.uniform(-4, 4, size=(n, 3)); X[:, 2] = rng.uniform(2, 6, n)
    k = 2 if half else 1
    d1 = np.zeros((rows // k + (rows % k), cols // k), np.uint16); d2 = np.zeros_like(d1)
    f2 = np.ones(n) if noise is None else noise; fs = np.ones(n) if spread is None else spread
    for i, p in enumerate(X):
        for d, q, f in ((d1, p, fs[i]), (d2, R @ p + t, fs[i] * f2[i])):
            x, y = rr._cam_to_image(rows, cols, q)
            row, col = rr._round_half_away(y / k), rr._round_half_away(x / k)
            if 0 <= row < d.shape[0] and 0 <= col < d.shape[1]:
                d[row, col] = min(65535, int(round(true_scale * f * np.linalg.norm(q) * 256)))
    return dict(eq_rows=rows, eq_cols=cols, rows1=rows, d1=d1, d2=d2, R=R, t=t * shrink, X=X * shrink)


def crafted_scene(values, half=True):
    """One point per (u1, u2) of values, each at a pixel of its own, R = identity, t = 0: point i reads u1 in map 1 and u2 in map 2 at the same pixel, and
    scale = u / 256 / |p| with |p| = 1 up to rounding; u1 == u2 gives two EQUAL scales (q == p bit for bit)."""
    k = 2 if half else 1
    mr, mc = (ROWS + 1) // k if half else ROWS, (COLS + 1) // k if half else COLS
    d1 = np.zeros((mr, mc), np.uint16); d2 = np.zeros_like(d1)
    X = []
    for i, (u1, u2) in enumerate(values):
        row, col = 5 + 2 * (i // 40), 5 + 2 * (i % 40)                      # map pixels two apart: the rounding of a centre cannot reach a neighbour
        lon = ((col * k) / COLS - 0.5) * 2 * np.pi; lat = (0.5 - (row * k) / ROWS) * np.pi
        p = np.array([np.cos(lat) * np.sin(lon), -np.sin(lat), np.cos(lat) * np.cos(lon)])
        x, y = rr._cam_to_image(ROWS, COLS, p)
        assert (rr._round_half_away(y / k), rr._round_half_away(x / k)) == (row, col)
        d1[row, col] = u1; d2[row, col] = u2
        X.append(p)
    return dict(eq_rows=ROWS, eq_cols=COLS, rows1=ROWS, d1=d1, d2=d2, R=np.eye(3), t=np.zeros(3), X=np.array(X).reshape(-1, 3))


def survivors(sc):
    """the scale list the reference builds, in point order (the loop of rr.scale_ref), or None when a map is missing"""
    d1, d2, R, t = sc["d1"], sc["d2"], sc["R"], sc["t"]
    if d1 is None or d2 is None:
        return None
    half = 1.0 if d1.shape[0] == (sc["rows1"] + 1) // 2 else 0.0
    out = []

    def one(d, q):
        x, y = rr._cam_to_image(sc["eq_rows"], sc["eq_cols"], q)
        row, col = rr._round_half_away(y / (1.0 + half)), rr._round_half_away(x / (1.0 + half))
        if not (col >= 0 and row >= 0 and col + 1 <= sc["eq_cols"] and row + 1 <= sc["eq_rows"]) or row >= d.shape[0] or col >= d.shape[1]:
            return None
        real = np.float32(d[row, col] / 256.0)
        return None if real <= 0 else np.float64(real) / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    for p in np.asarray(sc["X"], np.float64).reshape(-1, 3):
        s1 = one(d1, p)
        if s1 is None:
            continue
        q = np.array([(R[r, 0] * p[0] + R[r, 1] * p[1] + R[r, 2] * p[2]) + t[r] for r in range(3)])
        s2 = one(d2, q)
        if s2 is None or abs(s1 - s2) / min(s1, s2) > 0.2:
            continue
        out += [s1, s2]
    return out


def passes(scale):
    """(histogram passes run, list lengths after each) on a survivor list"""
    ran, sizes = 0, []
    for _ in range(2):
        num = len(scale)
        if num < 10:
            break
        mx, mn = max(scale), min(scale)
        if mx / mn < 1.2:
            break
        interval = (mx - mn) / 10
        histo = [[] for _ in range(10)]
        for s in scale:
            histo[max(0, min(int((s - mn - 1e-8) / interval), 9))].append(s)
        scale = [s for b in histo if len(b) > 0.1 * num for s in b]
        ran += 1; sizes.append(len(scale))
    return ran, sizes


def exit_of(result, consistent):
    """the exit the step took, read from its outputs: (ok, t, tri, points_with_depth, upper, lower)"""
    ok, _, _, pwd, up, lo = result
    if not ok:
        return "none"
    if up == 0.0 and lo == 0.0:
        return "median"
    return "early" if pwd == consistent else "histogram"


def reference(sc):
    return rr.scale_ref(sc["eq_rows"], sc["eq_cols"], sc["rows1"], sc["d1"], sc["d2"], sc["R"], sc["t"], sc["X"])


def _spread(seed, n):
    rng = np.random.default_rng(seed)
    return np.where(rng.uniform(size=n) < 0.6, rng.uniform(0.97, 1.03, n), rng.uniform(0.5, 1.6, n))


def size_scenes():
    """(name, scene, exit) for every size: all depths true (the early break; from 129 points on so many points share a pixel of the 48 x 96 maps that the spread
    reaches 1.2 and a histogram pass drops them) and a spread of factors (histogram passes)"""
    out = []
    for n in SIZES:
        out.append(("true%d" % n, depth_scene(10 + n, n), "none" if n == 4 else "early" if n <= 65 else "histogram"))
        if n >= 63:
            out.append(("histo%d" % n, depth_scene(20 + n, n, spread=_spread(n, n)), "histogram"))
    out.append(("histo40", depth_scene(61, 40, spread=_spread(3, 40)), "histogram"))
    return out


def uniform_bins(per_bin):
    """per_bin points in each of ten bins, the two scales of a point equal: every bin holds exactly a tenth of the list and is dropped, the list is empty after
    pass 1, the median of all of it is taken (ties at the median rank)"""
    vals = [(256 + 26 * b + j, 256 + 26 * b + j) for j in range(per_bin) for b in range(10)]
    return crafted_scene(vals)


def special_scenes():
    out = []
    out.append(("early100", crafted_scene([(640 + (i % 9), 640 + (i % 11)) for i in range(100)]), "early"))   # above one wave, no two points in one pixel
    out.append(("median20", uniform_bins(1), "median"))                         # 20 scales, every bin 2 = a tenth: dropped; even point count, ties at the rank
    out.append(("median140", uniform_bins(7), "median"))                        # 70 points, above one wave
    vals = [(256 + 26 * b, 256 + 26 * b) for b in range(9)] + [(256 + 26 * 9, 256 + 26 * 9 + 2), (256 + 26 * 9 + 1, 256 + 26 * 9 + 3)]
    out.append(("median22", crafted_scene(vals), "median"))                     # 11 points: nine bins of 2 dropped, the last holds 4 < 10: median, odd point count
    vals = [(300 + (i % 7), 300 + (i % 5)) for i in range(9)] + [(600, 600)] * 1
    out.append(("tenth", crafted_scene(vals), "histogram"))                     # 20 scales: 18 in bin 0, 2 in bin 9 = exactly a tenth: dropped
    out.append(("clamp", depth_scene(31, 40, spread=np.linspace(1.0, 1.15, 40) ** 8, true_scale=8.0, shrink=1e-8), None))
    full = depth_scene(6, 30, half=False)
    full["X"] = np.concatenate([full["X"], [[1e-9, 0.3, -5.0], [-1e-9, 0.3, -5.0], [0.0, 5.0, 0.0], [0.0, -5.0, 0.0]]])   # the seam from both sides, the two poles
    full["d1"][:, -1] = 1000; full["d1"][:, 0] = 1000; full["d1"][0, :] = 900; full["d1"][-1, :] = 900
    out.append(("seam_pole_full", full, None))
    ext = depth_scene(7, 50)
    filled = np.argwhere(ext["d1"] > 0)
    ext["d1"][tuple(filled[0])] = 0; ext["d1"][tuple(filled[1])] = 65535; ext["d2"][tuple(np.argwhere(ext["d2"] > 0)[2])] = 65535
    out.append(("zero_and_65535", ext, None))
    one = depth_scene(8, 30); one["d1"] = None
    out.append(("empty_map1", one, "none"))
    two = depth_scene(8, 30); two["d2"] = None
    out.append(("empty_map2", two, "none"))
    mixed = depth_scene(9, 120); mixed["d2"] = np.ascontiguousarray(mixed["d2"][:30, :50])
    out.append(("map2_smaller", mixed, None))
    mixed = depth_scene(12, 120, half=False); mixed["d2"] = depth_scene(12, 120, half=True)["d2"]
    out.append(("full_and_half", mixed, None))
    out.append(("inconsistent", depth_scene(5, 40, noise=np.full(40, 1.5)), "none"))
    out.append(("no_points", depth_scene(5, 0), "none"))
    return out


def all_scenes():
    return size_scenes() + special_scenes()


# ---- the host compile -------------------------------------------------------------------------------------------------------------------------
_CHECK = []


def build_check():
    """build/libscale_check.so: tests/cpp/scale_core_check.cpp with -ffp-contract=off"""
    if _CHECK:
        return _CHECK[0]
    out = os.path.join(ROOT, "build", "libscale_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out, os.path.join(ROOT, "tests", "cpp", "scale_core_check.cpp")])
    _CHECK.append(C.CDLL(out))
    return _CHECK[0]


def build_check_main():
    """the stand-alone program of the same file (its own main) under the host sanitizers"""
    out = os.path.join(ROOT, "build", "scale_check_main")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DSCALE_CHECK_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", out, os.path.join(ROOT, "tests", "cpp", "scale_core_check.cpp")])
    return out


def host_core(chk, sc, start=START):
    """the host compile of the core on one scene: (ok, t, tri, points_with_depth, upper, lower, exit, consistent)"""
    p = rr._ptr
    z = np.zeros((1, 1), np.uint16)
    d1, d2 = sc["d1"], sc["d2"]
    a = np.ascontiguousarray(d1 if d1 is not None else z, np.uint16); b = np.ascontiguousarray(d2 if d2 is not None else z, np.uint16)
    R = np.ascontiguousarray(sc["R"], np.float64); t = np.array(sc["t"], np.float64); tri = np.array(sc["X"], np.float64).reshape(-1, 3).copy()
    buf = tri if len(tri) else np.zeros((1, 3))
    out = np.array([start[0], start[1], start[2], 0, 0, 0], np.float64)
    ok = chk.chk_scale_pair(C.c_int(sc["eq_rows"]), C.c_int(sc["eq_cols"]), C.c_int(sc["rows1"]), p(a), C.c_int(a.shape[0] if d1 is not None else 0), C.c_int(a.shape[1]), p(b),
                            C.c_int(b.shape[0] if d2 is not None else 0), C.c_int(b.shape[1]), p(R), p(t), p(buf), C.c_int(len(tri)), p(out))
    return bool(ok), t, tri, int(out[0]), out[1], out[2], ("none", "mean", "median")[int(out[3])], int(out[4])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, ref):
    """ok, t, every coordinate, points_with_depth, upper, lower: bit for bit"""
    assert bool(got[0]) == bool(ref[0]) and int(got[3]) == int(ref[3]), (got[0], ref[0], got[3], ref[3])
    assert np.array_equal(bits(got[1]), bits(ref[1])), "t_21"
    assert np.array_equal(bits(got[2]), bits(ref[2])), "triangulated"
    assert np.array_equal(bits([got[4], got[5]]), bits([ref[4], ref[5]])), (got[4], got[5], ref[4], ref[5])
