"""K41's references for the tests.

1. The host compile of csrc/pvlm_sift_core.h (tests/cpp/sift_core_check.cpp, -ffp-contract=off): host_* below.
2. A numpy restatement: class Restatement, parametrised by the float type, so that the same formulas run in float32 and in float64 (what the tolerances of the
   refined fields are measured against).  What it follows pvlm.h for: the structure (pyramid, extrema, refinement, orientation, selection, descriptor) and every
   rule and constant stated there.  What equality to the last bit forces it to share with the core, and therefore does NOT check independently: the coefficients of
   the atan2 polynomial, the Taylor degrees of sin / cos, the association of every sum and product, the trilinear order and the 64-lane shape of the histogram sums.
   It is a second implementation in another language that catches slips (it caught a sign error in the cosine series), not an independent definition.  The checks
   that are independent of the core are in tests/test_sift_cpu.py: the blur against scipy.ndimage.correlate1d, atan2 / sin / cos / 2^x against numpy and math, and
   the single blob's position and scale.
3. Seeded test images: blobs plus low-amplitude noise, crops of one texture, and a jittered dot pattern that yields thousands of candidates in one octave."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from tests import depthfill_ref as dfr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32), ("response", np.float32), ("octave", np.int32)])
CAND = np.dtype([("octave", np.int32), ("layer", np.int32), ("r", np.int32), ("c", np.int32), ("x", np.float32), ("y", np.float32), ("size", np.float32),
                 ("response", np.float32), ("word", np.int32), ("det_layer", np.int32), ("det_r", np.int32), ("det_c", np.int32)])
COUNTERS = ("extrema", "moved", "reject_moves", "reject_contrast", "reject_edge", "candidates", "multi_peak", "keypoints")
_CHECK = []


def _ptr(a, t=None):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def build_check():
    """build/libsift_check.so: tests/cpp/sift_core_check.cpp with -ffp-contract=off"""
    if _CHECK:
        return _CHECK[0]
    out = os.path.join(ROOT, "build", "libsift_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out, os.path.join(ROOT, "tests", "cpp", "sift_core_check.cpp")])
    lib = C.CDLL(out)
    lib.chk_sift_extract.restype = C.c_longlong
    lib.chk_sift_select.restype = C.c_longlong
    lib.chk_sift_atan2_deg.restype = C.c_float
    lib.chk_sift_atan2_deg.argtypes = [C.c_float, C.c_float]
    lib.chk_sift_pow2.restype = C.c_float
    lib.chk_sift_pow2.argtypes = [C.c_float]
    _CHECK.append(lib)
    return lib


def build_check_main():
    """the stand-alone program of the same file (its own main) under the host sanitizers"""
    out = os.path.join(ROOT, "build", "sift_check_main")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DSIFT_CHECK_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", out, os.path.join(ROOT, "tests", "cpp", "sift_core_check.cpp")])
    return out


def host_sizes(rows, cols):
    r = np.zeros(32, np.int32); c = np.zeros(32, np.int32)
    n = build_check().chk_sift_sizes(C.c_int(rows), C.c_int(cols), _ptr(r), _ptr(c))
    return [(int(r[o]), int(c[o])) for o in range(n)]


def host_kernels():
    taps = np.zeros(6, np.int32); coeff = np.zeros((6, 27), np.float32)
    build_check().chk_sift_kernels(_ptr(taps), _ptr(coeff))
    return [coeff[i, :taps[i]].copy() for i in range(6)]


def host_doubled(img):
    img = np.ascontiguousarray(img, np.uint8)
    out = np.zeros((2 * img.shape[0], 2 * img.shape[1]), np.float32)
    build_check().chk_sift_doubled(_ptr(img), C.c_int(img.shape[0]), C.c_int(img.shape[1]), _ptr(out))
    return out


def host_pyramid(img, octave):
    img = np.ascontiguousarray(img, np.uint8)
    R, Cc = host_sizes(*img.shape)[octave]
    g = np.zeros((6, R, Cc), np.float32); d = np.zeros((5, R, Cc), np.float32)
    build_check().chk_sift_pyramid(_ptr(img), C.c_int(img.shape[0]), C.c_int(img.shape[1]), C.c_int(octave), _ptr(g), _ptr(d))
    return g, d


def host_detect(img):
    """(candidates CAND, keypoints before the selection KP, counters dict)"""
    img = np.ascontiguousarray(img, np.uint8)
    cap = 1 << 16
    cands = np.zeros(cap, CAND); kps = np.zeros(cap, KP); nc = C.c_longlong(0); nk = C.c_longlong(0); ct = np.zeros(8, np.int64)
    build_check().chk_sift_detect(_ptr(img), C.c_int(img.shape[0]), C.c_int(img.shape[1]), _ptr(cands), C.c_longlong(cap), C.byref(nc), _ptr(kps), C.c_longlong(cap),
                                  C.byref(nk), _ptr(ct))
    assert nc.value <= cap and nk.value <= cap
    return cands[:nc.value].copy(), kps[:nk.value].copy(), dict(zip(COUNTERS, (int(v) for v in ct)))


def host_extract(img, nfeatures, mask=None, root=False, threads=1, detected=None):
    """ExtractSIFTHost of one image: (keypoints KP, descriptors n x 128 float32); detected: a list that receives the keypoint count before the selection"""
    img = np.ascontiguousarray(img, np.uint8)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    cap = 1 << 16
    kps = np.zeros(cap, KP); desc = np.zeros((cap, 128), np.float32); det = C.c_longlong(0)
    n = build_check().chk_sift_extract(_ptr(img), C.c_int(img.shape[0]), C.c_int(img.shape[1]), _ptr(m), C.c_int(nfeatures), C.c_int(1 if root else 0), _ptr(kps), _ptr(desc),
                                       C.c_longlong(cap), C.c_int(threads), C.byref(det))
    assert n <= cap
    if detected is not None:
        detected.append(det.value)
    return kps[:n].copy(), desc[:n].copy()


def host_select(kps, nfeatures, rows, cols, mask=None):
    k = np.ascontiguousarray(kps, KP).copy()
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    if len(k) == 0:
        return k
    n = build_check().chk_sift_select(_ptr(k), C.c_longlong(len(k)), C.c_int(nfeatures), C.c_int(rows), C.c_int(cols), _ptr(m))
    return k[:n].copy()


def host_desc_finish(hist, root):
    h = np.ascontiguousarray(hist, np.float32); out = np.zeros(128, np.float32)
    build_check().chk_sift_desc_finish(_ptr(h), C.c_int(1 if root else 0), _ptr(out))
    return out


# ---- images ------------------------------------------------------------------------------------------------------------------------------------------------------
def blob_image(rows, cols, seed, blobs=None, noise=3):
    """a sum of seeded Gaussian blobs of both signs on a grey level, plus uniform noise of `noise` grey levels"""
    rng = np.random.default_rng(seed)
    nb = blobs if blobs is not None else 8 + rows * cols // 150
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    f = np.full((rows, cols), 110.0)
    for _ in range(nb):
        cy, cx = rng.uniform(0, rows), rng.uniform(0, cols)
        s = rng.uniform(1.2, 6.0); a = rng.uniform(40, 120) * rng.choice([-1.0, 1.0])
        e = rng.uniform(1.0, 2.2); th = rng.uniform(0, np.pi)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th); v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        f += a * np.exp(-(u * u / (e * e) + v * v) / (2 * s * s))
    f += rng.integers(0, noise + 1, (rows, cols))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def dot_image(rows, cols, seed, step=6):
    """small bright squares (2 or 3 pixels) on a jittered grid of `step` pixels plus noise: thousands of fine-scale extrema in the first octave"""
    rng = np.random.default_rng(seed)
    f = np.full((rows, cols), 60, np.int32)
    for y in range(4, rows - 4, step):
        for x in range(4, cols - 4, step):
            yy, xx = y + rng.integers(0, 3), x + rng.integers(0, 3)
            a = int(rng.integers(90, 190)); r = int(rng.integers(1, 3))
            f[yy:yy + r + 1, xx:xx + r + 1] += a
    f += rng.integers(0, 4, f.shape)
    return np.clip(f, 0, 255).astype(np.uint8)


def texture_crops(seed, rows=192, cols=256, shift=(16, 8)):
    """two crops of one seeded texture, the second shifted by (dx, dy) = shift pixels: a keypoint at (x, y) of the first is at (x - dx, y - dy) of the second"""
    big = blob_image(rows + shift[1], cols + shift[0], seed, blobs=260, noise=2)
    a = big[0:rows, 0:cols]
    b = big[shift[1]:shift[1] + rows, shift[0]:shift[0] + cols]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------------
SIGMA, K3 = 1.6, 1.2599210498948732


def octave_count(base_rows, base_cols):
    m = min(base_rows, base_cols)
    lg = int(math.floor(math.log2(m) + 0.5))          # round(log2 m); never a tie for an integer m
    return max(1, lg - 2 + 1)


def octave_sizes(rows, cols):
    r, c = 2 * rows, 2 * cols
    out = []
    for _ in range(octave_count(r, c)):
        out.append((r, c)); r //= 2; c //= 2
    return out


def sigmas():
    s = [math.sqrt(max(SIGMA * SIGMA - 1.0, 0.01))]
    prev = SIGMA
    for _ in range(1, 6):
        tot = prev * K3
        s.append(math.sqrt(tot * tot - prev * prev)); prev = tot
    return s


def kernels():
    out = []
    for s in sigmas():
        taps = int(math.floor(8.0 * s + 1.0 + 0.5)) | 1
        r = taps // 2
        x = np.arange(-r, r + 1, dtype=np.float64)
        e = dfr.exp_neg(x * x / (2.0 * s * s))
        tot = 0.0
        for v in e:
            tot = tot + v
        out.append((e / tot).astype(np.float32))
    return out


def reflect_index(n, r):
    """reflect-101 source indices of positions -r .. n - 1 + r, folded as often as needed"""
    idx = np.arange(-r, n + r)
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * (n - 1)
    idx = np.mod(idx, period)
    return np.where(idx >= n, period - idx, idx)


def blur(img, coeff, ft=np.float32):
    """rows then columns; s = s + c[k] * tap for k ascending, every operation rounded to ft"""
    coeff = coeff.astype(ft)
    r = len(coeff) // 2
    a = img.astype(ft)
    for axis in (1, 0):
        n = a.shape[axis]
        pad = np.take(a, reflect_index(n, r), axis=axis)
        s = np.zeros_like(a)
        for k in range(len(coeff)):
            tap = np.take(pad, np.arange(k, k + n), axis=axis)
            s = (s + (coeff[k] * tap).astype(ft)).astype(ft)
        a = s
    return a


def doubled(img, ft=np.float32):
    rows, cols = img.shape
    f = img.astype(ft)

    def axis_weights(n):
        d = np.arange(2 * n)
        src = (d + 0.5) / 2 - 0.5
        lo = np.floor(src).astype(int); fr = (src - lo).astype(ft)
        return np.clip(lo, 0, n - 1), np.clip(lo + 1, 0, n - 1), fr
    x0, x1, fx = axis_weights(cols); y0, y1, fy = axis_weights(rows)
    h = f[:, x0] * (1 - fx)[None, :] + f[:, x1] * fx[None, :]
    return (h[y0, :] * (1 - fy)[:, None] + h[y1, :] * fy[:, None]).astype(ft)


def pyramid(img, ft=np.float32):
    """[(gauss 6 x R x C, dog 5 x R x C)] per octave"""
    K = kernels()
    out = []
    base = blur(doubled(img, ft), K[0], ft)
    for o, (R, Cc) in enumerate(octave_sizes(*img.shape)):
        g = [base if o == 0 else out[-1][0][3][::2, ::2][:R, :Cc].copy()]
        for l in range(1, 6):
            g.append(blur(g[-1], K[l], ft))
        d = [(g[l + 1] - g[l]).astype(ft) for l in range(5)]
        out.append((np.stack(g), np.stack(d)))
    return out


def atan2_deg(y, x, ft=np.float32):
    """the definition's polynomial atan2 in degrees, scalars"""
    f = ft
    ax, ay = abs(f(x)), abs(f(y))
    mx, mn = (ax, ay) if ax > ay else (ay, ax)
    if mx == 0:
        return f(0)
    a = f(mn / mx); s = f(a * a)
    p = f(-0.01172120)
    for c in (0.05265332, -0.11643287, 0.19354346, -0.33262347, 0.99997726):
        p = f(f(p * s) + f(c))
    r = f(p * a)
    if ay > ax:
        r = f(f(1.57079637) - r)
    if x < 0:
        r = f(f(3.14159274) - r)
    if y < 0:
        r = f(f(6.28318548) - r)
    return f(r * f(57.2957802))


def atan2_deg_v(y, x, ft=np.float32):
    """the same on arrays"""
    y = y.astype(ft); x = x.astype(ft)
    ax, ay = np.abs(x), np.abs(y)
    mx = np.maximum(ax, ay); mn = np.minimum(ax, ay)
    zero = mx == 0
    a = (mn / np.where(zero, ft(1), mx)).astype(ft); s = (a * a).astype(ft)
    p = np.full_like(a, ft(-0.01172120))
    for c in (0.05265332, -0.11643287, 0.19354346, -0.33262347, 0.99997726):
        p = ((p * s).astype(ft) + ft(c)).astype(ft)
    r = (p * a).astype(ft)
    r = np.where(ay > ax, (ft(1.57079637) - r).astype(ft), r)
    r = np.where(x < 0, (ft(3.14159274) - r).astype(ft), r)
    r = np.where(y < 0, (ft(6.28318548) - r).astype(ft), r)
    return np.where(zero, ft(0), (r * ft(57.2957802)).astype(ft)).astype(ft)


def exp_neg_v(x, ft=np.float32):
    """(ft) e^-x of K37's exp_neg evaluated in double"""
    return dfr.exp_neg(np.asarray(x, np.float64)).astype(ft)


def pow2(t, ft=np.float32):
    return ft(4.0 * float(dfr.exp_neg(np.array([(2.0 - float(t)) * 0.6931471805599453]))[0]))


def sincos_deg(deg):
    a = float(deg)
    q = min(int(a / 90.0), 3)
    x = (a - 90.0 * q) * 0.017453292519943295; x2 = x * x
    s = 0.0
    for n in (23, 21, 19, 17, 15, 13, 11, 9, 7, 5, 3, 1):
        c = (-1.0 if (n // 2) % 2 else 1.0) / math.factorial(n)
        s = s * x2 + c
    s = s * x
    cs = 0.0
    for n in (22, 20, 18, 16, 14, 12, 10, 8, 6, 4, 2, 0):
        c = (-1.0 if (n // 2) % 2 else 1.0) / math.factorial(n)
        cs = cs * x2 + c
    return ((s, cs), (cs, -s), (-s, -cs), (-cs, s))[q]


def _rint(v):
    return int(np.rint(v))


class Restatement:
    """detect / select / describe of one image in float type ft"""

    def __init__(self, img, ft=np.float32, pyr=None):
        self.img = np.ascontiguousarray(img, np.uint8); self.ft = ft
        self.pyr = pyr if pyr is not None else pyramid(self.img, ft)
        self.counters = dict.fromkeys(COUNTERS, 0)

    # -- extrema and refinement
    def extrema(self, o):
        """integer (layer, r, c) of the detected extrema of octave o in (layer, row, column) order"""
        d = self.pyr[o][1]
        _, R, Cc = d.shape
        out = []
        if R <= 10 or Cc <= 10:
            return out
        for l in (1, 2, 3):
            v = d[l][5:R - 5, 5:Cc - 5]
            ge = np.ones(v.shape, bool); le = np.ones(v.shape, bool)
            for ll in (l - 1, l, l + 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        nb = d[ll][5 + dy:R - 5 + dy, 5 + dx:Cc - 5 + dx]
                        ge &= v >= nb; le &= v <= nb
            hit = (np.abs(v) > 1.0) & (((v > 0) & ge) | ((v < 0) & le))
            for r, c in zip(*np.nonzero(hit)):
                out.append((l, int(r) + 5, int(c) + 5))
        return out

    def refine(self, o, l, r, c):
        """None (with the rule counted) or the candidate record"""
        f = self.ft
        d = self.pyr[o][1]
        _, R, Cc = d.shape
        isc = f(f(1) / f(255)); ds = f(isc * f(0.5)); ss = isc; cs = f(isc * f(0.25))
        det_pos = (l, r, c)
        moved = False
        xi = xr = xc = f(0)
        for step in range(6):
            if step == 5:
                self.counters["reject_moves"] += 1; self.counters["moved"] += moved
                return None
            img, prv, nxt = d[l], d[l - 1], d[l + 1]
            g0 = f(f(img[r, c + 1] - img[r, c - 1]) * ds); g1 = f(f(img[r + 1, c] - img[r - 1, c]) * ds); g2 = f(f(nxt[r, c] - prv[r, c]) * ds)
            v2 = f(img[r, c] * f(2))
            dxx = f(f(f(img[r, c + 1] + img[r, c - 1]) - v2) * ss); dyy = f(f(f(img[r + 1, c] + img[r - 1, c]) - v2) * ss); dss = f(f(f(nxt[r, c] + prv[r, c]) - v2) * ss)
            dxy = f(f(f(f(img[r + 1, c + 1] - img[r + 1, c - 1]) - img[r - 1, c + 1]) + img[r - 1, c - 1]) * cs)
            dxs = f(f(f(f(nxt[r, c + 1] - nxt[r, c - 1]) - prv[r, c + 1]) + prv[r, c - 1]) * cs)
            dys = f(f(f(f(nxt[r + 1, c] - nxt[r - 1, c]) - prv[r + 1, c]) + prv[r - 1, c]) * cs)
            c00 = f(f(dyy * dss) - f(dys * dys)); c01 = f(f(dxs * dys) - f(dxy * dss)); c02 = f(f(dxy * dys) - f(dxs * dyy))
            c11 = f(f(dxx * dss) - f(dxs * dxs)); c12 = f(f(dxs * dxy) - f(dxx * dys)); c22 = f(f(dxx * dyy) - f(dxy * dxy))
            det = f(f(f(dxx * c00) + f(dxy * c01)) + f(dxs * c02))
            if det == 0:
                self.counters["reject_moves"] += 1; self.counters["moved"] += moved
                return None
            inv = f(f(1) / det)
            X0 = f(f(f(f(c00 * g0) + f(c01 * g1)) + f(c02 * g2)) * inv); X1 = f(f(f(f(c01 * g0) + f(c11 * g1)) + f(c12 * g2)) * inv)
            X2 = f(f(f(f(c02 * g0) + f(c12 * g1)) + f(c22 * g2)) * inv)
            xc, xr, xi = f(-X0), f(-X1), f(-X2)
            if abs(xi) < 0.5 and abs(xr) < 0.5 and abs(xc) < 0.5:
                break
            if not (abs(xi) < 1e6 and abs(xr) < 1e6 and abs(xc) < 1e6):
                self.counters["reject_moves"] += 1; self.counters["moved"] += moved
                return None
            c += _rint(xc); r += _rint(xr); l += _rint(xi)
            moved = True
            if l < 1 or l > 3 or c < 5 or c >= Cc - 5 or r < 5 or r >= R - 5:
                self.counters["reject_moves"] += 1; self.counters["moved"] += moved
                return None
        self.counters["moved"] += moved
        img, prv, nxt = d[l], d[l - 1], d[l + 1]
        g0 = f(f(img[r, c + 1] - img[r, c - 1]) * ds); g1 = f(f(img[r + 1, c] - img[r - 1, c]) * ds); g2 = f(f(nxt[r, c] - prv[r, c]) * ds)
        t = f(f(f(g0 * xc) + f(g1 * xr)) + f(g2 * xi))
        contr = f(f(img[r, c] * isc) + f(t * f(0.5)))
        if f(abs(contr) * f(3)) < f(0.04):
            self.counters["reject_contrast"] += 1
            return None
        v2 = f(img[r, c] * f(2))
        dxx = f(f(f(img[r, c + 1] + img[r, c - 1]) - v2) * ss); dyy = f(f(f(img[r + 1, c] + img[r - 1, c]) - v2) * ss)
        dxy = f(f(f(f(img[r + 1, c + 1] - img[r + 1, c - 1]) - img[r - 1, c + 1]) + img[r - 1, c - 1]) * cs)
        tr = f(dxx + dyy); det = f(f(dxx * dyy) - f(dxy * dxy))
        if det <= 0 or f(f(tr * tr) * f(10)) >= f(f(f(11) * f(11)) * det):
            self.counters["reject_edge"] += 1
            return None
        sc = f(1 << o)
        return dict(octave=o, layer=l, r=r, c=c, x=f(f(f(c) + xc) * sc), y=f(f(f(r) + xr) * sc),
                    size=f(f(f(f(SIGMA) * pow2(f(f(f(l) + xi) / f(3)), f)) * sc) * f(2)), response=f(abs(contr)),
                    word=o + (l << 8) + (_rint(f(f(xi + f(0.5)) * f(255))) << 16), det=det_pos)

    # -- orientation
    def angles(self, k):
        f = self.ft
        g = self.pyr[k["octave"]][0][k["layer"]]
        R, Cc = g.shape
        scl = f(f(k["size"] * f(0.5)) / f(1 << k["octave"]))
        radius = _rint(f(f(f(3) * f(1.5)) * scl))
        sg = f(f(1.5) * scl); inv = f(f(1) / f(f(2) * f(sg * sg)))
        side = 2 * radius + 1
        j = np.arange(side * side)
        i = j // side - radius; jj = j % side - radius
        y = k["r"] + i; x = k["c"] + jj
        ok = (y > 0) & (y < R - 1) & (x > 0) & (x < Cc - 1)
        j, i, jj, y, x = j[ok], i[ok], jj[ok], y[ok], x[ok]
        dx = (g[y, x + 1] - g[y, x - 1]).astype(f); dy = (g[y - 1, x] - g[y + 1, x]).astype(f)
        w = exp_neg_v(((i * i + jj * jj).astype(f) * inv).astype(f), f)
        mag = np.sqrt(((dx * dx).astype(f) + (dy * dy).astype(f)).astype(f)).astype(f)
        b = np.rint((f(f(36) / f(360)) * atan2_deg_v(dy, dx, f)).astype(f)).astype(int)
        b = np.where(b >= 36, b - 36, b); b = np.where(b < 0, b + 36, b)
        part = np.zeros((64, 36), f)
        np.add.at(part, (j % 64, b), (w * mag).astype(f))        # a lane's samples in ascending j: add.at is sequential
        raw = np.zeros(36, f)
        for lane in range(64):
            raw = (raw + part[lane]).astype(f)
        h = np.zeros(36, f)
        for q in range(36):
            h[q] = f(f(f(f(raw[q - 2] + raw[(q + 2) % 36]) * f(1 / 16)) + f(f(raw[q - 1] + raw[(q + 1) % 36]) * f(4 / 16))) + f(raw[q] * f(6 / 16)))
        thr = f(h.max() * f(0.8))
        out = []
        for q in range(36):
            lft, rgt = h[q - 1], h[(q + 1) % 36]
            if h[q] > lft and h[q] > rgt and h[q] >= thr:
                b = f(f(q) + f(f(f(0.5) * f(lft - rgt)) / f(f(lft - f(f(2) * h[q])) + rgt)))
                b = f(f(36) + b) if b < 0 else f(b - f(36)) if b >= 36 else b
                a = f(f(360) - f(f(f(360) / f(36)) * b))
                if abs(f(a - f(360))) < 1.1920929e-07:
                    a = f(0)
                out.append(a)
        return out

    def detect(self):
        """(candidates, keypoints before the selection as dicts) in the defined order"""
        cands, kps = [], []
        for o in range(len(self.pyr)):
            for (l, r, c) in self.extrema(o):
                self.counters["extrema"] += 1
                k = self.refine(o, l, r, c)
                if k is None:
                    continue
                a = self.angles(k)
                cands.append(k)
                self.counters["candidates"] += 1; self.counters["multi_peak"] += len(a) > 1; self.counters["keypoints"] += len(a)
                for ang in a:
                    kps.append(dict(x=k["x"], y=k["y"], size=k["size"], angle=ang, response=k["response"], octave=k["word"]))
        return cands, kps

    # -- selection
    def select(self, kps, nfeatures, mask=None):
        f = self.ft
        seen = set(); a = []
        for k in kps:
            key = (float(k["x"]), float(k["y"]), float(k["size"]), float(k["angle"]))
            if key in seen:
                continue
            seen.add(key); a.append(k)
        if nfeatures < len(a):
            thr = sorted((float(k["response"]) for k in a), reverse=True)[nfeatures - 1]
            a = [k for k in a if float(k["response"]) >= thr]
        out = []
        rows, cols = self.img.shape
        for k in a:
            k = dict(k)
            k["octave"] = (k["octave"] & ~255) | ((k["octave"] - 1) & 255)
            k["x"] = f(k["x"] * f(0.5)); k["y"] = f(k["y"] * f(0.5)); k["size"] = f(k["size"] * f(0.5))
            if mask is not None:
                my = min(max(_rint(k["y"]), 0), rows - 1); mx = min(max(_rint(k["x"]), 0), cols - 1)
                if mask[my, mx] == 0:
                    continue
            out.append(k)
        return out

    # -- descriptor
    def descriptor(self, k, root=False):
        f = self.ft
        oc = k["octave"] & 255; layer = (k["octave"] >> 8) & 255
        oc = oc if oc < 128 else oc - 256
        scale = f(1) / f(1 << oc) if oc >= 0 else f(1 << -oc)
        g = self.pyr[oc + 1][0][layer]
        R, Cc = g.shape
        size = f(k["size"] * scale); px = f(k["x"] * scale); py = f(k["y"] * scale)
        ang = f(f(360) - k["angle"])
        if abs(f(ang - f(360))) < 1.1920929e-07:
            ang = f(0)
        c0, r0 = _rint(px), _rint(py)
        sn, cs = sincos_deg(ang)
        hw = f(f(3) * f(size * f(0.5)))
        radius = min(_rint(f(f(f(hw * f(1.4142135623730951)) * f(5)) * f(0.5))), int(math.sqrt(float(Cc) * Cc + float(R) * R)))
        cos_t = f(f(cs) / hw); sin_t = f(f(sn) / hw)
        side = 2 * radius + 1
        j = np.arange(side * side)
        i = (j // side - radius); jj = (j % side - radius)
        fi, fj = i.astype(f), jj.astype(f)
        c_rot = ((fj * cos_t).astype(f) - (fi * sin_t).astype(f)).astype(f); r_rot = ((fj * sin_t).astype(f) + (fi * cos_t).astype(f)).astype(f)
        rbin = ((r_rot + f(2)).astype(f) - f(0.5)).astype(f); cbin = ((c_rot + f(2)).astype(f) - f(0.5)).astype(f)
        y = r0 + i; x = c0 + jj
        ok = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (y > 0) & (y < R - 1) & (x > 0) & (x < Cc - 1)
        j, y, x, c_rot, r_rot, rbin, cbin = j[ok], y[ok], x[ok], c_rot[ok], r_rot[ok], rbin[ok], cbin[ok]
        dx = (g[y, x + 1] - g[y, x - 1]).astype(f); dy = (g[y - 1, x] - g[y + 1, x]).astype(f)
        w = exp_neg_v(((((c_rot * c_rot).astype(f) + (r_rot * r_rot).astype(f)).astype(f)) * f(1 / 8)).astype(f), f)
        mag = (np.sqrt(((dx * dx).astype(f) + (dy * dy).astype(f)).astype(f)).astype(f) * w).astype(f)
        obin = ((atan2_deg_v(dy, dx, f) - ang).astype(f) * f(f(8) / f(360))).astype(f)
        r0f, c0f, o0f = np.floor(rbin), np.floor(cbin), np.floor(obin)
        rb = (rbin - r0f).astype(f); cb = (cbin - c0f).astype(f); ob = (obin - o0f).astype(f)
        o0 = o0f.astype(int); o0 = np.where(o0 < 0, o0 + 8, o0); o0 = np.where(o0 >= 8, o0 - 8, o0)
        v_r1 = (mag * rb).astype(f); v_r0 = (mag - v_r1).astype(f)
        v11 = (v_r1 * cb).astype(f); v10 = (v_r1 - v11).astype(f); v01 = (v_r0 * cb).astype(f); v00 = (v_r0 - v01).astype(f)
        vals = {}
        for (dr, dc), v in (((0, 0), v00), ((0, 1), v01), ((1, 0), v10), ((1, 1), v11)):
            hi = (v * ob).astype(f)
            vals[(dr, dc, 1)] = hi; vals[(dr, dc, 0)] = (v - hi).astype(f)
        part = np.zeros((64, 128), f)
        # a lane's samples in ascending j, a sample's eight contributions in the order dr, dc, do: one add.at over the interleaved list
        n = len(j)
        lanes = np.zeros((n, 8), int); bins = np.zeros((n, 8), int); vv = np.zeros((n, 8), f); good = np.zeros((n, 8), bool)
        for kk in range(8):
            dr, dc, do = kk >> 2, (kk >> 1) & 1, kk & 1
            rr = r0f.astype(int) + dr; cc = c0f.astype(int) + dc
            good[:, kk] = (rr >= 0) & (rr <= 3) & (cc >= 0) & (cc <= 3)
            bins[:, kk] = (np.clip(rr, 0, 3) * 4 + np.clip(cc, 0, 3)) * 8 + np.where(do == 1, (o0 + 1) & 7, o0)
            lanes[:, kk] = j % 64; vv[:, kk] = vals[(dr, dc, do)]
        gsel = good.ravel()
        np.add.at(part, (lanes.ravel()[gsel], bins.ravel()[gsel]), vv.ravel()[gsel])
        hist = np.zeros(128, f)
        for lane in range(64):
            hist = (hist + part[lane]).astype(f)
        return self.desc_finish(hist, root)

    def desc_finish(self, hist, root):
        f = self.ft
        n2 = f(0)
        for v in hist:
            n2 = f(n2 + f(v * v))
        thr = f(np.sqrt(n2) * f(0.2))
        cl = np.minimum(hist, thr).astype(f)
        n2 = f(0)
        for v in cl:
            n2 = f(n2 + f(v * v))
        nr = f(np.sqrt(n2))
        fac = f(f(512) / max(nr, f(1.1920929e-07)))
        q = np.clip(np.rint((cl * fac).astype(f)), 0, 255).astype(f)
        if not root:
            return q
        l1 = f(0)
        for v in q:
            l1 = f(l1 + v)
        if l1 == 0:
            return q
        return (np.sqrt((q / l1).astype(f)).astype(f) * f(512)).astype(f)

    def extract(self, nfeatures, mask=None, root=False):
        _, kps = self.detect()
        kps = self.select(kps, nfeatures, mask)
        desc = np.stack([self.descriptor(k, root) for k in kps]) if kps else np.zeros((0, 128), self.ft)
        return kps, desc


def kp_array(kps):
    out = np.zeros(len(kps), KP)
    for i, k in enumerate(kps):
        out[i] = (k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"])
    return out
