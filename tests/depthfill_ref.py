"""numpy restatement of K37 (DepthCompletion, util/DepthCompletion.cpp:154-316, and the uint16 conversion of SfM::ComputeDepthImage, sfm/SfM.cpp:170-226, as
panovlm_amd/csrc/pvlm_depthfill_core.h states them), the tests' input recipe and the ctypes wrappers of the host compile (tests/cpp/depthfill_core_check.cpp).
Written from the stage table alone: whole-image array operations, no link to the core header.  Every float operation is one float32 (or, in the bilateral, float64)
numpy operation in the stated order, so the equality with the host compile is bit for bit."""
import ctypes as C
import math as _math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
T_VALID, T_NEAR, T_MED = F(0.1), F(15.0), F(30.0)
DEPTHS = (2.0, 8.0, 15.0, 20.0, 30.0, 33.0, 39.99, 45.0, 26.0 / 256.0, 25.0 / 256.0)
MAX_DEPTH = 40.0


# ---- footprints and borders ------------------------------------------------------------------------------------------------------------------
def cross(k):
    f = np.zeros((k, k), bool); f[k // 2, :] = True; f[:, k // 2] = True
    return f


def full(k):
    return np.ones((k, k), bool)


def _morph(img, fp, is_max):
    """dilate / erode with a border that never wins: taps outside the image are ignored."""
    R, Cn = img.shape
    h = fp.shape[0] // 2
    pad = np.full((R + 2 * h, Cn + 2 * h), -np.inf if is_max else np.inf, F)
    pad[h:h + R, h:h + Cn] = img
    out = None
    for dr in range(-h, h + 1):
        for dc in range(-h, h + 1):
            if not fp[dr + h, dc + h]:
                continue
            v = pad[h + dr:h + dr + R, h + dc:h + dc + Cn]
            out = v.copy() if out is None else (np.maximum(out, v) if is_max else np.minimum(out, v))
    return out


def dilate(img, fp):
    return _morph(img, fp, True)


def erode(img, fp):
    return _morph(img, fp, False)


def median5(img):
    """medianBlur(.., 5) on CV_32F: replicated border, the 13th smallest of 25."""
    R, Cn = img.shape
    pad = np.pad(img, 2, mode="edge")
    stack = np.stack([pad[dr:dr + R, dc:dc + Cn] for dr in range(5) for dc in range(5)])
    return np.sort(stack, axis=0)[12]


def top_mask(valid):
    """row >= the first valid row of the column; a column without one counts from row 0 (ArgMax of an all-zero column)."""
    top = np.argmax(valid, axis=0)
    return np.arange(valid.shape[0])[:, None] >= top[None, :]


def sel(m, b, a):
    return np.where(m, b, a).astype(F)


def reflect101(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


# ---- exp_neg and the bilateral ----------------------------------------------------------------------------------------------------------------
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
TAYLOR = [1.0 / _math.factorial(i) for i in range(14)]           # 1 / i!, correctly rounded (i! is exact in a double)
WS = {0: 1.0, 1: 0.8824969025845955, 2: 0.7788007830714049, 4: 0.6065306597126334}


def exp_neg(x):
    """e^-x for x >= 0 from + * and bit operations only: Cody-Waite reduction by ln 2, the degree-13 Taylor polynomial in Horner order, 0.0 for x >= 708."""
    x = np.asarray(x, np.float64)
    big = x >= 708.0
    xs = np.where(big, 0.0, x)
    k = (xs * INV_LN2 + 0.5).astype(np.int64)
    kd = k.astype(np.float64)
    r = (kd * LN2_HI - xs) + kd * LN2_LO
    p = np.full(xs.shape, TAYLOR[13])
    for i in range(12, -1, -1):
        p = p * r + TAYLOR[i]
    s = ((1023 - k).astype(np.uint64) << np.uint64(52)).view(np.float64)
    return np.where(big, 0.0, p * s)


def bilateral(img):
    """Our bilateral (the header's deliberate divergence): 13 taps, dy then dx ascending, reflect-101, fp64 weights WS * exp_neg(2 D^2), ascending sums."""
    R, Cn = img.shape
    ri = np.array([[reflect101(r + d, R) for r in range(R)] for d in range(-2, 3)])
    ci = np.array([[reflect101(c + d, Cn) for c in range(Cn)] for d in range(-2, 3)])
    c64 = img.astype(np.float64)
    sw = np.zeros((R, Cn)); sv = np.zeros((R, Cn))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            d2 = dy * dy + dx * dx
            if d2 > 4:
                continue
            t = img[ri[dy + 2]][:, ci[dx + 2]].astype(np.float64)
            dl = t - c64
            w = WS[d2] * exp_neg(2.0 * (dl * dl))
            sw = sw + w
            sv = sv + w * t
    return (sv / sw).astype(F)


def bilateral_args(img):
    """every 2 D^2 the bilateral of img evaluates exp_neg at"""
    R, Cn = img.shape
    ri = np.array([[reflect101(r + d, R) for r in range(R)] for d in range(-2, 3)])
    ci = np.array([[reflect101(c + d, Cn) for c in range(Cn)] for d in range(-2, 3)])
    c64 = img.astype(np.float64)
    out = []
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dy * dy + dx * dx <= 4:
                dl = img[ri[dy + 2]][:, ci[dx + 2]].astype(np.float64) - c64
                out.append((2.0 * (dl * dl)).ravel())
    return np.unique(np.concatenate(out))


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------------
def to_u16(out):
    x = (out * F(256.0)).astype(F)
    return np.clip(np.rint(x), 0, 65535).astype(np.uint16)


def complete(d, max_depth, blend=sel):
    """DepthCompletion of one fp32 image.  Returns a dict: out (fp32), u16, and the counts the tests assert on.  blend: sel, or upstream's multiply-add form."""
    d = np.asarray(d, F)
    M = F(max_depth)
    s0 = blend(d <= M, d, np.zeros_like(d))
    near = (s0 > T_VALID) & (s0 <= T_NEAR); med = (s0 > T_NEAR) & (s0 <= T_MED); far = s0 > T_MED; v = s0 > T_VALID
    s1 = blend(v, (M - s0).astype(F), s0)
    valid_in = int(v.sum())
    zero = np.zeros_like(s1)
    df = dilate(blend(far, s1, zero), cross(3)); dm = dilate(blend(med, s1, zero), cross(5)); dn = dilate(blend(near, s1, zero), cross(7))
    s2 = s1
    s2 = blend(df > T_VALID, df, s2); s2 = blend(dm > T_VALID, dm, s2); s2 = blend(dn > T_VALID, dn, s2)
    s3 = erode(dilate(s2, full(5)), full(5))
    s4 = blend(s3 > T_VALID, median5(s3), s3)
    tm = top_mask(s4 > T_VALID)
    s5 = blend(~(s4 > T_VALID) & tm, dilate(s4, full(9)), s4)
    tm2 = top_mask(s5 > T_VALID)
    s7 = s5
    work = []
    for _ in range(6):
        e = (s7 < T_VALID) & tm2
        work.append(int(e.sum()))
        s7 = blend(e, dilate(s7, full(5)), s7)
    unfilled = int(((s7 < T_VALID) & tm2).sum())
    v = (s7 > T_VALID) & tm2
    s7 = blend(v, median5(s7), s7)
    s7b = s7
    s7 = blend(v, bilateral(s7), s7)
    out = blend(s7 > T_VALID, (M - s7).astype(F), s7)
    return dict(out=out, u16=to_u16(out), s7b=s7b, round_work=work, unfilled=unfilled, bands=(int(near.sum()), int(med.sum()), int(far.sum())),
                valid_in=valid_in, valid_out=int((out > T_VALID).sum()), cut_top=int((~tm2).sum()))


def muladd(m, b, a):
    """upstream's blend: a.mul(1 - m) + b.mul(m), m a 0 / 1 float image"""
    mf = np.asarray(m).astype(F)
    return (a * (F(1.0) - mf) + b * mf).astype(F)


# ---- the tests' input recipe -----------------------------------------------------------------------------------------------------------------
def recipe(rows, cols, p, seed=7, empty_col=None, bottom_col=None, top_col=None):
    """A sparse uint16 image: a share p of the pixels gets a depth of DEPTHS (x 256); the top fifth of the rows is empty; a 3-column stripe is empty (an empty
    column); one column is valid in the last row only and one in row 0.  The special columns default to places spread over the width."""
    rng = np.random.default_rng(seed)
    img = np.zeros((rows, cols), np.uint16)
    hit = rng.random((rows, cols)) < p
    vals = np.round(np.array(DEPTHS) * 256.0).astype(np.int64)
    img[hit] = vals[rng.integers(0, len(vals), int(hit.sum()))].astype(np.uint16)
    img[:rows // 5] = 0
    ec = cols // 3 if empty_col is None else empty_col
    bc = (2 * cols) // 3 if bottom_col is None else bottom_col
    tc = cols - 1 if top_col is None else top_col
    img[:, ec:ec + 3] = 0
    if bc < cols and not ec <= bc < ec + 3:
        img[:, bc] = 0; img[rows - 1, bc] = 2 * 256
    if tc < cols and not ec <= tc < ec + 3 and tc != bc:
        img[0, tc] = 8 * 256
    return img


def as_f32(u16):
    return (np.asarray(u16).astype(F) * F(1.0 / 256.0)).astype(F)


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------------
_CHECK = None


def build_check():
    global _CHECK
    if _CHECK is None:
        out = os.path.join(ROOT, "build", "libdepthfill_check.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out,
                               os.path.join(ROOT, "tests", "cpp", "depthfill_core_check.cpp")])
        _CHECK = C.CDLL(out)
        _CHECK.chk_median25.restype = C.c_float
    return _CHECK


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def host_completion(sparse, max_depth, n_threads=4):
    """chk_depth_completion on one image or a batch (uint16 or float32).  Returns (rc, dense float32, dense uint16, (valid_in, valid_out))."""
    sparse = np.ascontiguousarray(sparse)
    n = 1 if sparse.ndim == 2 else sparse.shape[0]
    rows, cols = sparse.shape[-2:]
    dense = np.zeros(sparse.shape, F); u16 = np.zeros(sparse.shape, np.uint16); st = np.zeros(2, np.int64)
    is16 = sparse.dtype == np.uint16
    rc = build_check().chk_depth_completion(C.c_int(rows), C.c_int(cols), C.c_int(n), _ptr(sparse if is16 else None), _ptr(None if is16 else sparse), C.c_float(max_depth),
                                            _ptr(dense), _ptr(u16), C.c_int(n_threads), _ptr(st))
    return rc, dense, u16, (int(st[0]), int(st[1]))


def host_depth_images(rows, cols, clouds, T_cl, size, max_depth, first_point=None, n_threads=4):
    clouds = [np.ascontiguousarray(c, F).reshape(-1, 3) for c in clouds]
    first = np.zeros(len(clouds) + 1, np.int64); first[1:] = np.cumsum([len(c) for c in clouds])
    if first_point is not None:
        first = np.ascontiguousarray(first_point, np.int64)
    xyz = np.ascontiguousarray(np.concatenate(clouds + [np.zeros((1, 3), F)]))
    T = np.ascontiguousarray(T_cl, np.float64).reshape(16)
    out = np.zeros((len(clouds), rows, cols), np.uint16)
    rc = build_check().chk_depth_images(C.c_int(rows), C.c_int(cols), C.c_int(len(clouds)), _ptr(first), _ptr(xyz), _ptr(T), C.c_uint(size), C.c_float(max_depth), _ptr(out),
                                        C.c_int(n_threads))
    return rc, out


def host_exp_neg(x):
    x = np.ascontiguousarray(x, np.float64); out = np.zeros_like(x)
    build_check().chk_exp_neg(C.c_longlong(x.size), _ptr(x), _ptr(out))
    return out


def synthetic_cloud(n, seed, radius=(1.0, 6.0)):
    """n LiDAR points on a VLP-16 like fan: 16 elevation rings, uniform azimuth, ranges in `radius`."""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-np.pi, np.pi, n); el = np.deg2rad(rng.integers(0, 16, n) * 2.0 - 15.0); rg = rng.uniform(radius[0], radius[1], n)
    return np.stack([rg * np.cos(el) * np.cos(az), rg * np.cos(el) * np.sin(az), rg * np.sin(el)], axis=1).astype(F)


T_CL = np.array([0, -1, 0, 0.02, 0, 0, -1, -0.05, 1, 0, 0, 0.01, 0, 0, 0, 1], np.float64)      # LiDAR x forward, z up -> camera z forward, y down
