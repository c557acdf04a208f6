"""numpy restatement of K33 (brute-force 2-NN SIFT matching, the ratio test, the pair filter of SfM::MatchImagePairs), the generators of the tests' descriptors
and the ctypes wrappers of the host compile (tests/cpp/match_core_check.cpp).  For integer-valued descriptors in 0..255 every fp32 operation of the definition
is exact (a d2 is at most 128 * 255^2 < 2^24), so the int64 restatement IS the definition; for float descriptors the fp64 evaluation is the reference and the
derived bounds below say how far the fp32 definition may be from it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 128
MATCH_DTYPE = np.dtype([("query", np.int32), ("train", np.int32), ("distance", np.float32)])
U = 2.0 ** -24
# d2_c = D (1 + th), |th| <= g_130: the difference (1 rounding), its square inside the fmaf and 128 accumulations, all terms >= 0
REL_D2 = 130 * U / (1 - 130 * U)
# sqrt halves the relative error (to first order; the square term covers the rest) and rounds once
REL_DIST = REL_D2 / 2 + REL_D2 ** 2 + U


def build_check():
    out = os.path.join(ROOT, "build", "libmatch_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out, os.path.join(ROOT, "tests", "cpp", "match_core_check.cpp")])
    return C.CDLL(out)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _desc(a):
    a = np.ascontiguousarray(a, np.float32)
    return a if a.ndim == 2 else a.reshape(-1, DIM)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
def d2_matrix(A, B, dtype):
    A = _desc(A).astype(dtype); B = _desc(B).astype(dtype)
    return ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)


def knn2_from_d2(d2):
    """The two smallest (d2, index) per row: indices (-1 where absent) and the d2 values (inf where absent, float64)."""
    n1, n2 = d2.shape
    idx = np.full((n1, 2), -1, np.int32); val = np.full((n1, 2), np.inf)
    if n2 > 0:
        order = np.argsort(d2, axis=1, kind="stable")[:, :2]        # stable: an exact tie goes to the lower index
        k = order.shape[1]
        idx[:, :k] = order
        val[:, :k] = np.take_along_axis(d2, order, 1)
    return idx, val


def d2_matrix_int(A, B):
    """d2_matrix(A, B, np.int64) for integer-valued descriptors in 0..255 without the n1 x n2 x 128 cube: |a|^2 + |b|^2 - 2 a.b through a float64 matmul.
    Every term and every partial sum is an integer below 128 * 255^2 * 4 < 2^25, so float64 is exact whatever order the matmul adds in."""
    A = _desc(A).astype(np.float64); B = _desc(B).astype(np.float64)
    for M in (A, B):
        assert (M == np.rint(M)).all() and (M >= 0).all() and (M <= 255).all()
    return ((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)).astype(np.int64)


def ref_knn2_int(A, B):
    """Integer-valued descriptors: (idx, dist float32) exactly as the definition gives them."""
    idx, val = knn2_from_d2(d2_matrix_int(A, B))
    return idx, np.sqrt(val.astype(np.float32))                     # a d2 < 2^24 is exact in float32; float32 sqrt is correctly rounded


def ref_match_sift(idx, dist, ratio):
    """The ratio test in float32 on knn2 output; records in query order."""
    dist = dist.astype(np.float32)
    ok = (idx[:, 1] >= 0) & (dist[:, 0] < np.float32(ratio) * dist[:, 1])
    m = np.zeros(int(ok.sum()), MATCH_DTYPE)
    m["query"] = np.nonzero(ok)[0]; m["train"] = idx[ok, 0]; m["distance"] = dist[ok, 0]
    return m


def ref_pair_filter(m, threshold):
    """sfm/SfM.cpp:266-275.  Returns (keep, records)."""
    if len(m) < threshold:
        return False, m[:0]
    dmax = m["distance"].max() if len(m) else np.float32(0)
    good = m[m["distance"].astype(np.float64) < 0.8 * np.float64(dmax)]
    if len(good) < threshold:
        return False, m[:0]
    return True, good


# ---- generators ------------------------------------------------------------------------------------------------------------------------------
def int_descriptors(rng, n1, n2):
    """Raw-SIFT-like rows in 0..255 with what the tie rules need: duplicated train rows (ties, d0 == d1), a query equal to a train row (d0 = 0)."""
    A = rng.integers(0, 256, size=(n1, DIM)).astype(np.float32)
    B = rng.integers(0, 256, size=(n2, DIM)).astype(np.float32)
    if n1 >= 1 and n2 >= 2:
        for q in range(0, n1, 7):                                   # planted near neighbours: a few components off a train row
            j = int(rng.integers(0, n2))
            A[q] = B[j]
            A[q, rng.integers(0, DIM, size=5)] = rng.integers(0, 256, size=5)
        A[0] = B[n2 - 1]                                            # d0 = 0
    if n2 >= 5:
        B[n2 - 2] = B[1]                                            # a duplicated train row: the tie goes to index 1
        if n1 >= 3:
            A[2] = B[1]                                             # ... and d0 == d1 == 0 for this query: no match
            A[1] = B[1]; A[1, 3] = (A[1, 3] + 9) % 256              # ... and d0 == d1 > 0 for this one
    return A, B


def float_descriptors(rng, n1, n2, noise=0.02):
    """RootSIFT-like rows (non-negative, unit norm) with planted matches: every third query is a perturbed train row."""
    def root(x):
        x = np.abs(x); x /= x.sum(1, keepdims=True)
        return np.sqrt(x).astype(np.float32)
    B = root(rng.gamma(0.6, size=(n2, DIM)))
    A = root(rng.gamma(0.6, size=(n1, DIM)))
    planted = np.full(n1, -1)
    for q in range(0, n1, 3):
        j = int(rng.integers(0, n2)); planted[q] = j
        A[q] = root(B[j:j + 1].astype(np.float64) ** 2 + noise * rng.gamma(0.6, size=(1, DIM)) / DIM)[0]
    return A, B, planted


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------
def host_knn2(chk, A, B, plain=False):
    A = _desc(A); B = _desc(B)
    idx = np.zeros((len(A), 2), np.int32); dist = np.zeros((len(A), 2), np.float32)
    (chk.chk_match_knn2_plain if plain else chk.chk_match_knn2)(_ptr(A), C.c_int(len(A)), _ptr(B), C.c_int(len(B)), _ptr(idx), _ptr(dist))
    return idx, dist


def host_match_sift(chk, A, B, ratio):
    A = _desc(A); B = _desc(B)
    out = np.zeros(max(len(A), 1), MATCH_DTYPE)
    n = chk.chk_match_sift(_ptr(A), C.c_int(len(A)), _ptr(B), C.c_int(len(B)), C.c_float(ratio), _ptr(out))
    return out[:n]


def host_pair_filter(chk, m, threshold):
    m = np.ascontiguousarray(m.copy())
    buf = m if len(m) else np.zeros(1, MATCH_DTYPE)
    n = chk.chk_pair_filter(_ptr(buf), C.c_int(len(m)), C.c_int(threshold))
    return (False, m[:0]) if n < 0 else (True, buf[:n])


def host_match_pairs(chk, descs, src, tgt, ratio, threshold, threads=4):
    """The host loop.  Returns (rc, keep, offsets, records)."""
    descs = [_desc(d) for d in descs]
    rows = np.array([len(d) for d in descs], np.int32)
    flat = np.ascontiguousarray(np.concatenate(descs + [np.zeros((1, DIM), np.float32)]))
    src = np.ascontiguousarray(src, np.int32); tgt = np.ascontiguousarray(tgt, np.int32)
    keep = np.zeros(len(src), np.uint8); off = np.zeros(len(src) + 1, np.int64)
    ok = (src >= 0) & (src < len(rows))
    out = np.zeros(max(int(rows[src[ok]].sum()), 1), MATCH_DTYPE)
    rc = chk.chk_match_pairs(C.c_int(len(rows)), _ptr(rows), _ptr(flat), C.c_int(len(src)), _ptr(src), _ptr(tgt), C.c_float(ratio), C.c_int(threshold), C.c_int(threads),
                             _ptr(keep), _ptr(off), _ptr(out))
    return rc, keep, off, out[:off[-1]] if rc == 0 else out[:0]


def host_screen(chk, a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    s = C.c_float(); E = C.c_float(); d2 = C.c_float()
    chk.chk_screen(_ptr(a), _ptr(b), C.byref(s), C.byref(E), C.byref(d2))
    return s.value, E.value, d2.value
