"""numpy restatement of K35 (the k-means codebook, the VLAD embedding and the neighbour lists of sfm/VLAD.cpp as panovlm_amd/csrc/pvlm_vlad_core.h states them), the
generators of the tests' descriptors and the ctypes wrappers of the host compile (tests/cpp/vlad_core_check.cpp).  A sequential chain is np.cumsum in the stated
dtype behind a leading zero (cumsum adds in index order), so the restatement follows the header's summation orders exactly.  The d2 chain c = fmaf(t, t, c) is
evaluated as float32(float64(t) * float64(t) + float64(c)): the product is exact in float64, the sum is rounded twice instead of once, which can move a d2 by one
float ulp in about 2^-29 of the steps; nearest_centres therefore reports the smallest relative gap between the best and the second-best centre, and the tests assert
that no gap is that small wherever they do not tie rows on purpose (an exact tie is exact in both evaluations)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import match_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 128
U = 2.0 ** -24
# Type 2 against numpy's pow.  Let u be the block-step values with numpy's pow and w the header's: |w_k - u_k| <= EPS |u_k| with EPS = 2^-23 (one float ulp).  The
# norm is 1-Lipschitz: | |w| - |u| | <= |w - u| <= EPS |u|; its fp64 evaluation (D squares, D additions, one sqrt, D = 128 book_size) is off by at most
# G = (D + 2) 2^-53 relatively on either side.  The quotient in fp64 and its rounding to float add 2^-53 and U = 2^-24 on either side.  So
# |w_k / N_w - u_k / N_u| <= |u_k / N_u| ((1 + EPS)(1 + G) / ((1 - EPS)(1 - G)) - 1 + 2 (U + 2^-53)), plus the float denormal spacing.
def type2_rel_bound(book_size):
    eps = 2.0 ** -23
    g = (DIM * book_size + 2) * 2.0 ** -53
    return (1 + eps) * (1 + g) / ((1 - eps) * (1 - g)) - 1 + 2 * (U + 2.0 ** -53)


def build_check():
    out = os.path.join(ROOT, "build", "libvlad_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out, os.path.join(ROOT, "tests", "cpp", "vlad_core_check.cpp")])
    lib = C.CDLL(out)
    lib.chk_root5.restype = C.c_double
    lib.chk_root5.argtypes = [C.c_double]
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _frames(descs):
    descs = [np.ascontiguousarray(d, np.float32).reshape(-1, DIM) for d in descs]
    rows = np.array([len(d) for d in descs], np.int32)
    flat = np.ascontiguousarray(np.concatenate(descs + [np.zeros((1, DIM), np.float32)]))
    return descs, rows, flat


def _chain(x, dtype, axis=0):
    """The last value of the sequential chain 0 + x[0] + x[1] + ... along `axis` in `dtype`."""
    x = np.asarray(x, dtype)
    z = np.zeros_like(np.take(x, [0], axis=axis)) if x.shape[axis] else np.zeros(tuple(1 if a == axis else s for a, s in enumerate(x.shape)), dtype)
    return np.take(np.cumsum(np.concatenate([z, x], axis=axis), axis=axis, dtype=dtype), -1, axis=axis)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
def d2_chains(X, Cn):
    """d2 of every row of X against every row of Cn by the k-ascending chain (see the module docstring); float32, rows x centres."""
    X = np.asarray(X, np.float32); Cn = np.asarray(Cn, np.float32)
    c = np.zeros((len(X), len(Cn)), np.float32)
    for k in range(DIM):
        t = (X[:, k, None] - Cn[None, :, k]).astype(np.float64)
        c = (t * t + c.astype(np.float64)).astype(np.float32)
    return c


def nearest_centres(X, codebook, alive):
    """(centre index per row, the smallest relative gap between the best and the second-best d2 that is not an exact tie)."""
    ids = np.nonzero(alive)[0]
    d2 = d2_chains(X, codebook[ids])
    best = np.argmin(d2, axis=1)                                    # the first minimum: an exact tie goes to the lower index
    gap = np.inf
    if len(ids) > 1 and len(X):
        s = np.sort(d2.astype(np.float64), axis=1)
        rel = (s[:, 1] - s[:, 0]) / np.maximum(s[:, 1], 1e-300)
        rel = rel[s[:, 1] != s[:, 0]]
        gap = rel.min() if len(rel) else np.inf
    return ids[best].astype(np.int32), gap


def chunked_mean(rows, chunk):
    """(float)(S / count), S the fp64 sum in runs of `chunk` ascending members, the run sums added in ascending order."""
    runs = [_chain(rows[a:a + chunk], np.float64) for a in range(0, len(rows), chunk)]
    return (_chain(np.array(runs), np.float64) / np.float64(len(rows))).astype(np.float32)


def ref_kmeans(X, book_size, max_iterations, init_rows, chunk):
    """Returns codebook, alive, assign, iterations, the smallest gap met."""
    X = np.asarray(X, np.float32).reshape(-1, DIM)
    codebook = X[np.asarray(init_rows, np.int64)].copy()
    alive = np.ones(book_size, np.uint8); assign = np.zeros(len(X), np.int32)
    changed = True; it = 0; gap = np.inf
    while it < max_iterations and changed:
        near, g = nearest_centres(X, codebook, alive)
        gap = min(gap, g)
        changed = bool((near != assign).any())
        assign = near
        for c in range(book_size):
            if not alive[c]:
                continue
            m = X[assign == c]
            if len(m) == 0:
                alive[c] = 0; codebook[c] = 0
            else:
                codebook[c] = chunked_mean(m, chunk)
        it += 1
    return codebook, alive, assign, it, gap


def ref_embed(X, codebook, alive, normalization):
    """The VLAD vector of one frame (float32, 128 * book_size) and the smallest nearest-centre gap."""
    X = np.asarray(X, np.float32).reshape(-1, DIM)
    book = len(codebook)
    alive = np.ones(book, np.uint8) if alive is None else np.asarray(alive, np.uint8)
    v = np.zeros((book, DIM), np.float32); gap = np.inf
    if len(X) and alive.any():
        near, gap = nearest_centres(X, codebook, alive)
        r = X - codebook[near]
        keep = np.ones(len(X), bool)
        if normalization == 2:
            n = np.sqrt(_chain(r.astype(np.float64) ** 2, np.float64, axis=1))
            keep = n != 0
            with np.errstate(invalid="ignore", divide="ignore"):
                r = (r.astype(np.float64) / n[:, None]).astype(np.float32)
        for c in range(book):
            v[c] = _chain(r[keep & (near == c)], np.float32)
    for c in range(book):
        b = v[c]
        if normalization == 0:
            v[c] = np.sign(b) * np.sqrt(np.abs(b))
        elif normalization == 1:
            bn = np.sqrt(_chain(b.astype(np.float64) ** 2, np.float64))
            if bn != 0:
                v[c] = (b.astype(np.float64) / bn).astype(np.float32)
        else:
            v[c] = np.sign(b) * np.power(np.abs(b).astype(np.float64), 0.2).astype(np.float32)
    N = np.sqrt(_chain(np.array([_chain(v[c].astype(np.float64) ** 2, np.float64) for c in range(book)]), np.float64))
    if N != 0:
        v = (v.astype(np.float64) / N).astype(np.float32)
    return v.reshape(-1), gap


def ref_neighbors(V, neighbor_size):
    V = np.asarray(V, np.float32)
    n = len(V)
    V64 = V.astype(np.float64)
    sim = np.array([[_chain(V64[i] * V64[j], np.float64) for j in range(n)] for i in range(n)]).reshape(n, n)
    m = min(neighbor_size, n)
    nb = np.array([np.lexsort((np.arange(n), -sim[i]))[:m] for i in range(n)], np.int32).reshape(n, m)
    return nb, sim


# ---- generators ------------------------------------------------------------------------------------------------------------------------------
ROWS = [0, 1, 33, 300, 127, 257]


def int_frames(rng, rows=ROWS):
    """Raw-SIFT-like rows in 0..255 drawn around a few prototypes, so that k-means has something to find."""
    protos = rng.integers(0, 256, size=(6, DIM))
    out = []
    for n in rows:
        p = protos[rng.integers(0, len(protos), size=n)]
        out.append(np.clip(p + rng.integers(-40, 41, size=(n, DIM)), 0, 255).astype(np.float32))
    return out


def float_frames(rng, rows=ROWS):
    """RootSIFT-like rows (non-negative, unit norm)."""
    return [match_ref.float_descriptors(rng, n, 2)[0] if n else np.zeros((0, DIM), np.float32) for n in rows]


def retrieval_scene(rng, groups=4, per_group=3, shared=120, own=20):
    """12 frames in 4 groups: the frames of a group share `shared` descriptor rows (RootSIFT-like), each perturbed, plus `own` rows of their own."""
    def root(x):
        x = np.abs(x); x /= x.sum(1, keepdims=True)
        return np.sqrt(x).astype(np.float32)
    frames = []
    for g in range(groups):
        base = rng.gamma(0.6, size=(shared, DIM))
        for _ in range(per_group):
            rows = np.concatenate([base + 0.02 * rng.gamma(0.6, size=base.shape), rng.gamma(0.6, size=(own, DIM))])
            frames.append(root(rows[rng.permutation(len(rows))]))
    return frames


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------
def host_kmeans(chk, descs, train_frames, book_size, max_iterations, init_rows, threads=4):
    """Returns (rc, codebook, alive, assign, iterations, dead_centres)."""
    descs, rows, flat = _frames(descs)
    tf = np.ascontiguousarray(train_frames, np.int32); init = np.ascontiguousarray(init_rows, np.int64)
    ok = (tf >= 0) & (tf < len(rows))
    n = int(rows[tf[ok]].sum())
    codebook = np.zeros((max(book_size, 1), DIM), np.float32); alive = np.zeros(max(book_size, 1), np.uint8); assign = np.zeros(max(n, 1), np.int32)
    it = C.c_int(0); dead = C.c_int(0)
    rc = chk.chk_vlad_kmeans(C.c_int(len(rows)), _ptr(rows), _ptr(flat), C.c_int(len(tf)), _ptr(tf), C.c_int(book_size), C.c_int(max_iterations), _ptr(init), C.c_int(threads),
                             _ptr(codebook), _ptr(alive), _ptr(assign), C.byref(it), C.byref(dead))
    return rc, codebook[:book_size], alive[:book_size], assign[:n], it.value, dead.value


def host_embed(chk, descs, codebook, alive, normalization, threads=4):
    descs, rows, flat = _frames(descs)
    codebook = np.ascontiguousarray(codebook, np.float32).reshape(-1, DIM)
    out = np.zeros((len(rows), DIM * len(codebook)), np.float32)
    a = None if alive is None else np.ascontiguousarray(alive, np.uint8)
    rc = chk.chk_vlad_embed(C.c_int(len(rows)), _ptr(rows), _ptr(flat), C.c_int(len(codebook)), _ptr(codebook), None if a is None else _ptr(a), C.c_int(normalization),
                            C.c_int(threads), _ptr(out))
    return rc, out


def host_neighbors(chk, V, book_size, neighbor_size, threads=4):
    V = np.ascontiguousarray(V, np.float32)
    n = len(V); m = max(min(neighbor_size, n), 0)
    nb = np.zeros((n, m), np.int32); sim = np.zeros((n, n), np.float64)
    rc = chk.chk_vlad_neighbors(_ptr(V), C.c_int(n), C.c_int(book_size), C.c_int(neighbor_size), C.c_int(threads), _ptr(nb), _ptr(sim))
    return rc, nb, sim


def host_root5_sweep(chk, threads=16):
    d = C.c_longlong(0); w = C.c_int(0)
    chk.chk_root5_sweep(C.c_int(threads), C.byref(d), C.byref(w))
    return d.value, w.value
