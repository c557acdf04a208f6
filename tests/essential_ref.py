"""numpy restatement of K34 (ComputeEssential, the AC-RANSAC chain of FindEssentialACRANSAC with ACRansac_NFA::ComputeNFA, DecomposeEssential, SfM::CheckRT and the
selection over the runs of SfM::FilterImagePairs), the synthetic two-view scenes of the tests and the ctypes wrappers of the host compile
(tests/cpp/essential_core_check.cpp).  The restatement uses numpy.linalg.eigh / svd and the real arcsin / log10 / arccos, and the same Philox-4x32-10 stream as
panovlm_amd/csrc/pvlm_essential_core.h: it agrees with the core by tolerance, and decision for decision on a scene whose decisions are not marginal."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH_DTYPE = np.dtype([("query", np.int32), ("train", np.int32), ("distance", np.float32)])
N_LDS = 1024
FRESH = 0x800
M32 = 0xFFFFFFFF


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------
def philox(c, k):
    c = list(c); k0, k1 = k
    for _ in range(10):
        a = 0xD2511F53 * c[0]; b = 0xCD9E8D57 * c[2]
        c = [(b >> 32) ^ c[1] ^ k0, b & M32, (a >> 32) ^ c[3] ^ k1, a & M32]
        k0 = (k0 + 0x9E3779B9) & M32; k1 = (k1 + 0xBB67AE85) & M32
    return c


def chain_key(seed, src, tgt, run):
    o = philox((src & M32, tgt & M32, run & M32, 0), (seed & M32, (seed >> 32) & M32))
    return o[0], o[1]


def sample8(key, k, m):
    if m == 8:
        return list(range(8))
    out, j = [], 0
    while len(out) < 8:
        for w in philox((k, j, 0, 0), key):
            i = (w * m) >> 32
            if i not in out and len(out) < 8:
                out.append(i)
        j += 1
    return out


def compute_essential(p1, p2):
    p1 = np.asarray(p1, np.float64); p2 = np.asarray(p2, np.float64)
    A = (p2[:, :, None] * p1[:, None, :]).reshape(-1, 9)
    w, v = np.linalg.eigh(A.T @ A)
    U, s, Vt = np.linalg.svd(v[:, 0].reshape(3, 3))
    return U @ np.diag([s[0], s[1], 0.0]) @ Vt, w, s


def residuals(E, p1, p2):
    q = p1.astype(np.float64) @ E.T
    z = (q * q).sum(1, keepdims=True)
    q = np.where(z > 0, q / np.sqrt(np.where(z > 0, z, 1)), q)
    with np.errstate(invalid="ignore"):
        return np.arcsin((p2.astype(np.float64) * q).sum(1)) ** 2


def nfa_tables(n):
    lg = np.concatenate([[0.0], np.log10(np.arange(1, n + 1))])
    ck = np.zeros(n + 1); cn = np.zeros(n + 1)
    for k in range(9, n + 1):
        ck[k] = ck[k - 1] + lg[k] - lg[k - 8]
    cn[1] = lg[n]
    for k in range(2, n + 1):
        cn[k] = cn[k - 1] + lg[n - k + 1] - lg[k]
    return np.log10(float(n - 8)), np.log10(0.5), cn, ck


def run_chain(b1, b2, m, seed, src, tgt, run, max_iterations, flags=0):
    """One chain.  Returns a dict: E, nfa, inliers (sorted-residual order), betters [(iteration, nfa)], iterations, gap: the smallest relative distance of any NFA
    comparison that decided something (the best of a scan against the runner-up, a hypothesis' NFA against minNFA, minNFA against 0)."""
    n = len(m)
    p1 = b1[m["query"]]; p2 = b2[m["train"]]
    log_e0, log_a0, cn, ck = nfa_tables(n)
    key = chain_key(seed, src, tgt, run)
    reserved = max_iterations // 10; limit = max_iterations - reserved
    minNFA = np.inf; bestE = np.zeros((3, 3)); cur = np.arange(n); it = 0; betters = []; gap = np.inf
    s1, s2 = [], []
    ks = np.arange(9, n + 1)
    while it < limit and it < max_iterations:
        pos = sample8(key, it, len(cur))
        if flags & FRESH:
            s1, s2 = [], []
        s1 += [p1[cur[i]] for i in pos]; s2 += [p2[cur[i]] for i in pos]
        E = compute_essential(np.array(s1), np.array(s2))[0]
        res = residuals(E, p1, p2)
        res = np.where(np.isnan(res), np.inf, res)
        order = np.lexsort((np.arange(n), res))
        sr = res[order]
        with np.errstate(divide="ignore"):
            nfa = log_e0 + (log_a0 + 0.25 * np.log10(sr[8:] + 2.0 ** -23)) * (ks - 8) + cn[9:] + ck[9:]
        nfa = np.where(np.isfinite(sr[8:]), nfa, np.inf)
        best_k = 0; best = np.inf
        if np.any(nfa < np.inf):
            j = int(np.argmin(nfa)); best = nfa[j]; best_k = int(ks[j])
            others = np.delete(nfa, j)
            if len(others):
                gap = min(gap, abs(others.min() - best) / max(abs(best), 1.0))
        better = best_k > 8 and best < minNFA
        if best_k > 8 and np.isfinite(minNFA):
            gap = min(gap, abs(best - minNFA) / max(abs(best), 1.0))
        if better:
            minNFA = best; bestE = E; betters.append((it, best))
            gap = min(gap, abs(minNFA) / 1.0)
        if (better and minNFA < 0) or (it + 1 == limit and reserved > 0):
            if best_k == 0:
                limit += 1; reserved -= 1
            else:
                cur = order[:best_k]
                if reserved > 0:
                    limit = it + 1 + reserved; reserved = 0
        it += 1
    model = not (minNFA >= 0)
    return dict(E=bestE if model else np.zeros((3, 3)), nfa=minNFA, inliers=np.array(cur if model else [], np.int64), betters=betters, iterations=it, gap=gap)


def decompose(E):
    U, _, Vt = np.linalg.svd(E)
    t = U[:, 2] / np.linalg.norm(U[:, 2])
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    r1 = U @ W @ Vt; r2 = U @ W.T @ Vt
    r1 = -r1 if np.linalg.det(r1) < 0 else r1
    r2 = -r2 if np.linalg.det(r2) < 0 else r2
    return [r1, r1, r2, r2], [t, -t, t, -t]


def triangulate_2view(R, t, p1, p2):
    p1 = p1.astype(np.float64); p2 = p2.astype(np.float64)
    t12 = -R.T @ t; b2 = p2 @ R                                          # rows: R^T p2
    out = np.full((len(p1), 3), np.nan)
    for i in range(len(p1)):
        A = np.array([[p1[i] @ p1[i], -(p1[i] @ b2[i])], [b2[i] @ p1[i], -(b2[i] @ b2[i])]])
        rhs = np.array([p1[i] @ t12, b2[i] @ t12])
        with np.errstate(all="ignore"):
            try:
                lam = np.linalg.solve(A, rhs)
            except np.linalg.LinAlgError:
                continue
        out[i] = (lam[0] * p1[i] + lam[1] * b2[i] + t12) / 2
    return out


def _angle_deg(a, b):
    with np.errstate(all="ignore"):
        c = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        return np.degrees(np.arccos(np.clip(c, -1, 1)))


def check_rt(R, t, p1, p2, sel):
    """CheckRT on the matches `sel` (ascending).  Returns (indices that count, their points)."""
    P = triangulate_2view(R, t, p1[sel], p2[sel])
    ok = np.isfinite(P).all(1)
    with np.errstate(all="ignore"):
        a1 = _angle_deg(P, p1[sel].astype(np.float64)); a2 = _angle_deg(P @ R.T + t, p2[sel].astype(np.float64))
    ok &= ~(a1 > 3) & ~(a2 > 3)
    return np.asarray(sel)[ok], P[ok]


def filter_pair(b1, b2, m, seed, src, tgt, n_runs, max_iterations, tri_threshold, flags=0):
    """The loop body of FilterImagePairs for one pair.  Returns a dict: keep, R, t, inlier_idx, triangulated, reasons (per run: 'zero', 'few', 'similar', 'ok')."""
    out = dict(keep=0, R=np.zeros((3, 3)), t=np.zeros(3), inlier_idx=np.zeros(0, np.int64), triangulated=np.zeros((0, 3)), reasons=[])
    if len(m) <= 8:
        return out
    p1 = b1[m["query"]]; p2 = b2[m["train"]]
    best = -1
    for run in range(n_runs):
        ch = run_chain(b1, b2, m, seed, src, tgt, run, max_iterations, flags)
        if len(ch["inliers"]) == 0:
            out["reasons"].append("zero"); continue
        sel = np.sort(ch["inliers"])
        Rs, ts = decompose(ch["E"])
        cand = [check_rt(Rs[j], ts[j], p1, p2, sel) for j in range(4)]
        num = [len(c[0]) for c in cand]
        j = int(np.argmax(num))
        if num[j] < tri_threshold:
            out["reasons"].append("few"); continue
        if sum(1 for x in num if x > 0.8 * num[j]) > 1:
            out["reasons"].append("similar"); continue
        out["reasons"].append("ok")
        if num[j] > best:
            best = num[j]
            out.update(keep=1, R=Rs[j], t=ts[j], inlier_idx=cand[j][0], triangulated=cand[j][1])
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def rodrigues(w):
    w = np.asarray(w, np.float64); th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def two_view_scene(rng, n, outlier_fraction=0.3, t=(1.0, 0.2, -0.1), w=(0.05, -0.2, 0.1), shuffle=True):
    """n matches between two spherical views: X_2 = R X_1 + t, bearings exact to float rounding; a fraction of the matches gets a random second bearing.  The keypoints of
    both frames are permuted, so that query != train.  Returns (b1, b2, matches, inlier mask per match, R, t)."""
    R = rodrigues(w); t = np.asarray(t, np.float64)
    X = rng.uniform(-4, 4, size=(n, 3)); X[np.linalg.norm(X, axis=1) < 0.5] += 1.5
    Y = X @ R.T + t
    n_out = int(round(outlier_fraction * n))
    inl = np.ones(n, bool); inl[rng.permutation(n)[:n_out]] = False
    Y[~inl] = rng.normal(size=(n_out, 3))
    b1 = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    b2 = (Y / np.linalg.norm(Y, axis=1, keepdims=True)).astype(np.float32)
    q = rng.permutation(n) if shuffle else np.arange(n); tr = rng.permutation(n) if shuffle else np.arange(n)
    f1 = np.zeros_like(b1); f2 = np.zeros_like(b2); f1[q] = b1; f2[tr] = b2
    m = np.zeros(n, MATCH_DTYPE); m["query"] = q; m["train"] = tr; m["distance"] = 1.0
    return f1, f2, m, inl, R, t


def rotation_error_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def direction_error_deg(a, b):
    return float(np.degrees(np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1, 1))))


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------
def build_check():
    out = os.path.join(ROOT, "build", "libessential_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out, os.path.join(ROOT, "tests", "cpp", "essential_core_check.cpp")])
    lib = C.CDLL(out)
    lib.chk_ess_angle_threshold.restype = C.c_double
    return lib


def build_check_main(sanitize=True):
    """The stand-alone program of the same file (its own main), with the host sanitizers."""
    out = os.path.join(ROOT, "build", "essential_check_main")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DESSENTIAL_CHECK_MAIN"] + san +
                          ["-o", out, os.path.join(ROOT, "tests", "cpp", "essential_core_check.cpp")])
    return out


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_fn(chk, name, x):
    x = np.ascontiguousarray(x, np.float64); y = np.zeros_like(x)
    getattr(chk, name)(_ptr(x), C.c_int(len(x)), _ptr(y))
    return y


def host_sample8(chk, seed, src, tgt, run, k, m):
    out = np.zeros(8, np.int32)
    chk.chk_ess_sample8(C.c_ulonglong(seed), C.c_int(src), C.c_int(tgt), C.c_int(run), C.c_int(k), C.c_int(m), _ptr(out))
    return out.tolist()


def host_compute(chk, p1, p2):
    p1 = np.ascontiguousarray(p1, np.float32); p2 = np.ascontiguousarray(p2, np.float32)
    E = np.zeros((3, 3)); sv = np.zeros(3)
    chk.chk_ess_compute(_ptr(p1), _ptr(p2), C.c_int(len(p1)), _ptr(E), _ptr(sv))
    return E, sv


def host_decompose(chk, E):
    E = np.ascontiguousarray(E, np.float64); R = np.zeros((4, 3, 3)); t = np.zeros((4, 3))
    chk.chk_ess_decompose(_ptr(E), _ptr(R), _ptr(t))
    return R, t


def host_chain(chk, b1, b2, m, seed, src, tgt, run, max_iterations, flags=0):
    b1 = np.ascontiguousarray(b1, np.float32); b2 = np.ascontiguousarray(b2, np.float32); m = np.ascontiguousarray(m, MATCH_DTYPE)
    E = np.zeros((3, 3)); nfa = C.c_double(); it = C.c_int(); nb = C.c_int()
    inl = np.zeros(len(m), np.int32); bi = np.zeros(max_iterations, np.int32); bn = np.zeros(max_iterations)
    k = chk.chk_ess_chain(_ptr(b1), _ptr(b2), _ptr(m), C.c_int(len(m)), C.c_ulonglong(seed), C.c_int(src), C.c_int(tgt), C.c_int(run), C.c_int(max_iterations), C.c_uint(flags),
                          _ptr(E), C.byref(nfa), C.byref(it), _ptr(inl), _ptr(bi), _ptr(bn), C.byref(nb))
    return dict(E=E, nfa=nfa.value, iterations=it.value, inliers=inl[:k].astype(np.int64), betters=list(zip(bi[:nb.value].tolist(), bn[:nb.value].tolist())))


def _flat(bearings):
    arrs = [np.ascontiguousarray(b, np.float32).reshape(-1, 3) for b in bearings]
    rows = np.array([len(a) for a in arrs], np.int32)
    return rows, np.ascontiguousarray(np.concatenate(arrs + [np.zeros((1, 3), np.float32)]))


def host_acransac(chk, bearings, src, tgt, off, m, n_runs, max_iterations, seed, flags=0, threads=8):
    """The host loop of the raw entry.  Returns (rc, dict like api.essential_acransac)."""
    rows, flat = _flat(bearings)
    src = np.ascontiguousarray(src, np.int32); tgt = np.ascontiguousarray(tgt, np.int32); off = np.ascontiguousarray(off, np.int64); m = np.ascontiguousarray(m, MATCH_DTYPE)
    nc = len(src) * max(n_runs, 0)
    E = np.zeros((len(src), max(n_runs, 0), 3, 3)); nfa = np.zeros((len(src), max(n_runs, 0))); ioff = np.zeros(nc + 1, np.int64)
    inl = np.zeros(max(len(m) * max(n_runs, 0), 1), np.int32); st = np.zeros(4, np.int64)
    rc = chk.chk_ess_acransac(C.c_int(len(rows)), _ptr(rows), _ptr(flat), C.c_int(len(src)), _ptr(src), _ptr(tgt), _ptr(off), _ptr(m), C.c_int(n_runs), C.c_int(max_iterations),
                              C.c_ulonglong(seed), C.c_uint(flags), C.c_int(threads), _ptr(E), _ptr(nfa), _ptr(ioff), _ptr(inl), _ptr(st))
    return rc, dict(E=E, nfa=nfa, offsets=ioff, inliers=inl[:ioff[-1]], chains=int(st[0]), hypotheses=int(st[1]))


def host_filter(chk, bearings, src, tgt, off, m, tri_threshold, n_runs, max_iterations, seed, flags=0, threads=8):
    """The host loop of the filter entry.  Returns (rc, dict like api.filter_image_pairs)."""
    rows, flat = _flat(bearings)
    src = np.ascontiguousarray(src, np.int32); tgt = np.ascontiguousarray(tgt, np.int32); off = np.ascontiguousarray(off, np.int64); m = np.ascontiguousarray(m, MATCH_DTYPE)
    keep = np.zeros(len(src), np.uint8); R = np.zeros((len(src), 3, 3)); t = np.zeros((len(src), 3)); ioff = np.zeros(len(src) + 1, np.int64)
    idx = np.zeros(max(len(m), 1), np.int32); tri = np.zeros((max(len(m), 1), 3)); st = np.zeros(4, np.int64)
    rc = chk.chk_ess_filter(C.c_int(len(rows)), _ptr(rows), _ptr(flat), C.c_int(len(src)), _ptr(src), _ptr(tgt), _ptr(off), _ptr(m), C.c_int(n_runs), C.c_int(max_iterations),
                            C.c_int(tri_threshold), C.c_ulonglong(seed), C.c_uint(flags), C.c_int(threads), _ptr(keep), _ptr(R), _ptr(t), _ptr(ioff), _ptr(idx), _ptr(tri), _ptr(st))
    return rc, dict(keep=keep, R_21=R, t_21=t, offsets=ioff, inlier_idx=idx[:ioff[-1]], triangulated=tri[:ioff[-1]], chains=int(st[0]), hypotheses=int(st[1]))
