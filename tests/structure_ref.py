"""numpy restatement of K32, written from the formulas of sfm/Triangulate.cpp:8-28, :117-139, :198-226, sfm/Structure.cpp:8-119,
base/Geometry.hpp:594-617 and util/Tracks.cpp:14-162: the two-view midpoint, the N-view algebraic eigenvector (numpy.linalg.eigh),
the inf skip rule, FilterTracksToFar, a literal TrackBuilder, and the generators of the tests (tests/test_structure_cpu.py, _gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import sfm_ba_ref as ba_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
U32_MAX = 0xFFFFFFFF


# ---- TriangulateNView -----------------------------------------------------------------------------------------------------------------
def two_view(T1, T2, b1, b2):
    """TriangulateNView's two-view branch on n tracks: T1, T2 n x 3 x 4 [R | t]_cw, b1, b2 n x 3 float32 bearings.  Returns the world
    points and cond(A) of the 2 x 2 system."""
    T1 = np.asarray(T1, np.float64); T2 = np.asarray(T2, np.float64)
    p1 = np.asarray(b1, np.float32).astype(np.float64); p2 = np.asarray(b2, np.float32).astype(np.float64)
    R1, t1, R2, t2 = T1[:, :, :3], T1[:, :, 3], T2[:, :, :3], T2[:, :, 3]
    with np.errstate(all="ignore"):
        R21 = np.einsum("nik,njk->nij", R2, R1)
        t21 = t2 - np.einsum("nij,nj->ni", R21, t1)
        t12 = -np.einsum("nji,nj->ni", R21, t21)
        q = np.einsum("nji,nj->ni", R21, p2)                       # bearing_2_in_1
        dot = lambda a, b: (a * b).sum(1)
        a00, a10, a01, a11 = dot(p1, p1), dot(q, p1), -dot(p1, q), -dot(q, q)
        r0, r1 = dot(p1, t12), dot(q, t12)
        invdet = 1.0 / (a00 * a11 - a10 * a01)
        l0 = (a11 * invdet) * r0 + (-a01 * invdet) * r1
        l1 = (-a10 * invdet) * r0 + (a00 * invdet) * r1
        P = (l0[:, None] * p1 + (l1[:, None] * q + t12)) / 2.0
        X = np.einsum("nji,nj->ni", R1, P) + (-np.einsum("nji,nj->ni", R1, t1))
        A = np.stack([np.stack([a00, a01], 1), np.stack([a10, a11], 1)], 1)
        cond = np.array([np.linalg.cond(a) if np.all(np.isfinite(a)) else np.inf for a in A])
    return X, cond


def ata_of_tracks(off, fid, bearings, T_cw):
    """AtA = sum cost^T cost, cost = P - n n^T P, per track: n_tracks x 4 x 4."""
    off = np.asarray(off, np.int64); T = np.asarray(T_cw, np.float64).reshape(-1, 3, 4)[np.asarray(fid)]
    b = np.asarray(bearings, np.float32).astype(np.float64)
    z = (b * b).sum(1)
    n = np.where(z[:, None] > 0, b / np.sqrt(np.where(z > 0, z, 1.0))[:, None], b)
    cost = T - np.einsum("ni,nj,njc->nic", n, n, T)
    per = np.einsum("nia,nib->nab", cost, cost)
    out = np.zeros((len(off) - 1, 4, 4))
    np.add.at(out, np.repeat(np.arange(len(off) - 1), np.diff(off)), per)
    return out


def n_view(off, fid, bearings, T_cw):
    """TriangulateNViewAlgebraic per track (every track, whatever its length): points, unit eigenvectors of the smallest eigenvalue, the
    eigenvalues ascending."""
    A = ata_of_tracks(off, fid, bearings, T_cw)
    w, V = np.linalg.eigh(A)
    v = V[:, :, 0]
    with np.errstate(all="ignore"):
        X = v[:, :3] / v[:, 3:4]
    return X, v, w, A


def triangulate_ref(off, fid, bearings, T_cw, frame_valid=None):
    """pvlm_triangulate_tracks on bearings: points and status (0 ok, 1 inf rule, 2 an observation in an invalid frame)."""
    off = np.asarray(off, np.int64); fid = np.asarray(fid); n = len(off) - 1
    T = np.asarray(T_cw, np.float64).reshape(-1, 3, 4); b = np.asarray(bearings, np.float32)
    X = np.full((n, 3), np.inf); length = np.diff(off)
    two = np.flatnonzero(length == 2)
    if len(two):
        i = off[two]
        X[two] = two_view(T[fid[i]], T[fid[i + 1]], b[i], b[i + 1])[0]
    many = np.flatnonzero(length > 2)
    if len(many):
        o2 = np.concatenate([[0], np.cumsum(length[many])])
        idx = np.concatenate([np.arange(off[t], off[t + 1]) for t in many])
        X[many] = n_view(o2, fid[idx], b[idx], T)[0]
    status = np.isinf(X).any(1).astype(np.uint8)
    if frame_valid is not None:
        fv = np.asarray(frame_valid, bool)
        bad = np.zeros(n, bool)
        np.logical_or.at(bad, np.repeat(np.arange(n), length), ~fv[fid])
        X[bad] = np.nan; status[bad] = 2
    return X, status


# ---- FilterTracksToFar ----------------------------------------------------------------------------------------------------------------
def filter_far_ref(off, fid, X, t_wc, threshold, frame_valid=None):
    """keep mask and average / (threshold baseline) per track (NaN where the comparison involves one)."""
    off = np.asarray(off, np.int64); fid = np.asarray(fid); X = np.asarray(X, np.float64); t_wc = np.asarray(t_wc, np.float64)
    n = len(off) - 1
    keep = np.ones(n, np.uint8); ratio = np.full(n, np.nan)
    for t in range(n):
        ids = sorted(set(int(f) for f in fid[off[t]:off[t + 1]]))
        c = [t_wc[f] for f in ids if frame_valid is None or frame_valid[f]]
        baseline = 0.0
        if len(c) > 1:
            baseline = -1.0
            for i in range(len(c) - 1):
                for j in range(i + 1, len(c)):
                    d = c[i] - c[j]
                    cur = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                    if cur > baseline:
                        baseline = cur
        s = 0.0
        for ci in c:
            d = ci - X[t]
            s = s + np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        with np.errstate(all="ignore"):
            avg = np.float64(s) / np.float64(len(c))
            if threshold * baseline < avg:
                keep[t] = 0
            ratio[t] = avg / (threshold * baseline)
    return keep, ratio


# ---- TrackBuilder, literally ------------------------------------------------------------------------------------------------------------
class UnionFind:
    def __init__(self, n):
        self.parent = list(range(n)); self.rank = [0] * n; self.size = [1] * n

    def find(self, i):
        if self.parent[i] != i:
            self.parent[i] = self.find(self.parent[i])
        return self.parent[i]

    def union(self, i, j):
        i = self.find(i); j = self.find(j)
        if i == j:
            return
        if self.rank[i] < self.rank[j]:
            self.parent[i] = j; self.size[j] += self.size[i]
        else:
            self.parent[j] = i; self.size[i] += self.size[j]
            if self.rank[i] == self.rank[j]:
                self.rank[i] += 1


def track_builder(pairs, matches, length=3):
    """TrackBuilder(false).Build / Filter(length) / ExportTracks: {track id: sorted [(image, keypoint)]}, GetMaxID()."""
    feats = sorted(set([(p[0], q) for p, ms in zip(pairs, matches) for q, _ in ms] + [(p[1], t) for p, ms in zip(pairs, matches) for _, t in ms]))
    f2i = {f: i for i, f in enumerate(feats)}
    max_id = (len(feats) - 1) & U32_MAX
    uf = UnionFind(len(feats))
    for p, ms in zip(pairs, matches):
        for q, t in ms:
            uf.union(f2i[(p[0], q)], f2i[(p[1], t)])
    images, bad = {}, set()
    for i, f in enumerate(feats):
        tid = uf.find(i)
        s = images.setdefault(tid, set())
        if f[0] in s:
            bad.add(tid)
        s.add(f[0])
    for tid, s in images.items():
        if len(s) < length:
            bad.add(tid)
    for i in range(len(feats)):
        r = uf.parent[i]
        if r in bad:
            uf.size[r] = 1; uf.parent[i] = U32_MAX
    tracks = {}
    for i, f in enumerate(feats):
        tid = uf.parent[i]
        if tid != U32_MAX and uf.size[tid] > 1:
            tracks.setdefault(tid, []).append(f)
    return {k: sorted(v) for k, v in sorted(tracks.items())}, max_id


# ---- generators -----------------------------------------------------------------------------------------------------------------------
def pose_tables(rng, n_frames, spread=3.0):
    """Random camera-to-world poses: T_cw n x 3 x 4 (rigid inverse), centres n x 3."""
    R = np.array([ba_ref.rot(rng.normal(size=3) * 0.5) for _ in range(n_frames)])
    c = rng.normal(size=(n_frames, 3)) * spread
    return np.array([ba_ref.rigid_inverse_3x4(R[f], c[f]) for f in range(n_frames)]), c


def random_tracks(rng, n_tracks, n_frames, lengths, T_cw=None, centres=None, noise=2e-3, min_parallax=np.deg2rad(2.0)):
    """Tracks of the given lengths (cycled) over distinct random frames: a world point 4 to 15 m from the frames' centroid, float32 bearings
    with `noise` rad of direction noise and random lengths (upstream's bearings are unit, the core must not rely on it).  Every pair of
    the first two rays of a track has at least min_parallax between them (the 2 x 2 system of a two-view track stays below cond 1e4)."""
    if T_cw is None:
        T_cw, centres = pose_tables(rng, n_frames)
    off = [0]; fid = []; b = []; X = []
    for t in range(n_tracks):
        L = int(lengths[t % len(lengths)])
        while True:
            fs = rng.choice(n_frames, size=L, replace=False) if L <= n_frames else rng.integers(0, n_frames, size=L)
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            P = centres[fs].mean(0) + d * rng.uniform(4.0, 15.0)
            rays = P - centres[fs]
            rays /= np.linalg.norm(rays, axis=1, keepdims=True)
            if L < 2 or np.arccos(np.clip(rays[0] @ rays[1], -1, 1)) >= min_parallax:
                break
        X.append(P)
        for f in fs:
            pc = T_cw[f, :, :3] @ P + T_cw[f, :, 3]
            n = pc / np.linalg.norm(pc) + rng.normal(size=3) * noise
            b.append(n * rng.uniform(0.5, 2.0)); fid.append(int(f))
        off.append(len(fid))
    return dict(T=np.ascontiguousarray(T_cw), centres=centres, off=np.array(off, np.int64), fid=np.array(fid, np.int32), b=np.array(b, np.float32).reshape(-1, 3),
                X=np.array(X).reshape(-1, 3))


def degenerate_tracks():
    """The three planted tracks: two identical bearings under identical poses (non-finite by IEEE, whatever that gives), three cameras at the
    origin looking along +z (AtA = diag(3, 3, 0, 0): the eigenvector is e_2, p(3) = 0 exactly, hnormalized gives an inf), one observation."""
    T = np.zeros((3, 3, 4)); T[:, :, :3] = np.eye(3)
    off = np.array([0, 2, 5, 6], np.int64)
    fid = np.array([0, 0, 0, 1, 2, 1], np.int32)
    b = np.array([[0.3, -0.2, 0.9], [0.3, -0.2, 0.9], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0.1, 0.2, 0.9]], np.float32)
    return dict(T=T, off=off, fid=fid, b=b)


def matches_of_tracks(tracks):
    """Image matches that rebuild the given tracks (lists of (frame, keypoint)): consecutive observations matched, grouped per image pair."""
    by_pair = {}
    for tr in tracks:
        for (f0, k0), (f1, k1) in zip(tr[:-1], tr[1:]):
            by_pair.setdefault((int(f0), int(f1)), []).append((int(k0), int(k1)))
    pairs = sorted(by_pair)
    return pairs, [by_pair[p] for p in pairs]


def rounded_scene(rng, n_frames=30, n_tracks=3000, planted=40, **kw):
    """The synthetic scene of sfm_ba_ref.trajectory_scene without keypoint noise, keypoints rounded to pixels; `planted` tracks of at least
    five observations get one observation moved by 40 deg along its meridian.  Returns the scene, the matches, the planted
    track indices."""
    sc = ba_ref.trajectory_scene(rng, n_frames=n_frames, n_tracks=n_tracks, noise_px=0.0, outlier_obs=0.0, **kw)
    sc["kps"] = [np.rint(k).astype(np.float32) for k in sc["kps"]]
    long_tracks = [i for i, tr in enumerate(sc["tracks"]) if len(tr) >= 5]
    bad = np.sort(rng.choice(long_tracks, size=planted, replace=False)) if planted else np.zeros(0, np.int64)
    shift = sc["rows"] * 40.0 / 180.0                          # 40 deg of latitude, towards the equator: 40 deg of angle at any longitude
    for t in bad:
        f, k = sc["tracks"][t][len(sc["tracks"][t]) // 2]
        v = sc["kps"][f][k, 1]
        sc["kps"][f][k, 1] = np.rint(v + shift if v < sc["rows"] / 2 else v - shift)
    pairs, matches = matches_of_tracks(sc["tracks"])
    return sc, pairs, matches, bad


def write_match_scene(path, sc, pairs, matches, R=None, t=None):
    """The input file of tests/cpp/pvlm_structure_driver.cpp."""
    R = sc["R0"] if R is None else R; t = sc["t0"] if t is None else t
    F = len(R)
    with open(path, "wb") as f:
        f.write(np.array([F, sc["rows"], sc["cols"], len(pairs)], np.int32).tobytes())
        for i in range(F):
            f.write(np.array([1], np.int32).tobytes())
            f.write(np.asarray(R[i], np.float64).tobytes()); f.write(np.asarray(t[i], np.float64).tobytes())
            f.write(np.array([len(sc["kps"][i])], np.int32).tobytes()); f.write(np.ascontiguousarray(sc["kps"][i], np.float32).tobytes())
        for p, ms in zip(pairs, matches):
            f.write(np.array([p[0], p[1], len(ms)], np.int32).tobytes()); f.write(np.array(ms, np.int32).reshape(-1, 2).tobytes())


# ---- the host compile of the cores (tests/cpp/structure_core_check.cpp), shared by the CPU and the GPU tests ----------------------------------
def build_check():
    out = os.path.join(ROOT, "build", "libstructure_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "structure_core_check.cpp")])
    return C.CDLL(out)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_triangulate(chk, off, fid, T, bearings=None, keypoints=None, frame_valid=None, rows=0, cols=0):
    off = np.ascontiguousarray(off, np.int64); fid = np.ascontiguousarray(fid, np.int32); T = np.ascontiguousarray(T, np.float64)
    b = None if bearings is None else np.ascontiguousarray(bearings, np.float32)
    kp = None if keypoints is None else np.ascontiguousarray(keypoints, np.float32)
    fv = None if frame_valid is None else np.ascontiguousarray(frame_valid, np.uint8)
    n = len(off) - 1
    X = np.zeros((n, 3)); st = np.zeros(n, np.uint8)
    chk.chk_triangulate(C.c_int(rows), C.c_int(cols), C.c_int(n), _ptr(off), _ptr(fid), _ptr(kp), _ptr(b), _ptr(T), _ptr(fv), _ptr(X), _ptr(st))
    return X, st


def host_filter_far(chk, off, fid, X, t_wc, threshold, frame_valid=None):
    off = np.ascontiguousarray(off, np.int64); fid = np.ascontiguousarray(fid, np.int32); X = np.ascontiguousarray(X, np.float64)
    t_wc = np.ascontiguousarray(t_wc, np.float64); fv = None if frame_valid is None else np.ascontiguousarray(frame_valid, np.uint8)
    keep = np.zeros(len(off) - 1, np.uint8)
    chk.chk_filter_far(C.c_int(len(off) - 1), _ptr(off), _ptr(fid), _ptr(X), _ptr(t_wc), _ptr(fv), C.c_double(threshold), _ptr(keep))
    return keep


def make_far_tracks():
    rng = np.random.default_rng(33)
    tr = random_tracks(rng, 2000, 12, [2, 3, 4, 6, 12, 20, 40])
    X = tr["X"].copy()
    far = rng.uniform(size=len(X)) < 0.4                       # push four in ten points away, some past 8 baselines
    cen = np.array([tr["centres"][tr["fid"][tr["off"][t]:tr["off"][t + 1]]].mean(0) for t in range(len(X))])
    X[far] = cen[far] + (X[far] - cen[far]) * rng.uniform(1.0, 12.0, size=(far.sum(), 1))
    valid = np.ones(12, np.uint8); valid[5] = 0
    return dict(off=tr["off"], fid=tr["fid"], X=X, t_wc=tr["centres"], valid=valid)
