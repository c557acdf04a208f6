"""CPU checks of K32: tests/cpp/structure_core_check.cpp compiles the per-track cores (csrc/pvlm_triangulate_core.h), the TrackBuilder
(host/pvlm_host_tracks.hpp) and the host logic of TriangulateTracks / EstimateStructure (host/pvlm_host_structure.hpp, the cores behind its
seam) for the host; they are compared with the numpy restatement of tests/structure_ref.py.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import sfm_ba_ref as ba_ref
from tests import structure_ref as ref
from tests.structure_ref import _ptr, host_filter_far, host_triangulate

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def chk():
    return ref.build_check()


# ---- 1. union-find and TrackBuilder -----------------------------------------------------------------------------------------------------
def host_track_builder(chk, pairs, matches, length=3):
    pij = np.ascontiguousarray(np.array(pairs, np.int32).reshape(-1, 2))
    moff = np.concatenate([[0], np.cumsum([len(m) for m in matches])]).astype(np.int64)
    m = np.ascontiguousarray(np.array([x for ms in matches for x in ms], np.int32).reshape(-1, 2))
    cap = 2 * len(m) + 1
    ids = np.zeros(cap, np.uint32); toff = np.zeros(cap + 1, np.int64); feats = np.zeros((cap, 2), np.uint32); max_id = C.c_ulonglong(0)
    n = chk.chk_track_builder(C.c_int(len(pairs)), _ptr(pij), _ptr(moff), _ptr(m), C.c_uint(length), _ptr(ids), _ptr(toff), _ptr(feats), C.byref(max_id))
    return {int(ids[k]): [tuple(int(v) for v in f) for f in feats[toff[k]:toff[k + 1]]] for k in range(n)}, max_id.value


def random_match_graph(rng, n_frames=6, n_matches=400, n_kp=60):
    pairs = [(i, j) for i in range(n_frames) for j in range(i + 1, n_frames)]
    matches = [[] for _ in pairs]
    for _ in range(n_matches):
        p = int(rng.integers(len(pairs)))
        matches[p].append((int(rng.integers(n_kp)), int(rng.integers(n_kp))))
    keep = [k for k in range(len(pairs)) if matches[k]]
    return [pairs[k] for k in keep], [matches[k] for k in keep]


@pytest.mark.parametrize("seed,n_matches,n_kp", [(0, 400, 60), (1, 400, 400), (2, 120, 200), (3, 30, 10)])
def test_track_builder_matches_literal_transcription(chk, seed, n_matches, n_kp):
    pairs, matches = random_match_graph(np.random.default_rng(seed), n_matches=n_matches, n_kp=n_kp)
    got, max_id = host_track_builder(chk, pairs, matches)
    exp, exp_max = ref.track_builder(pairs, matches)
    assert got == exp and max_id == exp_max
    assert list(got) == sorted(got)


def test_track_builder_planted_tracks(chk):
    # a chain over frames 0-1-2-3 (kept), a track that visits frame 0 twice (removed), a track of two frames (removed by Filter(3))
    pairs = [(0, 1), (1, 2), (2, 3), (0, 2)]
    matches = [[(0, 0), (5, 5), (7, 7)], [(0, 0), (5, 5)], [(0, 0)], [(6, 5)]]
    got, max_id = host_track_builder(chk, pairs, matches)
    exp, exp_max = ref.track_builder(pairs, matches)
    assert got == exp and max_id == exp_max
    assert len(got) == 1 and sorted(got.values())[0] == [(0, 0), (1, 0), (2, 0), (3, 0)]


def _frames_args(sc, R, t, valid=None):
    F = len(R)
    kp_off = np.concatenate([[0], np.cumsum([len(k) for k in sc["kps"]])]).astype(np.int64)
    kps = np.ascontiguousarray(np.concatenate(sc["kps"]), np.float32)
    v = np.ones(F, np.uint8) if valid is None else np.ascontiguousarray(valid, np.uint8)
    return F, v, np.ascontiguousarray(R, np.float64), np.ascontiguousarray(t, np.float64), kp_off, kps


def host_structure(chk, mode, sc, pairs, matches, R, t, threshold=8.0, valid=None):
    F, v, Rc, tc, kp_off, kps = _frames_args(sc, R, t, valid)
    pij = np.ascontiguousarray(np.array(pairs, np.int32).reshape(-1, 2))
    moff = np.concatenate([[0], np.cumsum([len(m) for m in matches])]).astype(np.int64)
    m = np.ascontiguousarray(np.array([x for ms in matches for x in ms], np.int32).reshape(-1, 2))
    cap = 2 * len(m) + 1
    ids = np.zeros(cap, np.uint32); X = np.zeros((cap, 3)); ret = C.c_longlong(0)
    n = chk.chk_structure(C.c_int(mode), C.c_double(threshold), C.c_int(F), C.c_int(sc["rows"]), C.c_int(sc["cols"]), _ptr(v), _ptr(Rc), _ptr(tc), _ptr(kp_off),
                          _ptr(kps), C.c_int(len(pairs)), _ptr(pij), _ptr(moff), _ptr(m), _ptr(ids), _ptr(X), C.byref(ret))
    return ids[:n].astype(np.int64), X[:n].copy(), ret.value


def test_strict_max_id_bound(chk):
    """The highest feature index is a root: union by rank makes the FIRST argument's root the parent on equal ranks, so matching the last
    feature (as query) to earlier ones makes it the track id = GetMaxID(), and `track_idx < max_track_id` never visits that track."""
    pairs2 = [(3, 0), (3, 1), (0, 1), (1, 2)]
    matches2 = [[(9, 1)], [(9, 2)], [(4, 4)], [(4, 4)]]
    got, max_id = host_track_builder(chk, pairs2, matches2)
    exp, exp_max = ref.track_builder(pairs2, matches2)
    assert got == exp and max_id == exp_max
    assert max_id in got and len(got) == 2                     # the root of {(3,9), (0,1), (1,2)} is the last feature
    # both tracks are real points seen from four cameras: only the strict bound keeps the first one out
    rows, cols = 720, 1440
    t = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0.5], [3.0, 0.2, 0]]); R = np.array([np.eye(3)] * 4)
    kps = [np.zeros((10, 2), np.float32) for _ in range(4)]
    for X, feats in ((np.array([1.0, 0.5, 6.0]), [(3, 9), (0, 1), (1, 2)]), (np.array([2.0, -1.0, 5.0]), [(0, 4), (1, 4), (2, 4)])):
        for f, k in feats:
            p = X - t[f]
            kps[f][k] = [cols * (0.5 + np.arctan2(p[0], p[2]) / (2 * np.pi)), rows * (0.5 + np.arcsin(p[1] / np.linalg.norm(p)) / np.pi)]
    sc = dict(rows=rows, cols=cols, kps=kps)
    ids, X, _ = host_structure(chk, 0, sc, pairs2, matches2, R, t)
    assert ids.tolist() == [i for i in got if i != max_id] and np.linalg.norm(X[0] - [2.0, -1.0, 5.0]) < 0.1
    # the same matches with the last feature as train index: (0,1) becomes the root, both tracks are visited
    pairs3 = [(0, 3), (1, 3), (0, 1), (1, 2)]
    matches3 = [[(1, 9)], [(2, 9)], [(4, 4)], [(4, 4)]]
    ids3, X3, _ = host_structure(chk, 0, sc, pairs3, matches3, R, t)
    assert len(ids3) == 2 and np.linalg.norm(X3[0] - [1.0, 0.5, 6.0]) < 0.1


# ---- 2. the core against structure_ref ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core_tracks():
    rng = np.random.default_rng(32)
    lengths = [2, 2, 3, 4, 5, 8, 12, 12, 3, 2]                 # 12 frames: distinct frames per track up to 12 ...
    a = ref.random_tracks(rng, 1600, 12, lengths)
    T, c = a["T"], a["centres"]
    b = ref.random_tracks(rng, 400, 12, [13, 20, 40, 40], T_cw=T, centres=c)     # ... and repeated frames up to length 40
    off = np.concatenate([a["off"], a["off"][-1] + b["off"][1:]])
    return dict(T=T, centres=c, off=off, fid=np.concatenate([a["fid"], b["fid"]]), b=np.concatenate([a["b"], b["b"]]), X=np.concatenate([a["X"], b["X"]]))


def test_two_view_matches_reference(chk, core_tracks):
    tr = core_tracks
    X, st = host_triangulate(chk, tr["off"], tr["fid"], tr["T"], bearings=tr["b"])
    two = np.flatnonzero(np.diff(tr["off"]) == 2)
    assert len(two) >= 400
    i = tr["off"][two]
    Xr, cond = ref.two_view(tr["T"][tr["fid"][i]], tr["T"][tr["fid"][i + 1]], tr["b"][i], tr["b"][i + 1])
    assert cond.max() < 1e4, cond.max()                        # parallax of at least 2 deg by construction
    err = np.linalg.norm(X[two] - Xr, axis=1) / np.linalg.norm(Xr, axis=1)
    print("two-view: max relative error / (64 eps cond) = %.3g, max cond %.3g" % ((err / (64 * EPS * cond)).max(), cond.max()))
    assert np.all(err <= 64 * EPS * cond)
    assert np.all(st[two] == 0)
    assert np.linalg.norm(X[two] - tr["X"][two], axis=1).max() < 2.0     # and it is the point the rays were made from, to their noise


def test_n_view_eigenvector_matches_eigh(chk, core_tracks):
    tr = core_tracks
    n = len(tr["off"]) - 1
    many = np.flatnonzero(np.diff(tr["off"]) > 2)
    assert np.diff(tr["off"]).max() == 40 and len(many) >= 1000
    ata = np.zeros((n, 10)); vec = np.zeros((n, 4)); w = np.zeros((n, 4))
    off = np.ascontiguousarray(tr["off"]); fid = np.ascontiguousarray(tr["fid"]); b = np.ascontiguousarray(tr["b"]); T = np.ascontiguousarray(tr["T"])
    chk.chk_nview_eig(C.c_int(n), _ptr(off), _ptr(fid), _ptr(b), _ptr(T), _ptr(ata), _ptr(vec), _ptr(w))
    Xr, vr, wr, A = ref.n_view(tr["off"], tr["fid"], tr["b"], tr["T"])
    gap = (wr[:, 1] - wr[:, 0]) / wr[:, 3]
    assert gap[many].min() >= 1e-6, gap[many].min()            # the reference's own assertion on the generated inputs
    sign = np.sign((vec * vr).sum(1))[:, None]
    dv = np.linalg.norm(vec * sign - vr, axis=1)
    bound = 64 * EPS / gap
    print("n-view: max eigenvector error / bound = %.3g, min gap ratio %.3g" % ((dv[many] / bound[many]).max(), gap[many].min()))
    assert np.all(dv[many] <= bound[many])
    assert np.all(np.abs(np.linalg.norm(vec[many], axis=1) - 1.0) <= 64 * EPS)
    # backward check on the core's own AtA: |AtA v - lambda v| <= 64 eps lambda_max
    iu = np.triu_indices(4)
    Ac = np.zeros((n, 4, 4)); Ac[:, iu[0], iu[1]] = ata; Ac[:, iu[1], iu[0]] = ata
    lam = w.min(1)
    res = np.linalg.norm(np.einsum("nij,nj->ni", Ac, vec) - lam[:, None] * vec, axis=1)
    print("n-view: max backward residual / (64 eps lambda_max) = %.3g" % (res[many] / (64 * EPS * w.max(1)[many])).max())
    assert np.all(res[many] <= 64 * EPS * w.max(1)[many])
    assert np.abs(Ac - A)[many].max() <= 64 * EPS * np.abs(A[many]).max()
    # and the points of the full call are the eigenvector's, hnormalized
    X, st = host_triangulate(chk, tr["off"], tr["fid"], tr["T"], bearings=tr["b"])
    assert np.array_equal(X[many], vec[many, :3] / vec[many, 3:4]) and np.all(st[many] == 0)
    assert np.linalg.norm(X[many] - tr["X"][many], axis=1).max() < 2.0


def test_degenerate_tracks(chk):
    d = ref.degenerate_tracks()
    X, st = host_triangulate(chk, d["off"], d["fid"], d["T"], bearings=d["b"])
    Xr, sr = ref.triangulate_ref(d["off"], d["fid"], d["b"], d["T"])
    # identical bearings under identical poses: non-finite; status and point are the reference's IEEE outcome
    assert not np.all(np.isfinite(X[0])) and st[0] == sr[0] and np.array_equal(X[0], Xr[0], equal_nan=True)
    assert st[1] == 1 and np.isinf(X[1]).any()                 # p(3) = 0 exactly
    assert st[2] == 1 and np.all(X[2] == np.inf)               # a single observation
    # an observation in an invalid frame: status 2, NaN point (the deliberate divergence)
    X2, st2 = host_triangulate(chk, d["off"], d["fid"], d["T"], bearings=d["b"], frame_valid=[1, 1, 0])
    assert st2.tolist() == [int(st[0]), 2, 1] and np.all(np.isnan(X2[1]))
    # a NaN point is kept (status 0), upstream's trap: det = p.p p.p - p.p p.p = 0 exactly and both right-hand sides are 0 (the two poses are
    # one), so lambda = inf * 0 = NaN on every coordinate
    assert np.all(np.isnan(X[0])) and st[0] == 0


# ---- 3. FilterTracksToFar ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_tracks():
    return ref.make_far_tracks()


def test_filter_far_matches_reference(chk, far_tracks):
    ft = far_tracks
    for valid in (None, ft["valid"]):
        keep_r, ratio = ref.filter_far_ref(ft["off"], ft["fid"], ft["X"], ft["t_wc"], 8.0, valid)
        assert (np.abs(ratio - 1.0) <= 1e-9).sum() == 0        # no decision within rounding of the threshold
        keep = host_filter_far(chk, ft["off"], ft["fid"], ft["X"], ft["t_wc"], 8.0, valid)
        assert np.array_equal(keep, keep_r)
        assert 100 < keep.sum() < len(keep) - 100


def test_filter_far_planted_cases(chk):
    t_wc = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 2.0, 0], [5.0, 5, 5]])
    valid = np.array([1, 1, 1, 0], np.uint8)
    off = np.array([0, 1, 2, 4, 7, 9, 10], np.int64)
    fid = np.array([0,  0,  3, 3,  1, 0, 1,  0, 3,  3], np.int32)
    X = np.array([[0.0, 0, 1e-3],        # one valid frame, the point not at the centre: baseline 0 < average -> removed
                  [0.0, 0, 0],           # one valid frame, the point AT the centre: 0 < 0 is false -> kept
                  [9.0, 9, 9],           # no valid frame: 0 / 0 = NaN -> kept
                  [0.5, 0, 7.9],         # frames 1, 0, 1 (one repeated): baseline 1, average < 8 -> kept
                  [0.0, 0, 1e-3],        # a valid and an invalid frame: one centre -> removed
                  [1.0, 1, 1]])          # one observation in an invalid frame -> kept (NaN)
    keep = host_filter_far(chk, off, fid, X, t_wc, 8.0, valid)
    keep_r, _ = ref.filter_far_ref(off, fid, X, t_wc, 8.0, valid)
    assert keep.tolist() == [0, 1, 1, 1, 0, 1] and np.array_equal(keep, keep_r)
    X[3] = [0.5, 0, 8.1]
    assert host_filter_far(chk, off, fid, X, t_wc, 8.0, valid)[3] == 0


# ---- 4. TriangulateTracks end to end, EstimateStructure's return rule ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return ref.rounded_scene(np.random.default_rng(34))


def point_error_bound(sc, track, X_true):
    """How far the algebraic point of a track can lie from X_true when every bearing is off by at most delta: the keypoints are rounded to
    pixels (<= 0.5 px on both axes: at most sqrt((pi / cols)^2 + (pi / (2 rows))^2) rad of direction) and un-projected in float (1e-6 rad).
    With Q_i = I - n_i n_i^T of the OBSERVED bearings and p_i = R_i X_true + t_i: |Q_i p_i| <= depth_i delta.  The least-squares point X_ls of
    sum |Q_i (R_i X + t_i)|^2 obeys H (X_ls - X_true) = -sum R_i^T Q_i p_i, H = sum R_i^T Q_i R_i, hence |X_ls - X_true| <= delta sum depth_i /
    lambda_min(H): depth and parallax of this very track.  The eigenvector point minimises the same sum over |X|^2 + 1, (H - l I) X = H X_ls with l
    the smallest eigenvalue, l <= sum (depth_i delta)^2 / (|X_true|^2 + 1): |X - X_ls| <= l / (lambda_min(H) - l) |X_ls|."""
    rows, cols = sc["rows"], sc["cols"]
    delta = np.sqrt((np.pi / cols) ** 2 + (np.pi / (2 * rows)) ** 2) + 1e-6
    H = np.zeros((3, 3)); depth = []
    for f, k in track:
        R = sc["R_true"][f].T; t = -R @ sc["t_true"][f]
        n = ba_ref.image_to_cam_point2i(rows, cols, sc["kps"][f][k][None]).astype(np.float64)[0]
        n /= np.linalg.norm(n)
        Q = np.eye(3) - np.outer(n, n)
        H += R.T @ Q @ R
        depth.append(np.linalg.norm(R @ X_true + t))
    lmin = np.linalg.eigvalsh(H)[0]
    ls = delta * np.sum(depth) / lmin
    lam = np.sum((np.array(depth) * delta) ** 2) / (X_true @ X_true + 1.0)
    if lam >= 0.5 * lmin:              # no parallax to speak of (a point next to the line of its cameras): half a pixel allows any distance
        return np.inf
    return ls + lam / (lmin - lam) * (np.linalg.norm(X_true) + ls)


def reprojection_sines(sc, track, X_true, X):
    """For a track of any parallax: the eigenvector's Rayleigh quotient l = sum |Q_i (R_i X + t_i)|^2 / (|X|^2 + 1) is the smallest eigenvalue,
    so it is at most the quotient at X_true, sum (depth_i delta)^2 / (|X_true|^2 + 1) (delta as in point_error_bound).  Hence every
    |Q_i p_i| <= sqrt(l_bound (|X|^2 + 1)): the sine of the angle between each observed bearing and the ray to the triangulated point is at
    most that over |p_i|.  Returns (sines, bounds) per observation."""
    rows, cols = sc["rows"], sc["cols"]
    delta = np.sqrt((np.pi / cols) ** 2 + (np.pi / (2 * rows)) ** 2) + 1e-6
    sines, dist, depth = [], [], []
    for f, k in track:
        R = sc["R_true"][f].T; t = -R @ sc["t_true"][f]
        n = ba_ref.image_to_cam_point2i(rows, cols, sc["kps"][f][k][None]).astype(np.float64)[0]
        n /= np.linalg.norm(n)
        p = R @ X + t
        sines.append(np.linalg.norm(p - n * (n @ p)) / np.linalg.norm(p)); dist.append(np.linalg.norm(p))
        depth.append(np.linalg.norm(R @ X_true + t))
    lam = np.sum((np.array(depth) * delta) ** 2) / (X_true @ X_true + 1.0)
    return np.array(sines), np.sqrt(lam * (X @ X + 1.0)) / np.array(dist) * (1.0 + 1e-9)


def test_triangulate_tracks_end_to_end(chk, scene):
    sc, pairs, matches, planted = scene
    ids, X, _ = host_structure(chk, 0, sc, pairs, matches, sc["R_true"], sc["t_true"])
    exp_tracks, max_id = ref.track_builder(pairs, matches)
    assert len(exp_tracks) == len(sc["tracks"])
    assert np.all(np.diff(ids) > 0)                            # ascending id
    by_id = {tid: feats for tid, feats in exp_tracks.items()}
    index_of = {tuple(sorted((int(f), int(k)) for f, k in tr)): i for i, tr in enumerate(sc["tracks"])}
    got = np.array([index_of[tuple(by_id[int(t)])] for t in ids])
    assert not set(planted.tolist()) & set(got.tolist())       # one observation 40 deg off: gone after the 25 deg filter
    clean = np.setdiff1d(np.arange(len(sc["tracks"])), planted)
    unvisited = [index_of[tuple(f)] for tid, f in exp_tracks.items() if tid >= max_id]
    assert np.array_equal(np.sort(got), np.setdiff1d(clean, unvisited))
    worst = 0.0; unbounded = 0; worst_sine = 0.0
    for i, t in zip(got, X):
        bound = point_error_bound(sc, sc["tracks"][i], sc["X_true"][i])
        err = np.linalg.norm(t - sc["X_true"][i])
        worst = max(worst, err / bound); unbounded += not np.isfinite(bound)
        assert err <= bound, (i, err, bound)
        sines, sine_bounds = reprojection_sines(sc, sc["tracks"][i], sc["X_true"][i], t)      # holds whatever the parallax
        worst_sine = max(worst_sine, (sines / sine_bounds).max())
        assert np.all(sines <= sine_bounds), (i, sines, sine_bounds)
    print("end to end: %d tracks, worst error / bound = %.3g, %d without a finite distance bound, worst reprojection sine / bound = %.3g" %
          (len(got), worst, unbounded, worst_sine))
    assert unbounded <= len(got) // 100


def test_estimate_structure_return_rule(chk, scene):
    sc, pairs, matches, planted = scene
    R, t = sc["R_true"], sc["t_true"]
    ids0, X0, _ = host_structure(chk, 0, sc, pairs, matches, R, t)
    # tracks over 3 to 6 frames 0.4 m apart, points 3 to 12 m away: some are further than 8 baselines, EstimateStructure removes them and is true
    ids1, X1, ret1 = host_structure(chk, 1, sc, pairs, matches, R, t)
    ids8, _, removed8 = host_structure(chk, 2, sc, pairs, matches, R, t, threshold=8.0)
    assert removed8 > 0 and ret1 == 1 and np.array_equal(ids1, ids8) and removed8 == len(ids0) - len(ids8)
    assert np.all(np.diff(ids8) > 0) and set(ids8.tolist()) <= set(ids0.tolist())          # the survivors keep their order
    _, _, removed_none = host_structure(chk, 2, sc, pairs, matches, R, t, threshold=1e9)
    assert removed_none == 0
    # every track over 6 frames (baseline 2 m, the point at most 13 m from any of them): nothing is removed, EstimateStructure is FALSE as upstream
    # writes it, and the structure is filled all the same
    sc6, pairs6, matches6, _ = ref.rounded_scene(np.random.default_rng(35), n_frames=12, n_tracks=200, planted=0, min_track=6, max_track=6)
    a, _, _ = host_structure(chk, 0, sc6, pairs6, matches6, sc6["R_true"], sc6["t_true"])
    b, _, ret = host_structure(chk, 1, sc6, pairs6, matches6, sc6["R_true"], sc6["t_true"])
    assert ret == 0 and len(b) > 150 and np.array_equal(a, b)
