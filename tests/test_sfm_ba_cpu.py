"""CPU checks of K31: the two-row reprojection kinds (PanoramaReprojResidual_2Angle / _Pixel, base/CostFunction.h:178-288) and the
track filters of SfM::GlobalBundleAdjustment (sfm/Structure.cpp:121-193).  tests/cpp/sfm_ba_math_check.cpp compiles the device bodies
(csrc/pvlm_reproj.h, pvlm_ba_core.h, pvlm_sfm_filter_core.h) for the host; they are compared with the numpy restatements of
tests/sfm_ba_ref.py — a Jet<9> for the functors, operation-by-operation for the filters.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sfm_ba_ref as ref
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


class View(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_cams", C.c_int), ("n_upairs", C.c_int), ("n_obs", C.c_longlong),
                ("pt_off", C.c_void_p), ("cam", C.c_void_p), ("obs_pt", C.c_void_p), ("s", C.c_void_p), ("X", C.c_void_p), ("Xc", C.c_void_p),
                ("scale", C.c_void_p), ("Vinv", C.c_void_p), ("gp", C.c_void_p), ("adj_off", C.c_void_p), ("adj_cam", C.c_void_p),
                ("adj_slot", C.c_void_p), ("frozen", C.c_void_p), ("w", C.c_double), ("loss", C.c_int), ("a", C.c_double)]


@pytest.fixture(scope="module")
def chk():
    out = os.path.join(ROOT, "build", "libsfm_ba_check.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "sfm_ba_math_check.cpp")])
    lib = C.CDLL(out)
    lib.chk2_cost.restype = C.c_double
    lib.chk_filter_threshold.restype = C.c_double
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def random_observations(rng, kind, n, rows=960, cols=1920, w=1.0):
    """n observations, each with its own pose: a quarter near the lon = +-pi seam (both sides), some with an angle-axis below the
    small-angle threshold, a tenth far from their keypoint (Huber's outer region).  Poles are kept out."""
    aa = rng.normal(size=(n, 3)) * 0.4
    tiny = rng.uniform(size=n) < 0.1
    aa[tiny] = rng.normal(size=(tiny.sum(), 3)) * 1e-9          # theta^2 < eps: AngleAxisRotatePoint's first-order branch
    t = rng.normal(size=(n, 3)) * 0.5
    tab = synth.pose_table(aa, t)
    pc = rng.normal(size=(n, 3)) * 2.0
    seam = rng.uniform(size=n) < 0.25
    pc[seam, 0] = rng.choice([-1.0, 1.0], size=seam.sum()) * rng.uniform(1e-4, 1e-2, size=seam.sum())
    pc[seam, 2] = -np.abs(pc[seam, 2]) - 0.5
    ok = pc[:, 0] ** 2 + pc[:, 2] ** 2 > 1e-6 * (pc ** 2).sum(1)
    pc[~ok, 2] += 1.0
    R = tab[:, :9].reshape(-1, 3, 3)
    X = np.einsum("nji,nj->ni", R, pc - tab[:, 18:])
    o = ref.project(ref.PIXEL, tab, X, rows, cols) + rng.normal(size=(n, 2)) * 2.0
    far = rng.uniform(size=n) < 0.1
    o[far] += rng.normal(size=(far.sum(), 2)) * 200.0
    if kind == ref.ANGLE2:   # sphere angles in (-pi, pi], the constructor wraps x < 0
        o = np.stack([(2 * o[:, 0] / cols - 1) * np.pi, (0.5 - o[:, 1] / rows) * np.pi], 1)
    return aa, t, tab, X, o


@pytest.mark.parametrize("kind", [ref.ANGLE2, ref.PIXEL])
def test_two_row_eval_matches_jet(chk, kind):
    rng = np.random.default_rng(31 + kind)
    n, rows, cols, w = 2000, 960, 1920, 1.7
    aa, t, tab, X, o = random_observations(rng, kind, n, rows, cols, w)
    r_ref, J_ref = ref.eval_jet(kind, aa, t, X, o, w, rows, cols)
    obs = o.copy()
    if kind == ref.ANGLE2:
        obs[:, 0] = np.where(obs[:, 0] < 0, obs[:, 0] + 2 * np.pi, obs[:, 0])    # what pvlm_ba_create_kind stores
    r = np.zeros(2 * n); J = np.zeros((2 * n, 9))
    tabc = np.ascontiguousarray(tab); Xc = np.ascontiguousarray(X); oc = np.ascontiguousarray(obs)
    chk.chk2_eval(C.c_int(kind), C.c_longlong(n), _ptr(tabc), _ptr(Xc), _ptr(oc), C.c_double(w), C.c_double(rows), C.c_double(cols), _ptr(r), _ptr(J))
    r = r.reshape(n, 2); J = J.reshape(n, 2, 9)
    scale = max(rows, cols) if kind == ref.PIXEL else 2 * np.pi
    assert np.all(np.abs(r - r_ref) <= 1e-6 * np.abs(r_ref) + 64 * EPS * w * scale), np.abs(r - r_ref).max()
    rowmax = np.abs(J_ref).max(axis=2, keepdims=True)
    assert np.all(np.abs(J - J_ref) <= 1e-6 * rowmax), (np.abs(J - J_ref) / rowmax).max()
    # the seam is not wrapped (upstream leaves it to Huber): both sides of lon = +-pi are present and far apart
    if kind == ref.PIXEL:
        assert (r[:, 0] > cols / 4).any() and (r[:, 0] < -cols / 4).any()


def test_pole_convention(chk):
    """p0 = p2 = 0: upstream's Jets give inf / NaN; the device bodies give zero derivatives and a finite residual."""
    tab = synth.pose_table(np.zeros((2, 3)), np.zeros((2, 3)))
    X = np.array([[0.0, 2.0, 0.0], [0.0, -3.0, 0.0]]); o = np.array([[10.0, 20.0], [30.0, 40.0]])
    for kind in (ref.ANGLE2, ref.PIXEL):
        r = np.zeros(4); J = np.ones((4, 9))
        chk.chk2_eval(C.c_int(kind), C.c_longlong(2), _ptr(tab), _ptr(X), _ptr(o), C.c_double(1.0), C.c_double(100.0), C.c_double(200.0), _ptr(r), _ptr(J))
        assert np.all(np.isfinite(r)) and np.all(J == 0.0)


class Set2:
    def __init__(self, b, kind, w, loss, a, frozen=None):
        self.kind, self.rows, self.cols = kind, float(b["rows"]), float(b["cols"])
        self.F = int(b["cam"].max()) + 1
        self.M = len(b["off"]) - 1
        obs = b["obs"].copy()
        if kind == ref.ANGLE2:
            obs[:, 0] = np.where(obs[:, 0] < 0, obs[:, 0] + 2 * np.pi, obs[:, 0])
        self.keep = dict(off=np.ascontiguousarray(b["off"], np.int64), cam=np.ascontiguousarray(b["cam"], np.int32),
                         obs_pt=np.repeat(np.arange(self.M), np.diff(b["off"])).astype(np.int32), s=np.ascontiguousarray(obs),
                         X=np.ascontiguousarray(b["X"], np.float64), Xc=np.zeros((self.M, 3)), scale=np.zeros((self.M, 3)), Vinv=np.zeros((self.M, 6)),
                         gp=np.zeros((self.M, 3)), frozen=None if frozen is None else np.ascontiguousarray(frozen, np.uint8))
        k = self.keep
        self.view = View(self.M, self.F, 0, len(b["cam"]), *[_ptr(k[n]).value for n in ("off", "cam", "obs_pt", "s", "X", "Xc", "scale", "Vinv", "gp")],
                         None, None, None, None if frozen is None else _ptr(k["frozen"]).value, w, loss, a)
        self.tab = np.ascontiguousarray(synth.pose_table(b["aa"], b["t"]))


@pytest.mark.parametrize("kind,loss", [(ref.PIXEL, 1), (ref.PIXEL, 0), (ref.ANGLE2, 1)])
def test_two_row_schur_matches_numpy(chk, kind, loss):
    rng = np.random.default_rng(7 + kind + 10 * loss)
    b = ref.random_bundle2(rng, kind, n_cams=5, n_points=40)
    w = 1.0
    a = 4.0 if kind == ref.PIXEL else 4.0 * np.pi / 180.0
    frozen = (rng.uniform(size=len(b["off"]) - 1) < 0.2).astype(np.uint8)
    s = Set2(b, kind, w, loss, a, frozen)
    F = s.F
    radius, mind, maxd = 1e3, 1e-6, 1e32
    S = np.zeros((6 * F, 6 * F)); vecs = np.zeros((F, 19)); gmax = C.c_double(0.0)
    chk.chk2_reduce(C.c_int(kind), C.byref(s.view), C.c_double(s.rows), C.c_double(s.cols), _ptr(s.tab), C.c_int(1), C.c_double(radius),
                    C.c_double(mind), C.c_double(maxd), _ptr(S), _ptr(vecs), C.byref(gmax))
    pt = np.repeat(np.arange(s.M), np.diff(b["off"]))
    rj, Jj = ref.eval_jet(kind, b["aa"][b["cam"]], b["t"][b["cam"]], b["X"][pt], b["obs"], w, b["rows"], b["cols"])
    e = ref.bundle_reference2(rj, Jj, b["off"], b["cam"], F, loss, a, None, radius, mind, maxd, frozen=frozen)
    if loss:
        assert (ref.huber_block(rj, loss, a)[0] < 1).any()        # some blocks are in Huber's outer region
    sc = np.abs(e["S"]).max()
    assert np.abs(S - e["S"]).max() <= 1e-8 * sc
    assert np.abs(vecs[:, :6].reshape(-1) - e["g"]).max() <= 1e-8 * np.abs(e["g"]).max()
    assert np.abs(vecs[:, 6:12] - e["Udiag"]).max() <= 1e-8 * np.abs(e["Udiag"]).max()
    assert np.abs(vecs[:, 12:18].reshape(-1) - e["gcam"]).max() <= 1e-8 * np.abs(e["gcam"]).max()
    assert abs(vecs[:, 18].sum() - e["cost"]) <= 1e-10 * e["cost"]
    assert abs(gmax.value - e["gmax"]) <= 1e-8 * e["gmax"]
    # back-substitution and cost at the candidate
    dcam = rng.normal(size=(F, 6)) * 1e-3
    out3 = np.zeros(3)
    chk.chk2_step(C.c_int(kind), C.byref(s.view), C.c_double(s.rows), C.c_double(s.cols), _ptr(s.tab), _ptr(np.ascontiguousarray(dcam)), _ptr(out3))
    Xc, o3 = ref.step_reference2(e, rj, Jj, b["off"], b["cam"], b["X"], dcam, loss, a, frozen=frozen)
    assert np.abs(s.keep["Xc"] - Xc).max() <= 1e-8 * max(1.0, np.abs(Xc - b["X"]).max())
    assert np.allclose(o3, out3, rtol=1e-7, atol=1e-12)
    cc = chk.chk2_cost(C.c_int(kind), C.byref(s.view), C.c_double(s.rows), C.c_double(s.cols), _ptr(s.tab), C.c_int(1))
    rc, _ = ref.eval_jet(kind, b["aa"][b["cam"]], b["t"][b["cam"]], s.keep["Xc"][pt], b["obs"], w, b["rows"], b["cols"])
    assert abs(cc - ref.huber_block(rc, loss, a)[1].sum()) <= 1e-10 * cc


# ---- track filters ------------------------------------------------------------------------------------------------------------------
def filter_scene(rng, rows=500, cols=1000, F=6, n_tracks=400):
    aa = rng.normal(size=(F, 3)) * 0.3; t = rng.normal(size=(F, 3)) * 0.5
    tab = synth.pose_table(aa, t)
    T = np.zeros((F, 3, 4))
    for f in range(F):
        T[f, :, :3] = tab[f, :9].reshape(3, 3); T[f, :, 3] = tab[f, 18:]
    T[F - 1] = 0.0                                   # a frame without a valid pose: Matrix4d::Zero()
    X = rng.normal(size=(n_tracks, 3)) * 3.0
    off = [0]; fid = []; kp = []
    for p in range(n_tracks):
        for f in rng.choice(F, size=int(rng.integers(1, 5)), replace=False):
            fid.append(int(f))
            pc = T[f, :, :3] @ X[p] + T[f, :, 3]
            if f == F - 1:
                u = np.array([cols / 2, rows / 2]) + rng.normal(size=2) * (3.0 if rng.uniform() < 0.5 else 300.0)
            else:
                lon = np.arctan2(pc[0], pc[2]); lat = -np.arcsin(pc[1] / np.linalg.norm(pc))
                u = np.array([cols * (0.5 + lon / (2 * np.pi)), rows * (0.5 - lat / np.pi)])
                u += rng.normal(size=2) * (30.0 if rng.uniform() < 0.1 else 1.0)
            kp.append(u)
        off.append(len(fid))
    return dict(rows=rows, cols=cols, off=np.array(off, np.int64), fid=np.array(fid, np.int32), kp=np.array(kp, np.float32), X=X, T=T)


def _filter(chk, mode, sc, thr):
    n = len(sc["off"]) - 1
    keep = np.zeros(n, np.uint8)
    off = np.ascontiguousarray(sc["off"]); fid = np.ascontiguousarray(sc["fid"]); kp = np.ascontiguousarray(sc["kp"])
    X = np.ascontiguousarray(sc["X"], np.float64); T = np.ascontiguousarray(sc["T"], np.float64)
    chk.chk_filter(C.c_int(mode), C.c_int(sc["rows"]), C.c_int(sc["cols"]), C.c_int(n), _ptr(off), _ptr(fid), _ptr(kp), _ptr(X), _ptr(T), C.c_double(thr), _ptr(keep))
    return keep


@pytest.mark.parametrize("mode,threshold", [(0, 4.0), (0, 10.0), (0, -1.0), (1, 0.5), (1, 2.0)])
def test_filter_core_matches_numpy(chk, mode, threshold):
    sc = filter_scene(np.random.default_rng(100 + mode))
    thr = chk.chk_filter_threshold(C.c_int(mode), C.c_double(threshold))
    assert thr == ref.filter_threshold(mode, threshold) or (mode == 1 and abs(thr - ref.filter_threshold(mode, threshold)) <= EPS)
    got = _filter(chk, mode, sc, thr)
    exp = ref.filter_ref(mode, sc["rows"], sc["cols"], sc["off"], sc["fid"], sc["kp"], sc["X"], sc["T"], thr)
    assert np.array_equal(got, exp)
    if threshold < 0:
        assert got.all()
    else:
        assert 0 < got.sum() < len(got)


def test_filter_planted_cases(chk):
    rows, cols = 500, 1000
    F = 2
    T = np.zeros((F, 3, 4)); T[0, :, :3] = np.eye(3)        # frame 0 identity, frame 1 invalid (zero)
    X = np.array([[0.3, -0.2, 2.0]] * 4)
    pc = X[0]
    lon = ref.fast_atan2(np.array([pc[0]]), np.array([pc[2]]))[0]
    lat = -ref.fast_atan2(np.array([pc[1]]), np.sqrt(np.array([pc[0] ** 2 + pc[2] ** 2])))[0]
    u, v = cols * (0.5 + lon / (2.0 * np.pi)), rows * (0.5 - lat / np.pi)
    kp0 = np.array([u + 1.3, v - 0.7], np.float32)
    sc = dict(rows=rows, cols=cols, off=np.array([0, 1, 2, 3, 4], np.int64), fid=np.array([0, 1, 1, 0], np.int32),
              kp=np.array([kp0, [cols / 2 + 2.0, rows / 2 - 1.0], [cols / 2 + 200.0, rows / 2], kp0], np.float32), X=X, T=T)
    dx = np.float64(kp0[0]) - u; dy = np.float64(kp0[1]) - v
    sq = dx * dx + dy * dy
    # pixel: within 1 ulp of the threshold (sq > thr rejects); the invalid frame projects to the image centre and can reject
    for thr, exp0 in ((sq, 1), (np.nextafter(sq, -np.inf), 0), (np.nextafter(sq, np.inf), 1)):
        got = _filter(chk, 0, sc, thr)
        assert np.array_equal(got, ref.filter_ref(0, rows, cols, sc["off"], sc["fid"], sc["kp"], X, T, thr))
        assert got[0] == exp0 and got[3] == exp0
        assert got[2] == 0                               # invalid frame, far from the centre
        assert got[1] == (1 if 5.0 <= thr else 0)        # invalid frame, sqrt(5) px from the centre
    assert _filter(chk, 0, sc, 9.0)[1] == 1 and _filter(chk, 0, sc, 4.0)[1] == 0
    assert _filter(chk, 0, sc, chk.chk_filter_threshold(C.c_int(0), C.c_double(-1.0))).all()
    # angle: NaN cosines of the invalid frame never reject; cos within 1 ulp of the threshold
    ray = ref.image_to_cam_point2i(rows, cols, kp0[None]).astype(np.float64)[0]
    c = (pc @ ray) / np.sqrt(pc @ pc) / np.sqrt(ray @ ray)
    c = (pc[0] * ray[0] + pc[1] * ray[1] + pc[2] * ray[2]) / np.sqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]) / np.sqrt(
        ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2])
    for thr, exp0 in ((c, 1), (np.nextafter(c, np.inf), 0), (np.nextafter(c, -np.inf), 1), (1.0, 0)):
        got = _filter(chk, 1, sc, thr)
        assert np.array_equal(got, ref.filter_ref(1, rows, cols, sc["off"], sc["fid"], sc["kp"], X, T, thr))
        assert got[0] == exp0 and got[1] == 1 and got[2] == 1


def test_image_to_cam_point2i_matches_numpy(chk):
    rng = np.random.default_rng(5)
    rows, cols = 960, 1920
    kp = np.concatenate([rng.uniform(0, [cols, rows], size=(5000, 2)), np.array([[0.5, 0.5], [1.5, 2.5], [cols - 0.5, rows - 0.5]])]).astype(np.float32)
    cam = np.zeros((len(kp), 3), np.float32)
    chk.chk_image_to_cam_point2i(C.c_int(rows), C.c_int(cols), C.c_longlong(len(kp)), _ptr(kp), _ptr(cam))
    assert np.array_equal(cam, ref.image_to_cam_point2i(rows, cols, kp))
