"""GPU checks of K31 through the C ABI: the two-row reprojection kinds (pvlm_ba_create_kind: PanoramaReprojResidual_2Angle / _Pixel,
base/CostFunction.h:178-288) against the numpy Jet and a numpy two-row Schur complement, bit-reproducible reduces, and the track
filter kernel (pvlm_filter_tracks, sfm/Structure.cpp:121-193) against its numpy restatement."""
import numpy as np
import pytest

from tests import sfm_ba_ref as ref
from tests import synth
from tests.test_sfm_ba_cpu import filter_scene, random_observations

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
KIND = {ref.ANGLE2: "angle2", ref.PIXEL: "pixel"}


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kind", [ref.ANGLE2, ref.PIXEL])
def test_eval_matches_jet(ctx, kind):
    import panovlm_amd as pv
    rng = np.random.default_rng(131 + kind)
    n, rows, cols, w = 2000, 960, 1920, 1.7
    aa, t, tab, X, o = random_observations(rng, kind, n, rows, cols, w)
    ctx.set_poses(aa, t)                                     # one camera and one point per observation
    bs = pv.BundleSet(ctx, np.arange(n + 1), np.arange(n), o, X, weight=w, kind=KIND[kind], rows=rows, cols=cols)
    r, J = bs.evaluate(jac=True)
    bs.close()
    r_ref, J_ref = ref.eval_jet(kind, aa, t, X, o, w, rows, cols)
    r = r.reshape(n, 2); J = J.reshape(n, 2, 9)
    scale = max(rows, cols) if kind == ref.PIXEL else 2 * np.pi
    assert np.all(np.abs(r - r_ref) <= 1e-6 * np.abs(r_ref) + 64 * EPS * w * scale), np.abs(r - r_ref).max()
    rowmax = np.abs(J_ref).max(axis=2, keepdims=True)
    assert np.all(np.abs(J - J_ref) <= 1e-6 * rowmax), (np.abs(J - J_ref) / rowmax).max()


def _bundle(ctx, kind, seed, frozen_share=0.0, n_cams=6, n_points=60):
    import panovlm_amd as pv
    rng = np.random.default_rng(seed)
    b = ref.random_bundle2(rng, kind, n_cams=n_cams, n_points=n_points)
    ctx.set_poses(b["aa"], b["t"])
    bs = pv.BundleSet(ctx, b["off"], b["cam"], b["obs"], b["X"], weight=1.0, kind=KIND[kind], rows=b["rows"], cols=b["cols"])
    frozen = (rng.uniform(size=len(b["off"]) - 1) < frozen_share).astype(np.uint8) if frozen_share else None
    if frozen is not None:
        bs.set_constant(frozen)
    return b, bs, frozen, rng


@pytest.mark.parametrize("kind,loss,frozen_share", [(ref.PIXEL, 1, 0.0), (ref.PIXEL, 0, 0.0), (ref.PIXEL, 1, 0.25), (ref.ANGLE2, 1, 0.0),
                                                    (ref.ANGLE2, 0, 0.25)])
def test_reduce_step_cost_match_numpy_schur(ctx, kind, loss, frozen_share):
    b, bs, frozen, rng = _bundle(ctx, kind, 17 + kind + 10 * loss + int(100 * frozen_share), frozen_share)
    a = 4.0 if kind == ref.PIXEL else 4.0 * np.pi / 180.0
    F = bs.n_cams
    r, J = bs.evaluate(jac=True)                      # the materialised rows the numpy Schur complement starts from
    r = r.reshape(-1, 2); J = J.reshape(-1, 2, 9)
    radius, mind, maxd = 1e3, 1e-6, 1e32
    packed = bs.reduce(loss, a, init_scale=True, radius=radius, min_diag=mind, max_diag=maxd)
    e = ref.bundle_reference2(r, J, b["off"], b["cam"], F, loss, a, None, radius, mind, maxd, frozen=frozen)
    S, g, cost, Ud, gmax = synth.bundle_unpack(packed, F, bs.ui, bs.uj)
    tol = 1e-9
    assert np.abs(S - e["S"]).max() <= tol * np.abs(e["S"]).max()
    assert np.abs(g - e["g"]).max() <= tol * np.abs(e["g"]).max()
    assert np.abs(Ud - e["Udiag"]).max() <= tol * np.abs(e["Udiag"]).max()
    gc = packed[-1 - 6 * F:-1]
    assert np.abs(gc - e["gcam"]).max() <= tol * np.abs(e["gcam"]).max()
    assert abs(cost - e["cost"]) <= tol * e["cost"]
    assert abs(gmax - e["gmax"]) <= tol * e["gmax"]
    if loss:
        assert (ref.huber_block(r, loss, a)[0] < 1).any()
    # a second reduce at the same state: the same bits (gather form, no atomics)
    again = bs.reduce(loss, a, init_scale=False, radius=radius, min_diag=mind, max_diag=maxd)
    assert np.array_equal(packed.view(np.uint64), again.view(np.uint64))
    # back-substitution, candidate cost, accept
    dcam = rng.normal(size=(F, 6)) * 1e-3
    out3 = bs.step(dcam, loss, a)
    Xc_ref, o3 = ref.step_reference2(e, r, J, b["off"], b["cam"], b["X"], dcam, loss, a, frozen=frozen)
    Xc = bs.points(candidate=True)
    assert np.abs(Xc - Xc_ref).max() <= tol * max(1.0, np.abs(Xc_ref).max())
    assert np.allclose(out3, o3, rtol=1e-9, atol=1e-15)
    if frozen is not None:
        assert np.array_equal(Xc[frozen == 1], b["X"][frozen == 1])
    cc = bs.cost(loss, a, candidate=True)
    pt = np.repeat(np.arange(len(b["off"]) - 1), np.diff(b["off"]))
    rc, _ = ref.eval_jet(kind, b["aa"][b["cam"]], b["t"][b["cam"]], Xc[pt], b["obs"], 1.0, b["rows"], b["cols"])
    assert abs(cc - ref.huber_block(rc, loss, a)[1].sum()) <= 1e-9 * cc
    assert abs(bs.cost(loss, a) - e["cost"]) <= 1e-12 * e["cost"]
    bs.accept()
    assert np.array_equal(bs.points(), Xc)
    bs.close()


def test_mixed_kinds_in_one_context(ctx):
    """Sets of all three kinds live side by side; the 1Angle set is unaffected by the two-row sets."""
    import panovlm_amd as pv
    rng = np.random.default_rng(3)
    b1 = synth.random_bundle(rng, n_cams=5, n_points=30)
    ctx.set_poses(b1["aa"], b1["t"])
    s1 = pv.BundleSet(ctx, b1["off"], b1["cam"], b1["bearing"], b1["X"])
    r1, J1 = s1.evaluate()
    s2 = pv.BundleSet(ctx, b1["off"], b1["cam"], rng.uniform(0, 100, size=(len(b1["cam"]), 2)), b1["X"], kind="pixel", rows=100, cols=200)
    r2, _ = s2.evaluate()
    assert r2.shape == (2 * len(b1["cam"]),)
    r1b, J1b = s1.evaluate()
    assert np.array_equal(r1, r1b) and np.array_equal(J1, J1b) and r1.shape == (len(b1["cam"]),)
    s1.close(); s2.close()


@pytest.mark.parametrize("mode,threshold", [(0, 4.0), (0, -1.0), (1, 2.0)])
def test_filter_tracks_mask_matches_numpy(ctx, mode, threshold):
    import panovlm_amd as pv
    sc = filter_scene(np.random.default_rng(200 + mode), n_tracks=5000)
    keep = pv.api.filter_tracks(ctx, "pixel" if mode == 0 else "angle", sc["rows"], sc["cols"], sc["off"], sc["fid"], sc["kp"], sc["X"], sc["T"], threshold)
    exp = ref.filter_ref(mode, sc["rows"], sc["cols"], sc["off"], sc["fid"], sc["kp"], sc["X"], sc["T"], ref.filter_threshold(mode, threshold))
    assert np.array_equal(keep, exp)
    if threshold < 0:
        assert keep.all()
    else:
        assert 0 < keep.sum() < len(keep)


# ---- host mirror through tests/cpp/pvlm_sfm_driver.cpp: SfMGlobalBA, GlobalBundleAdjustment, RefineCameraPose ------------------------
def _driver(args, timeout=600):
    import os
    import subprocess
    from panovlm_amd import build
    assert os.path.exists(build.SFM_DRIVER), "build() makes the driver"
    subprocess.run([build.SFM_DRIVER] + [str(a) for a in args], check=True, timeout=timeout)


def _rot_err(Ra, Rb):
    c = (np.einsum("nij,nij->n", Ra, Rb) - 1.0) / 2.0
    return np.arccos(np.clip(c, -1.0, 1.0))


def _centre_err(t, t_true):
    """camera-centre error after the best scale about frame 0 (the pixel residual leaves the scale free)"""
    d, e = t - t[:1], t_true - t_true[:1]
    s = float((d * e).sum() / max((d * d).sum(), 1e-300))
    return np.linalg.norm(s * d - e, axis=1)


def test_sfm_global_ba_pixel_converges_and_is_reproducible(tmp_path):
    sc = ref.trajectory_scene(np.random.default_rng(60), n_frames=60, n_tracks=20000)
    F = len(sc["R0"])
    ref.write_scene(tmp_path / "in.bin", sc)
    _driver(["ba", tmp_path / "in.bin", tmp_path / "a.bin", 2, 1, 1, 1])
    _driver(["ba", tmp_path / "in.bin", tmp_path / "b.bin", 2, 1, 1, 1])
    a = ref.read_result(tmp_path / "a.bin", F)
    b = open(tmp_path / "b.bin", "rb").read()
    assert a["ok"] == 1 and a["final_cost"] < a["initial_cost"]
    assert a["raw"] == b                                                     # a second run: the same bits
    assert np.array_equal(a["R"][0], sc["R0"][0]) and np.array_equal(a["t"][0], sc["t0"][0])     # the gauge frame, bit for bit
    assert len(a["ids"]) == len(sc["tracks"])                               # SfMGlobalBA does not filter
    r0, r1 = _rot_err(sc["R0"], sc["R_true"])[1:].mean(), _rot_err(a["R"], sc["R_true"])[1:].mean()
    c0, c1 = _centre_err(sc["t0"], sc["t_true"])[1:].mean(), _centre_err(a["t"], sc["t_true"])[1:].mean()
    print("rotation error %.3e -> %.3e rad, centre error %.3e -> %.3e m, cost %.4e -> %.4e, %d steps" %
          (r0, r1, c0, c1, a["initial_cost"], a["final_cost"], a["steps"]))
    assert r1 < r0 / 4 and c1 < c0 / 3


def test_global_bundle_adjustment_removes_the_planted_outlier_tracks(tmp_path):
    sc = ref.trajectory_scene(np.random.default_rng(61), n_frames=30, n_tracks=3000, outlier_obs=0.0, outlier_tracks=40, outlier_px=80.0,
                              rot_noise=np.deg2rad(0.5), trans_noise=0.02)
    F = len(sc["R0"])
    ref.write_scene(tmp_path / "in.bin", sc)
    _driver(["gba", tmp_path / "in.bin", tmp_path / "out.bin", 2, 40, 10])   # InitCameraPose: (PIXEL, 40) then (PIXEL, 10)
    o = ref.read_result(tmp_path / "out.bin", F)
    assert o["ok"] == 1
    removed = np.setdiff1d(np.arange(len(sc["tracks"])), o["ids"])
    assert np.array_equal(removed, sc["planted"])
    assert np.all(np.diff(o["ids"]) > 0)                                     # survivors keep their order


def test_refine_camera_pose_keeps_camera_lidar_transforms(tmp_path):
    rng = np.random.default_rng(62)
    sc = ref.trajectory_scene(rng, n_frames=12, n_tracks=1500)
    F = len(sc["R0"])
    R_cl = ref.rot([0.01, -0.02, 1.5]); t_cl = np.array([0.1, -0.3, 0.05])
    lidars = [(sc["R0"][i] @ R_cl, sc["R0"][i] @ t_cl + sc["t0"][i]) for i in range(F)]
    ref.write_scene(tmp_path / "in.bin", sc, lidars=lidars)
    _driver(["refine", tmp_path / "in.bin", tmp_path / "out.bin"])
    o = ref.read_result(tmp_path / "out.bin", F, F)
    assert o["ok"] == 1
    assert np.abs(o["R"][1:] - sc["R0"][1:]).max() > 1e-4                   # the cameras did move
    for i in range(F):
        before_R = sc["R0"][i].T @ lidars[i][0]; before_t = sc["R0"][i].T @ (lidars[i][1] - sc["t0"][i])
        after_R = o["R"][i].T @ o["lidar_R"][i]; after_t = o["R"][i].T @ (o["lidar_t"][i] - o["t"][i])
        assert np.abs(after_R - before_R).max() <= 1e-12 and np.abs(after_t - before_t).max() <= 1e-12


# ---- SfMGlobalBA against the CPU LM twin (lm_twin's trust-region policy, numpy two-row functors) ---------------------------------------
def _twin_start(oracle, sc):
    from tests import lm_twin
    frames = [dict(R_wc=sc["R0"][i], t_wc=sc["t0"][i], valid=1) for i in range(len(sc["R0"]))]
    aa, t = lm_twin.frame_params(oracle, frames)
    return aa, t, np.array(sc["X0"], np.float64).copy()


def _twin(oracle, sc, kind_of_track):
    from tests import lm_twin
    aa, t, X = _twin_start(oracle, sc)
    opt = lm_twin.Options(); opt.max_num_iterations = 50          # SetOptionsSfM: Ceres' default of 50 iterations
    res = ref.lm_twin_solve(ref.scene_groups(sc, kind_of_track), aa, t, X, {0}, opt)
    return res, aa, t, X


def _check_against_twin(o, res, aa, t, X, R_wc, t_wc):
    assert o["ok"] == 1
    assert abs(o["initial_cost"] - res["initial_cost"]) <= 1e-9 * res["initial_cost"]
    assert res["final_cost"] < 0.8 * res["initial_cost"]                     # the adjustment does something
    assert abs(o["final_cost"] - res["final_cost"]) <= 1e-6 * res["final_cost"]
    assert o["steps"] == res["successful"] and o["unsuccessful"] == res["unsuccessful"]
    assert np.abs(R_wc - np.array([synth.rodrigues(a).T for a in aa])).max() <= 1e-6
    assert np.abs(t_wc - np.array([-synth.rodrigues(a).T @ tt for a, tt in zip(aa, t)])).max() <= 1e-6
    assert np.abs(o["X"] - X).max() <= 1e-6 * max(1.0, np.abs(X).max())


@pytest.mark.parametrize("residual_type,kind", [(2, ref.PIXEL), (1, ref.ANGLE2)])
def test_sfm_global_ba_matches_cpu_twin(oracle, tmp_path, residual_type, kind):
    """SfMGlobalBA(PIXEL_RESIDUAL / ANGLE_RESIDUAL_2) through the host mirror (AddCameraResidual: the keypoint widened, or its float
    ImageToSphere; HuberLoss(4.0) / HuberLoss(4 deg); the first frame as gauge; SetOptionsSfM) against the dense twin."""
    sc = ref.trajectory_scene(np.random.default_rng(70 + kind), n_frames=6, n_tracks=150, outlier_obs=0.08)
    F = len(sc["R0"])
    ref.write_scene(tmp_path / "in.bin", sc)
    _driver(["ba", tmp_path / "in.bin", tmp_path / "out.bin", residual_type, 1, 1, 1])
    o = ref.read_result(tmp_path / "out.bin", F)
    res, aa, t, X = _twin(oracle, sc, lambda ti: kind)
    assert res["outer_blocks_at_start"] > 0                                   # the loss matters: some blocks start in Huber's outer region
    assert o["blocks"] == sum(len(tr) for tr in sc["tracks"])
    _check_against_twin(o, res, aa, t, X, o["R"], o["t"])
    assert np.array_equal(o["R"][0], sc["R0"][0]) and np.array_equal(o["t"][0], sc["t0"][0])


def test_mixed_kinds_in_one_problem_match_cpu_twin(oracle, tmp_path):
    """Pixel blocks (even tracks) and 2Angle blocks (odd tracks) in ONE Problem: two device sets, one Solve."""
    sc = ref.trajectory_scene(np.random.default_rng(75), n_frames=6, n_tracks=150, outlier_obs=0.08)
    F = len(sc["R0"])
    ref.write_scene(tmp_path / "in.bin", sc)
    _driver(["mixed", tmp_path / "in.bin", tmp_path / "out.bin"])
    o = ref.read_result(tmp_path / "out.bin", F)
    res, aa, t, X = _twin(oracle, sc, lambda ti: ref.PIXEL if ti % 2 == 0 else ref.ANGLE2)
    assert o["ok"] == 1
    assert abs(o["initial_cost"] - res["initial_cost"]) <= 1e-9 * res["initial_cost"]
    assert abs(o["final_cost"] - res["final_cost"]) <= 1e-6 * res["final_cost"]
    assert o["steps"] == res["successful"] and o["unsuccessful"] == res["unsuccessful"]
    aa_o = o["R"].reshape(F, 9)[:, :3]                                        # the driver writes the raw angle-axis / t_cw parameters
    assert np.abs(aa_o - aa).max() <= 1e-6 and np.abs(o["t"] - t).max() <= 1e-6
    assert np.abs(o["X"] - X).max() <= 1e-6 * max(1.0, np.abs(X).max())


def test_angle_filter_after_global_ba_and_camera_lidar_ba(tmp_path):
    """GlobalBundleAdjustment(ANGLE_RESIDUAL_2, 2 deg): the survivors are exactly the tracks FilterTracksAngleResidual keeps at the BA's
    result (numpy restatement on SfMGlobalBA's output).  CameraLidarOptimizer::GlobalBundleAdjustment is SfMGlobalBA(ANGLE_RESIDUAL_1)
    on its frames and the caller's structure: the same bits as the driver's SfMGlobalBA."""
    sc = ref.trajectory_scene(np.random.default_rng(76), n_frames=10, n_tracks=600, outlier_obs=0.0, outlier_tracks=12, outlier_px=80.0,
                              rot_noise=np.deg2rad(0.5), trans_noise=0.02)
    F = len(sc["R0"])
    ref.write_scene(tmp_path / "in.bin", sc)
    _driver(["ba", tmp_path / "in.bin", tmp_path / "ba.bin", 1, 1, 1, 1])
    _driver(["gba", tmp_path / "in.bin", tmp_path / "gba.bin", 1, 2.0])
    b = ref.read_result(tmp_path / "ba.bin", F)
    g = ref.read_result(tmp_path / "gba.bin", F)
    assert np.array_equal(g["R"], b["R"]) and np.array_equal(g["t"], b["t"])
    T = np.array([ref.rigid_inverse_3x4(R, tt) for R, tt in zip(b["R"], b["t"])])
    off = np.concatenate([[0], np.cumsum([len(tr) for tr in sc["tracks"]])])
    obs = [sorted(tuple(o) for o in tr) for tr in sc["tracks"]]
    fid = np.array([f for tr in obs for f, _ in tr], np.int32)
    kp = np.array([sc["kps"][f][k] for tr in obs for f, k in tr], np.float32)
    keep = ref.filter_ref(1, sc["rows"], sc["cols"], off, fid, kp, b["X"], T, ref.filter_threshold(1, 2.0))
    assert np.array_equal(g["ids"], np.flatnonzero(keep))
    assert set(sc["planted"].tolist()) <= set(np.flatnonzero(keep == 0).tolist())
    _driver(["ba", tmp_path / "in.bin", tmp_path / "ba0.bin", 0, 1, 1, 1])
    _driver(["clo_ba", tmp_path / "in.bin", tmp_path / "clo.bin"])
    a0, c0 = open(tmp_path / "ba0.bin", "rb").read(), open(tmp_path / "clo.bin", "rb").read()
    assert c0[:4] == a0[:4] and c0[4 + 16 + 12:] == a0[4 + 16 + 12:]            # ok flag, poses and points (the summary is not returned)


@pytest.mark.parametrize("kind", [ref.ANGLE2, ref.PIXEL])
def test_cost_function_evaluate_two_row(kind):
    """CostFunction::Evaluate of PanoramaReprojResidual_2Angle / _Pixel: r and Ceres' 2 x 3 row-major Jacobian of each block."""
    import subprocess
    from panovlm_amd import build
    rng = np.random.default_rng(80 + kind)
    rows, cols, w = 960, 1920, 1.3
    for _ in range(4):
        aa, t, X = rng.normal(size=3) * 0.3, rng.normal(size=3) * 0.5, rng.normal(size=3) * 3 + np.array([0, 0, 4.0])
        o = np.array([rng.uniform(0, cols), rng.uniform(0, rows)]) if kind == ref.PIXEL else np.array([rng.uniform(-np.pi, np.pi), rng.uniform(-1.5, 1.5)])
        args = [kind, o[0], o[1], rows, cols, *aa, *t, *X, w]
        out = subprocess.run([build.SFM_DRIVER, "eval2"] + ["%.17g" % a for a in args], check=True, capture_output=True, text=True).stdout.split()
        assert out[0] == "eval2" and out[1] == "1"
        v = np.array([float(x) for x in out[2:]])
        r_ref, J_ref = ref.eval_jet(kind, aa[None], t[None], X[None], o[None], w, rows, cols)
        assert np.all(np.abs(v[:2] - r_ref[0]) <= 1e-6 * np.abs(r_ref[0]) + 1e-12 * max(rows, cols))
        for b in range(3):
            Jb = v[2 + 6 * b:8 + 6 * b].reshape(2, 3)
            assert np.abs(Jb - J_ref[0][:, 3 * b:3 * b + 3]).max() <= 1e-6 * np.abs(J_ref[0]).max()
