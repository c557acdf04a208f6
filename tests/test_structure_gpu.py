"""GPU checks of K32 through the C ABI: pvlm_triangulate_tracks and pvlm_filter_tracks_far against the host compile of the same per-track
cores (tests/cpp/structure_core_check.cpp) bit for bit — the cores use + - * / sqrt only, without contraction on both sides — the keypoint
input against the bearing input, the argument checks, and the host mirror's chain TriangulateTracks -> EstimateStructure ->
GlobalBundleAdjustment through tests/cpp/pvlm_structure_driver.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sfm_ba_ref as ba_ref
from tests import structure_ref as ref
from tests.structure_ref import build_check, host_filter_far, host_triangulate, make_far_tracks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chk():
    return build_check()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


# ---- 5. bit-for-bit agreement with the host compile (bearings input) ---------------------------------------------------------------------
# the generated tracks alone, so that the kernel gets exactly 1, 63, 64, 65 and 1000 tracks
@pytest.mark.parametrize("n_tracks,lengths,n_frames", [(1, [3], 12), (63, [2, 3, 40], 12), (64, [2, 3, 40], 12), (65, [2, 3, 40], 12), (1000, [2, 3, 40], 12),
                                                       (65, [2], 12), (65, [3], 12), (65, [40], 12), (65, [2, 3, 40], 2), (1000, [2, 3, 40], 700)])
def test_triangulate_bits_equal_host_compile(ctx, chk, n_tracks, lengths, n_frames):
    import panovlm_amd as pv
    rng = np.random.default_rng(500 + n_tracks + 7 * len(lengths) + n_frames)
    tr = ref.random_tracks(rng, n_tracks, n_frames, lengths)
    assert len(tr["off"]) - 1 == n_tracks
    valid = np.ones(n_frames, np.uint8); valid[n_frames - 1] = 0      # every track through the last frame: status 2, NaN point
    for fv in (None, valid):
        X, st = pv.api.triangulate_tracks(ctx, 0, 0, tr["off"], tr["fid"], tr["T"], frame_valid=fv, bearings=tr["b"])
        assert len(st) == n_tracks
        Xh, sth = host_triangulate(chk, tr["off"], tr["fid"], tr["T"], bearings=tr["b"], frame_valid=fv)
        assert np.array_equal(st, sth) and _same_bits(X, Xh)
        if fv is not None:
            through = np.array([(tr["fid"][tr["off"][t]:tr["off"][t + 1]] == n_frames - 1).any() for t in range(n_tracks)])
            assert np.all(st[through] == 2) and np.all(np.isnan(X[through])) and np.all(st[~through] != 2)
            assert through.any() or n_tracks == 1
        else:
            assert np.all(st == 0)
    X2, st2 = pv.api.triangulate_tracks(ctx, 0, 0, tr["off"], tr["fid"], tr["T"], bearings=tr["b"])     # a second run: the same bits
    Xh, sth = host_triangulate(chk, tr["off"], tr["fid"], tr["T"], bearings=tr["b"])
    assert _same_bits(X2, Xh) and np.array_equal(st2, sth)


@pytest.mark.parametrize("alone", [True, False])
def test_degenerate_tracks_bits_equal_host_compile(ctx, chk, alone):
    """The three degenerate tracks of the CPU tests in a call of their own, and after 64 generated tracks (in the tail of a second wave)."""
    import panovlm_amd as pv
    d = ref.degenerate_tracks()
    if not alone:
        tr = ref.random_tracks(np.random.default_rng(55), 64, 12, [2, 3, 40])
        T = tr["T"].copy(); T[:3] = d["T"]                       # frames 0..2 take the degenerate tracks' poses
        d = dict(T=T, off=np.concatenate([tr["off"], tr["off"][-1] + d["off"][1:]]), fid=np.concatenate([tr["fid"], d["fid"]]),
                 b=np.concatenate([tr["b"], d["b"]]))
    for fv in (None, [1, 1, 0] + [1] * (len(d["T"]) - 3)):
        X, st = pv.api.triangulate_tracks(ctx, 0, 0, d["off"], d["fid"], d["T"], frame_valid=fv, bearings=d["b"])
        Xh, sth = host_triangulate(chk, d["off"], d["fid"], d["T"], bearings=d["b"], frame_valid=fv)
        assert np.array_equal(st, sth) and _same_bits(X, Xh)
        if fv is None:
            assert st[-3:].tolist() == [0, 1, 1] and np.all(np.isnan(X[-3])) and np.isinf(X[-2]).any() and np.all(X[-1] == np.inf)
        else:
            assert st[-3:].tolist() == [0, 2, 1] and np.all(np.isnan(X[-2]))


def test_result_is_independent_of_neighbours(ctx):
    import panovlm_amd as pv
    tr = ref.random_tracks(np.random.default_rng(77), 200, 12, [2, 3, 40, 7])
    X, st = pv.api.triangulate_tracks(ctx, 0, 0, tr["off"], tr["fid"], tr["T"], bearings=tr["b"])
    for t in (0, 63, 64, 130, 199):                              # each track alone: the same bits as inside the batch
        o0, o1 = tr["off"][t], tr["off"][t + 1]
        X1, st1 = pv.api.triangulate_tracks(ctx, 0, 0, [0, o1 - o0], tr["fid"][o0:o1], tr["T"], bearings=tr["b"][o0:o1])
        assert _same_bits(X1[0], X[t]) and st1[0] == st[t]


# ---- 6. keypoints input == bearings input fed pvlm_image_to_cam_f32 of the rounded keypoints ------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(720, 1440), (2880, 5760)])
def test_keypoints_input_matches_bearings_input(ctx, chk, rows, cols):
    import panovlm_amd as pv
    rng = np.random.default_rng(600 + rows)
    tr = ref.random_tracks(rng, 300, 12, [2, 3, 5, 40])
    n = len(tr["fid"])
    kp = rng.uniform([0, 0], [cols - 1, rows - 1], size=(n, 2)).astype(np.float32)
    kp[:40] = np.floor(kp[:40]) + 0.5                            # x.5: round half to even
    kp[40:60, 0] = rng.choice([0.0, 0.4, cols - 1.0, cols - 0.6, cols - 0.5], size=20)     # the seam columns
    kp[60:80, 1] = rng.choice([0.0, 0.3, rows - 1.0, rows - 0.5, rows - 0.7], size=20)     # the pole rows
    b = ctx.image_to_cam(rows, cols, np.rint(kp).astype(np.float32))
    Xk, sk = pv.api.triangulate_tracks(ctx, rows, cols, tr["off"], tr["fid"], tr["T"], keypoints=kp)
    Xb, sb = pv.api.triangulate_tracks(ctx, 0, 0, tr["off"], tr["fid"], tr["T"], bearings=b)
    assert np.array_equal(sk, sb) and _same_bits(Xk, Xb)
    Xh, sh = host_triangulate(chk, tr["off"], tr["fid"], tr["T"], bearings=b)
    assert np.array_equal(sk, sh) and _same_bits(Xk, Xh)


# ---- 7. pvlm_filter_tracks_far --------------------------------------------------------------------------------------------------------------
def test_filter_far_equals_host_compile(ctx, chk):
    import panovlm_amd as pv
    ft = make_far_tracks()
    for valid in (None, ft["valid"]):
        keep = pv.api.filter_tracks_far(ctx, ft["off"], ft["fid"], ft["X"], ft["t_wc"], 8.0, frame_valid=valid)
        assert np.array_equal(keep, host_filter_far(chk, ft["off"], ft["fid"], ft["X"], ft["t_wc"], 8.0, valid))
        assert np.array_equal(keep, ref.filter_far_ref(ft["off"], ft["fid"], ft["X"], ft["t_wc"], 8.0, valid)[0])
    for n in (1, 63, 64, 65, 1000):
        off = ft["off"][:n + 1]
        keep = pv.api.filter_tracks_far(ctx, off, ft["fid"][:off[-1]], ft["X"][:n], ft["t_wc"], 8.0, frame_valid=ft["valid"])
        assert np.array_equal(keep, host_filter_far(chk, off, ft["fid"][:off[-1]], ft["X"][:n], ft["t_wc"], 8.0, ft["valid"]))
    # non-finite points and centres take the same IEEE course
    X = ft["X"][:64].copy(); X[3] = np.nan; X[9, 1] = np.inf
    off = ft["off"][:65]
    keep = pv.api.filter_tracks_far(ctx, off, ft["fid"][:off[-1]], X, ft["t_wc"], 8.0)
    assert np.array_equal(keep, host_filter_far(chk, off, ft["fid"][:off[-1]], X, ft["t_wc"], 8.0)) and keep[3] == 1 and keep[9] == 0


# ---- 9. argument checks --------------------------------------------------------------------------------------------------------------------
def test_argument_checks(ctx):
    import panovlm_amd as pv
    from panovlm_amd.api import PvlmError
    tr = ref.random_tracks(np.random.default_rng(9), 5, 4, [3])
    kp = np.full((len(tr["fid"]), 2), 10.0, np.float32)
    with pytest.raises(PvlmError):
        pv.api.triangulate_tracks(ctx, 100, 200, tr["off"], tr["fid"], tr["T"], keypoints=kp, bearings=tr["b"])
    with pytest.raises(PvlmError):
        pv.api.triangulate_tracks(ctx, 100, 200, tr["off"], tr["fid"], tr["T"])
    lib = ctx.lib
    off = np.ascontiguousarray(tr["off"]); fid = np.ascontiguousarray(tr["fid"]); T = np.ascontiguousarray(tr["T"]); b = np.ascontiguousarray(tr["b"])
    X = np.full((5, 3), 7.0); st = np.full(5, 9, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda n, kpp, bp: lib.pvlm_triangulate_tracks(ctx._h, C.c_int(100), C.c_int(200), C.c_int(n), p(off), p(fid), kpp, bp, C.c_int(4), p(T), None, p(X), p(st))
    ERR_ARG = lib.pvlm_triangulate_tracks(None, 0, 0, 0, None, None, None, None, 0, None, None, None, None)
    assert ERR_ARG != 0
    assert call(5, p(kp), p(b)) == ERR_ARG and call(5, None, None) == ERR_ARG and call(-1, None, p(b)) == ERR_ARG
    assert call(0, None, p(b)) == 0 and np.all(X == 7.0) and np.all(st == 9)          # PVLM_OK, nothing written
    assert lib.pvlm_filter_tracks_far(ctx._h, C.c_int(-1), p(off), p(fid), p(X), C.c_int(4), p(T), None, C.c_double(8.0), p(st)) == ERR_ARG
    assert lib.pvlm_filter_tracks_far(ctx._h, C.c_int(0), p(off), p(fid), p(X), C.c_int(4), p(T), None, C.c_double(8.0), p(st)) == 0 and np.all(st == 9)
    assert call(5, None, p(b)) == 0 and np.all(st == 0)


# ---- 8. the host mirror through the C++ driver -------------------------------------------------------------------------------------------------
def _driver(exe, args, timeout=600):
    assert os.path.exists(exe), "build() makes the driver"
    subprocess.run([exe] + [str(a) for a in args], check=True, timeout=timeout)


def _rot_err(Ra, Rb):
    c = (np.einsum("nij,nij->n", Ra, Rb) - 1.0) / 2.0
    return np.arccos(np.clip(c, -1.0, 1.0))


def _centre_err(t, t_true):
    d, e = t - t[:1], t_true - t_true[:1]
    s = float((d * e).sum() / max((d * d).sum(), 1e-300))
    return np.linalg.norm(s * d - e, axis=1)


def test_chain_without_a_structure_from_outside(tmp_path):
    """TriangulateTracks, CameraLidarOptimizer::EstimateStructure and GlobalBundleAdjustment(PIXEL_RESIDUAL, 40) on the rounded scene of the CPU
    tests with the poses perturbed as in K31's convergence test (1.5 deg, 0.1 m; frame 0 exact).  The structure comes from the matches alone.
    The chain must end where K31's run from the TRUE structure ends (pvlm_sfm_driver ba on the same scene, points = X_true + 2 cm): the same
    criteria as that test (cost falls, rotation error below a quarter, centre error below a third of the start; that test has no cost tolerance
    of its own) and, this test's own bound, a final cost per residual block within 5 % of the floor the pixel rounding leaves, which K31's run
    reaches too (derived below).  Two runs give identical bytes."""
    from panovlm_amd import build
    sc, pairs, matches, planted = ref.rounded_scene(np.random.default_rng(34))
    F = len(sc["R0"])
    ref.write_match_scene(tmp_path / "in.bin", sc, pairs, matches)
    _driver(build.STRUCTURE_DRIVER, ["chain", tmp_path / "in.bin", tmp_path / "a.bin", 2, 40])
    _driver(build.STRUCTURE_DRIVER, ["chain", tmp_path / "in.bin", tmp_path / "b.bin", 2, 40])
    a = ba_ref.read_result(tmp_path / "a.bin", F)
    assert a["raw"] == open(tmp_path / "b.bin", "rb").read()
    o = 4 + 16 + 12 + 96 * F + 4 + 28 * len(a["ids"])
    n_tri, est_ret, n_est = np.frombuffer(a["raw"], np.int32, 3, o)
    tri_ids = np.frombuffer(a["raw"], np.dtype([("id", np.uint32), ("X", np.float64, 3)]), n_tri, o + 12)["id"]
    est_ids = np.frombuffer(a["raw"], np.uint32, n_est, o + 12 + 28 * n_tri)
    assert np.all(np.diff(tri_ids.astype(np.int64)) > 0) and np.all(np.diff(est_ids.astype(np.int64)) > 0)
    assert set(est_ids.tolist()) <= set(tri_ids.tolist()) and est_ret == (1 if n_est < n_tri else 0)
    assert n_tri > len(sc["tracks"]) // 2 and n_est > len(sc["tracks"]) // 3
    # K31's run on the same frames with the structure handed in
    clean = np.setdiff1d(np.arange(len(sc["tracks"])), planted)              # without the tracks that carry a planted 40 deg observation
    sck = dict(sc, tracks=[sc["tracks"][i] for i in clean], X0=sc["X0"][clean])
    ba_ref.write_scene(tmp_path / "k31.bin", sck)
    _driver(build.SFM_DRIVER, ["ba", tmp_path / "k31.bin", tmp_path / "k31_out.bin", 2, 1, 1, 1])
    k = ba_ref.read_result(tmp_path / "k31_out.bin", F)
    r0 = _rot_err(sc["R0"], sc["R_true"])[1:].mean(); c0 = _centre_err(sc["t0"], sc["t_true"])[1:].mean()
    r1 = _rot_err(a["R"], sc["R_true"])[1:].mean(); c1 = _centre_err(a["t"], sc["t_true"])[1:].mean()
    rk = _rot_err(k["R"], sc["R_true"])[1:].mean(); ck = _centre_err(k["t"], sc["t_true"])[1:].mean()
    print("chain: %d triangulated, %d after EstimateStructure (returned %d), %d after the BA's filter" % (n_tri, n_est, est_ret, len(a["ids"])))
    print("chain: cost %.4e -> %.4e over %d blocks (%.4e per block); K31 from the true structure: %.4e -> %.4e over %d blocks (%.4e per block)" %
          (a["initial_cost"], a["final_cost"], a["blocks"], a["final_cost"] / a["blocks"], k["initial_cost"], k["final_cost"], k["blocks"], k["final_cost"] / k["blocks"]))
    print("chain: rotation error %.3e -> %.3e rad (K31 %.3e), centre error %.3e -> %.3e m (K31 %.3e)" % (r0, r1, rk, c0, c1, ck))
    assert a["ok"] == 1 and k["ok"] == 1 and a["final_cost"] < a["initial_cost"]
    assert r1 < r0 / 4 and c1 < c0 / 3
    # the cost both runs must end at: every keypoint coordinate carries the rounding error of a pixel, uniform in [-0.5, 0.5] (variance 1 / 12), no
    # residual is near Huber's 4 px, so at the optimum of r residuals over q free parameters the cost 0.5 sum r^2 is (1 / 24)(r - q) up to its
    # sampling spread: var(u^2) / E(u^2)^2 = 0.8 per residual, 0.8 % over the 14 k degrees of freedom here; 5 % = five such deviations + 1 %
    def floor_per_block(blocks, tracks):
        r, q = 2.0 * blocks, 3.0 * tracks + 6.0 * (F - 1)
        return (r - q) / 24.0 / blocks
    fa, fk = floor_per_block(a["blocks"], n_est), floor_per_block(k["blocks"], len(clean))
    print("chain: cost per block / rounding floor = %.4f (K31 from the true structure: %.4f)" % (a["final_cost"] / a["blocks"] / fa, k["final_cost"] / k["blocks"] / fk))
    assert a["final_cost"] / a["blocks"] <= 1.05 * fa and k["final_cost"] / k["blocks"] <= 1.05 * fk
