"""CPU checks of K36: the host compile of panovlm_amd/csrc/pvlm_relpose_core.h (tests/cpp/relpose_core_check.cpp) against the independent numpy twin of
tests/relpose_ref.py, the knife-edge condition on every scene any K36 test uses, what the refinement has to achieve, and the write-back."""
import subprocess

import numpy as np
import pytest

from tests import essential_ref as er
from tests import relpose_ref as rr

KINDS = ("pixel", "angle2")


@pytest.fixture(scope="module")
def chk():
    return rr.build_check("off")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 2, 8, 65])
def test_host_compile_against_the_twin(chk, kind, n):
    sc = rr.size_scene(n)
    call = rr.assemble([sc])
    rc, h = rr.host_refine(chk, call, kind)
    assert rc == 0
    tw = rr.twin_refine(sc, kind)
    print(kind, n, h["summaries"][0], tw["initial_cost"], tw["final_cost"], tw["successful"], tw["unsuccessful"], tw["termination"])
    rr.check_against(h, 0, tw, h["triangulated"], kind)
    if n >= 8:
        assert tw["successful"] >= 2                              # a solve that moved, not two agreeing no-ops


@pytest.mark.parametrize("kind", KINDS)
def test_outlier_and_pole_scenes_against_the_twin(chk, kind):
    """the Huber branch with rejected steps, and the zero-derivative convention on the pole axis (the twin zeroes the Jacobian Jet arithmetic leaves as inf / NaN)"""
    for name, sc in (("outlier", rr.outlier_scene(40)), ("pole", rr.pole_scene())):
        rc, h = rr.host_refine(chk, rr.assemble([sc]), kind)
        assert rc == 0
        tw = rr.twin_refine(sc, kind)
        print(kind, name, h["summaries"][0], tw["successful"], tw["unsuccessful"], tw["termination"])
        rr.check_against(h, 0, tw, h["triangulated"], kind)


def test_knife_edge_every_scene_of_every_test():
    """both host builds (-ffp-contract=off / fast) take the same accept / reject sequence and end for the same reason on every scene the CPU and GPU tests use: what
    makes equal step counts a fair demand of the device"""
    for kind in KINDS:
        for name, sc in rr.all_scenes():
            same, a = rr.same_decisions(rr.assemble([sc]), kind)
            assert same, (kind, name)
            for it in (0, 3):
                same, _ = rr.same_decisions(rr.assemble([sc]), kind, it)
                assert same, (kind, name, it)


def test_outlier_scene_takes_the_huber_branch_and_rejects_steps(chk):
    sc = rr.outlier_scene()
    rc, h = rr.host_refine(chk, rr.assemble([sc]), "pixel")
    s = h["summaries"][0]
    assert rc == 0 and s["unsuccessful_steps"] >= 1 and s["successful_steps"] >= 2
    assert rr.outer_blocks(sc, "pixel", sc["R0"], sc["t0"], sc["X0"]) > 0                              # blocks in Huber's outer region at the start ...
    assert rr.outer_blocks(sc, "pixel", h["R_21"][0], h["t_21"][0], h["triangulated"]) > 0             # ... and at the end: the planted errors stay errors


@pytest.mark.parametrize("kind", KINDS)
def test_refinement_helps(chk, kind):
    for n in (65, 300):
        sc = rr.size_scene(n)
        rc, h = rr.host_refine(chk, rr.assemble([sc]), kind)
        assert rc == 0 and h["ok"][0] == 1
        assert er.rotation_error_deg(h["R_21"][0], sc["R_true"]) < er.rotation_error_deg(sc["R0"], sc["R_true"])
        assert er.direction_error_deg(h["t_21"][0], sc["t_true"]) < er.direction_error_deg(sc["t0"], sc["t_true"])
    for kind2 in KINDS:
        for name, sc in rr.all_scenes():
            rc, h = rr.host_refine(chk, rr.assemble([sc]), kind2)
            assert rc == 0 and h["summaries"]["final_cost"][0] <= h["summaries"]["initial_cost"][0], (kind2, name)


def test_write_back(chk):
    sc = rr.size_scene(65)
    call = rr.assemble([sc])
    rc, h = rr.host_refine(chk, call, "pixel")
    assert rc == 0
    assert abs(np.linalg.norm(h["t_21"][0]) - 1.0) <= 4 * np.finfo(np.float64).eps
    # the points carry the same factor: with max_num_iterations = 0 nothing moves, so the factor is |t_21 of the input|
    call["t_21"] = call["t_21"] * 2.5
    rc, z = rr.host_refine(chk, call, "pixel", max_num_iterations=0)
    s = np.linalg.norm(call["t_21"][0])
    assert rc == 0 and tuple(z["summaries"][0])[2:] == (0, 0, 0)
    assert np.array_equal(_bits(z["triangulated"]), _bits(call["triangulated"] / s)) and np.array_equal(_bits(z["t_21"][0]), _bits(call["t_21"][0] / s))
    assert np.abs(z["R_21"][0] - call["R_21"][0]).max() <= 1e-15
    # no inlier: bit-identical, ok = 1, zero steps
    e = rr.size_scene(0)
    call = rr.assemble([e])
    rc, h = rr.host_refine(chk, call, "pixel")
    assert rc == 0 and h["ok"][0] == 1 and tuple(h["summaries"][0]) == (0.0, 0.0, 0, 0, 6)
    assert np.array_equal(_bits(h["R_21"]), _bits(call["R_21"])) and np.array_equal(_bits(h["t_21"]), _bits(call["t_21"]))


def test_degenerate_scale_keeps_the_input(chk):
    """camera 2 at camera 1's centre and every point observed where it already projects: nothing moves, |t| = 0, the pair comes back as it went in with ok = 0"""
    sc = rr.size_scene(8)
    sc["t0"] = np.zeros(3); sc["R0"] = np.eye(3)
    X = sc["X0"]
    sc["kp1"] = rr.pixels_of(X); sc["kp2"] = sc["kp1"].copy()
    sc["matches"]["query"] = np.arange(8); sc["matches"]["train"] = np.arange(8)
    call = rr.assemble([sc])
    rc, h = rr.host_refine(chk, call, "pixel", max_num_iterations=0)
    assert rc == 0 and h["ok"][0] == 0
    assert np.array_equal(_bits(h["R_21"]), _bits(call["R_21"])) and np.array_equal(_bits(h["t_21"]), _bits(call["t_21"]))
    assert np.array_equal(_bits(h["triangulated"]), _bits(call["triangulated"]))


def test_argument_checks(chk):
    sc = rr.size_scene(8)
    call = rr.assemble([sc])
    def rc_of(kind="pixel", it=50, **kw):
        c = dict(call); c.update(kw)
        rc, h = rr.host_refine(chk, c, kind, it)
        if rc:
            assert np.array_equal(_bits(h["R_21"]), _bits(c["R_21"])) and np.array_equal(_bits(h["triangulated"]), _bits(c["triangulated"]))
        return rc
    assert rc_of() == 0
    idx = call["inlier_idx"].copy(); idx[2] = 8
    tri = call["triangulated"].copy(); tri[1, 1] = np.nan
    assert rc_of(inlier_idx=idx) == -1 and rc_of(triangulated=tri) == -1 and rc_of(kind=0) == -1 and rc_of(it=-1) == -1
    assert rc_of(src=np.array([5], np.int32)) == -1


def test_stand_alone_program_under_the_host_sanitizers():
    """tests/cpp/relpose_core_check.cpp with its own main under -fsanitize=address,undefined (0, 1, 65 and 300 points, both kinds)"""
    exe = rr.build_check_main(sanitize=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr


# ---- the host tail -----------------------------------------------------------------------------------------------------------------------------------
def _depth_scene(seed, n=60, half=True, true_scale=2.5, noise=None, spread=None):
    """n points in front of both cameras of a pair with |t_21| = 1, and the two depth maps that hold true_scale x depth at the pixel each point rounds to (the maps of a
    scene whose real baseline is true_scale).  noise: per-point factors on the depths of map 2; spread: per-point factors on both maps."""
    rng = np.random.default_rng(seed)
    R = er.rodrigues((0.02, -0.1, 0.03)); t = np.array([0.8, 0.1, -0.59]); t /= np.linalg.norm(t)
    X = rng.uniform(-4, 4, size=(n, 3)); X[:, 2] = rng.uniform(2, 6, n)
    rows, cols = rr.ROWS, rr.COLS
    k = 2 if half else 1
    d1 = np.zeros((rows // k + (rows % k), cols // k), np.uint16); d2 = np.zeros_like(d1)
    f2 = np.ones(n) if noise is None else noise; fs = np.ones(n) if spread is None else spread
    for i, p in enumerate(X):
        for d, q, f in ((d1, p, fs[i]), (d2, R @ p + t, fs[i] * f2[i])):
            x, y = rr._cam_to_image(rows, cols, q)
            row, col = rr._round_half_away(y / k), rr._round_half_away(x / k)
            if 0 <= row < d.shape[0] and 0 <= col < d.shape[1]:
                d[row, col] = min(65535, int(round(true_scale * f * np.linalg.norm(q) * 256)))
    return rows, cols, d1, d2, R, t, X


def _scale_both(chk, rows, cols, d1, d2, R, t, X):
    ref = rr.scale_ref(rows, cols, rows, d1, d2, R, t, X)
    got = rr.host_scale(chk, rows, cols, rows, d1, d2, R, t, X)
    assert got[0] == ref[0] and got[3] == ref[3]
    assert np.array_equal(_bits(got[1]), _bits(ref[1])) and np.array_equal(_bits(got[2]), _bits(ref[2])), "t_21 and the points bit for bit"
    assert np.array_equal(_bits([got[4], got[5]]), _bits([ref[4], ref[5]]))
    return got


@pytest.mark.parametrize("half", [True, False])
def test_scale_early_exit_on_half_and_full_size_maps(chk, half):
    """every scale within 1.2 of every other: the first pass breaks, the mean is taken"""
    ok, t, X, pwd, up, lo = _scale_both(chk, *_depth_scene(1, half=half))
    assert ok and pwd >= 50 and 0 < lo <= up < 1.2 * lo and abs(np.linalg.norm(t) - 2.5) < 0.02


def test_scale_histogram_path(chk):
    """scales spread over a factor 3 with most of them near the truth: two histogram passes keep the populated bins"""
    rng = np.random.default_rng(2)
    spread = np.where(rng.uniform(size=200) < 0.7, rng.uniform(0.97, 1.03, 200), rng.uniform(0.5, 1.6, 200))
    ok, t, X, pwd, up, lo = _scale_both(chk, *_depth_scene(2, n=200, spread=spread))
    assert ok and up > 0 and 10 <= pwd < 200 and up / lo < 1.6 / 0.5


def test_scale_median_fallback(chk):
    """twelve scales spread over a factor 2.3, the two of a point 15 % apart and so in different bins: most bins hold one scale (not more than a tenth of twelve),
    fewer than 10 scales are left after the first pass, the median of all twelve is taken"""
    spread = np.linspace(1.0, 2.0, 6)
    ok, t, X, pwd, up, lo = _scale_both(chk, *_depth_scene(3, n=6, spread=spread, noise=np.full(6, 1.15)))
    assert ok and (up, lo) == (0.0, 0.0) and pwd == 6


def test_scale_too_few_points_inconsistent_depths_and_no_map(chk):
    rows, cols, d1, d2, R, t, X = _depth_scene(4, n=4)
    got = _scale_both(chk, rows, cols, d1, d2, R, t, X)                         # 8 scales < 10
    assert not got[0] and np.array_equal(got[1], t) and (got[3], got[4], got[5]) == (0, -1.0, -1.0)
    got = _scale_both(chk, *_depth_scene(5, n=40, noise=np.full(40, 1.5)))      # the two depths disagree by more than 0.2 everywhere
    assert not got[0]
    got = _scale_both(chk, rows, cols, None, d2, R, t, X)
    assert not got[0]


def test_scale_point_projecting_outside(chk):
    """a point whose rounded pixel falls on the last column + 1 (longitude +pi) is skipped by IsInside, in the restatement and in the mirror alike"""
    rows, cols, d1, d2, R, t, X = _depth_scene(6, n=30, half=False)
    X = np.concatenate([X, [[1e-9, 0.3, -5.0], [-1e-9, 0.3, -5.0]]])            # longitude just below +pi and just above -pi
    d1[:, -1] = 1000; d1[:, 0] = 1000
    full = _scale_both(chk, rows, cols, d1, d2, R, t, X)
    assert full[0]
    x_hi, _ = rr._cam_to_image(rows, cols, X[-2])
    assert rr._round_half_away(x_hi) == cols                                   # the case is the one it claims to be


def test_largest_biconnected_graph(chk):
    g = lambda pairs: rr.host_graph(chk, pairs)
    keep, nodes = g([(0, 1), (1, 2), (2, 3)])                                   # a path: every edge is a bridge
    assert keep == [0, 0, 0] and nodes == [0]
    keep, nodes = g([(3, 4), (0, 1), (1, 2), (0, 2), (2, 3)])                   # a cycle with a pendant chain
    assert keep == [0, 1, 1, 1, 0] and nodes == [0, 1, 2]
    keep, nodes = g([(5, 6), (6, 7), (5, 7), (7, 1), (1, 2), (2, 3), (1, 3)])   # two triangles joined by a bridge: the one with the lower frame id
    assert keep == [0, 0, 0, 0, 1, 1, 1] and nodes == [1, 2, 3]
    keep, nodes = g([(0, 1), (1, 2), (0, 2), (10, 11), (11, 12), (12, 13), (10, 13)])   # two cycles of different size
    assert keep == [0, 0, 0, 1, 1, 1, 1] and nodes == [10, 11, 12, 13]
    assert g([]) == ([], [])
    keep, nodes = g([(0, 1), (1, 0), (1, 2)])                                   # (a, b) and (b, a) are two parallel edges: no bridge between them
    assert keep == [1, 1, 0] and nodes == [0, 1]


def test_final_sort_with_the_comparator_as_written(chk):
    pairs = [(1, 2), (0, 3), (2, 3), (0, 1), (1, 3), (0, 2)]
    assert rr.host_sort(chk, pairs) == rr.sort_ref(pairs)
    rng = np.random.default_rng(3)
    more = [(int(a), int(b)) for a, b in rng.integers(0, 9, size=(40, 2))]
    assert rr.host_sort(chk, more) == rr.sort_ref(more)


def test_filter_image_pairs_full_through_the_host_functions():
    """pvlm::MatchImagePairsHost -> pvlm::FilterImagePairsFullHost (FilterImagePairsHost, RefineRelativePosesHost, SetTranslationScaleDepthMap, LargestBiconnectedGraph,
    the final sort) of the host mirror on the driver's six-frame scene, no device: two triangles joined by a bridge, the one with the lower frame ids survives in
    upstream's order with the scene's baselines and poses (the driver checks it)"""
    from panovlm_amd import build
    build.build_host()
    out = subprocess.run([build.RELPOSE_DRIVER, "host"], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host route only" in out.stdout and out.stdout.count("pair (") == 3
