"""CPU checks of K45: the host compile of panovlm_amd/csrc/pvlm_rotstart_core.h (tests/cpp/rotstart_core_check.cpp: shift-and-invert subspace iteration) against the
independent numpy restatement of upstream's RotationAveragingLeastSquare in tests/rotstart_ref.py (dense A^T A, eigh, svd), the invariance of the result to the
start, what the start has to achieve, the info values and the refused arguments, the host mirror's method 2, and the stand-alone sanitizer program."""
import subprocess

import numpy as np
import pytest

from tests import rotavg_ref as rr
from tests import rotstart_ref as rs

NAMES = list(rs.scenes().keys())
NOISY = [n for n in NAMES if n != "exact"]


def _angle(name):
    return rr.largest_angle(rs.reference(name)["rotations"], rs.host(name)["rotations"])


@pytest.mark.parametrize("name", NAMES)
def test_scene_against_reference(name):
    """info 0, three solves per iteration, camera 0 the identity to rounding, every rotation within rotstart_ref.TOL of upstream's dense method"""
    h = rs.host(name)
    a = _angle(name)
    print(name, "iterations", h["iterations"], "solves", h["solves"], "residual %.3e" % h["residual"], "theta", h["theta"], "angle to the reference %.3e rad" % a)
    assert h["rc"] == 0 and h["info"] == 0 and h["solves"] == 3 * h["iterations"] and 1 <= h["iterations"] <= rs.MAX_ITERATIONS
    assert h["residual"] <= rs.TOL_REL
    assert np.abs(h["rotations"][0] - np.eye(3)).max() <= 8 * np.finfo(np.float64).eps
    for R in h["rotations"]:
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and np.linalg.det(R) > 0
    assert a <= rs.TOL, (a, rs.TOL)
    # the Ritz values are the three eigenvalues of smallest magnitude
    lam = rs.reference(name)["eigenvalues"]
    assert np.abs(np.sort(h["theta"]) - np.sort(lam[:3])).max() <= 1e-12 * max(1.0, float(lam[3]))


def test_measured_is_the_maximum():
    """rotstart_ref.MEASURED is what it says: the largest angle over the scenes, within its own last digit"""
    worst = max(_angle(n) for n in NAMES)
    print("measured %.4e recorded %.4e" % (worst, rs.MEASURED))
    assert worst <= rs.MEASURED <= 1.1 * worst


@pytest.mark.parametrize("name", NAMES)
def test_invariant_to_the_start(name):
    """the spanning-tree start and the same start times one fixed improper orthogonal matrix (determinant -1) give the same rotations: the result depends on the
    subspace alone, and the sign rule with the product by R_0^T removes the common factor"""
    sc = rs.scenes()[name]
    turned = rs.host_least_square(sc, R0=np.array([R @ rs.IMPROPER_Q for R in sc["R0"]]))
    assert abs(np.linalg.det(rs.IMPROPER_Q) + 1) < 1e-15
    a = rr.largest_angle(turned["rotations"], rs.host(name)["rotations"])
    print(name, "iterations", turned["iterations"], rs.host(name)["iterations"], "angle %.3e" % a)
    assert turned["rc"] == 0 and turned["info"] == 0
    assert a <= rs.TOL


def test_any_start_of_full_rank():
    """a random 3 F x 3 start (nothing like rotations) reaches the same subspace"""
    sc = rs.scenes()["rand12"]
    h = rs.host_least_square(sc, R0=np.random.default_rng(5).normal(size=(sc["F"], 3, 3)))
    assert h["info"] == 0 and rr.largest_angle(h["rotations"], rs.host("rand12")["rotations"]) <= rs.TOL
    print("iterations from a random start", h["iterations"])


def test_truth():
    """noise-free: the true R_c R_0^T to 1e-12.  With a degree of noise per pair: as close to the truth as upstream's method is (a comparison of the two distances,
    which may differ by what the two results differ by)"""
    sc = rs.scenes()["exact"]
    assert rr.largest_angle(rs.host("exact")["rotations"], sc["truth"]) <= 1e-12
    assert np.abs(rs.host("exact")["rotations"] - sc["truth"]).max() <= 1e-12
    for name in NOISY:
        truth = rs.scenes()[name]["truth"]
        mine, theirs = rr.largest_angle(rs.host(name)["rotations"], truth), rr.largest_angle(rs.reference(name)["rotations"], truth)
        print(name, "to the truth: host compile %.6e reference %.6e rad" % (mine, theirs))
        assert mine <= theirs + rs.TOL


def _untouched(h, sc, R0=None):
    return np.array_equal(h["rotations"], sc["R0"] if R0 is None else R0)


def test_info_values():
    """-2: max_iterations = 1 on band200; -3: a start whose Gram matrix is singular (all zero; two equal columns); k > 0: an R_21 that is ten times a rotation makes
    M + sigma I indefinite.  The rotations stay as they came every time; the summary says what happened."""
    sc = rs.scenes()["band200"]
    h = rs.host_least_square(sc, max_iterations=1)
    assert h["rc"] == 0 and h["info"] == -2 and h["iterations"] == 1 and h["solves"] == 3 and h["residual"] > rs.TOL_REL and _untouched(h, sc)
    sc = rs.scenes()["rand12"]
    zero = np.zeros_like(sc["R0"])
    h = rs.host_least_square(sc, R0=zero)
    assert h["rc"] == 0 and h["info"] == -3 and h["iterations"] == 0 and _untouched(h, sc, zero)
    twice = sc["R0"].copy(); twice[:, :, 2] = twice[:, :, 1]
    h = rs.host_least_square(sc, R0=twice)
    assert h["rc"] == 0 and h["info"] == -3 and _untouched(h, sc, twice)
    R = sc["R_21"].copy(); R[3] *= 10.0
    h = rs.host_least_square(dict(sc, R_21=R))
    assert h["rc"] == 0 and h["info"] > 0 and _untouched(h, sc)


def test_refused_arguments():
    """every PVLM_ERR_ARG case through the host compile's entry: -1, the rotations and the summary untouched"""
    sc = rs.scenes()["rand12"]
    calls = rs.bad_calls(sc)
    assert len(calls) >= 15
    for name, bad, kw in calls:
        h = rs.host_least_square(bad, **kw)
        assert h["rc"] == -1, name
        assert np.array_equal(h["rotations"], np.asarray(bad["R0"]), equal_nan=True), name
        assert (h["iterations"], h["solves"], h["info"], h["residual"]) == (-7, -7, -7, -7.0) and np.all(h["theta"] == -7.0), name
    h = rs.host_least_square(sc, summary=False)
    assert h["rc"] == -1 and _untouched(h, sc)


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------------
def _after_triplet(g):
    """the pairs of the mirror scene that EstimateGlobalRotation hands its averaging: LargestBiconnectedGraph, FilterByTriplet(0.1) (the restatements K40's tests use)"""
    e = rr.estimate_ref(g)
    return e, e["after_triplet"]


def test_least_square_by_hand():
    """RotationAveragingLeastSquare of the mirror on a scene's pairs equals the host compile called directly from numpy's spanning-tree start within
    rotstart_ref.TOL (the two starts differ in the last bit: numpy's matmul may order the three products of an entry differently); a list that does not reach every
    camera is refused with the rotations untouched"""
    sc = rs.scenes()["band5"]
    g = dict(F=sc["F"], R_wc=np.zeros((sc["F"], 3, 3)), t_wc=np.zeros((sc["F"], 3)),
             pairs=[dict(first=int(i), second=int(j), R_21=R, t_21=np.zeros(3), upper=0.0, lower=0.0) for i, j, R in zip(sc["first"], sc["second"], sc["R_21"])])
    d = rs.run_driver(g, "lsq", "host")
    assert d["ok"] == 1
    assert rr.largest_angle(np.array([d["rotations"][c] for c in range(sc["F"])]), rs.host("band5")["rotations"]) <= rs.TOL
    cut = dict(g, pairs=[p for p in g["pairs"] if 4 not in (p["first"], p["second"])])
    d = rs.run_driver(cut, "lsq", "host")
    assert d["ok"] == 0 and all(np.all(d["rotations"][c] == -7.0) for c in range(sc["F"]))


def test_estimate_global_rotation_method_2_host():
    """EstimateGlobalRotation(method 2, enable_l2_start) on K40's mirror scene, host route.  Upstream's method 2 is the least-square start and RotationAveragingL2
    and nothing else (sfm/SfM.cpp:859-869): it has no FilterPairs, which is part of RotationAveragingL1 alone.  So the surviving pairs are those the graph and triplet
    filters leave — method 1's survivors plus the pairs its X84 filter drops (the pair planted 0.08 degrees off among them), which the test states both ways.
    Every rotation within 0.02 degrees of the truth, the bound of the method-1 test on this scene; pair.R_21 = R_2w R_1w^T written back; no message."""
    g = rr.mirror_scene()
    e, after_triplet = _after_triplet(g)
    d = rs.run_driver(g, "estimate", "host", 2, 1, 1)
    assert d["ok"] == 1 and d["message"] == ""
    assert d["pairs"] == after_triplet
    one = rr.run_driver(g, "estimate", "host", 1, 1)
    assert set(one["pairs"]) < set(d["pairs"]) and (5, 7) in set(d["pairs"]) - set(one["pairs"]) and (8, 10) not in d["pairs"]
    R0 = g["R_cw_true"][0]
    truth = max(rr.angle_between(d["R_wc"][i].T, g["R_cw_true"][i] @ R0.T) for i in range(g["F"]))
    both = max(rr.angle_between(d["R_wc"][i].T, one["R_wc"][i].T) for i in range(g["F"]))
    print("method 2 against the truth %.5f degrees, against method 1 %.5f degrees" % (np.degrees(truth), np.degrees(both)))
    assert all(d["valid"][i] == 0 for i in range(g["F"]))          # rotations only: no frame has a translation yet
    assert np.degrees(truth) < 0.02
    for (i, j), R21 in zip(d["pairs"], d["R_21"]):
        assert np.abs(R21 - d["R_wc"][j].T @ d["R_wc"][i]).max() <= 4 * np.finfo(np.float64).eps


def test_method_2_without_the_flag_is_refused_as_before():
    g = rr.mirror_scene()
    d = rs.run_driver(g, "estimate", "host", 2, 1, 0)
    old = rr.run_driver(g, "estimate", "host", 2, 1)
    text = "Rotation averaging method not supported: L2 needs the eigenvectors of a dense 3 F x 3 F matrix for its start and is not built"
    assert d["ok"] == 0 and old["ok"] == 0 and d["message"] == old["message"] == text


def test_rotation_then_translation_method_2():
    """method 2 into EstimateGlobalTranslation (method 1): every frame gets a pose; the bounds of K40's chain test"""
    g = rr.mirror_scene()
    c = rs.run_driver(g, "chain", "host", 2, 1, 1)
    assert c["ok"] == 1 and c["translation_ok"] == 1, (c["message"], c["translation_message"])
    assert all(c["valid"][i] == 1 for i in range(g["F"]))
    s, worst = rr.chain_error(g, c)
    print("scale %.4f, largest centre error %.5f m" % (s, worst))
    assert 0.9 - 1e-6 <= s <= 1.3 + 1e-6 and worst < 2e-3


def test_sanitizer_main():
    """tests/cpp/rotstart_core_check.cpp with its own main under -fsanitize=address,undefined: 2 cameras, a noise-free band of 40, a band of 70 with noise, and the
    same stopped after one iteration (info -2, nothing written)"""
    from panovlm_amd import build
    out = subprocess.run([build.build_rotstart_check(main=True, sanitize=True)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
