"""CPU checks of K44: the host compile of panovlm_amd/csrc/pvlm_bata_core.h (tests/cpp/bata_core_check.cpp) against the independent numpy reference of
tests/bata_ref.py (the dense KKT system and the dense normal equations), the knife-edge condition on every scene any K44 test uses, what BATA has to achieve, and the
host mirror's TranslationAveragingBATA / EstimateGlobalTranslation on the host compile (tests/cpp/pvlm_bata_driver.cpp)."""
import subprocess

import numpy as np
import pytest

from tests import bata_ref as br

NAMES = list(br.scenes().keys())
_HOST = {}


def _host(name):
    if name not in _HOST:
        sc, kw = br.scenes()[name]
        _HOST[name] = br.host_solve(sc, **kw)
    return _HOST[name]


def test_group_size():
    assert br.host_group_size() == br.G


@pytest.mark.parametrize("name", NAMES)
def test_knife_edge(name):
    """Every scene of the K44 tests is admitted: on the reference no e_k within 1e-9 (relative) of robust_threshold, no d_k . tij_k with |cos| < 1e-6, no camera
    left with a total weight below 1e-9 of the largest — at every pass.  A scene that fails is replaced in bata_ref.SEEDS, never skipped."""
    ref = br.reference(name)
    assert ref["knife"] == [], ref["knife"]


@pytest.mark.parametrize("name", NAMES)
def test_host_against_reference(name):
    """info = 0; centres, LUD centres and scales within bata_ref.TOL = ten times the largest difference the host compile shows against the reference over these
    scenes (bata_ref.MEASURED: 8.7e-13 in a centre, 3.5e-13 in a LUD centre, 4.5e-13 relative in a scale); the dropped rows (scale +inf) are the same rows."""
    ref, h = br.reference(name), _host(name)
    assert h["rc"] == 0 and h["info"] == 0
    d = br.differences(h, ref)
    print(name, "differences", d)
    assert np.all(h["centres"][0] == 0.0) and np.all(h["lud_centres"][0] == 0.0)
    for k in br.TOL:
        assert d[k] <= br.TOL[k], (k, d[k], br.TOL[k])


def test_measured_is_the_maximum():
    """bata_ref.MEASURED is what it says: the largest difference over the scenes, each figure within its own last digit"""
    worst = {k: 0.0 for k in br.TOL}
    for name in NAMES:
        d = br.differences(_host(name), br.reference(name))
        worst = {k: max(worst[k], d[k]) for k in worst}
    print("largest differences host compile - reference:", worst)
    for k in worst:
        assert worst[k] <= br.MEASURED[k], (k, worst[k])
        assert worst[k] >= 0.8 * br.MEASURED[k], (k, worst[k])


def test_noise_free_recovers_the_truth():
    """exact directions: the true centres up to one positive common factor and camera 0's shift.  Tolerance: ten times what the numpy reference itself reaches on
    the scene (bata_ref.REF_EXACT = 3.2e-15, in the solver's unit)."""
    sc, kw = br.scenes()["exact"]
    ref, h = br.reference("exact"), _host("exact")
    f_ref, truth_ref = br.align(ref["centres"], sc["centres"]); e_ref = np.abs(ref["centres"] - truth_ref).max()
    f, truth = br.align(h["centres"], sc["centres"]); e = np.abs(h["centres"] - truth).max()
    print("factor %.6f, distance from the truth: reference %.3e, host compile %.3e" % (f, e_ref, e))
    assert e_ref <= br.REF_EXACT
    assert f > 0 and e <= 10 * br.REF_EXACT


def test_outliers_leave_the_inliers_in_place():
    """about 10 % gross outlier directions, half of them reversed (their scale turns negative and the row drops, BATA.cpp:156): every camera none of whose pairs is an
    outlier stays within ten times the distance the reference reaches (bata_ref.REF_OUTLIER = 6.5e-2 in the solver's unit)"""
    sc, kw = br.scenes()["outlier"]
    ref, h = br.reference("outlier"), _host("outlier")
    touched = set(sc["first"][sc["bad"]].tolist()) | set(sc["second"][sc["bad"]].tolist())
    good = [c for c in range(sc["F"]) if c not in touched]
    assert len(sc["bad"]) == 15 and len(good) >= 10
    assert np.isinf(ref["scales"]).sum() >= 3 and np.array_equal(np.isinf(h["scales"]), np.isinf(ref["scales"]))
    e_ref = np.linalg.norm(ref["centres"] - br.align(ref["centres"], sc["centres"])[1], axis=1)[good].max()
    e = np.linalg.norm(h["centres"] - br.align(h["centres"], sc["centres"])[1], axis=1)[good].max()
    print("largest distance of an inlier camera: reference %.3e, host compile %.3e" % (e_ref, e))
    assert e_ref <= br.REF_OUTLIER
    assert e <= 10 * br.REF_OUTLIER


def test_both_weight_branches():
    """Wvec = 1 below the threshold and thr / e above it are both taken (from the reference's weights), in the outlier scene and over all scenes"""
    w = np.concatenate(br.reference("outlier")["wvec"])
    assert (w == 1.0).sum() > 0 and ((w > 0) & (w < 1)).sum() > 0
    for name in ("P257", "F65", "scaled"):
        w = np.concatenate(br.reference(name)["wvec"])
        assert (w == 1.0).sum() > 0 and ((w > 0) & (w < 1)).sum() > 0, name


@pytest.mark.parametrize("name", ["outlier", "hub9", "id2"])
def test_one_outer_is_the_lud_stage(name):
    """outer_iteration = 1: the centres are the LUD centres bit for bit, and those of the full call's LUD stage"""
    sc, kw = br.scenes()[name]
    h = br.host_solve(sc, outer_iteration=1)
    assert h["info"] == 0
    assert np.array_equal(h["centres"].view(np.uint64), h["lud_centres"].view(np.uint64))
    assert np.array_equal(h["lud_centres"].view(np.uint64), _host(name)["lud_centres"].view(np.uint64))
    ref = br.bata_ref(sc, outer_iteration=1)
    assert np.array_equal(ref["centres"], ref["lud_centres"]) and np.abs(h["centres"] - ref["centres"]).max() <= br.TOL["lud"]


def test_ids_are_shifted():
    """ids that start at 2 give the bits of the same list with ids from 0 (BATA.cpp:197, :207)"""
    sc, kw = br.scenes()["id2"]
    low = dict(sc); low["first"] = sc["first"] - 2; low["second"] = sc["second"] - 2; low["n_cameras"] = sc["F"]
    a, b = _host("id2"), br.host_solve(low)
    assert a["info"] == b["info"] == 0 and np.array_equal(a["centres"].view(np.uint64), b["centres"].view(np.uint64))


def test_two_components_not_positive_definite():
    h = br.host_solve(br.disconnected())
    assert h["rc"] == 0 and h["info"] > 0 and h["untouched"]


def test_not_finite_is_minus_one():
    """two cameras on one point cannot be arranged from outside; the same exit is reached by delta = -1: the weights (|r|^2 - 1)^-1/2 of the second LUD pass are NaN"""
    sc, kw = br.scenes()["scaled"]
    h = br.host_solve(sc, delta=-1.0)
    assert h["rc"] == 0 and h["info"] == -1 and h["untouched"]


def test_no_pairs():
    sc = dict(F=0, P=0, n_cameras=4, first=np.zeros(0, np.int32), second=np.zeros(0, np.int32), dir=np.zeros((0, 3)), s0=np.zeros(0))
    h = br.host_solve(sc)
    assert h["rc"] == 0 and h["info"] == -2 and h["untouched"]


def test_arguments_refused():
    sc, kw = br.scenes()["P3"]
    for name, bad in br.bad_calls(sc):
        h = br.host_solve(bad, **bad.get("kw", {}))
        assert h["rc"] == -1 and h["info"] == -7 and h["untouched"], name


def test_sanitizer_main():
    """tests/cpp/bata_core_check.cpp with its own main under -fsanitize=address,undefined (3, 9, 70 and 100 cameras, and a graph of two components)"""
    from panovlm_amd import build
    out = subprocess.run([build.build_bata_check(main=True, sanitize=True)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------------
def test_mirror_method_5_is_bata_by_hand():
    """EstimateGlobalTranslation(method 5, enable_bata) on the host compile against TranslationAveragingBATA applied by hand: all frames with a rotation and one
    biconnected component, so both re-indexings are the identity; no DLT start (BATA does not read the start).  t_wc = -R_wc t_cw."""
    g = br.mirror_graph()
    est = br.run_driver(g, "estimate", "host", method=5, seed=7, init_dlt=0, enable_bata=1)
    hand = br.run_driver(g, "bata", "host", seed=7)
    assert est["ok"] == 1 and hand["ok"] == 1, est["message"]
    assert sorted(est["pairs"]) == sorted((p["first"], p["second"]) for p in g["pairs"])
    for i in range(g["F"]):
        assert est["valid"][i] == 1
        want = -g["R_wc"][i] @ hand["t"][i]
        assert np.abs(est["t_wc"][i] - want).max() <= 8 * np.finfo(np.float64).eps * max(1.0, np.abs(want).max()), i
    # and what the numbers are: the reference on the observations of :496 with the driver's start scales
    obs = np.array([g["R_wc"][p["first"]] @ p["t_21"] for p in g["pairs"]])
    sc = dict(F=g["F"], P=g["P"], n_cameras=g["F"], first=np.array([p["first"] for p in g["pairs"]], np.int32), second=np.array([p["second"] for p in g["pairs"]], np.int32),
              dir=obs / np.linalg.norm(obs, axis=1)[:, None], s0=np.array([hand["scale0"][k] for k in range(g["P"])]))
    ref = br.bata_ref(sc)
    assert ref["knife"] == []
    t_cw = np.array([-g["R_wc"][i].T @ ref["centres"][i] for i in range(g["F"])])
    assert np.abs(t_cw - np.array([hand["t"][i] for i in range(g["F"])])).max() <= br.TOL["centres"]


def test_mirror_method_5_needs_the_flag():
    g = br.mirror_graph()
    est = br.run_driver(g, "estimate", "host", method=5, seed=7, init_dlt=0, enable_bata=0)
    assert est["ok"] == 0 and est["message"] == "Translaton average method not supported"
    for method in (2, 3, 6):
        est = br.run_driver(g, "estimate", "host", method=method, seed=7, init_dlt=0, enable_bata=1)
        assert est["ok"] == 0 and est["message"] == "Translaton average method not supported", method


def test_mirror_seed_moves_only_the_unscaled_start():
    g = br.mirror_graph()
    a = br.run_driver(g, "bata", "host", seed=7); b = br.run_driver(g, "bata", "host", seed=8); c = br.run_driver(g, "bata", "host", seed=7)
    free = [k for k, p in enumerate(g["pairs"]) if abs(np.linalg.norm(p["t_21"]) - 1.0) < 1e-12]
    assert len(free) == 3
    for k, p in enumerate(g["pairs"]):
        if k in free:
            assert a["scale0"][k] != b["scale0"][k] and 0 < a["scale0"][k] <= 1 and 0 < b["scale0"][k] <= 1
        else:
            assert a["scale0"][k] == b["scale0"][k] and abs(a["scale0"][k] - np.linalg.norm(p["t_21"])) <= 1e-14 * a["scale0"][k]
    assert a["scale0"] == c["scale0"] and all(np.array_equal(a["t"][i], c["t"][i]) for i in a["t"])


def test_mirror_failure_text():
    """a pair list whose BATA system is not positive definite cannot pass LargestBiconnectedGraph; the text is reached through a relative translation of zero length"""
    g = br.mirror_graph()
    g["pairs"][4]["t_21"] = np.zeros(3)
    est = br.run_driver(g, "estimate", "host", method=5, seed=7, init_dlt=0, enable_bata=1)
    assert est["ok"] == 0 and est["message"] == "Translation average BATA failed"
