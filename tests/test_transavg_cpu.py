"""CPU checks of K42: the host compile of panovlm_amd/csrc/pvlm_transavg_core.h (tests/cpp/transavg_core_check.cpp) against the independent numpy reference of
tests/transavg_ref.py (the unreduced dense system), the knife-edge condition on every scene any K42 test uses, what the averaging has to achieve, the DLT against
numpy.linalg.lstsq, and the host mirror's EstimateGlobalTranslation / TranslationAveragingL2IRLS on the host compile (tests/cpp/pvlm_transavg_driver.cpp)."""
import subprocess

import numpy as np
import pytest

from tests import transavg_ref as tr

NAMES = list(tr.scenes().keys())


def _host(name):
    sc, kw = tr.scenes()[name]
    return tr.host_solve(sc, tr.dlt_start(sc), **kw)


def test_group_size():
    assert tr.host_group_size() == tr.G


@pytest.mark.parametrize("name", NAMES)
def test_knife_edge(name):
    """Every scene of the K42 tests, on the reference: no step quality within a factor 2 of min_relative_decrease, no termination test within a factor 2 of its
    tolerance, no scale within 1e-9 s0 of a ScaleFactor bound or a parameter bound unless it was clamped onto it — at every evaluated point after the start (the
    start's scales are the call's inputs: both sides compare the same bits there, nothing is rounded).  A seed that fails is replaced in transavg_ref.SEEDS."""
    ref = tr.reference(name)
    assert ref["knife"] == [], ref["knife"]


@pytest.mark.parametrize("name", NAMES)
def test_host_against_reference(name):
    """Equal accepted / rejected step counts and termination codes; translations, scales, weights and costs within transavg_ref.TOL = ten times the largest
    difference the host compile shows against the reference over these scenes (transavg_ref.MEASURED: 7.6e-12 m in a translation, 9.2e-12 in a scale, 2.2e-12 in
    a weight, 2.4e-15 in the final cost; so the tolerances are 7.6e-11, 9.2e-11, 2.2e-11 and 2.4e-14)."""
    ref, h = tr.reference(name), _host(name)
    assert h["rc"] == 0
    d = tr.differences(h, ref)
    print(name, "steps", h["successful"], h["unsuccessful"], "termination", h["termination"], "differences", d)
    assert (h["successful"], h["unsuccessful"], h["termination"]) == (ref["successful"], ref["unsuccessful"], ref["termination"])
    assert abs(h["initial_cost"] - ref["initial_cost"]) <= tr.TOL["cost"]
    for k in tr.TOL:
        assert d[k] <= tr.TOL[k], (k, d[k], tr.TOL[k])


def test_measured_is_the_maximum():
    """transavg_ref.MEASURED is what it says: the largest difference over the scenes, each figure within its own last digit"""
    worst = {k: 0.0 for k in tr.TOL}
    for name in NAMES:
        d = tr.differences(_host(name), tr.reference(name))
        worst = {k: max(worst[k], d[k]) for k in worst}
    print("largest differences host compile - reference:", worst)
    for k in worst:
        assert worst[k] <= tr.MEASURED[k], (k, worst[k])


def test_noise_free_stays_at_the_truth():
    sc, kw = tr.scenes()["exact"]
    h = _host("exact")
    assert np.abs(tr.dlt_start(sc) - sc["truth"]).max() <= 1e-10 * sc["size"]
    assert np.abs(h["translations"] - sc["truth"]).max() <= 1e-10 * sc["size"]
    assert h["final_cost"] <= 1e-20 and h["initial_cost"] == h["final_cost"]


def test_outliers_end_ten_times_closer():
    """15 % outlier pairs: the DLT start is metres off, the SoftL1 solve ends at least ten times closer to the truth"""
    sc, kw = tr.scenes()["outlier15"]
    h = _host("outlier15")
    e0 = np.abs(tr.dlt_start(sc) - sc["truth"]).max(); e1 = np.abs(h["translations"] - sc["truth"]).max()
    print("error of the DLT start %.3f m, after the solve %.3f m" % (e0, e1))
    assert 10 * e1 <= e0


def test_clamped_scales():
    """a scaled pair whose length is wrong tenfold each way ends exactly on its parameter bounds 3 s0 and 0.5 s0"""
    sc, kw = tr.scenes()["clamp"]
    h = _host("clamp")
    assert h["scales"][4] == 3.0 * sc["scales"][4] and h["scales"][9] == 0.5 * sc["scales"][9]


def test_weights_as_written():
    """weight = (|t2 - R t1 - s t_21| + 1e-2)^-0.5 with t_21 NOT normalised (TranslationAveraging.cpp:165)"""
    sc, kw = tr.scenes()["scaled"]
    h = _host("scaled")
    r = h["translations"][sc["second"]] - np.einsum("pij,pj->pi", sc["R_21"], h["translations"][sc["first"]]) - h["scales"][:, None] * sc["t_21"]
    assert np.allclose(h["weight"], (np.linalg.norm(r, axis=1) + 1e-2) ** -0.5, rtol=1e-13, atol=0)


def test_zero_iterations():
    sc, kw = tr.scenes()["scaled"]
    t0 = tr.dlt_start(sc)
    h = tr.host_solve(sc, t0, max_num_iterations=0)
    assert np.array_equal(h["translations"], t0) and np.array_equal(h["scales"], sc["scales"]) and h["initial_cost"] == h["final_cost"]
    assert (h["successful"], h["unsuccessful"], h["termination"]) == (0, 0, 0)


@pytest.mark.parametrize("name", ["exact", "scaled", "hub9", "F65"])
def test_dlt_against_lstsq(name):
    """The DLT (normal equations, camera 0 fixed at zero) against numpy.linalg.lstsq (the minimum-norm solution of the rank-deficient system) after SetToOrigin on
    both sides, which removes the gauge t_i = R_i c.  Tolerance: the normal equations square the condition number kappa of the system with the gauge fixed, so the two
    differ by about kappa^2 eps relative to the largest translation; 100 kappa^2 eps |t|_max, kappa computed here."""
    sc, kw = tr.scenes()[name]
    rc, info, t = tr.host_dlt(sc)
    assert rc == 0 and info == 0 and np.all(t[0] == 0.0)
    ref = tr.dlt_ref(sc)
    a = tr.set_to_origin(t, sc["R_cw"], sc["origin"]); b = tr.set_to_origin(ref, sc["R_cw"], sc["origin"])
    kappa = tr.dlt_condition(sc)
    tol = 100 * kappa ** 2 * np.finfo(np.float64).eps * np.abs(b).max()
    print(name, "kappa %.1f" % kappa, "difference %.3e" % np.abs(a - b).max(), "tolerance %.3e" % tol)
    assert np.abs(a - b).max() <= tol
    assert np.abs(t - tr.dlt_fixed_ref(sc)).max() <= tol


def test_dlt_not_connected():
    sc = tr.scene(1, [(0, 1), (1, 2), (0, 2), (3, 4)], 5)
    rc, info, t = tr.host_dlt(sc)
    assert rc == 0 and info > 0 and np.all(t == -7.0)


def test_arguments_refused():
    sc, kw = tr.scenes()["P3"]
    for name, bad in tr.bad_calls(sc):
        h = tr.host_solve(bad, bad.get("t0", np.zeros((bad["F"], 3))), max_num_iterations=bad.get("max_num_iterations", 50))
        assert h["rc"] == -1, name
        assert np.array_equal(h["scales"].view(np.uint64), np.asarray(bad["scales"], np.float64).view(np.uint64)) and np.all(h["weight"] == 1.0), name


def test_sanitizer_main():
    """tests/cpp/transavg_core_check.cpp with its own main under -fsanitize=address,undefined (1, 3, 9, 70 and 300 cameras)"""
    from panovlm_amd import build
    out = subprocess.run([build.build_transavg_check(main=True, sanitize=True)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------------
def test_estimate_global_translation_host():
    """EstimateGlobalTranslation on the host compile, on a small list with a frame without rotation, unscaled pairs, a bridge that LargestBiconnectedGraph removes
    and an origin that is not frame 0 — against the same operations done here in numpy around the host compile's DLT and solve."""
    g = tr.mirror_scene()
    out = tr.run_driver(g, "estimate", "host", method=1)
    assert out["ok"] == 1, out["message"]
    exp = tr.estimate_ref(g)
    assert exp["origin_frame"] == 1
    assert out["pairs"] == exp["pairs"]
    assert (6, 8) not in out["pairs"] and (0, 1) not in out["pairs"]
    for i in range(g["F"]):
        if i in exp["t_wc"]:
            assert out["valid"][i] == 1
            assert np.abs(out["t_wc"][i] - exp["t_wc"][i]).max() <= tr.TOL["t"], (i, out["t_wc"][i], exp["t_wc"][i])
            assert np.abs(out["R_wc"][i] - exp["R_wc"][i]).max() <= 1e-15
        else:                                    # frame 0 (behind the bridge) and frame 8 (no rotation) are not touched
            assert out["valid"][i] == 0 and np.array_equal(out["t_wc"][i], g["t_wc"][i]) and np.array_equal(out["R_wc"][i], g["R_wc"][i])
    assert np.all(out["t_wc"][1] == 0.0)
    # the truth in frame 1's gauge.  The cost does not fix the overall scale: every scale may sit anywhere between lower_scale_ratio and upper_scale_ratio times its
    # start without penalty, and the unscaled pairs' unit lengths pull the DLT start short — so the centres are compared up to one common factor inside those ratios
    got = np.array([out["t_wc"][i] for i in exp["truth_t_wc"]]); truth = np.array(list(exp["truth_t_wc"].values()))
    alpha = float((got * truth).sum() / (truth * truth).sum())
    print("common factor %.4f, largest deviation %.3e m" % (alpha, np.abs(got - alpha * truth).max()))
    assert 0.9 - 1e-3 <= alpha <= 1.3 + 1e-3
    assert np.abs(got - alpha * truth).max() <= 0.01 * g["size"]


def test_estimate_refuses_dlt_overrun():
    """sfm/SfM.cpp:1183: all pairs under the global indices into an output sized by the scaled component; frame 7 hangs on unscaled pairs only, its index does not fit"""
    g = tr.mirror_scene(frame7_scaled=False)
    out = tr.run_driver(g, "estimate", "host", method=1)
    assert out["ok"] == 0 and "1183" in out["message"]
    # with the scaled pairs only the list fits again
    out = tr.run_driver(g, "estimate", "host", method=1, use_all_pairs=0)
    assert out["ok"] == 1 and out["valid"][7] == 0 and all(7 not in p for p in out["pairs"])


def test_estimate_methods_not_built():
    g = tr.mirror_scene()
    for method in (2, 3, 5, 6, 0):
        out = tr.run_driver(g, "estimate", "host", method=method)
        assert out["ok"] == 0 and out["message"] == "Translaton average method not supported"
    assert tr.run_driver(g, "estimate", "host", method=4)["ok"] == 1


def test_l2irls_stop_rule():
    """TranslationAveragingL2IRLS: cost < 10 stops after the first solve (:443); on a scene a thousand times larger with outliers the first cost is above 10 and the
    loop goes on until the cost moves by less than 5 % or num_iteration is reached.
    The drop of pairs with a negative scale (:452-466) is built as written, but no input found reaches it through this entry: every scale starts at |t_21| or 1, a
    scaled pair is held at or above 0.5 s0 by its parameter bound, and an unscaled pair below 1 pays 0.5 (1 - s)^2 against a SoftLOneLoss(0.01) whose pull is at most
    0.01 — at convergence its scale sits near 0.99, and where the 50 iterations run out first it was still between 0.63 and 0.93 on scenes of 8 km and 80 km with a
    reversed unscaled pair (three seeds each), never negative.  Asserted here: nothing is dropped."""
    small = tr.irls_scene(size=8.0)
    out = tr.run_driver(small, "irls", "host", num_iteration=5)
    assert out["ok"] == 1 and out["iterations"] == 1 and out["n_pairs"] == small["P"]
    big = tr.irls_scene(size=8000.0)
    out = tr.run_driver(big, "irls", "host", num_iteration=4)
    print("iterations", out["iterations"])
    assert out["ok"] == 1 and 2 <= out["iterations"] <= 4 and out["n_pairs"] == big["P"]
    one = tr.run_driver(big, "irls", "host", num_iteration=1)
    assert one["iterations"] == 1
