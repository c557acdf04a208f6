"""CPU checks of K47 (TranslationAveragingL1): the host compile of panovlm_amd/csrc/pvlm_translp_core.h (tests/cpp/translp_core_check.cpp) against the certificate
that needs no reference, against HiGHS on the literal transcription of tests/translp_ref.py, the admission rule of every scene, the gauge, the argument checks, and
the host mirror's TranslationAveragingL1 / EstimateGlobalTranslation on the host route.  No GPU."""
import subprocess

import numpy as np
import pytest

from tests import transavg_ref as tr
from tests import translp_ref as lp

NAMES = list(lp.SCENE_LIST.keys())


def test_group_size():
    assert lp.host_group_size() == lp.G


def test_scene_shapes():
    """what the scene list claims about itself"""
    S = lp.scenes()
    assert all(sc["F"] <= 40 and len(sc["triplets"]) <= 400 for sc in S.values())
    assert len(S["one-triplet"]["triplets"]) == 1 and len(S["K4"]["triplets"]) == 4
    assert np.all(np.bincount(S["K4"]["triplet_pairs"].reshape(-1)) == 2)
    for name, degree in (("hub-G-1", lp.G - 1), ("hub-G", lp.G), ("hub-G+1", lp.G + 1), ("hub-3G", 3 * lp.G)):
        assert np.sum(S[name]["triplets"] == 0) == degree
    assert np.bincount(S["book"]["triplet_pairs"].reshape(-1))[0] == lp.G + 3
    assert lp.n_loose(S["loose"]) == 2 and lp.n_components(S["two-components"]) == 2 and sorted(lp.pinned_cameras(S["two-components"])) == [0, 4]
    assert S["origin-5"]["origin"] == 5
    assert np.allclose(np.linalg.norm(S["unit"]["t_21"], axis=1), 1.0) and np.linalg.norm(S["metric"]["t_21"], axis=1).max() > 3.0


@pytest.mark.parametrize("name", NAMES)
def test_admitted(name):
    """no knife-edge stop: the list in translp_ref.SCENE_LIST is the list that runs, and every scene of it converges with its last gap below half the tolerance and
    the one before above twice"""
    h = lp.host(name)
    assert h["rc"] == 0 and h["termination"] == 0 and h["bumps"] == 0
    assert lp.admitted(h), h["gaps"][-2:]


@pytest.mark.parametrize("name", NAMES)
def test_certificate(name):
    sc, h = lp.scenes()[name], lp.host(name)
    lp.check_certificate(sc, h["translations"], h["gamma"], h["duals"], h["lam"])
    # and with the lambdas a caller of the C ABI has to find for itself
    lp.check_certificate(sc, h["translations"], h["gamma"], h["duals"])
    assert abs(h["dual_objective"] - lp.certificate(sc, h["translations"], h["gamma"], h["duals"], h["lam"])["dual_objective"]) <= 1e-12 * max(1.0, h["gamma"])


@pytest.mark.parametrize("name", NAMES)
def test_gamma_against_highs(name):
    """assertion 2: gamma against HiGHS on the literal programme"""
    h, r = lp.host(name), lp.reference(name)
    assert r["status"] == 0
    if name in lp.ZERO_GAMMA:
        print("gamma", h["gamma"], "HiGHS", r["gamma"])
        assert r["gamma"] <= 1e-7 and 0.0 <= h["gamma"] <= 2 * lp.GAP_TOL
        return
    rel = abs(h["gamma"] - r["gamma"]) / r["gamma"]
    print("gamma", h["gamma"], "HiGHS", r["gamma"], "relative", rel)
    assert rel <= lp.MEASURED["gamma"]


def test_measured_is_the_maximum():
    worst = max(abs(lp.host(n)["gamma"] - lp.reference(n)["gamma"]) / lp.reference(n)["gamma"] for n in NAMES if n not in lp.ZERO_GAMMA)
    print("largest relative difference of gamma", worst)
    assert 0.5 * lp.MEASURED["gamma"] <= worst <= lp.MEASURED["gamma"] < 1e-7
    assert lp.TOL["gamma"] == 10 * lp.MEASURED["gamma"]


@pytest.mark.parametrize("name", NAMES)
def test_gauge(name):
    sc, h = lp.scenes()[name], lp.host(name)
    assert (h["n_components"], h["n_loose"]) == (lp.n_components(sc), lp.n_loose(sc))
    used = np.zeros(sc["F"], bool); used[sc["triplets"].reshape(-1)] = True
    assert np.all(h["translations"][~used] == 0.0) and np.all(h["translations"][lp.pinned_cameras(sc)] == 0.0)
    free = used.copy(); free[lp.pinned_cameras(sc)] = False
    assert np.all(np.any(h["translations"][free] != 0.0, axis=1))


def test_two_components_gamma_is_the_larger():
    """the components share gamma alone: the optimum is the larger of the two components' own"""
    sc = lp.scenes()["two-components"]
    own = []
    for cams in ((0, 1, 2, 3), (4, 5, 6, 7)):
        keep = [p for p in range(sc["P"]) if sc["first"][p] in cams and sc["second"][p] in cams]
        sub = lp.with_triplets(dict(F=8, P=len(keep), first=sc["first"][keep], second=sc["second"][keep], R_21=sc["R_21"][keep], t_21=sc["t_21"][keep], origin=cams[0]))
        own.append(lp.lp_ref(sub)["gamma"])
    g = lp.host("two-components")["gamma"]
    print("components", own, "together", g)
    assert min(own) < 0.9 * max(own) and abs(g - max(own)) <= lp.MEASURED["gamma"] * max(own)


def test_lambda_bounds_active_and_not():
    sc, h = lp.scenes()["metric"], lp.host("metric")
    slack = h["lam"] - lp.lower_bounds(sc)
    print("metric: lambda - lo from", slack.min(), "to", slack.max())
    assert 0.0 <= slack.min() <= 2 * lp.FEAS_TOL
    sc, h = lp.scenes()["exact-small"], lp.host("exact-small")
    slack = h["lam"] - lp.lower_bounds(sc)
    print("exact-small: lambda - lo from", slack.min(), "to", slack.max())
    assert slack.min() > 0.1


def test_iteration_limit():
    sc = lp.scenes()["hub-G"]
    h = lp.host_l1(sc, dict(max_iterations=3))
    assert (h["rc"], h["termination"], h["iterations"]) == (0, 1, 3) and len(h["gaps"]) == 4
    assert h["gap"] > lp.GAP_TOL and np.all(h["duals"] > 0.0) and np.any(h["translations"] != 0.0)
    # the iterate is strictly feasible all the way
    c = lp.certificate(sc, h["translations"], h["gamma"], h["duals"], h["lam"])
    assert c["primal"] < 0.0 and c["bound"] < 0.0


def test_start_is_ignored():
    sc = lp.scenes()["K4"]
    t = np.arange(12.0).reshape(4, 3); t[sc["origin"]] = 0.0
    a, b = lp.host_l1(sc, dict(translations=t)), lp.host("K4")
    assert np.array_equal(a["translations"], b["translations"]) and a["gamma"] == b["gamma"]


def test_arguments_refused():
    sc = lp.scenes()["loose"]
    for what, mod in lp.bad_calls(sc):
        h = lp.host_l1(sc, mod)
        start = lp.call_arrays(sc, mod)["translations"]
        assert h["rc"] == -1, what
        assert np.array_equal(h["translations"], start, equal_nan=True) and np.all(h["duals"] == -7.0) and h["termination"] == -7, what


def test_no_triplets():
    sc = lp.with_triplets(tr.scene(1, tr.chain_pairs(6, 1), 6))
    assert len(sc["triplets"]) == 0
    t = np.ones((6, 3)); t[0] = 0.0
    h = lp.host_l1(sc, dict(translations=t))
    assert (h["rc"], h["termination"]) == (0, 6) and np.array_equal(h["translations"], t)


def test_sanitizer_main():
    """the stand-alone program of the host compile under the address and undefined-behaviour sanitizers"""
    from panovlm_amd import build
    exe = build.build_translp_check(main=True, sanitize=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout[-1500:], res.stderr[-1500:])
    assert res.returncode == 0


# ---- the host mirror -------------------------------------------------------------------------------------------------------------------------
def test_mirror_function_by_hand():
    """TranslationAveragingL1 on the host route: FindTriplet, the call, the write-back — the host compile's own result"""
    for name in ("K4", "loose", "two-components"):
        sc = lp.scenes()[name]
        o = lp.run_driver(lp.scene_graph(sc), "l1", "host")
        assert o["ok"] == 1
        assert np.array_equal(np.array([o["t"][i] for i in range(sc["F"])]), lp.host(name)["translations"])


def test_mirror_repeated_pair_resolves_to_the_last():
    sc = lp.scenes()["K4"]
    o = lp.run_driver(lp.scene_graph(sc, duplicate=(2, 5.0)), "l1", "host")
    assert o["ok"] == 1
    assert np.array_equal(np.array([o["t"][i] for i in range(sc["F"])]), lp.host("K4")["translations"])


def test_mirror_no_triplets():
    sc = tr.scene(1, tr.chain_pairs(5, 1), 5)
    o = lp.run_driver(lp.scene_graph(sc), "l1", "host")
    assert o["ok"] == 1 and all(np.all(o["t"][i] == 0.0) for i in range(5))


def test_estimate_flag_default_off():
    o = lp.run_driver(tr.mirror_scene(), "estimate", "host", enable=0)
    assert o["ok"] == 0 and o["message"] == "Translaton average method not supported"


def test_estimate_global_translation_host():
    """EstimateGlobalTranslation(2) with enable_l1 on the mirror scene: the frames it keeps, and its translations are feasible for HiGHS's optimum of the programme it
    solved"""
    g = tr.mirror_scene()
    o = lp.run_driver(g, "estimate", "host", enable=1)
    assert o["ok"] == 1 and [i for i in range(g["F"]) if o["valid"][i]] == [1, 2, 3, 4, 5, 6, 7]
    sc, t = lp.estimate_problem(g, o)
    gam, ref = lp.primal_gamma(sc, t), lp.lp_ref(sc)["gamma"]
    print("gamma of the translations", gam, "HiGHS", ref, "triplets", len(sc["triplets"]))
    assert len(sc["triplets"]) > 0 and ref > 1e-3
    assert abs(gam - ref) <= lp.TOL["gamma"] * ref + 2 * lp.FEAS_TOL
