"""CPU checks of K46: the host compile of panovlm_amd/csrc/pvlm_transdir_core.h (tests/cpp/transdir_core_check.cpp) against the independent numpy reference of
tests/transdir_ref.py (the full dense system), the knife-edge condition on every scene any K46 test uses, what the two methods have to achieve, and the host
mirror's TranslationAveragingL2Chordal / TranslationAveragingLUD / EstimateGlobalTranslation on the host compile (tests/cpp/pvlm_transdir_driver.cpp)."""
import subprocess

import numpy as np
import pytest

from tests import transavg_ref as tr
from tests import transdir_ref as td

NAMES = list(td.scenes().keys())


def _host(name):
    problem, sc, kw = td.scenes()[name]
    return td.host_solve(problem, sc, **kw)


def _error(c, sc):
    return float(np.linalg.norm(c - sc["truth"], axis=1).max())


def test_group_size():
    assert td.host_group_size() == td.G


@pytest.mark.parametrize("name", NAMES)
def test_knife_edge(name):
    """Every scene of the K46 tests, on the reference: no step quality within a factor 2 of min_relative_decrease, no termination test within a factor 2 of its
    tolerance, no scale within 1e-9 s0 of a ScaleFactor bound or a parameter bound unless it was clamped onto it, no Huber argument within 1e-9 of a^2 — at every
    evaluated point (for the scales: after the start, whose scales are the call's inputs and compared bit for bit).  A seed that fails is replaced in
    transdir_ref.SEEDS."""
    ref = td.reference(name)
    assert ref["knife"] == [], ref["knife"]


@pytest.mark.parametrize("name", NAMES)
def test_host_against_reference(name):
    """Equal accepted / rejected step counts and termination codes; centres, scales, weights, costs and sum_e within transdir_ref.TOL = ten times the largest
    difference the host compile shows against the reference over these scenes (transdir_ref.MEASURED: 2.1e-10 m in a centre, 4.7e-9 in a scale, 3.2e-9 in a weight,
    1.7e-9 in the final cost, 3.4e-9 in sum_e — the clamp scene's figures; the others stay below 3e-10).  transdir_ref.COMPARE says why the LUD scenes run 12
    iterations and the chordal scenes come without outlier pairs."""
    ref, h = td.reference(name), _host(name)
    assert h["rc"] == 0
    d = td.differences(h, ref)
    print(name, "steps", h["successful"], h["unsuccessful"], "termination", h["termination"], "differences", d)
    assert (h["successful"], h["unsuccessful"], h["termination"]) == (ref["successful"], ref["unsuccessful"], ref["termination"])
    assert h["successful"] >= 3
    assert abs(h["initial_cost"] - ref["initial_cost"]) <= td.TOL["cost"]
    for k in td.TOL:
        assert d[k] <= td.TOL[k], (k, d[k], td.TOL[k])


def test_measured_is_the_maximum():
    """transdir_ref.MEASURED is what it says: the largest difference over the scenes, each figure within its own last digit"""
    worst = {k: 0.0 for k in td.TOL}
    for name in NAMES:
        d = td.differences(_host(name), td.reference(name))
        worst = {k: max(worst[k], d[k]) for k in worst}
    print("largest differences host compile - reference:", worst)
    for k in worst:
        assert worst[k] <= td.MEASURED[k], (k, worst[k])


def test_chordal_ends_closer():
    """the issue's trial (20 cameras in an 8 m box, 70 pairs, 2 degrees of direction noise, a start 0.3 m per coordinate off the truth) at the default 300
    iterations: after the least-squares scale fit — the cost does not see the scale — the result is closer to the truth than the start was"""
    problem, sc, kw = td.scenes()["chordal-trial"]
    for r in (td.reference("chordal-trial"), _host("chordal-trial")):
        e0, e1 = _error(td.scale_fit(sc["start"], sc["truth"]), sc), _error(td.scale_fit(r["centres"], sc["truth"]), sc)
        print("largest centre error after the scale fit: start %.3f m, end %.3f m, ratio %.3f; steps %d + %d" % (e0, e1, e1 / e0, r["successful"], r["unsuccessful"]))
        assert e1 < e0
        assert r["termination"] == 1


def test_lud_irls_ends_closer():
    """the trial's graph with 15 % outlier pairs, three LUD solves at the default 50 iterations with the weights fed back: every solve of the reference passes the
    knife-edge condition, and both the reference and the host compile end closer to the truth than they started (values are not compared: transdir_ref.COMPARE)"""
    sc = td.irls_scene()
    refs, hs = td.irls_reference(), td.host_irls(sc, 3)
    for r in refs:
        assert r["knife"] == [], r["knife"]
    e0 = _error(sc["start"], sc)
    for what, rs in (("reference", refs), ("host compile", hs)):
        e = [_error(r["centres"], sc) for r in rs]
        print(what, "largest centre error: start %.3f m, after the solves" % e0, ["%.3f" % v for v in e], "ratio %.3f" % (e[-1] / e0), "steps",
              [(r["successful"], r["unsuccessful"]) for r in rs], "sum_e", ["%.2f" % r["sum_e"] for r in rs])
        assert e[-1] < e0


@pytest.mark.parametrize("problem", ["chordal", "lud"])
def test_zero_iterations(problem):
    problem, sc, kw = td.scenes()[problem + "-P63"]
    h = td.host_solve(problem, sc, **dict(kw, max_num_iterations=0))
    assert np.array_equal(h["centres"], sc["start"]) and h["initial_cost"] == h["final_cost"]
    assert (h["successful"], h["unsuccessful"], h["termination"]) == (0, 0, 0)
    if problem == "lud":
        assert np.array_equal(h["scales"], sc["scales"])
        e = np.linalg.norm(sc["start"][sc["first"]] - sc["start"][sc["second"]] - sc["scales"][:, None] * sc["dir"], axis=1)
        assert np.allclose(h["weight"], (e + 1e-2) ** -0.5, rtol=1e-13, atol=0) and abs(h["sum_e"] - e.sum()) <= 1e-12 * e.sum()


def test_zero_error_pair_is_finite():
    """|e| == 0 at the linearisation point (c1 = (1, 0, 0), c2 = 0, dir = (1, 0, 0), s = 1): the pair is a zero row, the result is finite (upstream's Jet gives a
    derivative that is not finite there and Ceres fails the solve: the stated divergence)"""
    sc = dict(F=2, P=1, first=np.array([0], np.int32), second=np.array([1], np.int32), dir=np.array([[1.0, 0, 0]]), scales=np.array([1.0]), origin=1,
              start=np.array([[1.0, 0, 0], [0, 0, 0]]))
    h, ref = td.host_solve("lud", sc), td.solve_ref("lud", sc)
    assert h["rc"] == 0 and np.isfinite(h["centres"]).all() and np.isfinite(h["scales"]).all() and np.isfinite([h["initial_cost"], h["final_cost"], h["sum_e"]]).all()
    assert (h["successful"], h["unsuccessful"], h["termination"]) == (ref["successful"], ref["unsuccessful"], ref["termination"]) == (0, 0, 2)
    assert np.array_equal(h["centres"], sc["start"]) and h["scales"][0] == 1.0 and h["sum_e"] == 0.0 and h["weight"][0] == 1e-2 ** -0.5
    # the same pair inside a triangle whose other pairs are off: the zero row does not stop the others
    tri = dict(F=3, P=3, first=np.array([0, 1, 0], np.int32), second=np.array([1, 2, 2], np.int32), scales=np.array([1.0, 1.5, 2.0]), origin=1,
               dir=np.array([[1.0, 0, 0], [0, 1.0, 0], [0.6, 0.8, 0]]), start=np.array([[1.0, 0, 0], [0, 0, 0], [0.3, -1.2, 0.4]]))
    h = td.host_solve("lud", tri)
    assert h["rc"] == 0 and np.isfinite(h["centres"]).all() and np.isfinite(h["scales"]).all() and h["successful"] >= 1 and h["final_cost"] < h["initial_cost"]


def test_chordal_coincident_cameras():
    """two cameras on one point at the start: the cost is not finite, termination 5, the centres come back as they went in"""
    problem, sc, kw = td.scenes()["chordal-P3"]
    c0 = sc["start"].copy(); c0[sc["first"][1]] = c0[sc["second"][1]]
    h, ref = td.host_solve("chordal", sc, c0), td.solve_ref("chordal", sc, c0)
    assert h["rc"] == 0 and h["termination"] == ref["termination"] == 5 and (h["successful"], h["unsuccessful"]) == (0, 0)
    assert not np.isfinite(h["initial_cost"]) and np.array_equal(h["centres"].view(np.uint64), c0.view(np.uint64))


def test_clamped_scales():
    """a scaled pair whose length is wrong tenfold each way ends exactly on its parameter bounds 3 s0 and 0.5 s0"""
    problem, sc, kw = td.scenes()["lud-clamp"]
    h = _host("lud-clamp")
    assert h["scales"][4] == 3.0 * sc["scales"][4] and h["scales"][9] == 0.5 * sc["scales"][9]


@pytest.mark.parametrize("name", ["lud-unscaled", "lud-P257", "lud-hub17"])
def test_unscaled_pairs_stay_at_or_above_one(name):
    """a pair that comes in with scale 1 has the parameter lower bound 1 (:578) — K42's has none — and some end exactly on it"""
    problem, sc, kw = td.scenes()[name]
    h = _host(name)
    free = sc["scales"] == 1
    assert free.any() and np.all(h["scales"][free] >= 1.0)
    print(name, "unscaled pairs", int(free.sum()), "on the bound", int((h["scales"][free] == 1.0).sum()), "smallest", h["scales"][free].min())
    if name == "lud-unscaled":
        # one metre is below every distance of the scene but a few: the pairs of close cameras are held on the bound
        short = np.linalg.norm(sc["truth"][sc["first"]] - sc["truth"][sc["second"]], axis=1) < 0.9
        assert np.all(h["scales"][free & short] == 1.0)


def test_weights_as_written():
    """the weight w_p is applied (cost 0.5 w^2 |e| per pair at the start), and weight_out = (|e| + 1e-2)^-0.5, sum_e = sum |e| on dir"""
    problem, sc, kw = td.scenes()["lud-scaled"]
    w = 0.5 + np.arange(sc["P"]) % 3
    h = td.host_solve("lud", sc, weight=w, **kw)
    e0 = np.linalg.norm(sc["start"][sc["first"]] - sc["start"][sc["second"]] - sc["scales"][:, None] * sc["dir"], axis=1)
    assert abs(h["initial_cost"] - 0.5 * (w * w * e0).sum()) <= 1e-12 * h["initial_cost"]
    assert h["initial_cost"] != _host("lud-scaled")["initial_cost"]
    e = np.linalg.norm(h["centres"][sc["first"]] - h["centres"][sc["second"]] - h["scales"][:, None] * sc["dir"], axis=1)
    assert np.allclose(h["weight"], (e + 1e-2) ** -0.5, rtol=1e-13, atol=0) and abs(h["sum_e"] - e.sum()) <= 1e-12 * e.sum()
    ref = td.solve_ref("lud", sc, weight=w, **kw)
    assert (h["successful"], h["unsuccessful"]) == (ref["successful"], ref["unsuccessful"]) and np.abs(h["centres"] - ref["centres"]).max() <= td.TOL["c"]


def test_arguments_refused():
    problem, sc, kw = td.scenes()["lud-P3"]
    for name, bad, lud_only in td.bad_calls(sc):
        for problem in ("lud",) if lud_only else ("chordal", "lud"):
            h = td.host_solve(problem, bad, weight=bad.get("weight"), max_num_iterations=bad.get("max_num_iterations", 5))
            assert h["rc"] == -1, (name, problem)
            assert np.array_equal(h["centres"].view(np.uint64), np.asarray(bad["start"], np.float64).view(np.uint64)) and h["initial_cost"] == -7.0, (name, problem)
            if problem == "lud":
                assert np.array_equal(h["scales"].view(np.uint64), np.asarray(bad["scales"], np.float64).view(np.uint64)) and h["sum_e"] == -7.0, name
                assert np.array_equal(h["weight"], np.ones(sc["P"]) if bad.get("weight") is None else bad["weight"]), name


def test_no_pairs():
    sc = dict(F=2, P=0, first=np.zeros(0, np.int32), second=np.zeros(0, np.int32), dir=np.zeros((0, 3)), scales=np.zeros(0), origin=1, start=np.array([[1.0, 2, 3], [0, 0, 0]]))
    for problem in ("chordal", "lud"):
        h = td.host_solve(problem, sc)
        assert h["rc"] == 0 and h["termination"] == 6 and np.array_equal(h["centres"], sc["start"]) and (h["initial_cost"], h["final_cost"]) == (0, 0)
    assert h["sum_e"] == -7.0


def test_sanitizer_main():
    """tests/cpp/transdir_core_check.cpp with its own main under -fsanitize=address,undefined (1, 3, 9, 70 and 300 cameras, both problems)"""
    from panovlm_amd import build
    out = subprocess.run([build.build_transdir_check(main=True, sanitize=True)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------------
def test_estimate_global_translation_host():
    """EstimateGlobalTranslation on transavg_ref.mirror_scene() with methods 3 and 6 under their flags returns ok, with the frames and pairs method 1 keeps; the
    scene is noise-free, so the chordal result is the truth in frame 1's gauge up to one common factor (its scale is a gauge).  LUD is held to a finite result
    only: the scene's two unscaled pairs pay 0.5 (s - 2)^2 for every metre past two (ScaleFactor(2, 1), :576) and pull their cameras 0.7 m off — upstream's
    formulation, printed here."""
    g = tr.mirror_scene()
    base = tr.run_driver(g, "estimate", "host", method=1)
    for method in (3, 6):
        out = td.run_driver(g, "estimate", "host", method=method)
        assert out["ok"] == 1, out["message"]
        assert out["pairs"] == base["pairs"] and out["valid"] == base["valid"]
        assert np.all(out["t_wc"][1] == 0.0)
        ids = [i for i in range(g["F"]) if out["valid"][i]]
        got = np.array([out["t_wc"][i] for i in ids]); truth = np.array([g["R_wc"][1].T @ (g["centres"][i] - g["centres"][1]) for i in ids])
        alpha = float((got * truth).sum() / (truth * truth).sum())
        print("method", method, "common factor %.4f, largest deviation %.3e m" % (alpha, np.abs(got - alpha * truth).max()))
        assert np.isfinite(got).all()
        if method == 3:
            assert np.abs(got - alpha * truth).max() <= 0.01 * g["size"]


def test_estimate_lud_graph_is_well_conditioned():
    """the admission of transdir_ref.lud_estimate_graph(), on which tests/test_transdir_gpu.py compares method 6's two routes by value: one ulp of one t_21 moves
    the host route's result by less than MEASURED["c"] (on mirror_scene() the same change moves it by 6e-6 m: printed)"""
    def moved(g):
        a = td.run_driver(g, "estimate", "host", method=6)
        g["pairs"][1]["t_21"][0] = np.nextafter(g["pairs"][1]["t_21"][0], 9.0)
        b = td.run_driver(g, "estimate", "host", method=6)
        assert a["ok"] == 1 and b["ok"] == 1 and a["valid"] == b["valid"]
        return max(np.abs(a["t_wc"][i] - b["t_wc"][i]).max() for i in range(g["F"]) if a["valid"][i])
    got, mirror = moved(td.lud_estimate_graph()), moved(tr.mirror_scene())
    print("one ulp of one t_21 moves method 6 by %.3e m on the admitted graph, by %.3e m on mirror_scene()" % (got, mirror))
    assert got <= td.MEASURED["c"]


def test_estimate_flags_default_off():
    """without their flags methods 3 and 6 keep upstream's refusal (tests/test_transavg_cpu.py::test_estimate_methods_not_built pins the same through K42's driver)"""
    g = tr.mirror_scene()
    for method in (3, 6):
        out = tr.run_driver(g, "estimate", "host", method=method)
        assert out["ok"] == 0 and out["message"] == "Translaton average method not supported"


def test_mirror_functions_by_hand():
    """TranslationAveragingL2Chordal and TranslationAveragingLUD from the DLT start, the frames as cameras: t_cw comes back finite with camera 0 at zero"""
    g = tr.irls_scene(size=8.0)
    for mode in ("chordal", "lud"):
        out = td.run_driver(g, mode, "host", num_iteration=2)
        t = np.array([out["t"][i] for i in range(g["F"])])
        assert out["ok"] == 1 and out["n_pairs"] == g["P"] and np.isfinite(t).all() and np.all(t[0] == 0.0)


def test_lud_stop_rule():
    """TranslationAveragingLUD: sum |e| < 10 stops after the first solve (:628); on a scene a thousand times larger the first sum is above 10 and the loop goes on
    until the sum moves by less than 5 % or num_iteration is reached.  The drop of pairs with a negative scale (:635-651) is built as written, but no input reaches
    it: every scale is held at or above 0.5 s0 or 1 by its parameter bound.  Asserted here: nothing is dropped."""
    sc = tr.scene(9, tr.chain_pairs(12, 3), 12, noise_deg=1.0, size=2.0)        # 30 scaled pairs a metre long, a degree off: the sum is well below 10
    small = dict(F=12, R_wc=np.array([r.T for r in sc["R_cw"]]), t_wc=np.full((12, 3), np.inf), P=sc["P"],
                 pairs=[dict(first=int(sc["first"][p]), second=int(sc["second"][p]), R_21=sc["R_21"][p], t_21=sc["t_21"][p], upper=0.0, lower=0.0) for p in range(sc["P"])])
    out = td.run_driver(small, "lud", "host", num_iteration=5)
    assert out["ok"] == 1 and out["iterations"] == 1 and out["n_pairs"] == small["P"]
    big = tr.irls_scene(size=8000.0)
    out = td.run_driver(big, "lud", "host", num_iteration=4)
    print("solves", out["iterations"])
    assert out["ok"] == 1 and 2 <= out["iterations"] <= 4 and out["n_pairs"] == big["P"]
    one = td.run_driver(big, "lud", "host", num_iteration=1)
    assert one["iterations"] == 1
