"""GPU checks of K47 through the C ABI: pvlm_transavg_l1 on every scene of tests/translp_ref.py — the certificate that needs no reference, the host compile of the
same core (tests/cpp/translp_core_check.cpp) with equal iteration counts (every scene was admitted on the CPU as no knife-edge stop) and gamma within
translp_ref.TOL, every scene again with the grids held to one workgroup, bit-reproducibility, the argument checks, and EstimateGlobalTranslation(2) through the
device against its host-compile route.  Translation differences between device and host compile are printed, not asserted: the optimum is a face (see pvlm.h)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import transavg_ref as tr
from tests import translp_ref as lp

pytestmark = pytest.mark.gpu

NAMES = list(lp.SCENE_LIST.keys())
ERR_ARG = -1      # pvlm_status PVLM_ERR_ARG
SUMMARY = ("gamma", "dual_objective", "gap", "primal_residual", "dual_residual", "iterations", "bumps", "n_components", "n_loose", "termination")


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _gpu(ctx, sc, mod=None, check=True, want_duals=True):
    from panovlm_amd import api
    a = lp.call_arrays(sc, mod)
    g = api.transavg_l1(ctx, a["first"], a["second"], a["R_21"], a["t_21"], a["triplet_pairs"], a["origin"], a["translations"], a["max_iterations"], a["gap_tol"],
                        a["feas_tol"], want_duals=want_duals, check=check)
    assert g["guard_intact"]
    return g


def _held(ctx, sc, **kw):
    os.environ["PVLM_TRANSLP_MAX_BLOCKS"] = "1"
    try:
        return _gpu(ctx, sc, **kw)
    finally:
        del os.environ["PVLM_TRANSLP_MAX_BLOCKS"]


def _against_host(g, h, scale=None):
    """assertion 3.  scale: what the tolerance of gamma is relative to — gamma itself, or 1 for a scene whose gamma* is zero (the scale of the stop rule)"""
    print("device", [g[k] for k in SUMMARY], "host", [h[k] for k in SUMMARY], "largest translation difference", float(np.abs(g["translations"] - h["translations"]).max()))
    assert (g["rc"], h["rc"]) == (0, 0)
    for k in ("termination", "n_components", "n_loose", "bumps", "iterations"):
        assert g[k] == h[k], k
    assert abs(g["gamma"] - h["gamma"]) <= lp.TOL["gamma"] * (abs(h["gamma"]) if scale is None else scale)


def _same_bits(a, b):
    assert np.array_equal(_bits(a["translations"]), _bits(b["translations"])) and np.array_equal(_bits(a["duals"]), _bits(b["duals"]))
    for k in SUMMARY:
        assert a[k] == b[k], k


def test_group_size(ctx):
    from panovlm_amd import api
    assert api.translp_group_size() == lp.G == lp.host_group_size()


@pytest.mark.parametrize("name", NAMES)
def test_scene(ctx, name):
    """one triplet; K4; a pair and cameras in no triplet; two components and their two pins; a hub in G - 1, G, G + 1 and 3 G triplets; a pair in G + 3; lambda bounds
    active and none active (gamma* = 0); unit and metric t_21; outlier pairs; an origin that is not camera 0; 360 triplets on 40 cameras"""
    sc = lp.scenes()[name]
    g = _gpu(ctx, sc)
    assert g["termination"] == 0
    lp.check_certificate(sc, g["translations"], g["gamma"], g["duals"])
    _against_host(g, lp.host(name), 1.0 if name in lp.ZERO_GAMMA else None)
    assert abs(g["dual_objective"] - lp.certificate(sc, g["translations"], g["gamma"], g["duals"])["dual_objective"]) <= 1e-12 * max(1.0, g["gamma"])


@pytest.mark.parametrize("name", NAMES)
def test_scene_one_workgroup(ctx, name):
    """every scene with PVLM_TRANSLP_MAX_BLOCKS=1: the gathers stride past 32 rows (cameras, pairs), the per-triplet kernels past 256 triplets (F40), the update
    past 256 rows.  The same bits as the unrestricted call, which is itself the same from run to run (assertion 4)."""
    sc = lp.scenes()[name]
    free, again, held = _gpu(ctx, sc), _gpu(ctx, sc), _held(ctx, sc)
    _against_host(held, lp.host(name), 1.0 if name in lp.ZERO_GAMMA else None)
    _same_bits(free, again)
    _same_bits(held, free)


def test_duals_are_optional(ctx):
    sc = lp.scenes()["hub-G+1"]
    a, b = _gpu(ctx, sc), _gpu(ctx, sc, want_duals=False)
    assert b["duals"] is None and np.array_equal(_bits(a["translations"]), _bits(b["translations"])) and a["gamma"] == b["gamma"]


def test_iteration_limit(ctx):
    sc = lp.scenes()["hub-G"]
    g = _gpu(ctx, sc, dict(max_iterations=3))
    assert (g["termination"], g["iterations"]) == (1, 3) and np.all(g["duals"] > 0.0) and np.any(g["translations"] != 0.0)
    _against_host(g, lp.host_l1(sc, dict(max_iterations=3)))


def test_no_triplets(ctx):
    """termination 6 touches nothing but the summary"""
    sc = lp.with_triplets(tr.scene(1, tr.chain_pairs(6, 1), 6))
    t = np.ones((6, 3)); t[0] = 0.0
    g = _gpu(ctx, sc, dict(translations=t))
    assert (g["rc"], g["termination"], g["iterations"]) == (0, 6, 0) and np.array_equal(g["translations"], t) and g["duals"].size == 0


def test_arguments_refused(ctx):
    """assertion 5: every PVLM_ERR_ARG case leaves the outputs and their guard words as they were"""
    from panovlm_amd import api
    sc = lp.scenes()["loose"]
    for what, mod in lp.bad_calls(sc):
        g = _gpu(ctx, sc, mod, check=False)
        start = lp.call_arrays(sc, mod)["translations"]
        assert g["rc"] == ERR_ARG, what
        assert np.array_equal(g["translations"], start, equal_nan=True) and np.all(g["duals"] == -7.0) and g["termination"] == -7 and g["gamma"] == -7.0, what
    a = lp.call_arrays(sc)
    T, P, F = len(a["triplet_pairs"]), len(a["first"]), a["F"]
    t = np.zeros((F, 3)); duals = np.full((T, 19), -7.0)
    prm = api.TranslpParams(60, 1e-9, 1e-9); sm = api.TranslpSummary(-7.0, -7.0, -7.0, -7.0, -7.0, -7, -7, -7, -7, -7)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    full = [ctx._h, C.c_int(F), C.c_int(P), ptr(a["first"]), ptr(a["second"]), ptr(a["R_21"]), ptr(a["t_21"]), C.c_int(T), ptr(a["triplet_pairs"]), C.c_int(a["origin"]), ptr(t),
            ptr(duals), C.byref(prm), C.byref(sm)]
    for k in (0, 3, 4, 5, 6, 8, 10, 12, 13):
        args = list(full); args[k] = None
        assert ctx.lib.pvlm_transavg_l1(*args) == ERR_ARG, k
        assert np.all(t == 0.0) and np.all(duals == -7.0) and sm.termination == -7
    assert ctx.lib.pvlm_transavg_l1(*full) == 0 and sm.termination == 0


def test_estimate_global_translation_device(ctx):
    """assertion 6: EstimateGlobalTranslation(2) with enable_l1 through the device and through the host compile — ok, the same frames and pairs kept, gamma of the
    translations (max |e| at each triplet's best lambda) equal within TOL between the routes and against HiGHS on the programme that was solved; without the flag
    today's refusal"""
    g = tr.mirror_scene()
    d, h = lp.run_driver(g, "estimate", "device", enable=1), lp.run_driver(g, "estimate", "host", enable=1)
    assert d["ok"] == 1 and h["ok"] == 1 and d["valid"] == h["valid"] and d["pairs"] == h["pairs"]
    (sc, td), (_, th) = lp.estimate_problem(g, d), lp.estimate_problem(g, h)
    gd, gh, ref = lp.primal_gamma(sc, td), lp.primal_gamma(sc, th), lp.lp_ref(sc)["gamma"]
    print("gamma device", gd, "host", gh, "HiGHS", ref, "largest translation difference", float(np.abs(td - th).max()))
    assert abs(gd - gh) <= lp.TOL["gamma"] * gh + 2 * lp.FEAS_TOL
    assert abs(gd - ref) <= lp.TOL["gamma"] * ref + 2 * lp.FEAS_TOL
    off = lp.run_driver(g, "estimate", "device", enable=0)
    assert off["ok"] == 0 and off["message"] == "Translaton average method not supported"


def test_mirror_function_device(ctx):
    sc = lp.scenes()["two-components"]
    o = lp.run_driver(lp.scene_graph(sc, duplicate=(3, 4.0)), "l1", "device")
    assert o["ok"] == 1
    t = np.array([o["t"][i] for i in range(sc["F"])])
    gam = lp.primal_gamma(sc, t)
    assert abs(gam - lp.host("two-components")["gamma"]) <= lp.TOL["gamma"] * gam + 2 * lp.FEAS_TOL
