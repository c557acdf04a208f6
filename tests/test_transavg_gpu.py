"""GPU checks of K42 through the C ABI: pvlm_transavg_solve / pvlm_transavg_dlt against the host compile of the same core (tests/cpp/transavg_core_check.cpp) with
the tolerance of tests/test_transavg_cpu.py (transavg_ref.TOL) and equal step counts and termination codes — every scene here was held to the knife-edge condition
there — bit-reproducibility, the argument checks, and EstimateGlobalTranslation through the device against its host-compile route."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import transavg_ref as tr

pytestmark = pytest.mark.gpu

NAMES = list(tr.scenes().keys())
ERR_ARG = -1      # pvlm_status PVLM_ERR_ARG


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _gpu(ctx, sc, t0, s0=None, loss_a=0.01, upper_ratio=1.3, lower_ratio=0.9, max_num_iterations=50, check=True):
    from panovlm_amd import api
    g = api.transavg_solve(ctx, sc["first"], sc["second"], sc["R_21"], sc["t_21"], sc["scales"] if s0 is None else s0, sc["origin"], t0, None, loss_a, upper_ratio,
                           lower_ratio, max_num_iterations, check=check)
    assert g["guard_intact"]
    g["successful"], g["unsuccessful"] = g["successful_steps"], g["unsuccessful_steps"]
    return g


def _against_host(g, h):
    d = tr.differences(g, h)
    print("device", g["successful"], g["unsuccessful"], g["termination"], "host", h["successful"], h["unsuccessful"], h["termination"], "differences", d)
    assert h["rc"] == 0 and g["rc"] == 0
    assert (g["successful"], g["unsuccessful"], g["termination"]) == (h["successful"], h["unsuccessful"], h["termination"])
    assert abs(g["initial_cost"] - h["initial_cost"]) <= tr.TOL["cost"]
    for k in tr.TOL:
        assert d[k] <= tr.TOL[k], (k, d[k], tr.TOL[k])


def test_group_size(ctx):
    from panovlm_amd import api
    assert api.transavg_group_size() == tr.G == tr.host_group_size()


@pytest.mark.parametrize("name", NAMES)
def test_scene_against_host(ctx, name):
    """pairs 3, 63, 64, 65, 4 * 64 + 1; cameras 3, 64, 65; a hub of degree G - 1, G, G + 1, 2 G + 1; the origin first, in the middle and last; lists that are not
    sorted, with first > second and with a repeated pair; all-scaled, all-unscaled and mixed; scales clamped at 3 s0 and 0.5 s0; no loss; Room's ratios"""
    sc, kw = tr.scenes()[name]
    t0 = tr.dlt_start(sc)
    g = _gpu(ctx, sc, t0, **kw)
    _against_host(g, tr.host_solve(sc, t0, **kw))
    if name == "clamp":
        assert g["scales"][4] == 3.0 * sc["scales"][4] and g["scales"][9] == 0.5 * sc["scales"][9]


def test_past_a_grid_stride_trip(ctx):
    """257 pairs with the per-pair kernels held to ONE workgroup of 256 lanes (PVLM_TRANSAVG_MAX_BLOCKS): the last pair is reached by the second trip of the stride
    loop, 90 cameras by the second and third trip of the gather's.  The same bits as the unrestricted call."""
    sc, kw = tr.scenes()["P257"]
    t0 = tr.dlt_start(sc)
    free = _gpu(ctx, sc, t0, **kw)
    os.environ["PVLM_TRANSAVG_MAX_BLOCKS"] = "1"
    try:
        held = _gpu(ctx, sc, t0, **kw)
    finally:
        del os.environ["PVLM_TRANSAVG_MAX_BLOCKS"]
    _against_host(held, tr.host_solve(sc, t0, **kw))
    for k in ("translations", "scales", "weight"):
        assert np.array_equal(_bits(held[k]), _bits(free[k])), k
    assert (held["initial_cost"], held["final_cost"]) == (free["initial_cost"], free["final_cost"])


@pytest.mark.parametrize("name", ["hub17", "F65"])
def test_two_runs_same_bits(ctx, name):
    sc, kw = tr.scenes()[name]
    t0 = tr.dlt_start(sc)
    a, b = _gpu(ctx, sc, t0, **kw), _gpu(ctx, sc, t0, **kw)
    for k in ("translations", "scales", "weight"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    for k in ("initial_cost", "final_cost", "successful", "unsuccessful", "termination"):
        assert a[k] == b[k], k


def test_zero_iterations(ctx):
    """inputs come back bit for bit, initial cost = final cost"""
    sc, kw = tr.scenes()["scaled"]
    t0 = tr.dlt_start(sc)
    g = _gpu(ctx, sc, t0, max_num_iterations=0)
    assert np.array_equal(_bits(g["translations"]), _bits(t0)) and np.array_equal(_bits(g["scales"]), _bits(sc["scales"]))
    assert g["initial_cost"] == g["final_cost"] and (g["successful"], g["unsuccessful"], g["termination"]) == (0, 0, 0)
    _against_host(g, tr.host_solve(sc, t0, max_num_iterations=0))


def test_no_pairs(ctx):
    from panovlm_amd import api
    g = api.transavg_solve(ctx, [], [], np.zeros((0, 9)), np.zeros((0, 3)), [], 1, np.array([[1.0, 2, 3], [0, 0, 0]]))
    assert g["termination"] == 6 and g["initial_cost"] == 0 and g["final_cost"] == 0 and np.array_equal(g["translations"], [[1.0, 2, 3], [0, 0, 0]]) and g["guard_intact"]


@pytest.mark.parametrize("name", ["P3", "exact", "scaled", "hub9", "F65"])
def test_dlt_against_host(ctx, name):
    """the DLT entry against the host compile; tolerance as test_transavg_cpu.py::test_dlt_against_lstsq (two Cholesky factorisations of the same normal equations)"""
    from panovlm_amd import api
    sc, kw = tr.scenes()[name]
    g = api.transavg_dlt(ctx, sc["F"], sc["first"], sc["second"], sc["R_21"], sc["t_21"])
    rc, info, h = tr.host_dlt(sc)
    tol = 100 * tr.dlt_condition(sc) ** 2 * np.finfo(np.float64).eps * np.abs(h).max()
    print(name, "difference %.3e" % np.abs(g["translations"] - h).max(), "tolerance %.3e" % tol)
    assert g["guard_intact"] and g["info"] == 0 and info == 0 and np.all(g["translations"][0] == 0.0)
    assert np.abs(g["translations"] - h).max() <= tol


def test_dlt_not_connected(ctx):
    from panovlm_amd import api
    sc = tr.scene(1, [(0, 1), (1, 2), (0, 2), (3, 4)], 5)
    g = api.transavg_dlt(ctx, sc["F"], sc["first"], sc["second"], sc["R_21"], sc["t_21"])
    assert g["rc"] == 0 and g["info"] > 0 and np.all(g["translations"] == -7.0) and g["guard_intact"]


def test_arguments_refused(ctx):
    """every PVLM_ERR_ARG case leaves the outputs untouched: the inputs come back bit for bit, the guard words stand"""
    from panovlm_amd import api
    sc, kw = tr.scenes()["P3"]
    for name, bad in tr.bad_calls(sc):
        t0 = bad.get("t0", np.zeros((bad["F"], 3)))
        g = _gpu(ctx, bad, t0, max_num_iterations=bad.get("max_num_iterations", 50), check=False)
        assert g["rc"] == ERR_ARG, name
        assert np.array_equal(_bits(g["translations"]), _bits(t0)) and np.array_equal(_bits(g["scales"]), _bits(bad["scales"])) and np.all(g["weight"] == 1.0), name
        assert g["termination"] == -7 and g["initial_cost"] == -7.0, name
        if "t0" not in bad and "max_num_iterations" not in bad and bad["origin"] == sc["origin"] and np.isfinite(bad["scales"]).all():
            d = api.transavg_dlt(ctx, bad["F"], bad["first"], bad["second"], bad["R_21"], bad["t_21"], check=False)
            assert d["rc"] == ERR_ARG and np.all(d["translations"] == -7.0) and d["info"] == -7 and d["guard_intact"], name
    # NULLs
    first = np.ascontiguousarray(sc["first"], np.int32); second = np.ascontiguousarray(sc["second"], np.int32)
    R = np.ascontiguousarray(sc["R_21"], np.float64); t21 = np.ascontiguousarray(sc["t_21"], np.float64)
    s = sc["scales"].copy(); t = np.zeros((3, 3)); w = np.ones(3); prm = api.TransavgParams(0.01, 1.3, 0.9, 50); sm = api.TransavgSummary(-7.0, -7.0, -7, -7, -7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    full = [p(first), p(second), p(R), p(t21), p(s)]
    for hole in range(5):
        a = list(full); a[hole] = None
        rc = ctx.lib.pvlm_transavg_solve(ctx._h, 3, 3, a[0], a[1], a[2], a[3], a[4], 0, p(t), p(w), C.byref(prm), C.byref(sm))
        assert rc == ERR_ARG and sm.termination == -7 and np.all(t == 0) and np.all(w == 1), hole
    for args in ((None, p(w), C.byref(prm), C.byref(sm)), (p(t), None, C.byref(prm), C.byref(sm)), (p(t), p(w), None, C.byref(sm)), (p(t), p(w), C.byref(prm), None)):
        rc = ctx.lib.pvlm_transavg_solve(ctx._h, 3, 3, *full, 0, *args)
        assert rc == ERR_ARG and sm.termination == -7 and np.all(t == 0) and np.all(w == 1)
    info = C.c_int(-7)
    assert ctx.lib.pvlm_transavg_dlt(ctx._h, 3, 3, p(first), p(second), p(R), p(t21), None, C.byref(info)) == ERR_ARG and info.value == -7
    assert ctx.lib.pvlm_transavg_dlt(ctx._h, 3, 3, p(first), p(second), p(R), p(t21), p(t), None) == ERR_ARG and np.all(t == 0)


def test_estimate_global_translation_device(ctx):
    """EstimateGlobalTranslation through the device equals its host-compile route on the CPU test's small list, within the same tolerance; so does L2IRLS"""
    g = tr.mirror_scene()
    for method in (1, 4):
        d = tr.run_driver(g, "estimate", "device", method=method); h = tr.run_driver(g, "estimate", "host", method=method)
        assert d["ok"] == 1 and h["ok"] == 1, (d["message"], h["message"])
        assert d["pairs"] == h["pairs"] and d["valid"] == h["valid"]
        worst = max(np.abs(d["t_wc"][i] - h["t_wc"][i]).max() for i in range(g["F"]) if h["valid"][i])
        print("method", method, "largest difference %.3e" % worst)
        assert worst <= tr.TOL["t"]
    bad = tr.run_driver(tr.mirror_scene(frame7_scaled=False), "estimate", "device", method=1)
    assert bad["ok"] == 0 and "1183" in bad["message"]
