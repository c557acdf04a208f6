"""GPU checks of K46 through the C ABI: pvlm_transavg_chordal / pvlm_transavg_lud against the host compile of the same core (tests/cpp/transdir_core_check.cpp)
with the tolerance of tests/test_transdir_cpu.py (transdir_ref.TOL) and equal step counts and termination codes — every scene here was held to the knife-edge
condition there — bit-reproducibility, the argument checks, and EstimateGlobalTranslation through the device against its host-compile route."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import transavg_ref as tr
from tests import transdir_ref as td

pytestmark = pytest.mark.gpu

NAMES = list(td.scenes().keys())
ERR_ARG = -1      # pvlm_status PVLM_ERR_ARG


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _gpu(ctx, problem, sc, c0=None, weight=None, loss_a=0.5, upper_ratio=1.3, lower_ratio=0.9, max_num_iterations=None, check=True):
    from panovlm_amd import api
    c0 = sc["start"] if c0 is None else c0
    if max_num_iterations is None:
        max_num_iterations = td.POLICY[problem][2]
    if problem == "chordal":
        g = api.transavg_chordal(ctx, sc["first"], sc["second"], sc["dir"], sc["origin"], c0, loss_a, max_num_iterations, check=check)
        g.update(scales=None, weight=None, sum_e=None)
    else:
        g = api.transavg_lud(ctx, sc["first"], sc["second"], sc["dir"], sc["scales"], weight, sc["origin"], c0, upper_ratio, lower_ratio, max_num_iterations, check=check)
    assert g["guard_intact"]
    g["successful"], g["unsuccessful"] = g["successful_steps"], g["unsuccessful_steps"]
    return g


def _against_host(g, h):
    d = td.differences(g, h)
    print("device", g["successful"], g["unsuccessful"], g["termination"], "host", h["successful"], h["unsuccessful"], h["termination"], "differences", d)
    assert h["rc"] == 0 and g["rc"] == 0
    assert (g["successful"], g["unsuccessful"], g["termination"]) == (h["successful"], h["unsuccessful"], h["termination"])
    assert abs(g["initial_cost"] - h["initial_cost"]) <= td.TOL["cost"]
    for k in td.TOL:
        assert d[k] <= td.TOL[k], (k, d[k], td.TOL[k])


def _same_bits(a, b):
    for k in ("centres", "scales", "weight"):
        if a[k] is not None:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    for k in ("initial_cost", "final_cost", "sum_e", "successful", "unsuccessful", "termination"):
        assert a[k] == b[k], k


def test_group_size(ctx):
    from panovlm_amd import api
    assert api.transdir_group_size() == td.G == td.host_group_size()


@pytest.mark.parametrize("name", NAMES)
def test_scene_against_host(ctx, name):
    """both problems on: pairs 3, 63, 64, 65, 4 * 64 + 1; cameras 3, 64, 65; a hub of degree G - 1, G, G + 1, 2 G + 1; the origin first, in the middle and last;
    lists that are not sorted, with first > second and with a repeated pair; for LUD all-scaled, all-unscaled and mixed lists, scales clamped at 3 s0 and 0.5 s0,
    Room's ratios; for chordal a threshold every pair is inside and one that some are past"""
    problem, sc, kw = td.scenes()[name]
    g = _gpu(ctx, problem, sc, **kw)
    _against_host(g, td.host_solve(problem, sc, **kw))
    if name == "lud-clamp":
        assert g["scales"][4] == 3.0 * sc["scales"][4] and g["scales"][9] == 0.5 * sc["scales"][9]
    if problem == "lud":
        assert np.all(g["scales"][sc["scales"] == 1] >= 1.0)


def test_weights_applied(ctx):
    problem, sc, kw = td.scenes()["lud-scaled"]
    w = 0.5 + np.arange(sc["P"]) % 3
    g = _gpu(ctx, "lud", sc, weight=w, **kw)
    _against_host(g, td.host_solve("lud", sc, weight=w, **kw))
    assert g["initial_cost"] != _gpu(ctx, "lud", sc, **kw)["initial_cost"]


@pytest.mark.parametrize("problem", ["chordal", "lud"])
def test_past_a_grid_stride_trip(ctx, problem):
    """257 pairs with the per-pair kernels held to ONE workgroup of 256 lanes (PVLM_TRANSDIR_MAX_BLOCKS): the last pair is reached by the second trip of the stride
    loop, 90 cameras by the second and third trip of the gather's.  The same bits as the unrestricted call."""
    problem, sc, kw = td.scenes()[problem + "-P257"]
    free = _gpu(ctx, problem, sc, **kw)
    os.environ["PVLM_TRANSDIR_MAX_BLOCKS"] = "1"
    try:
        held = _gpu(ctx, problem, sc, **kw)
    finally:
        del os.environ["PVLM_TRANSDIR_MAX_BLOCKS"]
    _against_host(held, td.host_solve(problem, sc, **kw))
    _same_bits(held, free)


@pytest.mark.parametrize("name", ["chordal-hub17", "lud-hub17", "chordal-F65", "lud-F65"])
def test_two_runs_same_bits(ctx, name):
    problem, sc, kw = td.scenes()[name]
    _same_bits(_gpu(ctx, problem, sc, **kw), _gpu(ctx, problem, sc, **kw))


@pytest.mark.parametrize("problem", ["chordal", "lud"])
def test_zero_iterations(ctx, problem):
    """inputs come back bit for bit, initial cost = final cost"""
    problem, sc, kw = td.scenes()[problem + "-P63"]
    kw = dict(kw, max_num_iterations=0)
    g = _gpu(ctx, problem, sc, **kw)
    assert np.array_equal(_bits(g["centres"]), _bits(sc["start"])) and g["initial_cost"] == g["final_cost"]
    assert (g["successful"], g["unsuccessful"], g["termination"]) == (0, 0, 0)
    if problem == "lud":
        assert np.array_equal(_bits(g["scales"]), _bits(sc["scales"]))
    _against_host(g, td.host_solve(problem, sc, **kw))


def test_coincident_cameras(ctx):
    """chordal with two cameras on one point at the start: termination 5, the centres untouched"""
    problem, sc, kw = td.scenes()["chordal-P3"]
    c0 = sc["start"].copy(); c0[sc["first"][1]] = c0[sc["second"][1]]
    g = _gpu(ctx, "chordal", sc, c0)
    assert g["rc"] == 0 and g["termination"] == 5 and not np.isfinite(g["initial_cost"]) and np.array_equal(_bits(g["centres"]), _bits(c0))


def test_zero_error_pair(ctx):
    sc = dict(F=2, P=1, first=np.array([0], np.int32), second=np.array([1], np.int32), dir=np.array([[1.0, 0, 0]]), scales=np.array([1.0]), origin=1,
              start=np.array([[1.0, 0, 0], [0, 0, 0]]))
    g = _gpu(ctx, "lud", sc)
    assert g["termination"] == 2 and np.array_equal(g["centres"], sc["start"]) and g["scales"][0] == 1.0 and g["sum_e"] == 0.0


def test_no_pairs(ctx):
    from panovlm_amd import api
    c0 = np.array([[1.0, 2, 3], [0, 0, 0]])
    g = api.transavg_chordal(ctx, [], [], np.zeros((0, 3)), 1, c0)
    assert g["termination"] == 6 and g["initial_cost"] == 0 and g["final_cost"] == 0 and np.array_equal(g["centres"], c0) and g["guard_intact"]
    g = api.transavg_lud(ctx, [], [], np.zeros((0, 3)), [], None, 1, c0)
    assert g["termination"] == 6 and g["initial_cost"] == 0 and g["final_cost"] == 0 and np.array_equal(g["centres"], c0) and g["sum_e"] == -7.0 and g["guard_intact"]


def test_arguments_refused(ctx):
    """every PVLM_ERR_ARG case leaves the outputs untouched: the inputs come back bit for bit, the guard words stand"""
    from panovlm_amd import api
    problem, sc, kw = td.scenes()["lud-P3"]
    for name, bad, lud_only in td.bad_calls(sc):
        for problem in ("lud",) if lud_only else ("chordal", "lud"):
            g = _gpu(ctx, problem, bad, weight=bad.get("weight"), max_num_iterations=bad.get("max_num_iterations", 5), check=False)
            assert g["rc"] == ERR_ARG, (name, problem)
            assert np.array_equal(_bits(g["centres"]), _bits(bad["start"])) and g["termination"] == -7 and g["initial_cost"] == -7.0, (name, problem)
            if problem == "lud":
                assert np.array_equal(_bits(g["scales"]), _bits(bad["scales"])) and g["sum_e"] == -7.0, name
                assert np.array_equal(g["weight"], np.ones(sc["P"]) if bad.get("weight") is None else bad["weight"]), name
    # NULLs
    first = np.ascontiguousarray(sc["first"], np.int32); second = np.ascontiguousarray(sc["second"], np.int32); d = np.ascontiguousarray(sc["dir"], np.float64)
    s = sc["scales"].copy(); c = np.zeros((3, 3)); w = np.ones(3); sum_e = C.c_double(-7.0)
    cp = api.TransdirChordalParams(0.5, 300); lp = api.TransdirLudParams(1.3, 0.9, 50); sm = api.TransavgSummary(-7.0, -7.0, -7, -7, -7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for hole in range(6):
        a = [p(first), p(second), p(d), p(c), C.byref(cp), C.byref(sm)]; a[hole] = None
        rc = ctx.lib.pvlm_transavg_chordal(ctx._h, 3, 3, a[0], a[1], a[2], 0, a[3], a[4], a[5])
        assert rc == ERR_ARG and sm.termination == -7 and np.all(c == 0), hole
    for hole in range(9):
        a = [p(first), p(second), p(d), p(s), p(w), p(c), C.byref(lp), C.byref(sum_e), C.byref(sm)]; a[hole] = None
        rc = ctx.lib.pvlm_transavg_lud(ctx._h, 3, 3, a[0], a[1], a[2], a[3], a[4], 0, a[5], a[6], a[7], a[8])
        assert rc == ERR_ARG and sm.termination == -7 and np.all(c == 0) and np.all(w == 1) and np.array_equal(s, sc["scales"]) and sum_e.value == -7.0, hole


def test_estimate_global_translation_device(ctx):
    """EstimateGlobalTranslation through the device equals its host-compile route within the same tolerance: method 3 on the CPU test's small list, method 6 on
    transdir_ref.lud_estimate_graph(), the graph admitted on the CPU because LUD at its defaults is well conditioned there.  On the small list method 6's routes
    agree in what they keep; their values are printed, not compared: one ulp of an input moves them by 6e-6 m there (measured on the MI355X: 5.6e-4 m apart there,
    3.1e-15 m on the admitted graph, 1.2e-12 m for method 3)."""
    for method, g in ((3, tr.mirror_scene()), (6, td.lud_estimate_graph()), (6, tr.mirror_scene())):
        d = td.run_driver(g, "estimate", "device", method=method); h = td.run_driver(g, "estimate", "host", method=method)
        assert d["ok"] == 1 and h["ok"] == 1, (d["message"], h["message"])
        assert d["pairs"] == h["pairs"] and d["valid"] == h["valid"]
        worst = max(np.abs(d["t_wc"][i] - h["t_wc"][i]).max() for i in range(g["F"]) if h["valid"][i])
        print("method", method, "frames", g["F"], "largest difference %.3e" % worst)
        assert np.isfinite(worst)
        if method == 3 or g["F"] == 4:
            assert worst <= td.TOL["c"]
