"""GPU checks of K45 through the C ABI: pvlm_rotavg_least_square against the host compile of the same core (tests/cpp/rotstart_core_check.cpp) with the tolerance of
tests/test_rotstart_cpu.py (rotstart_ref.TOL) and equal iteration counts and info, the stride loops, bit-reproducibility, the refused arguments and the info values,
and EstimateGlobalRotation(method 2, enable_l2_start) through the device against its host-compile route, alone and chained into EstimateGlobalTranslation."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import rotavg_ref as rr
from tests import rotstart_ref as rs

pytestmark = pytest.mark.gpu

NAMES = list(rs.scenes().keys())
ERR_ARG = -1      # pvlm_status PVLM_ERR_ARG


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _gpu(ctx, sc, R0=None, check=True, **kw):
    from panovlm_amd import api
    g = api.rotavg_least_square(ctx, sc["first"], sc["second"], sc["R_21"], sc["R0"] if R0 is None else R0, check=check, **kw)
    assert g["guard_intact"]
    return g


def _sentinel(g):
    return (g["iterations"], g["solves"], g["info"], g["residual"]) == (-7, -7, -7, -7.0) and bool(np.all(g["theta"] == -7.0))


@pytest.mark.parametrize("name", NAMES)
def test_scene_against_host(ctx, name):
    """2, 3, 5, 12, 40, 64, 200 and 300 cameras; a tree; a hub of degree 63; the noise-free scene; the shuffled list with half its pairs turned round"""
    g, h = _gpu(ctx, rs.scenes()[name]), rs.host(name)
    a = rr.largest_angle(g["rotations"], h["rotations"])
    print(name, "iterations", g["iterations"], h["iterations"], "residual %.3e %.3e" % (g["residual"], h["residual"]), "device - host compile %.3e rad" % a)
    assert g["rc"] == 0 and h["rc"] == 0 and g["info"] == h["info"] == 0
    assert g["iterations"] == h["iterations"] and g["solves"] == h["solves"] == 3 * g["iterations"]
    assert a <= rs.TOL, (a, rs.TOL)
    assert np.abs(g["theta"] - h["theta"]).max() <= 1e-12 * rs.scenes()[name]["P"]


@pytest.mark.parametrize("name", ["rand300", "hub64"])
def test_past_a_grid_stride_trip(ctx, name):
    """the kernels held to ONE workgroup (PVLM_ROTAVG_MAX_BLOCKS): 300 cameras and 1 200 pairs are reached by later trips of the stride loops, the gather's 32 cameras
    per trip many times over; rand300 sends the camera tree past one 256-leaf chunk, the hub's row passes the 8 lanes of its group eight times.  The same bits as the
    unrestricted call."""
    sc = rs.scenes()[name]
    free = _gpu(ctx, sc)
    os.environ["PVLM_ROTAVG_MAX_BLOCKS"] = "1"
    try:
        held = _gpu(ctx, sc)
    finally:
        del os.environ["PVLM_ROTAVG_MAX_BLOCKS"]
    assert free["info"] == held["info"] == 0 and free["iterations"] == held["iterations"]
    assert np.array_equal(_bits(free["rotations"]), _bits(held["rotations"])) and np.array_equal(_bits(free["theta"]), _bits(held["theta"]))
    assert _bits(free["residual"]) == _bits(held["residual"])


def test_bit_reproducible(ctx):
    for name in ("band200", "rand300"):
        a, b = _gpu(ctx, rs.scenes()[name]), _gpu(ctx, rs.scenes()[name])
        assert np.array_equal(_bits(a["rotations"]), _bits(b["rotations"])) and np.array_equal(_bits(a["theta"]), _bits(b["theta"]))
        assert (a["iterations"], a["info"]) == (b["iterations"], b["info"]) and _bits(a["residual"]) == _bits(b["residual"])


def test_refused_arguments(ctx):
    """every PVLM_ERR_ARG case: the status, the rotations untouched, the summary still the sentinel"""
    from panovlm_amd import api
    sc = rs.scenes()["rand12"]
    for name, bad, kw in rs.bad_calls(sc):
        g = _gpu(ctx, bad, check=False, **kw)
        assert g["rc"] == ERR_ARG, name
        assert np.array_equal(g["rotations"], np.asarray(bad["R0"]).reshape(-1, 3, 3), equal_nan=True), name
        assert _sentinel(g), name
    first, second, P, R21, F, rot = api._rotavg_inputs(sc["first"], sc["second"], sc["R_21"], sc["R0"])
    prm = api.RotavgLsqParams(1e-9, 1e-12, 100)
    sm = api.RotavgLsqSummary(-7, -7, -7, -7.0, (C.c_double * 3)(-7.0, -7.0, -7.0))
    before = rot.copy()
    args = [C.c_int(F), C.c_int(P), api._p(first, C.c_int), api._p(second, C.c_int), api._p(R21, C.c_double), api._p(rot, C.c_double), C.byref(prm), C.byref(sm)]
    for k in (2, 3, 4, 5, 6, 7):                                  # a NULL in the place of every pointer
        a = list(args); a[k] = None
        assert ctx.lib.pvlm_rotavg_least_square(ctx._h, *a) == ERR_ARG, k
        assert np.array_equal(rot, before) and (sm.iterations, sm.solves, sm.info, sm.residual) == (-7, -7, -7, -7.0)


def test_info_values(ctx):
    """-2 (max_iterations = 1 on band200), -3 (a start whose Gram matrix is singular), k > 0 (an R_21 of ten times a rotation): the rotations stay as they came, the
    info equals the host compile's"""
    sc = rs.scenes()["band200"]
    g, h = _gpu(ctx, sc, max_iterations=1), rs.host_least_square(sc, max_iterations=1)
    assert g["rc"] == 0 and g["info"] == h["info"] == -2 and g["iterations"] == 1 and g["solves"] == 3 and np.array_equal(_bits(g["rotations"]), _bits(sc["R0"]))
    sc = rs.scenes()["rand12"]
    for start in (np.zeros_like(sc["R0"]), np.concatenate([sc["R0"][:, :, :2], sc["R0"][:, :, 1:2]], axis=2)):
        g, h = _gpu(ctx, sc, R0=start), rs.host_least_square(sc, R0=start)
        assert g["rc"] == 0 and g["info"] == h["info"] == -3 and g["iterations"] == 0 and np.array_equal(_bits(g["rotations"]), _bits(start))
    R = sc["R_21"].copy(); R[3] *= 10.0
    g, h = _gpu(ctx, dict(sc, R_21=R)), rs.host_least_square(dict(sc, R_21=R))
    assert g["rc"] == 0 and g["info"] > 0 and h["info"] > 0 and np.array_equal(_bits(g["rotations"]), _bits(sc["R0"]))


# ---- the host mirror through the device ----------------------------------------------------------------------------------------------------------
def test_estimate_global_rotation_method_2_device():
    """EstimateGlobalRotation(method 2, enable_l2_start) through the device against the host route: the same pairs, the rotations within rotstart_ref.TOL plus K40's
    tolerance of the L2 stage; without the flag the refusal and its text as before"""
    g = rr.mirror_scene()
    d, h = rs.run_driver(g, "estimate", "device", 2, 1, 1), rs.run_driver(g, "estimate", "host", 2, 1, 1)
    assert d["ok"] == 1 and h["ok"] == 1 and d["message"] == "" and d["pairs"] == h["pairs"]
    worst = max(rr.angle_between(d["R_wc"][i], h["R_wc"][i]) for i in range(g["F"]))
    print("device - host route %.3e rad" % worst)
    assert worst <= rs.TOL + rr.TOL["angle_l2"]
    for (i, j), R21 in zip(d["pairs"], d["R_21"]):
        assert np.abs(R21 - d["R_wc"][j].T @ d["R_wc"][i]).max() <= 4 * np.finfo(np.float64).eps
    bad = rs.run_driver(g, "estimate", "device", 2, 1, 0)
    assert bad["ok"] == 0 and "not supported" in bad["message"]


def test_rotation_then_translation_method_2_device():
    """method 2 into EstimateGlobalTranslation (method 1), all on the device: every frame gets a pose; the bounds of K40's chain test"""
    g = rr.mirror_scene()
    c = rs.run_driver(g, "chain", "device", 2, 1, 1)
    assert c["ok"] == 1 and c["translation_ok"] == 1, (c["message"], c["translation_message"])
    assert all(c["valid"][i] == 1 for i in range(g["F"]))
    s, worst = rr.chain_error(g, c)
    print("scale %.4f, largest centre error %.5f m" % (s, worst))
    assert 0.9 - 1e-6 <= s <= 1.3 + 1e-6 and worst < 2e-3
