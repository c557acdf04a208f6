"""GPU checks of K44 through the C ABI: pvlm_transavg_bata against the host compile of the same core (tests/cpp/bata_core_check.cpp) with the tolerance of
tests/test_bata_cpu.py (bata_ref.TOL) and equal info — every scene here was held to the knife-edge condition there — bit-reproducibility, the argument checks, and
EstimateGlobalTranslation(method 5, enable_bata) through the device against its host-compile route."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bata_ref as br

pytestmark = pytest.mark.gpu

NAMES = list(br.scenes().keys())
ERR_ARG = -1      # pvlm_status PVLM_ERR_ARG
_HOST = {}


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _host(name):
    if name not in _HOST:
        sc, kw = br.scenes()[name]
        _HOST[name] = br.host_solve(sc, **kw)
    return _HOST[name]


def _gpu(ctx, sc, check=True, **kw):
    from panovlm_amd import api
    g = api.bata_solve(ctx, sc["n_cameras"], sc["first"], sc["second"], sc["dir"], sc["s0"], check=check, **kw)
    assert g["guard_intact"]
    return g


def _against_host(g, h):
    assert h["rc"] == 0 and g["rc"] == 0 and g["info"] == h["info"] == 0
    d = br.differences(g, h)
    print("differences device - host compile", d)
    assert np.all(g["centres"][0] == 0.0) and np.all(g["lud_centres"][0] == 0.0)
    for k in br.TOL:
        assert d[k] <= br.TOL[k], (k, d[k], br.TOL[k])


def _same_bits(a, b):
    for k in ("centres", "lud_centres", "scales"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["info"] == b["info"]


def test_group_size(ctx):
    from panovlm_amd import api
    assert api.bata_group_size() == br.G == br.host_group_size()


@pytest.mark.parametrize("name", NAMES)
def test_scene_against_host(ctx, name):
    """pairs 3, 63, 64, 65, 257; cameras 3, 64, 65; a hub of degree G - 1, G, G + 1, 2 G + 1; ids that start at 2; lists that are not sorted, with first > second and
    with one repeated pair; all-scaled, all-unscaled and mixed; the noise-free and the outlier scene; a short call"""
    sc, kw = br.scenes()[name]
    g = _gpu(ctx, sc, **kw)
    assert g["F"] == sc["F"]
    _against_host(g, _host(name))


def test_past_a_grid_stride_trip(ctx):
    """257 pairs with the kernels held to ONE workgroup of 256 lanes (PVLM_BATA_MAX_BLOCKS): the last pair is reached by the second trip of the stride loop, 90
    cameras by the second and third trip of the gather's.  The same bits as the unrestricted call."""
    sc, kw = br.scenes()["P257"]
    free = _gpu(ctx, sc, **kw)
    os.environ["PVLM_BATA_MAX_BLOCKS"] = "1"
    try:
        held = _gpu(ctx, sc, **kw)
    finally:
        del os.environ["PVLM_BATA_MAX_BLOCKS"]
    _against_host(held, _host("P257"))
    _same_bits(held, free)


@pytest.mark.parametrize("name", ["hub17", "F65"])
def test_two_runs_same_bits(ctx, name):
    sc, kw = br.scenes()[name]
    _same_bits(_gpu(ctx, sc, **kw), _gpu(ctx, sc, **kw))


@pytest.mark.parametrize("name", ["outlier", "hub9"])
def test_one_outer_is_the_lud_stage(ctx, name):
    """outer_iteration = 1: the centres are the LUD centres bit for bit, and the bits of the full call's LUD stage"""
    sc, kw = br.scenes()[name]
    g = _gpu(ctx, sc, outer_iteration=1)
    assert g["info"] == 0 and np.array_equal(_bits(g["centres"]), _bits(g["lud_centres"]))
    assert np.array_equal(_bits(g["lud_centres"]), _bits(_gpu(ctx, sc)["lud_centres"]))
    _against_host(g, br.host_solve(sc, outer_iteration=1))


def test_ids_are_shifted(ctx):
    sc, kw = br.scenes()["id2"]
    low = dict(sc); low["first"] = sc["first"] - 2; low["second"] = sc["second"] - 2; low["n_cameras"] = sc["F"]
    _same_bits(_gpu(ctx, sc), _gpu(ctx, low))


def test_two_components_not_positive_definite(ctx):
    sc = br.disconnected()
    g = _gpu(ctx, sc)
    h = br.host_solve(sc)
    assert g["rc"] == 0 and g["info"] > 0 and h["info"] > 0 and g["untouched"] and g["guard_intact"]


def test_not_finite_is_minus_one(ctx):
    sc, kw = br.scenes()["scaled"]
    g = _gpu(ctx, sc, delta=-1.0)
    assert g["rc"] == 0 and g["info"] == -1 == br.host_solve(sc, delta=-1.0)["info"] and g["untouched"]


def test_no_pairs(ctx):
    from panovlm_amd import api
    g = api.bata_solve(ctx, 4, [], [], np.zeros((0, 3)), [])
    assert g["rc"] == 0 and g["info"] == -2 and g["untouched"] and g["guard_intact"]


def test_arguments_refused(ctx):
    """every PVLM_ERR_ARG case, with nothing touched"""
    from panovlm_amd import api
    sc, kw = br.scenes()["P3"]
    for name, bad in br.bad_calls(sc):
        g = _gpu(ctx, bad, check=False, **bad.get("kw", {}))
        assert g["rc"] == ERR_ARG and g["info"] == -7 and g["untouched"], name
    # NULL pointers
    first = np.ascontiguousarray(sc["first"], np.int32); second = np.ascontiguousarray(sc["second"], np.int32)
    d = np.ascontiguousarray(sc["dir"], np.float64); s0 = np.ascontiguousarray(sc["s0"], np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cen = np.full((3, 3), -7.0); prm = api.BataParams(1e-6, 10, 10, 10, 0.1); info = C.c_int(-7)
    full = [p(first), p(second), p(d), p(s0), C.byref(prm), p(cen)]
    for k in range(len(full)):
        a = list(full); a[k] = None
        rc = ctx.lib.pvlm_transavg_bata(ctx._h, 3, 3, a[0], a[1], a[2], a[3], a[4], a[5], None, None, C.byref(info))
        assert rc == ERR_ARG and info.value == -7 and np.all(cen == -7.0), k
    assert ctx.lib.pvlm_transavg_bata(ctx._h, 3, 3, *full, None, None, None) == ERR_ARG and np.all(cen == -7.0)
    # the optional outputs may be NULL
    assert ctx.lib.pvlm_transavg_bata(ctx._h, 3, 3, *full, None, None, C.byref(info)) == 0 and info.value == 0
    assert np.array_equal(_bits(cen), _bits(_gpu(ctx, sc)["centres"]))


def test_estimate_global_translation_device_against_host(ctx):
    """EstimateGlobalTranslation(method 5, enable_bata) through the device against the host-compile route, with and without the DLT start"""
    g = br.mirror_graph()
    for init_dlt in (0, 1):
        dev = br.run_driver(g, "estimate", "device", method=5, seed=7, init_dlt=init_dlt, enable_bata=1)
        host = br.run_driver(g, "estimate", "host", method=5, seed=7, init_dlt=init_dlt, enable_bata=1)
        assert dev["ok"] == 1 and host["ok"] == 1, (dev["message"], host["message"])
        assert dev["pairs"] == host["pairs"]
        for i in range(g["F"]):
            assert dev["valid"][i] == host["valid"][i] == 1
            assert np.abs(dev["t_wc"][i] - host["t_wc"][i]).max() <= br.TOL["centres"], i
    off = br.run_driver(g, "estimate", "device", method=5, seed=7, init_dlt=0, enable_bata=0)
    assert off["ok"] == 0 and off["message"] == "Translaton average method not supported"
