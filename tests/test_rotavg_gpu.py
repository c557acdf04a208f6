"""GPU checks of K40 through the C ABI: pvlm_rotavg_l1 / pvlm_rotavg_l2 against the host compile of the same core (tests/cpp/rotavg_core_check.cpp) with the tolerance
of tests/test_rotavg_cpu.py (rotavg_ref.TOL) and equal iteration counts, info and termination codes — every scene here was held to the knife-edge condition there —
bit-reproducibility, the kernels held to one workgroup, and the argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import rotavg_ref as rr

pytestmark = pytest.mark.gpu

NAMES = list(rr.scenes().keys())
ERR_ARG = -1      # pvlm_status PVLM_ERR_ARG


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _l1(ctx, sc, check=True):
    from panovlm_amd import api
    g = api.rotavg_l1(ctx, sc["first"], sc["second"], sc["R_21"], sc["start"], sc["R0"], check=check)
    assert g["guard_intact"]
    g.update(l1=g["l1_iterations"], admm=g["admm_iterations"], irls=g["irls_iterations"])
    return g


def _l2(ctx, sc, R_in, check=True, **kw):
    from panovlm_amd import api
    g = api.rotavg_l2(ctx, sc["first"], sc["second"], sc["R_21"], R_in, check=check, **kw)
    assert g["guard_intact"]
    g.update(successful=g["successful_steps"], unsuccessful=g["unsuccessful_steps"])
    return g


def test_group_size(ctx):
    from panovlm_amd import api
    assert api.rotavg_group_size() == rr.G == rr.host_group_size()


@pytest.mark.parametrize("name", NAMES)
def test_scene_against_host(ctx, name):
    """a triangle, K4 with start_idx in the middle, a 9-ring with chords, a hub of degree G - 1, G, G + 1, 2 G + 1, F - 1 = 63, 64, 65 (the lane stride of the dense
    product; F = 65: the per-camera groups pass one workgroup), noise-free (info > 0 at the first IRLS system) and 10 % outliers; lists that are not sorted, with
    first > second.  The L2 stage starts from the host compile's L1 result on both sides."""
    sc = rr.scenes()[name]
    g1 = _l1(ctx, sc); h1 = rr.host_l1(sc)
    g2 = _l2(ctx, sc, h1["rotations"]); h2 = rr.host_l2(sc, h1["rotations"])
    d = dict(angle_l1=rr.largest_angle(g1["rotations"], h1["rotations"]), angle_l2=rr.largest_angle(g2["rotations"], h2["rotations"]), cost=abs(g2["final_cost"] - h2["final_cost"]))
    print(name, "device", rr.counts_l1(g1), rr.counts_l2(g2), "host", rr.counts_l1(h1), rr.counts_l2(h2), "differences", d)
    assert g1["rc"] == 0 and g2["rc"] == 0 and h1["rc"] == 0 and h2["rc"] == 0
    assert rr.counts_l1(g1) == rr.counts_l1(h1)
    assert rr.counts_l2(g2) == rr.counts_l2(h2)
    assert abs(g2["initial_cost"] - h2["initial_cost"]) <= rr.TOL["cost"]
    for k in d:
        assert d[k] <= rr.TOL[k], (k, d[k], rr.TOL[k])
    assert np.array_equal(g1["rotations"][sc["start"]], np.eye(3))


def test_past_a_grid_stride_trip(ctx):
    """F65 (65 cameras, 189 pairs) with every kernel held to ONE workgroup (PVLM_ROTAVG_MAX_BLOCKS): the dense product reaches its 64 rows in sixteen trips of four, the
    gathers their 65 cameras in three trips of 32.  The same bits as the unrestricted call."""
    sc = rr.scenes()["F65"]
    free1 = _l1(ctx, sc); free2 = _l2(ctx, sc, free1["rotations"])
    os.environ["PVLM_ROTAVG_MAX_BLOCKS"] = "1"
    try:
        held1 = _l1(ctx, sc); held2 = _l2(ctx, sc, free1["rotations"])
    finally:
        del os.environ["PVLM_ROTAVG_MAX_BLOCKS"]
    assert np.array_equal(_bits(held1["rotations"]), _bits(free1["rotations"])) and rr.counts_l1(held1) == rr.counts_l1(free1)
    assert np.array_equal(_bits(held2["rotations"]), _bits(free2["rotations"])) and rr.counts_l2(held2) == rr.counts_l2(free2)
    assert (held2["initial_cost"], held2["final_cost"]) == (free2["initial_cost"], free2["final_cost"])


def test_l2_pairs_past_a_grid_stride_trip(ctx):
    """The scenes above have at most 189 pairs, so the L2 stage's per-pair kernels (the pair-graph layer's, shared with K42 and K46) never take a second trip of
    their stride loop there.  90 cameras, each paired with its next three: 264 pairs, two trips of 256 when the kernels are held to ONE workgroup.  Five LM
    iterations from the spanning-tree start, free and held: the same bits in the rotations, both costs, both step counts and the termination."""
    sc = rr.scene(490, rr.chain_pairs(90, 3), 90)
    assert sc["P"] == 264
    free = _l2(ctx, sc, sc["R0"], max_num_iterations=5)
    os.environ["PVLM_ROTAVG_MAX_BLOCKS"] = "1"
    try:
        held = _l2(ctx, sc, sc["R0"], max_num_iterations=5)
    finally:
        del os.environ["PVLM_ROTAVG_MAX_BLOCKS"]
    print("free", rr.counts_l2(free), free["initial_cost"], free["final_cost"], "held", rr.counts_l2(held), held["initial_cost"], held["final_cost"])
    assert free["rc"] == 0 and held["rc"] == 0 and free["successful"] + free["unsuccessful"] > 0
    assert np.array_equal(_bits(held["rotations"]), _bits(free["rotations"])) and rr.counts_l2(held) == rr.counts_l2(free)
    assert (held["initial_cost"], held["final_cost"]) == (free["initial_cost"], free["final_cost"])


@pytest.mark.parametrize("name", ["hub17", "F66"])
def test_two_runs_same_bits(ctx, name):
    sc = rr.scenes()[name]
    a, b = _l1(ctx, sc), _l1(ctx, sc)
    assert np.array_equal(_bits(a["rotations"]), _bits(b["rotations"])) and rr.counts_l1(a) == rr.counts_l1(b) and a["info"] == b["info"]
    c, d = _l2(ctx, sc, a["rotations"]), _l2(ctx, sc, a["rotations"])
    assert np.array_equal(_bits(c["rotations"]), _bits(d["rotations"]))
    for k in ("initial_cost", "final_cost", "successful", "unsuccessful", "termination"):
        assert c[k] == d[k], k


def test_single_camera_and_no_pairs(ctx):
    from panovlm_amd import api
    g = api.rotavg_l1(ctx, [], [], np.zeros((0, 9)), 0, np.eye(3)[None])
    assert (g["l1_iterations"], g["admm_iterations"], g["irls_iterations"], g["info"]) == (0, 0, 0, 0) and np.array_equal(g["rotations"][0], np.eye(3)) and g["guard_intact"]
    g = api.rotavg_l2(ctx, [], [], np.zeros((0, 9)), np.eye(3)[None])
    assert g["termination"] == 6 and g["initial_cost"] == 0 and g["final_cost"] == 0 and np.array_equal(g["rotations"][0], np.eye(3)) and g["guard_intact"]


def test_arguments_refused(ctx):
    """every PVLM_ERR_ARG case leaves the outputs untouched: the rotations come back bit for bit, the summaries and the guard words stand"""
    from panovlm_amd import api
    sc = rr.scenes()["K4"]
    for name, bad in rr.bad_calls(sc):
        g = _l1(ctx, bad, check=False)
        assert g["rc"] == ERR_ARG and np.array_equal(_bits(g["rotations"]), _bits(bad["R0"])), name
        assert (g["l1"], g["admm"], g["irls"], g["info"]) == (-7, -7, -7, -7), name
        if "start" not in name:
            g = _l2(ctx, bad, bad["R0"], check=False)
            assert g["rc"] == ERR_ARG and np.array_equal(_bits(g["rotations"]), _bits(bad["R0"])) and g["termination"] == -7 and g["initial_cost"] == -7.0, name
    g = _l2(ctx, sc, sc["R0"], check=False, max_num_iterations=-1)
    assert g["rc"] == ERR_ARG and g["termination"] == -7 and np.array_equal(_bits(g["rotations"]), _bits(sc["R0"]))
    g = _l2(ctx, sc, sc["R0"], check=False, loss_a=np.nan)
    assert g["rc"] == ERR_ARG and g["termination"] == -7
    # NULLs
    first = np.ascontiguousarray(sc["first"], np.int32); second = np.ascontiguousarray(sc["second"], np.int32); R = np.ascontiguousarray(sc["R_21"], np.float64)
    rot = np.ascontiguousarray(sc["R0"], np.float64).copy(); keep = rot.copy()
    s1 = api.RotavgL1Summary(-7, -7, -7, -7); s2 = api.TransavgSummary(-7.0, -7.0, -7, -7, -7); prm = api.RotavgL2Params(0.07, 50)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    full = [p(first), p(second), p(R)]
    for hole in range(3):
        a = list(full); a[hole] = None
        assert ctx.lib.pvlm_rotavg_l1(ctx._h, 4, 6, a[0], a[1], a[2], sc["start"], p(rot), C.byref(s1)) == ERR_ARG and s1.info == -7 and np.array_equal(rot, keep), hole
        assert ctx.lib.pvlm_rotavg_l2(ctx._h, 4, 6, a[0], a[1], a[2], p(rot), C.byref(prm), C.byref(s2)) == ERR_ARG and s2.termination == -7 and np.array_equal(rot, keep), hole
    assert ctx.lib.pvlm_rotavg_l1(ctx._h, 4, 6, *full, sc["start"], None, C.byref(s1)) == ERR_ARG and s1.info == -7
    assert ctx.lib.pvlm_rotavg_l1(ctx._h, 4, 6, *full, sc["start"], p(rot), None) == ERR_ARG and np.array_equal(rot, keep)
    assert ctx.lib.pvlm_rotavg_l2(ctx._h, 4, 6, *full, None, C.byref(prm), C.byref(s2)) == ERR_ARG and s2.termination == -7
    assert ctx.lib.pvlm_rotavg_l2(ctx._h, 4, 6, *full, p(rot), None, C.byref(s2)) == ERR_ARG and s2.termination == -7 and np.array_equal(rot, keep)
    assert ctx.lib.pvlm_rotavg_l2(ctx._h, 4, 6, *full, p(rot), C.byref(prm), None) == ERR_ARG and np.array_equal(rot, keep)


def test_estimate_global_rotation_device(ctx):
    """EstimateGlobalRotation through the device equals its host-compile route on the CPU test's mirror scene: the same surviving pairs (the triplet test and the
    X84 threshold take the same decisions), rotations within the tolerance of the L1 stages; the chain into EstimateGlobalTranslation gives every frame a pose and keeps the surviving pairs, its
    centres within the CPU test's 2 mm of the truth up to the free scale"""
    g = rr.mirror_scene()
    d = rr.run_driver(g, "estimate", "device", 1, 1); h = rr.run_driver(g, "estimate", "host", 1, 1)
    assert d["ok"] == 1 and h["ok"] == 1, (d["message"], h["message"])
    assert d["pairs"] == h["pairs"] and d["valid"] == h["valid"]
    worst = max(rr.angle_between(d["R_wc"][i], h["R_wc"][i]) for i in range(g["F"]))
    print("largest rotation difference %.3e rad" % worst)
    assert worst <= rr.TOL["angle_l1"]
    d = rr.run_driver(g, "chain", "device", 1, 1); h = rr.run_driver(g, "chain", "host", 1, 1)
    assert d["ok"] == 1 and h["ok"] == 1 and d["translation_ok"] == 1 and h["translation_ok"] == 1 and d["pairs"] == h["pairs"] and d["valid"] == h["valid"]
    s, far = rr.chain_error(g, d)
    print("scale %.4f, largest centre error %.5f m" % (s, far))
    assert 0.9 - 1e-6 <= s <= 1.3 + 1e-6 and far < 2e-3
    bad = rr.run_driver(g, "estimate", "device", 2, 1)
    assert bad["ok"] == 0 and "not supported" in bad["message"]
