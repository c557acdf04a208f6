"""CPU checks of K40: the host compile of panovlm_amd/csrc/pvlm_rotavg_core.h (tests/cpp/rotavg_core_check.cpp) against the independent numpy reference of
tests/rotavg_ref.py (the full 2 P rows, dense solves, a dense LM), the knife-edge condition on every scene any K40 test uses, the analytic Jacobians against central
differences, what the averaging has to achieve, and the refused arguments."""
import subprocess

import numpy as np
import pytest

from tests import rotavg_ref as rr

NAMES = list(rr.scenes().keys())


def test_constants():
    assert rr.host_group_size() == rr.G and rr.host_tile() == rr.TILE
    F = [rr.scenes()[n]["F"] for n in NAMES]
    assert {rr.TILE, rr.TILE + 1, rr.TILE + 2} <= set(F)          # F - 1 on both sides of the dense product's lane stride


@pytest.mark.parametrize("name", NAMES)
def test_knife_edge(name):
    """A scene is admitted only if the reference gives the same iteration counts of all three stages, the same info and the same termination with every stopping
    threshold scaled by 1 - 1e-6 and by 1 + 1e-6, and no IRLS factorisation was decided by rounding.  A seed that fails is replaced in rotavg_ref.SEEDS and the
    candidate recorded in rotavg_ref.DROPPED (at most one candidate in five)."""
    sc = rr.scenes()[name]
    a, b = rr.reference(name)
    assert not a["knife"], a["knife"]
    for s in (1 - 1e-6, 1 + 1e-6):
        a2 = rr.l1_ref(sc, scale=s)
        assert rr.counts_l1(a2) == rr.counts_l1(a), (s, rr.counts_l1(a2), rr.counts_l1(a))
        assert rr.counts_l2(rr.l2_ref(sc, a["rotations"], scale=s)) == rr.counts_l2(b), s
    assert 5 * len(rr.DROPPED) <= len(NAMES) + len(rr.DROPPED)


def _differences(name):
    sc = rr.scenes()[name]
    a, b = rr.reference(name)
    h1 = rr.host_l1(sc); h2 = rr.host_l2(sc, a["rotations"])
    d = dict(angle_l1=rr.largest_angle(a["rotations"], h1["rotations"]), angle_l2=rr.largest_angle(b["rotations"], h2["rotations"]), cost=abs(b["final_cost"] - h2["final_cost"]))
    return a, b, h1, h2, d


@pytest.mark.parametrize("name", NAMES)
def test_scene_against_reference(name):
    """Equal iteration counts of the L1, ADMM and IRLS loops, equal info, equal accepted / rejected steps and termination of the L2 stage; rotations (the angle of
    R^T R_ref) and the L2 cost within rotavg_ref.TOL = ten times the largest difference the host compile shows against the reference over these scenes
    (rotavg_ref.MEASURED).  The L2 stage starts from the reference's L1 result on both sides."""
    a, b, h1, h2, d = _differences(name)
    print(name, "L1", rr.counts_l1(a), rr.counts_l1(h1), "L2", rr.counts_l2(b), rr.counts_l2(h2), d)
    assert h1["rc"] == 0 and h2["rc"] == 0
    assert rr.counts_l1(h1) == rr.counts_l1(a)
    assert rr.counts_l2(h2) == rr.counts_l2(b)
    assert abs(h2["initial_cost"] - b["initial_cost"]) <= rr.TOL["cost"]
    for k in d:
        assert d[k] <= rr.TOL[k], (k, d[k], rr.TOL[k])
    sc = rr.scenes()[name]
    assert np.array_equal(h1["rotations"][sc["start"]], np.eye(3))


def test_measured_is_the_maximum():
    """rotavg_ref.MEASURED is what it says: the largest difference over the scenes, each figure within its own last digit — but for the angle after the L1 stages,
    which is rounding amplified by the IRLS systems' condition numbers (1e15 to 1e17) and moves with the order of numpy's sums (the BLAS thread count changes
    F64 and F66 between 6e-6 and 1.3e-5): that one is held from above and to its order of magnitude"""
    worst = {k: 0.0 for k in rr.MEASURED}
    for name in NAMES:
        d = _differences(name)[4]
        for k in d:
            worst[k] = max(worst[k], float(d[k]))
    worst["x84"] = _x84()[0]
    print("measured", worst, "recorded", rr.MEASURED)
    for k in worst:
        assert worst[k] <= rr.MEASURED[k] and rr.MEASURED[k] <= (10 if k == "angle_l1" else 1.1) * worst[k] + 1e-300, (k, worst[k], rr.MEASURED[k])


def test_jacobians_against_central_differences():
    """the analytic 3 x 3 Jacobians of the core, and those of the reference (right-perturbation form), against central differences of the core's own residual: step
    1e-6, so truncation h^2 |r'''| / 6 ~ 1e-12 and rounding eps / h ~ 1e-10 per entry; bound 1e-8.  Small, moderate and large (2.5 rad) camera rotations, a
    residual near zero and one of 1 rad."""
    rng = np.random.default_rng(17)
    h = 1e-6
    for scale1, scale2, off in ((1e-9, 1e-9, 0.0), (0.3, 0.5, 0.02), (2.5, 1.0, 0.02), (0.7, 2.5, 1.0), (1e-4, 0.2, 1e-5)):
        aa1 = rng.normal(size=3); aa1 *= scale1 / np.linalg.norm(aa1)
        aa2 = rng.normal(size=3); aa2 *= scale2 / np.linalg.norm(aa2)
        e = rng.normal(size=3); e *= off / np.linalg.norm(e)
        R21 = rr.exp_so3(e) @ rr.exp_so3(aa2) @ rr.exp_so3(aa1).T
        r, J1, J2 = rr.host_l2_pair(aa1, aa2, R21)
        rr_, K1, K2 = rr.l2_pair_ref(aa1, aa2, R21)
        N1 = np.zeros((3, 3)); N2 = np.zeros((3, 3))
        for k in range(3):
            d = np.zeros(3); d[k] = h
            N1[:, k] = (rr.host_l2_pair(aa1 + d, aa2, R21)[0] - rr.host_l2_pair(aa1 - d, aa2, R21)[0]) / (2 * h)
            N2[:, k] = (rr.host_l2_pair(aa1, aa2 + d, R21)[0] - rr.host_l2_pair(aa1, aa2 - d, R21)[0]) / (2 * h)
        worst = max(np.abs(J1 - N1).max(), np.abs(J2 - N2).max(), np.abs(K1 - N1).max(), np.abs(K2 - N2).max())
        print("rotations %.1e %.1e residual %.1e: largest difference %.2e, core against reference %.2e" % (scale1, scale2, off, worst, max(np.abs(J1 - K1).max(), np.abs(J2 - K2).max())))
        assert np.abs(r - rr_).max() <= 1e-14 and worst <= 1e-8


def test_what_the_averaging_achieves():
    """10 % outlier pairs (random rotations): the spanning-tree start is off by radians, the L1 stages bring every camera within 6 degrees of the truth (noise 1
    degree per pair) and the L2 stage stays there; noise-free: the start is the truth and stays it, the first IRLS system has infinite weights: info > 0"""
    sc = rr.scenes()["outlier10"]
    h1 = rr.host_l1(sc); h2 = rr.host_l2(sc, h1["rotations"])
    start, after1, after2 = (rr.largest_angle(R, sc["truth"]) for R in (sc["R0"], h1["rotations"], h2["rotations"]))
    print("largest angle to the truth: start %.3f, after L1 %.4f, after L2 %.4f rad" % (start, after1, after2))
    assert start > 0.5 and after1 < np.radians(6) and after2 < np.radians(6) and h1["info"] == 0 and h2["final_cost"] <= h2["initial_cost"]
    sc = rr.scenes()["exact"]
    h1 = rr.host_l1(sc)
    assert h1["info"] > 0 and h1["irls"] == 0 and rr.largest_angle(h1["rotations"], sc["truth"]) < 1e-14


def test_arguments_refused():
    """every PVLM_ERR_ARG case of the host compile leaves the rotations untouched"""
    sc = rr.scenes()["K4"]
    for name, bad in rr.bad_calls(sc):
        h = rr.host_l1(bad)
        assert h["rc"] == -1 and np.array_equal(h["rotations"].view(np.uint64), np.ascontiguousarray(bad["R0"]).view(np.uint64)) and h["l1"] == -7, name
        if "start" not in name:
            h = rr.host_l2(bad, bad["R0"])
            assert h["rc"] == -1 and np.array_equal(h["rotations"].view(np.uint64), np.ascontiguousarray(bad["R0"]).view(np.uint64)), name
    assert rr.host_l2(sc, sc["R0"], max_num_iterations=-1)["rc"] == -1


def test_single_camera_and_no_pairs():
    one = dict(F=1, P=0, first=np.zeros(0, np.int32), second=np.zeros(0, np.int32), R_21=np.zeros((0, 3, 3)), start=0, R0=np.eye(3)[None])
    h = rr.host_l1(one)
    assert h["rc"] == 0 and (h["l1"], h["admm"], h["irls"], h["info"]) == (0, 0, 0, 0) and np.array_equal(h["rotations"][0], np.eye(3))
    h = rr.host_l2(one, one["R0"])
    assert h["rc"] == 0 and h["termination"] == 6 and np.array_equal(h["rotations"][0], np.eye(3))


def test_core_check_under_the_host_sanitizers():
    """tests/cpp/rotavg_core_check.cpp with its own main under -fsanitize=address,undefined (1, 3, 9, 70 and 200 cameras)"""
    from panovlm_amd import build
    out = subprocess.run([build.build_rotavg_check(main=True, sanitize=True)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr


# ---- the host mirror: EstimateGlobalRotation on the host compile (tests/cpp/pvlm_rotavg_driver.cpp) ---------------------------------------------------------------
def test_find_triplet_and_filter_by_triplet():
    """FindTriplet and FilterByTriplet against their plain-Python restatements on the mirror scene (46 pairs, 64 triplets): the pair planted 5 degrees off has no
    triplet that passes 0.1 degrees and is dropped; the pair planted 0.08 degrees off passes (the measure as written reads 0.82 of the angle)"""
    g = rr.mirror_scene()
    edges = [(p["first"], p["second"]) for p in g["pairs"]]
    t = rr.run_driver(g, "triplets")
    assert t["triplets"] == rr.find_triplet_ref(edges) and len(t["triplets"]) == 64
    f = rr.run_driver(g, "filter_triplet", "host", 0.1)
    kept, covered = rr.filter_by_triplet_ref(g["pairs"], 0.1)
    assert f["pairs"] == [(p["first"], p["second"]) for p in kept] and f["covered"] == covered
    assert (8, 10) in edges and (8, 10) not in f["pairs"] and (5, 7) in f["pairs"] and len(f["pairs"]) == len(edges) - 1
    # a loose threshold keeps everything, a pair with first > second is refused (upstream asserts)
    assert rr.run_driver(g, "filter_triplet", "host", 10.0)["pairs"] == edges
    turned = dict(g, pairs=[dict(p, first=p["second"], second=p["first"]) if k == 3 else p for k, p in enumerate(g["pairs"])])
    assert rr.run_driver(turned, "filter_triplet", "host", 10.0)["pairs"] == []


def test_spanning_tree_start():
    """RotationAveragingSpanningTree (Kruskal over the list in list order, walked breadth-first from start_idx) against its Python restatement, bit for bit: products
    of the same two matrices in the same order; a start in the middle, a shuffled list with turned pairs; a list that does not reach every camera is refused"""
    for name, start in (("ring9", 8), ("hub9", 5), ("F65", 32)):
        sc = rr.scenes()[name]
        g = dict(F=sc["F"], R_wc=np.zeros((sc["F"], 3, 3)), t_wc=np.zeros((sc["F"], 3)),
                 pairs=[dict(first=int(sc["first"][p]), second=int(sc["second"][p]), R_21=sc["R_21"][p], t_21=np.zeros(3), upper=0.0, lower=0.0) for p in range(sc["P"])])
        d = rr.run_driver(g, "tree", "host", start)
        want = rr.spanning_tree_start(sc["F"], sc["first"], sc["second"], sc["R_21"], start)
        assert d["ok"] == 1
        worst = max(np.abs(d["rotations"][c] - want[c]).max() for c in range(sc["F"]))
        print(name, "largest difference", worst)
        assert worst <= 4 * np.finfo(np.float64).eps          # numpy's matmul may order the three products of an entry differently
        assert np.array_equal(d["rotations"][start], np.eye(3))
    cut = dict(g, pairs=[p for p in g["pairs"] if 7 not in (p["first"], p["second"])])
    assert rr.run_driver(cut, "tree", "host", 0)["ok"] == 0


def _x84():
    """(difference of the two X84 thresholds, the driver's result, the restatement's, the pairs) on the mirror scene after its L1 stages"""
    g = rr.mirror_scene()
    e = rr.estimate_ref(g)
    assert sorted(e["R_cw"]) == list(range(g["F"]))           # every frame survives the filters: the frames are the cameras
    pairs = [p for p in g["pairs"] if (p["first"], p["second"]) in e["after_triplet"]]
    d = rr.run_driver(dict(g, R_wc=np.array([R.T for R in e["l1_rotations"]]), pairs=pairs), "filter_pairs")
    ref = rr.filter_pairs_ref(pairs, e["l1_rotations"])
    return abs(d["threshold"] - ref[0]), d, ref, pairs


def test_filter_pairs_x84():
    """FilterPairs with the X84 threshold and the frame rule against the Python restatement, on the rotations the averaging gives for the mirror scene: the pair
    planted 0.08 degrees off is dropped, a rejected pair of an end frame comes back by the frame rule.  The threshold within rotavg_ref.TOL["x84"]; no pair error
    within 1 % of the threshold (the scene's own knife edge)."""
    diff, d, (threshold, kept, err), pairs = _x84()
    print("threshold %.6f degrees, difference %.3e rad" % (np.degrees(threshold), diff))
    assert diff <= rr.TOL["x84"]
    assert np.abs(err / threshold - 1).min() > 0.01
    assert d["pairs"] == [(pairs[i]["first"], pairs[i]["second"]) for i in kept]
    assert (5, 7) not in d["pairs"] and len(d["pairs"]) < len(pairs)
    assert any(err[i] >= threshold for i in kept)             # the frame rule took a rejected pair back


def test_estimate_global_rotation_host():
    """EstimateGlobalRotation on the host compile against the Python restatement around the same two solves: the same surviving pairs, the rotations to rounding,
    pair.R_21 = R_2w R_1w^T written back, every rotation within 0.02 degrees of the truth (noise 0.01 degrees per pair); method 2 is refused with a message"""
    g = rr.mirror_scene()
    e = rr.estimate_ref(g)
    d = rr.run_driver(g, "estimate", "host", 1, 1)
    assert d["ok"] == 1 and d["message"] == "" and d["pairs"] == e["pairs"]
    worst = max(rr.angle_between(d["R_wc"][i].T, e["R_cw"][i]) for i in e["R_cw"])
    R0 = g["R_cw_true"][0]
    truth = max(rr.angle_between(d["R_wc"][i].T, g["R_cw_true"][i] @ R0.T) for i in e["R_cw"])
    print("against the restatement %.3e rad, against the truth %.5f degrees" % (worst, np.degrees(truth)))
    assert worst <= rr.TOL["angle_l2"] and np.degrees(truth) < 0.02
    for (i, j), R21 in zip(d["pairs"], d["R_21"]):
        assert np.abs(R21 - d["R_wc"][j].T @ d["R_wc"][i]).max() <= 4 * np.finfo(np.float64).eps
    bad = rr.run_driver(g, "estimate", "host", 2, 1)
    assert bad["ok"] == 0 and "not supported" in bad["message"]


def test_rotation_then_translation():
    """the point of K40: image pairs to camera poses without leaving the library.  EstimateGlobalRotation, then the existing EstimateGlobalTranslation (method 1) on
    its frames and pairs: every frame gets a pose; the centres equal the truth up to the one scale translation averaging leaves free inside its bounds
    [0.9, 1.3], within 2 mm in an 8 m scene (rotations 0.01 degrees off turn an 8 m baseline by 1.4 mm)"""
    g = rr.mirror_scene()
    c = rr.run_driver(g, "chain", "host", 1, 1)
    assert c["ok"] == 1 and c["translation_ok"] == 1, (c["message"], c["translation_message"])
    assert all(c["valid"][i] == 1 for i in range(g["F"]))
    s, worst = rr.chain_error(g, c)
    print("scale %.4f, largest centre error %.5f m" % (s, worst))
    assert 0.9 - 1e-6 <= s <= 1.3 + 1e-6 and worst < 2e-3
