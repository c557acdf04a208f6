"""K48 without a GPU: the host compile of csrc/pvlm_triplet_core.h (tests/cpp/triplet_core_check.cpp) against find_triplet_ref and the literal triplet test of
tests/rotavg_ref.py on the scenes of tests/triplet_ref.py, the capacity rule, every argument refusal, and the host mirror's FindTripletDevice /
FilterByTripletDevice on the host-compile route through tests/cpp/pvlm_triplet_driver.cpp."""
import ctypes as C

import numpy as np
import pytest

from tests import rotavg_ref as rr
from tests import triplet_ref as tr

NAMES = list(tr.scenes())


def test_constants_are_the_cores():
    lib = tr.check_lib()
    assert lib.chk_triplet_group_size() == tr.GROUP
    assert lib.chk_triplet_band() == tr.BAND


@pytest.mark.parametrize("name", NAMES)
def test_find_equals_the_reference(name):
    sc, r = tr.scenes()[name], tr.reference(name)
    f = tr.host_find(sc["F"], sc["first"], sc["second"])
    assert f["rc"] == 0 and f["needed"] == len(r["triplets"]) and f["guard_intact"]
    assert np.array_equal(f["triplets"], r["triplets"])
    assert np.array_equal(f["triplet_pairs"], r["triplet_pairs"])
    assert np.array_equal(f["pair_counts"], r["pair_counts"]) and int(f["pair_counts"].sum()) == f["needed"]
    # the caller-index contract, from the list itself: the three pairs are (i,j), (j,k), (i,k)
    t, tp = f["triplets"], f["triplet_pairs"]
    if len(t):
        assert np.array_equal(sc["first"][tp[:, 0]], t[:, 0]) and np.array_equal(sc["second"][tp[:, 0]], t[:, 1])
        assert np.array_equal(sc["first"][tp[:, 1]], t[:, 1]) and np.array_equal(sc["second"][tp[:, 1]], t[:, 2])
        assert np.array_equal(sc["first"][tp[:, 2]], t[:, 0]) and np.array_equal(sc["second"][tp[:, 2]], t[:, 2])


def test_shuffled_list_shows_the_caller_index_contract():
    sc = tr.scenes()["K4-shuffled"]
    key = sc["first"].astype(np.int64) * sc["F"] + sc["second"]
    assert np.any(np.diff(key) < 0)                     # the list is not in rank order
    f = tr.host_find(sc["F"], sc["first"], sc["second"])
    g = tr.host_find(sc["F"], np.sort(key) // sc["F"], np.sort(key) % sc["F"])
    assert np.array_equal(f["triplets"], g["triplets"]) and not np.array_equal(f["triplet_pairs"], g["triplet_pairs"])


@pytest.mark.parametrize("name", NAMES)
def test_filter_equals_the_reference(name):
    sc, r = tr.scenes()[name], tr.reference(name)
    h = tr.host_filter(sc["F"], sc["first"], sc["second"], sc["R_21"], sc["threshold"])
    assert h["rc"] == 0 and h["guard_intact"]
    assert np.array_equal(h["keep"], r["keep"])
    assert (h["n_triplets"], h["n_kept_triplets"], h["n_kept_pairs"]) == (len(r["triplets"]), r["n_kept_triplets"], int(r["keep"].sum()))
    if sc["planted"]:
        assert h["n_uncertain"] >= 1
    else:
        assert h["n_uncertain"] == 0


def test_keep_is_the_pair_set_of_filter_by_triplet_ref_before_its_biconnected_step():
    """on the mirror scene the biconnected step removes nothing more, so filter_by_triplet_ref's list is the keep bytes' pair set"""
    sc = tr.scenes()["mirror"]
    g = rr.mirror_scene()
    left, _ = rr.filter_by_triplet_ref(g["pairs"], 0.1)
    h = tr.host_filter(sc["F"], sc["first"], sc["second"], sc["R_21"], 0.1)
    assert [(p["first"], p["second"]) for p in left] == [(int(sc["first"][p]), int(sc["second"][p])) for p in range(sc["P"]) if h["keep"][p]]
    assert 0 < h["keep"].sum() < sc["P"]


def test_thresholds_at_the_ends():
    sc = tr.scenes()["noisy"]
    n = len(tr.reference("noisy")["triplets"])
    for thr, kept in ((0.0, 0), (-3.0, 0), (180.5, n), (1e9, n)):
        h = tr.host_filter(sc["F"], sc["first"], sc["second"], sc["R_21"], thr)
        assert h["rc"] == 0 and h["n_kept_triplets"] == kept and h["n_uncertain"] == 0, thr


def test_measure_is_the_reference_measure():
    """c against numpy's, and the literal decision against triplet_angle_deg, on the triplets of the noisy scene"""
    sc, r = tr.scenes()["noisy"], tr.reference("noisy")
    lib = tr.check_lib()
    out = np.zeros(3)
    for (a, b, c), c_ref, kept in zip(r["triplet_pairs"], r["c"], r["kept"]):
        R = [np.ascontiguousarray(sc["R_21"][k]) for k in (a, b, c)]
        lib.chk_triplet_measure(tr._p(R[0]), tr._p(R[1]), tr._p(R[2]), C.c_double(sc["threshold"]), tr._p(out))
        # each side rounds at most 9 times on the way to c (product, two sums per 3-term dot, twice nested; two sums of the trace; the division) over terms
        # whose absolute values add up to at most sqrt(3) per unit of c: 2 sides x 9 x 2^-53 x sqrt(3)
        assert abs(out[0] - c_ref) <= 2 * 9 * 2.0 ** -53 * np.sqrt(3.0)
        assert out[2] == float(kept) and out[1] == float(kept)


def test_nan_rotation_is_kept_as_the_mirror_keeps_it():
    sc = tr.scenes()["triangle"]
    R = sc["R_21"].copy(); R[1, 0, 2] = np.nan
    assert rr.triplet_angle_deg(R[0], R[1], R[2]) == 0.0           # min(1.0, max(nan, -1.0)) is 1.0
    for thr in (sc["threshold"], 1e-6):
        h = tr.host_filter(sc["F"], sc["first"], sc["second"], R, thr)
        assert h["rc"] == 0 and h["keep"].tolist() == [1, 1, 1] and h["n_kept_triplets"] == 1


def test_capacity_rule():
    sc, r = tr.scenes()["noisy"], tr.reference("noisy")
    n = len(r["triplets"])
    for cap in (n - 1, 1, 0):
        f = tr.host_find(sc["F"], sc["first"], sc["second"], capacity=cap)
        assert f["rc"] == -5 and f["needed"] == n and f["guard_intact"]
        assert np.array_equal(f["triplets"], r["triplets"][:cap]) and np.array_equal(f["triplet_pairs"], r["triplet_pairs"][:cap])
        assert np.array_equal(f["pair_counts"], r["pair_counts"])
    f = tr.host_find(sc["F"], sc["first"], sc["second"], capacity=n + 5)
    assert f["rc"] == 0 and f["guard_intact"] and np.array_equal(f["triplets"], r["triplets"])
    # one output alone; no output: a count, whatever the capacity
    f = tr.host_find(sc["F"], sc["first"], sc["second"], want_triplets=False, capacity=n)
    assert f["rc"] == 0 and f["triplets"] is None and np.array_equal(f["triplet_pairs"], r["triplet_pairs"])
    f = tr.host_find(sc["F"], sc["first"], sc["second"], want_triplets=False, want_pairs=False, capacity=0, want_counts=False)
    assert f["rc"] == 0 and f["needed"] == n


def test_argument_refusals_write_nothing():
    sc = tr.scenes()["noisy"]
    for what, first, second, thr in tr.bad_calls(sc):
        f = tr.host_find(sc["F"], first, second, capacity=400)
        assert f["rc"] == -1 and f["untouched"], what
        h = tr.host_filter(sc["F"], first, second, sc["R_21"], thr)
        assert h["rc"] == -1 and h["untouched"], what
    for thr in (np.nan, np.inf, -np.inf):
        h = tr.host_filter(sc["F"], sc["first"], sc["second"], sc["R_21"], thr)
        assert h["rc"] == -1 and h["untouched"], thr
    for null in ("R", "keep", "stats"):
        h = tr.host_filter(sc["F"], sc["first"], sc["second"], sc["R_21"], 2.0, null=(null,))
        assert h["rc"] == -1 and h["untouched"], null
    f = tr.host_find(sc["F"], sc["first"], sc["second"], capacity=-1)
    assert f["rc"] == -1 and f["untouched"]
    f = tr.host_find(sc["F"], sc["first"], sc["second"], capacity=400, needed_ptr=False)
    assert f["rc"] == -1 and f["untouched"]
    f = tr.host_find(-1, sc["first"], sc["second"], capacity=400)
    assert f["rc"] == -1 and f["untouched"]


def test_stand_alone_program_under_the_host_sanitizers():
    import subprocess
    from panovlm_amd import build
    exe = build.build_triplet_check(main=True, sanitize=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "triplets 54740" in res.stdout and "bad 1" not in res.stdout


def _ints(lines):
    return np.array([[int(v) for v in ln.split()] for ln in lines], np.int64).reshape(-1, 3)


@pytest.mark.parametrize("name", ["K4-shuffled", "gaps", "mirror", "noisy"])
def test_mirror_find_triplet_device_on_the_host_route(name):
    sc, r = tr.scenes()[name], tr.reference(name)
    d = tr.run_driver(tr.scene_graph(sc), "find", "host")["lines"]
    assert np.array_equal(_ints(d["triplet"]), _ints(d["ref_triplet"])) and np.array_equal(_ints(d["triplet"]), r["triplets"])
    assert np.array_equal(_ints(d["tpairs"]), _ints(d["ref_tpairs"]))


def _pairs(d):
    return [ln.split() for ln in d["lines"].get("pair", [])]


@pytest.mark.parametrize("name", ["mirror", "noisy", "planted"])
def test_mirror_filter_by_triplet_device_on_the_host_route(name):
    """FilterByTriplet and FilterByTripletDevice on a list that names one pair twice: the last rotation wins, and every list entry of a kept pair survives"""
    sc = tr.scenes()[name]
    for p, R in ((0, sc["R_21"][0]), (sc["P"] // 2, rr.exp_so3(np.array([0.0, 0.3, 0.0])) @ sc["R_21"][sc["P"] // 2])):
        g = tr.scene_graph(sc, duplicate=(p, R))
        a = tr.run_driver(g, "filter", "host", sc["threshold"], 0)
        b = tr.run_driver(g, "filter", "host", sc["threshold"], 1)
        assert _pairs(a) == _pairs(b) and a["lines"].get("covered") == b["lines"].get("covered")
        assert len(_pairs(b)) > 0
        named = [(w[0], w[1]) for w in _pairs(b)]
        twice = (str(int(sc["first"][p])), str(int(sc["second"][p])))
        assert named.count(twice) in (0, 2)
    st = [int(v) for v in b["lines"]["stats"][0].split()]
    assert st[0] == len(tr.reference(name)["triplets"])
    if sc["planted"]:
        assert st[2] >= 1


def test_mirror_estimate_global_rotation_host_with_and_without_the_flag():
    g = rr.mirror_scene()
    for p in g["pairs"]:
        p.setdefault("upper", 0.0); p.setdefault("lower", 0.0)
    a = tr.run_driver(g, "estimate", "host", 1, 0)
    b = tr.run_driver(g, "estimate", "host", 1, 1)
    assert a["ok"] == 1 and b["ok"] == 1
    assert a["lines"]["pair"] == b["lines"]["pair"] and a["lines"]["frame"] == b["lines"]["frame"]
