"""K49 without a GPU: the literal host loop of csrc/pvlm_neighbor_sfm_core.h (tests/cpp/neighbor_sfm_core_check.cpp) and the host mirror's SelectNeighborSFM /
SelectNeighborViews on the host route (tests/cpp/pvlm_neighbor_driver.cpp) against the Python restatement of tests/neighbor_sfm_ref.py.

The host loop and the reference share libm's acos; numpy's float32 power need not be glibc's powf to the bit, so scores are compared within the core's bound
((n + 2) * 2^-23 * score) except where they are exact by construction."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import neighbor_sfm_ref as nr


def test_constants_are_the_cores():
    lib = nr.check_lib()
    assert lib.chk_ns_norm_band() == nr.NORM_BAND
    assert lib.chk_ns_bound(C.c_float(3.0), C.c_int(5)) == nr.bound(3.0, 5)
    # float += double rounds once, from the double sum
    assert lib.chk_ns_add_to_cell(C.c_float(1.0), C.c_double(2.0 ** -24 + 2.0 ** -40)) == np.float32(1.0 + 2.0 ** -23)


def test_five_views_by_hand():
    sc, r = nr.scenes()["five"], nr.reference("five", 2, 0.0)
    h = nr.host_select(sc, 2, 0.0)
    assert h["rc"] == 0 and h["guard_intact"]
    rows = [nr.host_row(sc, v)[0] for v in range(5)]
    S = np.array(rows)
    # a saturates at 1; the three branches of f: 1 (equal depths), 1.6^2 / 2 / 2 and 0.5^2
    assert S[0, 1] == 1.0 and S[1, 0] == 1.0
    assert S[0, 2] == np.float32(1.6 * 1.6 / 2.0 / 2.0) and S[2, 0] == 0.25
    # rays atan(0.05) apart: a = (angle in degrees / 10)^1.5 < 1, f = (10 / sqrt(100.25))^2 one way and 1 the other
    a = (math.degrees(math.atan(0.05)) / 10.0) ** 1.5
    assert a < 1 and abs(S[3, 0] - a) <= 2 * nr.F32_EPS * a and abs(S[0, 3] - a * 100.0 / 100.25) <= 2 * nr.F32_EPS * a
    # the point on the line through both centres: cosine 1, angle 0, no contribution, no candidate
    assert S[1, 4] == 0 and S[4, 1] == 0 and int((S > 0).sum()) == 6 == h["n_candidates"]
    assert np.array_equal(S, r["score"]) or np.all(np.abs(S - r["score"]) <= 3 * nr.F32_EPS * r["score"])
    # row 0 takes its two best, rows 1 to 3 have fewer than neighbor_size, row 4 none
    assert list(h["n_neighbors"]) == [2, 1, 1, 1, 0] and list(h["ids"][0]) == [1, 2] and list(h["ids"][4]) == [-1, -1]
    nr.assert_equals_reference(h, r, sc, 2)


@pytest.mark.parametrize("name,K,threshold", nr.CERTAIN)
def test_host_loop_equals_the_reference(name, K, threshold):
    sc, r = nr.scenes()[name], nr.reference(name, K, threshold)
    h = nr.host_select(sc, K, threshold)
    assert h["rc"] == 0 and h["guard_intact"] and h["n_uncertain"] == 0
    nr.assert_equals_reference(h, r, sc, K)


@pytest.mark.parametrize("name,K,threshold", nr.CERTAIN)
def test_fixtures_show_no_uncertain_row(name, K, threshold):
    """the scenes on which the GPU tests demand n_uncertain == 0 show none in the reference's own numbers, by the same bound"""
    assert nr.reference(name, K, threshold)["stats"]["n_uncertain"] == 0


@pytest.mark.parametrize("name,row", [("random70", 0), ("random70", 69), ("busy", 0), ("repeat", 1), ("repeat-random", 3)])
def test_row_form_equals_the_dense_loop(name, row):
    """the row restricted to the view's own tracks — what an uncertain row falls back to — is the dense loop's row, counts included"""
    sc, r = nr.scenes()[name], nr.reference(name, 1, 0.0)
    s, n = nr.host_row(sc, row)
    assert np.array_equal(n, r["count"][row])
    assert np.all(np.abs(s.astype(np.float64) - r["score"][row]) <= [nr.bound(v, c) for v, c in zip(r["score"][row], r["count"][row])])
    assert np.array_equal(s > 0, r["score"][row] > 0)


def test_neighbor_size_larger_than_any_row():
    sc, r = nr.scenes()["random70"], nr.reference("random70", 100, 0.0)
    h = nr.host_select(sc, 100, 0.0)
    assert int(h["n_neighbors"].max()) == 69 and all(len(x["ids"]) == 69 for x in r["rows"])      # every other view, never the view itself


def test_equal_scores_go_by_column_descending():
    sc, r = nr.scenes()["tie"], nr.reference("tie", 3, 0.0)
    s, _ = nr.host_row(sc, 0)
    assert s[1] == s[2] > 0                                    # mirrored geometry: equal to the bit
    h = nr.host_select(sc, 3, 0.0)
    assert list(h["ids"][0]) == [3, 2, 1] == r["rows"][0]["ids"]
    assert r["rows"][0]["uncertain"]                           # and the certainty test sees it


def test_near_tie_is_seen_by_the_certainty_test():
    r = nr.reference("near-tie", 3, 0.0)
    assert r["rows"][0]["uncertain"] and r["stats"]["n_uncertain"] >= 1


def test_repeated_view_reaches_the_diagonal():
    sc, r = nr.scenes()["repeat"], nr.reference("repeat", 4, -1.0)
    assert r["stats"]["n_repeat_tracks"] == 1
    assert r["count"][1, 1] == 2 and r["score"][1, 1] > 0      # (1, 1) of the one track: both of its products land in the diagonal cell
    assert r["count"][0, 1] == 2 and r["count"][2, 1] == 3     # the track adds twice to the cells of its other views ((1, 2) has one more track)
    h = nr.host_select(sc, 4, -1.0)
    assert list(h["ids"][1]) == [2, 0, 3, 1]                   # view 1 is its own (last) neighbour, as upstream has it
    nr.assert_equals_reference(h, r, sc, 4)


def test_the_norm_is_compared_with_the_squared_threshold():
    """min_distance = 2 gives the threshold 4: the best-scored partner at distance 3 is dropped, the one at 5 is kept"""
    sc = nr.scenes()["distance"]
    out = nr.run_driver(sc, "views", "host", 3, 1, 2.0)
    assert out["ok"] == 1 and out["rows"][0]["ids"] == [2]
    nr.assert_driver_equals_reference(out, nr.reference("distance", 3, 4.0))
    free = nr.run_driver(sc, "views", "host", 3, 1, 0.0)
    assert free["rows"][0]["ids"] == [1, 2, 3]


def test_mirror_host_route_equals_the_reference():
    sc, r = nr.scenes()["random70"], nr.reference("random70", 8, 0.5)
    out = nr.run_driver(sc, "sfm", "host", 8, 0.5)
    assert out["ok"] == 1 and out["stats"]["n_contributions"] == r["stats"]["n_contributions"] and out["stats"]["n_uncertain"] == 0
    nr.assert_driver_equals_reference(out, r)


def test_select_neighbor_views_dispatch():
    sc = nr.scenes()["five"]
    sfm = nr.run_driver(sc, "views", "host", 2, 1, 0.0)
    assert sfm["ok"] == 1 and [x["ids"] for x in sfm["rows"]] == [[1, 2], [0], [0], [0], []]
    knn = nr.run_driver(sc, "views", "host", 2, 2, 0.0)
    assert knn["ok"] == 1 and [x["ids"] for x in knn["rows"]][:2] == [[3, 1], [3, 0]] and len(knn["rows"][4]["ids"]) == 2      # nearest centres, not shared tracks
    unknown = nr.run_driver(sc, "views", "host", 2, 3, 0.0)
    assert unknown["ok"] == 0 and [x["ids"] for x in unknown["rows"]] == [[]] * 5
    empty = dict(sc, tracks=[])
    assert nr.run_driver(empty, "views", "host", 2, 1, 0.0)["ok"] == 0          # "SfM points are empty"
    assert nr.run_driver(empty, "views", "host", 2, 2, 0.0)["ok"] == 1          # the nearest-centre method needs no structure


def test_invalid_pose_view_is_refused():
    sc = nr.scenes()["five"]
    bad = dict(sc, valid=np.array([1, 1, 0, 1, 1], np.uint8))
    h = nr.host_select(bad, 2, 0.0)
    assert h["rc"] == -1 and h["untouched"]
    out = nr.run_driver(bad, "sfm", "host", 2, 0.0)
    assert out["ok"] == 0 and [x["ids"] for x in out["rows"]] == [[]] * 5
    # a view without a pose that no track names is no obstacle
    lonely = dict(sc, valid=np.array([1, 1, 1, 1, 0], np.uint8), tracks=sc["tracks"][:3])
    assert nr.host_select(lonely, 2, 0.0)["rc"] == 0
    # an image id past the frames
    far = dict(sc, tracks=sc["tracks"] + [(np.zeros(3), [(1, 9), (5, 0)])])
    assert nr.host_select(far, 2, 0.0)["rc"] == -1 and nr.run_driver(far, "sfm", "host", 2, 0.0)["ok"] == 0
