"""GPU checks of K49 through the C ABI (pvlm_mvs_select_neighbors_sfm, pvlm_mvs_neighbor_sfm_score_row) and through the host mirror's device route
(tests/cpp/pvlm_neighbor_driver.cpp), against the literal host loop of csrc/pvlm_neighbor_sfm_core.h (the host mirror's host route): neighbour ids and counts equal on
every row, R_nr / t_nr equal to the bit, every accepted score and every read-back row within (n + 2) * 2^-23 * score of the host loop's.  On the scenes of
neighbor_sfm_ref.CERTAIN the device must decide every row itself (n_uncertain == 0), so the host fall-back cannot hide a wrong kernel."""
import os

import numpy as np
import pytest

from tests import neighbor_sfm_ref as nr

pytestmark = pytest.mark.gpu

ERR_ARG = -1      # pvlm_status


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


class _env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k in self.kw:
            del os.environ[k]


def _select(ctx, sc, K, threshold, **kw):
    from panovlm_amd import api
    off, views, pts = nr.csr(sc)
    d = api.mvs_select_neighbors_sfm(ctx, sc["T_wc"], sc["valid"], off, views[:off[-1]], pts, K, threshold, **kw)
    assert d["guard_intact"]
    return d


def _row(ctx, sc, row):
    from panovlm_amd import api
    off, views, pts = nr.csr(sc)
    return api.mvs_neighbor_sfm_score_row(ctx, sc["T_wc"], sc["valid"], off, views[:off[-1]], pts, row)


_HOST = {}


def _host(name, K, threshold):
    """the literal host loop on a named scene, computed once"""
    key = (name, K, threshold)
    if key not in _HOST:
        _HOST[key] = nr.host_select(nr.scenes()[name], K, threshold)
        assert _HOST[key]["rc"] == 0
    return _HOST[key]


def _assert_equals_host(d, h, sc):
    assert d["rc"] == 0
    assert np.array_equal(d["n_neighbors"], h["n_neighbors"]) and np.array_equal(d["ids"], h["ids"])
    assert np.array_equal(d["R_nr"].view(np.uint32), h["R_nr"].view(np.uint32)) and np.array_equal(d["t_nr"].view(np.uint32), h["t_nr"].view(np.uint32))
    counts = {}
    for r in range(sc["F"]):
        for j in range(int(h["n_neighbors"][r])):
            if r not in counts:
                counts[r] = nr.host_row(sc, r)[1]
            assert abs(float(d["scores"][r, j]) - float(h["scores"][r, j])) <= nr.bound(h["scores"][r, j], counts[r][h["ids"][r, j]]), (r, j)
        assert np.all(d["scores"][r, int(h["n_neighbors"][r]):] == 0)
    for k in ("n_candidates", "n_contributions", "n_repeat_tracks"):
        assert d[k] == h[k], k


def test_tile_constant(ctx):
    from panovlm_amd import api
    assert api.neighbor_sfm_tile_cols() == nr.TILE_COLS


@pytest.mark.parametrize("name,K,threshold", nr.CERTAIN)
def test_device_equals_the_host_loop_and_decides_every_row(ctx, name, K, threshold):
    """five views; 70 views with 3 000 tracks and one track of all 70 views (more partners than a wave has lanes), neighbor_size 8 and 100 (more than any row has);
    a view with more lane items than one pass takes; tracks that repeat a view; rows with none and with fewer than neighbor_size candidates; the threshold quirk"""
    sc = nr.scenes()[name]
    d = _select(ctx, sc, K, threshold)
    _assert_equals_host(d, _host(name, K, threshold), sc)
    assert d["n_uncertain"] == 0


@pytest.mark.parametrize("name,K,threshold", [("random70", 8, 0.5), ("repeat-random", 4, 0.25)])
def test_column_tile_of_32_changes_nothing(ctx, name, K, threshold):
    sc = nr.scenes()[name]
    whole = _select(ctx, sc, K, threshold)
    with _env(PVLM_NEIGHBOR_TILE="32"):
        tiled = _select(ctx, sc, K, threshold)
        row = _row(ctx, sc, sc["F"] - 1)
    for k in whole:
        assert np.array_equal(np.asarray(whole[k]), np.asarray(tiled[k])), k
    assert tiled["n_uncertain"] == 0
    one = _row(ctx, sc, sc["F"] - 1)
    assert np.array_equal(row[0].view(np.uint32), one[0].view(np.uint32)) and np.array_equal(row[1], one[1])


@pytest.mark.parametrize("name,row", [("five", 0), ("five", 4), ("random70", 0), ("random70", 37), ("random70", 69), ("busy", 0), ("repeat", 1), ("repeat-random", 3)])
def test_read_back_row_is_within_the_bound(ctx, name, row):
    sc = nr.scenes()[name]
    s, n = _row(ctx, sc, row)
    hs, hn = nr.host_row(sc, row)
    assert np.array_equal(n, hn)
    assert np.array_equal(s > 0, hs > 0)
    assert np.all(np.abs(s.astype(np.float64) - hs) <= [nr.bound(v, c) for v, c in zip(hs, hn)])


def test_five_view_row_where_the_scores_are_exact(ctx):
    s, _ = _row(ctx, nr.scenes()["five"], 0)
    assert s[1] == 1.0 and s[2] == np.float32(1.6 * 1.6 / 2.0 / 2.0) and s[0] == 0 and s[4] == 0


def test_repeated_view_on_the_device(ctx):
    sc = nr.scenes()["repeat"]
    d = _select(ctx, sc, 4, -1.0)
    assert d["n_repeat_tracks"] == 1 and d["n_uncertain"] == 0
    assert list(d["ids"][1]) == [2, 0, 3, 1]                   # its own neighbour through the diagonal cell
    s, n = _row(ctx, sc, 1)
    assert n[1] == 2 and s[1] > 0


@pytest.mark.parametrize("name", ["tie", "near-tie"])
def test_near_tie_goes_to_the_host_and_equals_it(ctx, name):
    sc = nr.scenes()[name]
    d = _select(ctx, sc, 3, 0.0)
    assert d["n_uncertain"] >= 1
    h = _host(name, 3, 0.0)
    _assert_equals_host(d, h, sc)
    assert np.array_equal(d["scores"][0].view(np.uint32), h["scores"][0].view(np.uint32))      # row 0 is the host's own


def test_norm_next_to_the_threshold_goes_to_the_host(ctx):
    sc = nr.scenes()["distance"]
    d = _select(ctx, sc, 3, 5.0)                                # view 2 lies at distance 5 of view 0, to the bit
    assert d["n_uncertain"] >= 1
    _assert_equals_host(d, nr.host_select(sc, 3, 5.0), sc)


def test_refusals_touch_nothing(ctx):
    sc = nr.scenes()["five"]
    bad = dict(sc, valid=np.array([1, 1, 0, 1, 1], np.uint8))
    d = _select(ctx, bad, 2, 0.0, check=False)
    assert d["rc"] == ERR_ARG and np.all(d["n_neighbors"] == -7) and np.all(d["ids"] == -7) and d["n_uncertain"] == -7
    far = dict(sc, tracks=sc["tracks"] + [(np.zeros(3), [(1, 9), (5, 0)])])
    assert _select(ctx, far, 2, 0.0, check=False)["rc"] == ERR_ARG
    unsorted_views = dict(sc, tracks=[(X, obs[::-1]) for X, obs in sc["tracks"]])
    assert _select(ctx, unsorted_views, 2, 0.0, check=False)["rc"] == ERR_ARG
    assert _select(ctx, sc, -1, 0.0, check=False)["rc"] == ERR_ARG
    assert _select(ctx, sc, 2, float("nan"), check=False)["rc"] == ERR_ARG


def test_mirror_device_route_equals_its_host_route(ctx):
    sc = nr.scenes()["random70"]
    dev = nr.run_driver(sc, "sfm", "device", 8, 0.5)
    host = nr.run_driver(sc, "sfm", "host", 8, 0.5)
    assert dev["ok"] == 1 and host["ok"] == 1 and dev["stats"]["n_uncertain"] == 0
    for a, b in zip(dev["rows"], host["rows"]):
        assert a["ids"] == b["ids"] and a["R_nr"] == b["R_nr"] and a["t_nr"] == b["t_nr"]
    assert {k: v for k, v in dev["stats"].items() if k != "n_uncertain"} == {k: v for k, v in host["stats"].items() if k != "n_uncertain"}
    views = nr.run_driver(nr.scenes()["distance"], "views", "device", 3, 1, 2.0)
    assert views["ok"] == 1 and views["rows"][0]["ids"] == [2]
