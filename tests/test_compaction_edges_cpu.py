"""Without a GPU: the constants of tests/compact_edges.py parse; the numpy restatements of K33 and K34 agree with the host compiles at the multi-tile shapes of
tests/test_compaction_edges_gpu.py (so "GPU equals host compile" there rests on a checked reference); and the inputs of those GPU tests, by the reference alone,
put kept records on both sides of every tile edge."""
import numpy as np
import pytest

from tests import compact_edges as ce
from tests import essential_ref as er
from tests import match_ref as mr


@pytest.fixture(scope="module")
def mchk():
    return mr.build_check()


@pytest.fixture(scope="module")
def echk():
    return er.build_check()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_records(a, b):
    return len(a) == len(b) and np.array_equal(a["query"], b["query"]) and np.array_equal(a["train"], b["train"]) and np.array_equal(_bits(a["distance"]), _bits(b["distance"]))


def test_constants_parse_from_the_sources():
    assert ce.TILE == ce.THREADS * ce.ROUNDS and ce.TILE > ce.THREADS >= 64 and ce.SCAN >= 64
    assert ce.EXACT_ITEMS == 4 * ce.EXACT_GRID > 0 and ce.FALLBACK_ITEMS == 4 * ce.FALLBACK_GRID > 0 and ce.SCREEN_Q > 0
    # what the one-batch / one-piece shapes of the GPU tests need
    assert ce.MATCH_BATCH_PAIRS > 2 * ce.SCAN + 16 and ce.MATCH_BATCH_QUERIES > ce.EXACT_ITEMS + 5
    assert ce.ESS_BATCH_CHAINS > 2 * ce.SCAN + 16 and ce.PIECE_SCANS > 2 * ce.SCAN + 1 and ce.PIECE_PAIRS > 2 * ce.SCAN + 1
    assert ce.PIECE_POINTS > 300 * (2 * ce.SCAN + 1)
    with pytest.raises(ValueError):
        ce._one("pvlm_compact.h", r"constexpr int kNoSuchConstant = (\d+);")
    assert ce.edge_rows(ce.TILE + 1) == [ce.TILE - 2, ce.TILE - 1, ce.TILE]
    assert ce.rounds_at_edges(ce.TILE + 1) == [(ce.TILE - ce.THREADS, ce.TILE), (ce.TILE, ce.TILE + 1)] and ce.rounds_at_edges(ce.TILE - 1) == []


def test_matmul_d2_equals_the_cube():
    A, B = mr.int_descriptors(np.random.default_rng(1), 127, 129)
    assert np.array_equal(mr.d2_matrix_int(A, B), mr.d2_matrix(A, B, np.int64))
    A[:] = 255; B[:] = 0
    assert (mr.d2_matrix_int(A, B) == 128 * 255 * 255).all()


@pytest.mark.parametrize("n1", [ce.TILE + 1, 2 * ce.TILE + 1])
def test_match_restatement_equals_host_compile_past_one_tile(mchk, n1):
    rng = np.random.default_rng(1000 + 37 * n1 + ce.MATCH_N2)
    A, B = mr.int_descriptors(rng, n1, ce.MATCH_N2)
    idx, dist = mr.host_knn2(mchk, A, B)
    ridx, rdist = mr.ref_knn2_int(A, B)
    assert np.array_equal(idx, ridx) and np.array_equal(_bits(dist), _bits(rdist))
    for ratio in (0.8, 1.0):
        rm = mr.ref_match_sift(ridx, rdist, ratio)
        assert _same_records(mr.host_match_sift(mchk, A, B, ratio), rm) and len(rm) > n1 // 8
        for thr in (0, 5, len(rm) + 1):
            rc, keep, off, rec = mr.host_match_pairs(mchk, [A, B], [0], [1], ratio, thr)
            rkeep, rgood = mr.ref_pair_filter(rm, thr)
            assert rc == 0 and bool(keep[0]) == rkeep == (thr <= 5) and _same_records(rec, rgood) and off[1] == len(rgood)


@pytest.mark.parametrize("n1", ce.MATCH_EDGE_N1)
def test_match_edge_inputs_keep_records_on_both_sides_of_every_tile_edge(mchk, n1):
    """the inputs of the GPU tile-edge test, by the numpy restatement alone (and the host compile agrees with it)"""
    A, B = ce.match_edge_descriptors(n1)
    ridx, rdist = mr.ref_knn2_int(A, B)
    rkeep, rgood = mr.ref_pair_filter(mr.ref_match_sift(ridx, rdist, 0.8), 5)
    assert rkeep and ce.match_edges_reached(rgood["query"], n1)
    assert 0 < len(rgood) < n1 // 4                                  # most queries are dropped: ranks differ from query numbers everywhere
    rc, keep, off, rec = mr.host_match_pairs(mchk, [A, B], [0], [1], 0.8, 5)
    assert rc == 0 and keep[0] == 1 and _same_records(rec, rgood)


def test_essential_restatement_equals_host_compile_past_one_tile(echk):
    n = ce.TILE + 1
    b1, b2, m = ce.essential_edge_scene(n)
    r = er.run_chain(b1, b2, m, ce.ESS_SEED, 0, 1, 0, ce.ESS_ITERS)
    h = er.host_chain(echk, b1, b2, m, ce.ESS_SEED, 0, 1, 0, ce.ESS_ITERS)
    print("n = %d: %d iterations, minNFA %.12g (numpy %.12g), smallest gap %.3g, %d inliers" % (n, h["iterations"], h["nfa"], r["nfa"], r["gap"], len(r["inliers"])))
    assert r["gap"] > 1e-9
    assert [k for k, _ in h["betters"]] == [k for k, _ in r["betters"]] and len(h["betters"]) > 0
    assert h["iterations"] == r["iterations"]
    assert h["inliers"].tolist() == r["inliers"].tolist() and len(r["inliers"]) > ce.TILE // 2
    ref = er.filter_pair(b1, b2, m, ce.ESS_SEED, 0, 1, ce.ESS_RUNS, ce.ESS_ITERS, ce.ESS_TRI)
    rc, f = er.host_filter(echk, [b1, b2], [0], [1], [0, n], m, ce.ESS_TRI, ce.ESS_RUNS, ce.ESS_ITERS, ce.ESS_SEED)
    assert rc == 0 and f["keep"][0] == ref["keep"] == 1
    assert np.array_equal(f["inlier_idx"], ref["inlier_idx"])
    assert ce.essential_edges_reached(ref["inlier_idx"], n)


@pytest.mark.parametrize("n", ce.ESS_EDGE_N)
def test_essential_edge_inputs_keep_inliers_on_both_sides_of_every_tile_edge(echk, n):
    """the inputs of the GPU tile-edge test, by the host compile alone"""
    b1, b2, m = ce.essential_edge_scene(n)
    rc, f = er.host_filter(echk, [b1, b2], [0], [1], [0, n], m, ce.ESS_TRI, ce.ESS_RUNS, ce.ESS_ITERS, ce.ESS_SEED)
    assert rc == 0 and f["keep"][0] == 1 and ce.essential_edges_reached(f["inlier_idx"], n)
    assert len(f["inlier_idx"]) < n                                  # some matches are dropped: ranks differ from match numbers
    second = f["inlier_idx"][f["inlier_idx"] >= ce.TILE]
    assert n == ce.TILE or len(second) > 0


def test_fuse_and_colorize_edge_inputs_mix_kept_and_dropped_rows_at_every_tile_edge():
    """the inputs of the K29 / K30 tile-edge tests: their builders assert, by the numpy restatements alone, that the rows e - 1, e and n - 1 are kept and the rows
    e - 2, e + 1 and n - 2 dropped; and the scan-trip inputs of K34 are of one batch"""
    from tests import test_compaction_edges_gpu as g
    clouds, poses = g._fuse_edge_clouds()
    assert [len(c) for c in clouds[-len(g.EDGE_SIZES):]] == g.EDGE_SIZES
    clouds, Ts, images = g._colorize_edge_pairs()
    assert [len(c) for c in clouds[-len(g.EDGE_SIZES):]] == g.EDGE_SIZES and all(T is not None for T in Ts[-len(g.EDGE_SIZES):])
    for n_pairs in (ce.SCAN + 1, 2 * ce.SCAN + 1):
        bearings, src, tgt, off, ms, sizes = g._essential_scan_inputs(n_pairs)
        assert len(src) == n_pairs <= ce.ESS_BATCH_CHAINS and off[-1] <= ce.ESS_BATCH_MATCHES and set(sizes) == {8, 9, 10, 11, 12}
