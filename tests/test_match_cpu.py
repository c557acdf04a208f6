"""CPU checks of K33: the host compile of panovlm_amd/csrc/pvlm_match_core.h (tests/cpp/match_core_check.cpp) against the numpy restatement of
tests/match_ref.py.  (a) integer descriptors: everything bit for bit; (b) float descriptors: distances within the derived bound of fp64, decisions where the
fp64 margins exceed it; (c) the pair filter's edges; (d) the screening bound E against fp64 on adversarial inputs."""
import numpy as np
import pytest

from tests import match_ref as ref

SHAPES = [(1, 2), (2, 1), (0, 5), (5, 0), (31, 33), (33, 31), (127, 129), (300, 257)]


@pytest.fixture(scope="module")
def chk():
    return ref.build_check()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_records(a, b):
    return len(a) == len(b) and np.array_equal(a["query"], b["query"]) and np.array_equal(a["train"], b["train"]) and np.array_equal(_bits(a["distance"]), _bits(b["distance"]))


# ---- (a) integer-valued descriptors: the int64 restatement is the definition ---------------------------------------------------------------------
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_int_descriptors_equal_restatement_bit_for_bit(chk, n1, n2):
    rng = np.random.default_rng(1000 + 37 * n1 + n2)
    A, B = ref.int_descriptors(rng, n1, n2)
    idx, dist = ref.host_knn2(chk, A, B)
    ridx, rdist = ref.ref_knn2_int(A, B)
    assert np.array_equal(idx, ridx) and np.array_equal(_bits(dist), _bits(rdist))
    pidx, pdist = ref.host_knn2(chk, A, B, plain=True)               # the eight-row host loop equals the per-row statement
    assert np.array_equal(idx, pidx) and np.array_equal(_bits(dist), _bits(pdist))
    for ratio in (0.6, 0.8, 1.0):
        m = ref.host_match_sift(chk, A, B, ratio)
        rm = ref.ref_match_sift(ridx, rdist, ratio)
        assert _same_records(m, rm)
        if n2 < 2 or n1 == 0:
            assert len(m) == 0                                       # an empty side, or the one-row train side (the documented divergence)
        for thr in (0, 1, 5, 40):
            rc, keep, off, rec = ref.host_match_pairs(chk, [A, B], [0], [1], ratio, thr)
            rkeep, rgood = ref.ref_pair_filter(rm, thr)
            assert rc == 0 and bool(keep[0]) == rkeep and _same_records(rec, rgood) and off[1] == len(rgood)
    if n2 >= 5 and n1 >= 3:
        assert idx[2].tolist() == [1, n2 - 2] and dist[2].tolist() == [0.0, 0.0]          # the duplicated row: the tie goes to the lower index
        assert idx[1].tolist() == [1, n2 - 2] and dist[1, 0] == dist[1, 1] > 0
        assert not np.isin([1, 2], ref.host_match_sift(chk, A, B, 1.0)["query"]).any()     # d0 == d1 is no match, even at ratio 1
        assert idx[0, 0] == n2 - 1 and dist[0, 0] == 0.0                                   # a query equal to a train row


# ---- (b) RootSIFT-like float descriptors against fp64 ------------------------------------------------------------------------------------------------
def test_float_descriptors_within_bound_of_fp64(chk):
    n1, n2, ratio = 300, 257, 0.8
    A, B, planted = ref.float_descriptors(np.random.default_rng(7), n1, n2)
    D = ref.d2_matrix(A, B, np.float64)
    order = np.argsort(D, axis=1, kind="stable")[:, :3]
    d = np.take_along_axis(D, order, 1)
    dist64 = np.sqrt(d)
    # queries whose fp64 margins exceed the bound: first against second, second against third, the ratio test
    m01 = (d[:, 1] - d[:, 0]) > 2 * ref.REL_D2 * d[:, 1]
    m12 = (d[:, 2] - d[:, 1]) > 2 * ref.REL_D2 * d[:, 2]
    rhs = ratio * dist64[:, 1]
    mr = np.abs(dist64[:, 0] - rhs) > (2 * ref.REL_DIST + 2 * ref.U) * rhs
    clear = m01 & m12 & mr
    assert (~clear).sum() <= 0.01 * n1, (~clear).sum()               # the fp64 reference alone, before anything is compared
    idx, dist = ref.host_knn2(chk, A, B)
    # distances: of the rows the host compile chose, against fp64 of those same rows
    chosen = np.take_along_axis(D, idx.astype(np.int64), 1)
    assert np.all(np.abs(dist.astype(np.float64) - np.sqrt(chosen)) <= ref.REL_DIST * np.sqrt(chosen))
    assert np.array_equal(idx[clear], order[clear, :2])
    m = ref.host_match_sift(chk, A, B, ratio)
    is_match = np.zeros(n1, bool); is_match[m["query"]] = True
    assert np.array_equal(is_match[clear], (dist64[:, 0] < rhs)[clear])
    hit = planted >= 0
    assert np.all(idx[hit, 0] == planted[hit]) and is_match[hit].mean() > 0.9      # the planted matches are found


# ---- (c) the pair filter ---------------------------------------------------------------------------------------------------------------------
def _records(dist):
    m = np.zeros(len(dist), ref.MATCH_DTYPE)
    m["query"] = np.arange(len(dist)); m["train"] = np.arange(len(dist))[::-1]; m["distance"] = dist
    return m


def test_pair_filter_edges(chk):
    # 10 -> dmax; 8 is exactly 0.8 * dmax in double: the strict < removes it; 7.999999 stays
    m = _records(np.array([1, 10, 8, 7.999999, 3], np.float32))
    for thr, expect in ((3, True), (4, False)):                       # three survive: a count at the threshold and one below it (second stage)
        keep, good = ref.host_pair_filter(chk, m, thr)
        rkeep, rgood = ref.ref_pair_filter(m, thr)
        assert keep == rkeep == expect
        if expect:
            assert good["query"].tolist() == rgood["query"].tolist() == [0, 3, 4]
    assert ref.host_pair_filter(chk, m, 5)[0] is False and ref.host_pair_filter(chk, m[:4], 5)[0] is False      # first stage: at the threshold, one below
    assert ref.ref_pair_filter(m, 5)[0] is False                                                               # (five matches pass stage one, three are left)
    keep, good = ref.host_pair_filter(chk, _records(np.array([2, 2, 2], np.float32)), 0)
    assert keep and len(good) == 0                                   # every match is at dmax: none is < 0.8 dmax; threshold 0 keeps the empty pair
    # the product is a double: 0.8 * (double)dmax, not float
    dmax = np.float32(1.2345678)
    edge = np.float32(0.8 * np.float64(dmax))                         # rounded to float: may land on either side of the double product
    m = _records(np.array([dmax, edge, np.nextafter(edge, np.float32(0))], np.float32))
    keep, good = ref.host_pair_filter(chk, m, 0)
    rkeep, rgood = ref.ref_pair_filter(m, 0)
    assert keep and good["query"].tolist() == rgood["query"].tolist()


def test_negative_threshold_is_an_argument_error(chk):
    A, B = ref.int_descriptors(np.random.default_rng(3), 31, 33)
    rc, _, _, _ = ref.host_match_pairs(chk, [A, B], [0], [1], 0.8, -1)
    assert rc == -1                                                   # PVLM_ERR_ARG
    assert ref.host_match_pairs(chk, [A, B], [0], [2], 0.8, 1)[0] == -1


# ---- (d) the screening bound ---------------------------------------------------------------------------------------------------------------------
def test_screening_bound_holds_against_fp64(chk):
    rng = np.random.default_rng(11)
    worst = 0.0
    cases = []
    for scale in (1.0, 255.0, 1e4, 1e-3):
        a = (rng.uniform(0.5, 1.0, ref.DIM) * scale).astype(np.float32)
        cases.append((a, a.copy()))                                                             # large norms, true distance 0
        cases.append((a, np.nextafter(a, np.float32(np.inf))))                                  # ... and one ulp per component
        b = a.copy(); b[5] = np.nextafter(b[5], np.float32(0))
        cases.append((a, b))                                                                    # ... and one ulp in one component
        sgn = np.where(np.arange(ref.DIM) % 2 == 0, 1, -1).astype(np.float32)
        cases.append((a, (rng.uniform(0.5, 1.0, ref.DIM) * scale).astype(np.float32) * sgn))    # alternating signs of the a.b terms: the dot cancels
        cases.append((a * sgn, a * np.roll(sgn, 1)))                                            # a.b = -|a|^2
        cases.append(((rng.normal(size=ref.DIM) * scale).astype(np.float32), (rng.normal(size=ref.DIM) * scale).astype(np.float32)))
    for a, b in cases:
        s, E, d2 = ref.host_screen(chk, a, b)
        true = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum())
        assert abs(s - true) <= E, (s, true, E)
        assert abs(d2 - true) <= ref.REL_D2 * true + 1e-300
        worst = max(worst, abs(s - true) / E)
    assert 0 < worst <= 1
    # the certificate never accepts what the bound cannot separate
    assert chk.chk_certified(ref.C.c_float(10.0), ref.C.c_float(1.0), ref.C.c_float(8.9)) == 1
    assert chk.chk_certified(ref.C.c_float(10.0), ref.C.c_float(1.0), ref.C.c_float(9.0)) == 0
    assert chk.chk_certified(ref.C.c_float(np.inf), ref.C.c_float(1.0), ref.C.c_float(1.0)) == 0
    assert chk.chk_certified(ref.C.c_float(10.0), ref.C.c_float(np.inf), ref.C.c_float(1.0)) == 0
    assert chk.chk_certified(ref.C.c_float(10.0), ref.C.c_float(1.0), ref.C.c_float(np.inf)) == 0
