"""CPU checks of K35: the host compile of panovlm_amd/csrc/pvlm_vlad_core.h (tests/cpp/vlad_core_check.cpp) against the numpy restatement of tests/vlad_ref.py."""
import ctypes as C

import numpy as np
import pytest

from tests import vlad_ref as ref

# A nearest-centre gap the restated chain cannot close: a double rounding moves one partial sum by one float ulp (2^-23 relatively, at most), the later steps only
# add non-negative terms to it, so the final d2 moves by about that much; four times that on either side.  Integer-valued rows are exact in both evaluations.
GAP = 2.0 ** -21


@pytest.fixture(scope="module")
def chk():
    return ref.build_check()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _kmeans_equal(chk, frames, train, book, max_it, init, expect_dead=0, exact=False):
    rc, cb, alive, assign, it, dead = ref.host_kmeans(chk, frames, train, book, max_it, init)
    assert rc == 0
    X = np.concatenate([frames[f] for f in train])
    rcb, ralive, rassign, rit, gap = ref.ref_kmeans(X, book, max_it, init, chk.chk_vlad_sum_chunk())
    assert exact or gap > GAP
    assert it == rit and np.array_equal(alive, ralive) and np.array_equal(assign, rassign) and np.array_equal(_bits(cb), _bits(rcb))
    assert dead == expect_dead == int((alive == 0).sum())
    return cb, alive, assign, it


@pytest.mark.parametrize("book", [1, 2, 5, 128])
def test_kmeans_int_descriptors(chk, book):
    rng = np.random.default_rng(100 + book)
    frames = ref.int_frames(rng)
    train = [3, 0, 5, 2]
    n = sum(len(frames[f]) for f in train)
    init = rng.choice(n, book, replace=False)
    cb, alive, assign, it = _kmeans_equal(chk, frames, train, book, 25, init, exact=True)
    if book == 5:
        assert 1 < it < 25                                          # this one converges before the limit


@pytest.mark.parametrize("book", [2, 5])
def test_kmeans_float_descriptors_chunked_order(chk, book):
    """718 RootSIFT-like rows: with 2 centres one of them has more than kSumChunk members, so the run sums are added."""
    rng = np.random.default_rng(200 + book)
    frames = ref.float_frames(rng)
    train = [1, 2, 3, 4, 5]
    n = sum(len(frames[f]) for f in train)
    assert n == 718
    cb, alive, assign, it = _kmeans_equal(chk, frames, train, book, 25, rng.choice(n, book, replace=False))
    assert np.bincount(assign, minlength=book).max() > chk.chk_vlad_sum_chunk()


@pytest.mark.parametrize("max_it", [0, 1])
def test_kmeans_iteration_limits(chk, max_it):
    rng = np.random.default_rng(300)
    frames = ref.int_frames(rng)
    init = [5, 17, 250]
    cb, alive, assign, it = _kmeans_equal(chk, frames, [3, 4], 3, max_it, init, exact=True)
    assert it == max_it
    if max_it == 0:
        X = np.concatenate([frames[3], frames[4]])
        assert np.array_equal(cb, X[init]) and not assign.any()


def test_duplicate_init_rows_give_a_dead_centre(chk):
    """Two centres start as the same row: every row ties between them, the tie goes to the lower index, the higher one dies and its block stays zero."""
    rng = np.random.default_rng(400)
    frames = ref.int_frames(rng)
    cb, alive, assign, it = _kmeans_equal(chk, frames, [3, 5], 4, 25, [10, 40, 10, 300], expect_dead=1, exact=True)
    assert alive.tolist() == [1, 1, 0, 1] and not cb[2].any() and not (assign == 2).any()
    for t in (0, 1, 2):
        rc, V = ref.host_embed(chk, frames, cb, alive, t)
        assert rc == 0 and not V.reshape(len(frames), 4, ref.DIM)[:, 2].any()
        for f in (2, 3):
            want, _ = ref.ref_embed(frames[f], cb, alive, t)        # integer rows, but means are not integers: the gap is checked on the float tests
            if t < 2:
                assert np.array_equal(V[f], want)


@pytest.mark.parametrize("normalization", [0, 1])
@pytest.mark.parametrize("book", [1, 2, 5, 128])
def test_embedding_types_0_and_1_equal_restatement(chk, book, normalization):
    rng = np.random.default_rng(500 + book)
    frames = ref.float_frames(rng)
    X = np.concatenate(frames)
    rc, cb, alive, _, _, _ = ref.host_kmeans(chk, frames, list(range(len(frames))), book, 3, rng.choice(len(X), book, replace=False))
    assert rc == 0
    rc, V = ref.host_embed(chk, frames, cb, alive, normalization)
    assert rc == 0
    for f in range(len(frames)):
        want, gap = ref.ref_embed(frames[f], cb, alive, normalization)
        assert gap > GAP
        assert np.array_equal(V[f], want), (f, book)
    assert not V[0].any()                                           # the frame without rows: a zero vector, not NaN


@pytest.mark.parametrize("book", [2, 128])
def test_embedding_type_2_within_one_ulp_of_pow(chk, book):
    rng = np.random.default_rng(600 + book)
    frames = ref.float_frames(rng)
    X = np.concatenate(frames)
    rc, cb, alive, _, _, _ = ref.host_kmeans(chk, frames, list(range(len(frames))), book, 3, rng.choice(len(X), book, replace=False))
    # a row equal to its centre: its residual is zero and it contributes nothing (no NaN)
    frames[2] = frames[2].copy(); frames[2][7] = cb[np.nonzero(alive)[0][0]]
    rc, V = ref.host_embed(chk, frames, cb, alive, 2)
    assert rc == 0 and np.isfinite(V).all() and not V[0].any()
    bound = ref.type2_rel_bound(book)
    for f in range(len(frames)):
        want, gap = ref.ref_embed(frames[f], cb, alive, 2)
        assert gap > GAP
        err = np.abs(V[f].astype(np.float64) - want.astype(np.float64))
        assert (err <= bound * np.abs(want).astype(np.float64) + 2.0 ** -149).all(), (f, err.max())
    n = np.linalg.norm(V[1:].astype(np.float64), axis=1)
    assert np.allclose(n, 1.0, atol=1e-6)
    # the zero-residual row alone: a frame made of one centre row gives a zero vector
    rc, V1 = ref.host_embed(chk, [cb[np.nonzero(alive)[0][0]][None]], cb, alive, 2)
    assert rc == 0 and not V1.any()


def test_root5_every_float_within_one_ulp(chk):
    """Every non-negative finite float against (float)pow((double)x, 0.2): the counts recorded in pvlm_vlad_core.h and DESIGN.md."""
    differing, worst = ref.host_root5_sweep(chk)
    print("root5: %d floats differ, largest difference %d ulp" % (differing, worst))
    assert worst <= 1
    assert chk.chk_root5(0.0) == 0.0 and chk.chk_root5(32.0) == 2.0 and chk.chk_root5(1.0) == 1.0


def test_neighbors_equal_restatement_and_ties(chk):
    rng = np.random.default_rng(700)
    frames = ref.float_frames(rng, [40, 60, 50, 60, 33, 0, 45])
    frames[3] = frames[1].copy()                                    # two identical frames: equal similarities to everything, the tie goes to the lower index
    X = np.concatenate(frames)
    rc, cb, alive, _, _, _ = ref.host_kmeans(chk, frames, list(range(len(frames))), 5, 5, rng.choice(len(X), 5, replace=False))
    rc, V = ref.host_embed(chk, frames, cb, alive, 2)
    assert rc == 0 and np.array_equal(_bits(V[1]), _bits(V[3]))
    for m in (1, 3, 7, 50):                                         # 50: neighbor_size above n
        rc, nb, sim = ref.host_neighbors(chk, V, 5, m)
        want_nb, want_sim = ref.ref_neighbors(V, m)
        assert rc == 0 and nb.shape == (7, min(m, 7))
        assert np.array_equal(nb, want_nb) and np.array_equal(sim, want_sim)
        assert np.array_equal(sim.view(np.uint64), sim.T.copy().view(np.uint64))
    rc, nb, sim = ref.host_neighbors(chk, V, 5, 3)
    assert nb[1, :2].tolist() == [1, 3] and nb[3, :2].tolist() == [1, 3]       # sim(1, 1) == sim(1, 3) == sim(3, 3): index order
    assert nb[5].tolist() == [0, 1, 2]                              # the zero vector: every similarity is 0, index order
    assert ref.host_neighbors(chk, V, 5, 0)[0] == -1


def test_argument_rules(chk):
    frames = ref.int_frames(np.random.default_rng(800))
    assert ref.host_kmeans(chk, frames, [3], 0, 5, [])[0] == -1
    assert ref.host_kmeans(chk, frames, [1], 2, 5, [0, 0])[0] == -1              # more centres than training rows
    assert ref.host_kmeans(chk, frames, [3], 2, 5, [0, 300])[0] == -1            # an init row out of range
    assert ref.host_kmeans(chk, frames, [6], 2, 5, [0, 1])[0] == -1              # a frame out of range
    assert ref.host_kmeans(chk, frames, [3], 2, -1, [0, 1])[0] == -1
    cb = np.ones((2, ref.DIM), np.float32); cb[1, 5] = np.nan
    assert ref.host_embed(chk, frames, cb, None, 2)[0] == -1
    assert ref.host_embed(chk, frames, cb, [1, 0], 2)[0] == 0                    # ... unless the row is dead
    assert ref.host_embed(chk, frames, cb[:1], None, 3)[0] == -1
