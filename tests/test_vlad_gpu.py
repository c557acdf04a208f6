"""GPU checks of K35 through the C ABI: pvlm_vlad_kmeans, pvlm_vlad_embed (all three types), pvlm_vladset_read and pvlm_vlad_neighbors against the host compile of the
same core (tests/cpp/vlad_core_check.cpp) bit for bit, in both flag modes; the same under a small PVLM_VLAD_BATCH_ROWS; a dead centre and a zero residual; a forced
fallback; the argument checks; and the host mirror's InitImagePairs into MatchImagePairs through tests/cpp/pvlm_vlad_driver.cpp."""
import os
import subprocess

import numpy as np
import pytest

from tests import vlad_ref as ref

pytestmark = pytest.mark.gpu

EXACT = 0x400
TRAIN = [3, 1, 5, 0, 2]            # 300 + 1 + 257 + 0 + 33 rows: unsorted, an empty frame, a one-row frame


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chk():
    return ref.build_check()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_against_host(ctx, chk, frames, train, book, init, max_it=25, neighbor_size=3):
    """kmeans, embed (types 0, 1, 2), read and neighbours in both modes against the host compile; returns the fast mode's (kmeans stats, embed stats)."""
    import panovlm_amd as pv
    rc, hcb, halive, hassign, hit, hdead = ref.host_kmeans(chk, frames, train, book, max_it, init)
    assert rc == 0
    hV = {t: ref.host_embed(chk, frames, hcb, halive, t)[1] for t in (0, 1, 2)}
    hnb = {t: ref.host_neighbors(chk, hV[t], book, neighbor_size) for t in (0, 1, 2)}
    ds = pv.api.DescSet(ctx, frames)
    out = None
    try:
        for flags in (EXACT, 0):
            cb, alive, assign, st = pv.api.vlad_kmeans(ctx, ds, train, book, max_it, init, flags)
            assert np.array_equal(_bits(cb), _bits(hcb)) and np.array_equal(alive, halive) and np.array_equal(assign, hassign), flags
            assert st["iterations"] == hit and st["dead_centres"] == hdead and st["queries"] == hit * len(hassign)
            if flags == EXACT:
                assert st["fallback_queries"] == st["queries"]
            for t in (0, 1, 2):
                vs = pv.api.vlad_embed(ctx, ds, cb, alive, t, flags)
                try:
                    V = vs.read()
                    assert np.array_equal(_bits(V), _bits(hV[t])), (flags, t)
                    assert vs.stats["queries"] == sum(len(f) for f in frames) and vs.stats["dead_centres"] == hdead
                    if flags == EXACT:
                        assert vs.stats["fallback_queries"] == vs.stats["queries"]
                    nb, sim = pv.api.vlad_neighbors(ctx, vs, neighbor_size, want_sim=True)
                    assert np.array_equal(nb, hnb[t][1]) and np.array_equal(sim.view(np.uint64), hnb[t][2].view(np.uint64)), (flags, t)
                    nb2, none = pv.api.vlad_neighbors(ctx, vs, neighbor_size)
                    assert none is None and np.array_equal(nb2, nb)
                    est = vs.stats
                finally:
                    vs.close()
            out = (st, est)
        return out
    finally:
        ds.close()


@pytest.mark.parametrize("book", [1, 2, 5, 128])
def test_int_descriptors_equal_host_compile(ctx, chk, book):
    rng = np.random.default_rng(1100 + book)
    frames = ref.int_frames(rng)
    n = sum(len(frames[f]) for f in TRAIN)
    _check_against_host(ctx, chk, frames, TRAIN, book, rng.choice(n, book, replace=False), neighbor_size=3 if book != 2 else 50)     # 50: above n


@pytest.mark.parametrize("book", [2, 5, 128])
def test_float_descriptors_equal_host_compile(ctx, chk, book):
    """RootSIFT-like rows; with 2 centres over 718 rows one centre has more than kSumChunk members."""
    rng = np.random.default_rng(1200 + book)
    frames = ref.float_frames(rng)
    train = [1, 2, 3, 4, 5]
    kst, est = _check_against_host(ctx, chk, frames, train, book, rng.choice(718, book, replace=False), max_it=6)
    if book >= 5:                                                    # fewer than four centres leave the screening no fourth candidate to bound the rest with
        assert kst["fallback_queries"] < kst["queries"] and est["fallback_queries"] < est["queries"]


def test_small_batches_give_identical_results(ctx, chk, monkeypatch):
    rng = np.random.default_rng(1300)
    frames = ref.float_frames(rng)
    init = rng.choice(591, 5, replace=False)
    kst, est = _check_against_host(ctx, chk, frames, TRAIN, 5, init, max_it=4)
    assert kst["batches"] == 1 and est["batches"] == 1
    monkeypatch.setenv("PVLM_VLAD_BATCH_ROWS", "160")                # whole frames only: 300 and 257 rows are batches of their own, the small frames share one
    kst, est = _check_against_host(ctx, chk, frames, TRAIN, 5, init, max_it=4)
    assert kst["batches"] >= 3 and est["batches"] >= 3


def test_dead_centre_and_zero_residual(ctx, chk):
    """Duplicated init_rows: the higher of the two centres dies.  A frame holding one row equal to a centre: a zero vector under type 2, no NaN."""
    import panovlm_amd as pv
    rng = np.random.default_rng(1400)
    frames = ref.int_frames(rng)
    kst, est = _check_against_host(ctx, chk, frames, [3, 5], 4, [10, 40, 10, 300])
    assert kst["dead_centres"] == 1 and est["dead_centres"] == 1
    rc, cb, alive, _, _, _ = ref.host_kmeans(chk, frames, [3, 5], 4, 25, [10, 40, 10, 300])
    assert alive.tolist() == [1, 1, 0, 1]
    two = [cb[1][None].copy(), frames[2]]
    ds = pv.api.DescSet(ctx, two)
    try:
        for flags in (EXACT, 0):
            vs = pv.api.vlad_embed(ctx, ds, cb, alive, 2, flags)
            V = vs.read(); vs.close()
            assert not V[0].any() and np.isfinite(V).all() and not V.reshape(2, 4, ref.DIM)[:, 2].any()
            assert np.array_equal(_bits(V), _bits(ref.host_embed(chk, two, cb, alive, 2)[1]))
    finally:
        ds.close()


def test_forced_fallback_by_ties(ctx, chk):
    """Six identical copies of a query's nearest centre at scattered indices (more than the 4 candidates) and one more centre an ulp further in one component: the
    certificate cannot hold for that row, the fallback decides (the tie goes to the lowest index), and the vectors equal exact mode and the host compile."""
    import panovlm_amd as pv
    rng = np.random.default_rng(1500)
    frames = ref.float_frames(rng, [40, 33])
    cb = ref.float_frames(rng, [200])[0]
    near = frames[0][3].copy(); near[7] = np.nextafter(near[7], np.float32(1))
    near2 = near.copy(); near2[9] = np.nextafter(near2[9], np.float32(1))
    cb[50] = near2
    for j in (3, 77, 78, 120, 160, 199):
        cb[j] = near
    ds = pv.api.DescSet(ctx, frames)
    try:
        hV = ref.host_embed(chk, frames, cb, None, 2)[1]
        assert hV.reshape(2, 200, ref.DIM)[0, 3].any() and not hV.reshape(2, 200, ref.DIM)[0, 77].any()      # the six-way tie goes to the lowest index
        for flags in (EXACT, 0):
            vs = pv.api.vlad_embed(ctx, ds, cb, None, 2, flags)
            V = vs.read(); st = vs.stats; vs.close()
            assert np.array_equal(_bits(V), _bits(hV)), flags
        assert 0 < st["fallback_queries"] < st["queries"]
    finally:
        ds.close()


def test_argument_checks(ctx):
    import panovlm_amd as pv
    frames = ref.int_frames(np.random.default_rng(1600))
    ds = pv.api.DescSet(ctx, frames)
    other = pv.Context(0)
    try:
        bad = [lambda: pv.api.vlad_kmeans(ctx, ds, [3], 0, 5, []),
               lambda: pv.api.vlad_kmeans(ctx, ds, [1], 2, 5, [0, 0]),           # more centres than training rows
               lambda: pv.api.vlad_kmeans(ctx, ds, [3], 2, 5, [0, 300]),         # an init row out of range
               lambda: pv.api.vlad_kmeans(ctx, ds, [3], 2, 5, [0, -1]),
               lambda: pv.api.vlad_kmeans(ctx, ds, [6], 2, 5, [0, 1]),           # a frame out of range
               lambda: pv.api.vlad_kmeans(ctx, ds, [3], 2, -1, [0, 1]),
               lambda: pv.api.vlad_kmeans(other, ds, [3], 2, 5, [0, 1])]         # another context
        cb = np.ones((2, ref.DIM), np.float32)
        nan = cb.copy(); nan[1, 5] = np.nan
        bad += [lambda: pv.api.vlad_embed(ctx, ds, nan), lambda: pv.api.vlad_embed(ctx, ds, cb, None, 3), lambda: pv.api.vlad_embed(ctx, ds, cb, None, -1),
                lambda: pv.api.vlad_embed(other, ds, cb)]
        for call in bad:
            with pytest.raises(pv.api.PvlmError):
                call()
        vs = pv.api.vlad_embed(ctx, ds, nan, [1, 0])                 # ... unless the row is dead
        try:
            assert np.isfinite(vs.read()).all()
            for call in (lambda: pv.api.vlad_neighbors(ctx, vs, 0), lambda: pv.api.vlad_neighbors(other, vs, 3)):
                with pytest.raises(pv.api.PvlmError):
                    call()
        finally:
            vs.close()
        cb0, alive0, assign0, st0 = pv.api.vlad_kmeans(ctx, ds, [3], 2, 0, [7, 9])
        assert np.array_equal(cb0, frames[3][[7, 9]]) and alive0.all() and not assign0.any() and st0["iterations"] == 0
    finally:
        ds.close(); other.close()


def test_retrieval_and_init_image_pairs_chain(chk, tmp_path):
    """12 frames in 4 groups of 3 whose frames share most descriptor rows, perturbed; book_size 16.  Every frame's 3 nearest neighbours are itself and its group;
    InitImagePairs(VLAD | CONTIGUOUS) equals InitImagePairsHost; the pair list runs through MatchImagePairs."""
    from panovlm_amd import build
    frames = ref.retrieval_scene(np.random.default_rng(1700))
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(frames)], np.int32).tobytes())
        for d in frames:
            f.write(np.array([len(d)], np.int32).tobytes()); f.write(d.tobytes())
    exe = build.VLAD_DRIVER
    assert os.path.exists(exe), "build() makes the driver"
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "16", "7"], check=True, timeout=300)
    raw = np.frombuffer(open(tmp_path / "out.bin", "rb").read(), np.int32)
    ok, same_as_host, n_pairs, matched_pairs = raw[:4]
    nb = raw[4:4 + 36].reshape(12, 3)
    pairs = raw[40:40 + 2 * n_pairs].reshape(-1, 2)
    assert ok == 1 and same_as_host == 1
    for i in range(12):
        assert sorted(nb[i].tolist()) == [3 * (i // 3), 3 * (i // 3) + 1, 3 * (i // 3) + 2], (i, nb[i])
    # 12 frames: the contiguous window of 20 gives all 66 pairs first, in (i, j) order; VLAD's min(15, 12) neighbours add nothing new
    assert n_pairs == 66 and pairs.tolist() == [[i, j] for i in range(12) for j in range(i + 1, 12)]
    assert matched_pairs >= 12                                       # at least the pairs inside the groups survive MatchImagePairs
