"""GPU checks of K33 through the C ABI: pvlm_match_knn2 and pvlm_match_pairs against the host compile of the same core (tests/cpp/match_core_check.cpp) bit for
bit, in both flag modes; a ragged batch against the per-pair results; two inputs that force the fallback; a capacity that is too small; the argument checks; and
the host mirror's chain MatchImagePairs -> TriangulateTracks through tests/cpp/pvlm_match_driver.cpp."""
import os
import subprocess

import numpy as np
import pytest

from tests import match_ref as ref
from tests import sfm_ba_ref as ba_ref

pytestmark = pytest.mark.gpu

EXACT = 0x400
SHAPES = [(1, 2), (2, 1), (0, 5), (5, 0), (31, 33), (33, 31), (127, 129), (300, 257)]


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


def _same_records(a, b):
    return len(a) == len(b) and np.array_equal(a["query"], b["query"]) and np.array_equal(a["train"], b["train"]) and np.array_equal(_bits(a["distance"]), _bits(b["distance"]))


def _check_against_host(ctx, chk, descs, src, tgt, ratio, thr, expect_fallback=None):
    """knn2 and match_pairs of the pair list in both modes against the host compile; returns the fast mode's stats."""
    import panovlm_amd as pv
    ds = pv.api.DescSet(ctx, descs)
    try:
        hidx = np.concatenate([ref.host_knn2(chk, descs[s], descs[t])[0] for s, t in zip(src, tgt)] + [np.zeros((0, 2), np.int32)])
        hdist = np.concatenate([ref.host_knn2(chk, descs[s], descs[t])[1] for s, t in zip(src, tgt)] + [np.zeros((0, 2), np.float32)])
        rc, hkeep, hoff, hrec = ref.host_match_pairs(chk, descs, src, tgt, ratio, thr)
        assert rc == 0
        stats = None
        for flags in (EXACT, 0):
            idx, dist, st = pv.api.match_knn2(ctx, ds, src, tgt, flags)
            assert np.array_equal(idx, hidx) and np.array_equal(_bits(dist), _bits(hdist)), flags
            r = pv.api.match_pairs(ctx, ds, src, tgt, ratio, thr, flags)
            assert not r["overflow"] and np.array_equal(r["keep"], hkeep) and np.array_equal(r["offsets"], hoff) and _same_records(r["matches"], hrec), flags
            assert r["needed"] == hoff[-1] and r["stats"]["queries"] == len(hidx) == st["queries"]
            stats = r["stats"]
            if flags == EXACT:
                assert stats["fallback_queries"] == stats["queries"]
        if expect_fallback is not None:
            assert (stats["fallback_queries"] > 0) == expect_fallback, stats
        return stats
    finally:
        ds.close()


@pytest.mark.parametrize("n1,n2", SHAPES)
def test_int_descriptors_equal_host_compile(ctx, chk, n1, n2):
    A, B = ref.int_descriptors(np.random.default_rng(1000 + 37 * n1 + n2), n1, n2)
    for thr in (0, 5):
        _check_against_host(ctx, chk, [A, B], [0], [1], 0.8, thr)


def test_float_descriptors_equal_host_compile(ctx, chk):
    A, B, _ = ref.float_descriptors(np.random.default_rng(7), 300, 257)
    st = _check_against_host(ctx, chk, [A, B], [0, 1], [1, 0], 0.8, 10)
    assert st["fallback_queries"] < st["queries"]                    # the screening path certifies at least some of these


def test_ragged_batch_equals_per_pair(ctx, chk, monkeypatch):
    """Row counts 0, 1, 33, 300 (and 127, 257) in one batch; frame 3 is a source and a target; src == tgt once."""
    import panovlm_amd as pv
    rng = np.random.default_rng(21)
    rows = [0, 1, 33, 300, 127, 257]
    descs = [rng.integers(0, 256, size=(n, ref.DIM)).astype(np.float32) for n in rows]
    descs[4][:20] = descs[3][5:25]; descs[5][:30] = descs[3][100:130]; descs[2][:10] = descs[3][:10]      # shared rows: real matches
    src = [3, 2, 3, 0, 1, 4, 3, 5, 2]
    tgt = [4, 3, 3, 3, 3, 1, 0, 3, 5]
    st = _check_against_host(ctx, chk, descs, src, tgt, 0.8, 3)
    assert st["batches"] == 1
    # the same list cut into batches of at most 320 queries (a larger pair is a batch of its own): offsets, records and knn2 rows accumulate across batches
    monkeypatch.setenv("PVLM_MATCH_BATCH_QUERIES", "320")
    st = _check_against_host(ctx, chk, descs, src, tgt, 0.8, 3)
    assert st["batches"] >= 5
    monkeypatch.delenv("PVLM_MATCH_BATCH_QUERIES")
    ds = pv.api.DescSet(ctx, descs)
    try:
        for flags in (0, EXACT):
            whole = pv.api.match_pairs(ctx, ds, src, tgt, 0.8, 3, flags)
            for p, (s, t) in enumerate(zip(src, tgt)):
                one = pv.api.match_pairs(ctx, ds, [s], [t], 0.8, 3, flags)
                assert one["keep"][0] == whole["keep"][p] and _same_records(one["matches"], whole["matches"][whole["offsets"][p]:whole["offsets"][p + 1]])
    finally:
        ds.close()


def test_forced_fallback_by_ties(ctx, chk):
    """Next to the query's nearest row two train rows differ by one ulp in one component; six identical copies of the second-nearest row sit at scattered indices
    (more copies than the 4 candidates): the certificate cannot hold, the fallback decides, and the results equal exact mode."""
    rng = np.random.default_rng(5)
    A, B, _ = ref.float_descriptors(rng, 40, 200)
    q = A[3].copy()
    near = q.copy(); near[7] = np.nextafter(near[7], np.float32(1))                # the nearest row
    near2 = near.copy(); near2[9] = np.nextafter(near2[9], np.float32(1))          # the second nearest: one ulp in one component next to it
    B[50] = near
    for j in (3, 77, 78, 120, 160, 199):
        B[j] = near2
    idx, _ = ref.host_knn2(chk, A, B)
    assert idx[3].tolist() == [50, 3]                                              # the six-way tie goes to the lowest index
    _check_against_host(ctx, chk, [A, B], [0], [1], 0.8, 0, expect_fallback=True)


def test_forced_fallback_by_large_norms(ctx, chk):
    """Norms so large that E exceeds the gap between the second and the third neighbour: offsets of 4096 on every component, neighbours a few units apart."""
    rng = np.random.default_rng(6)
    base = np.float32(4096.0)
    B = (base + rng.integers(0, 8, size=(100, ref.DIM))).astype(np.float32)
    A = (base + rng.integers(0, 8, size=(37, ref.DIM))).astype(np.float32)
    st = _check_against_host(ctx, chk, [A, B], [0], [1], 0.9, 0, expect_fallback=True)
    assert st["fallback_queries"] == st["queries"]                   # E = 264 u (|a|^2 + |b|^2) ~ 6.8e4 against d2 ~ 1.3e3


def test_capacity_too_small_reports_needed(ctx, chk, monkeypatch):
    """A capacity that cuts the second pair in the middle, one that cuts the first, and none at all (out = NULL): `needed`, keep and the offsets are those of the full
    call, the records that fit are the first ones, and the sentinel records behind the capacity are untouched.  Once more with one pair per batch."""
    import ctypes as C
    import panovlm_amd as pv
    A, B = ref.int_descriptors(np.random.default_rng(1000 + 37 * 300 + 257), 300, 257)
    ds = pv.api.DescSet(ctx, [A, B])
    try:
        for batch_queries in (None, 300):
            if batch_queries:
                monkeypatch.setenv("PVLM_MATCH_BATCH_QUERIES", str(batch_queries))
            full = pv.api.match_pairs(ctx, ds, [0, 0], [1, 1], 1.0, 1)
            assert full["needed"] >= 10 and not full["overflow"] and full["guard_intact"] and full["stats"]["batches"] == (2 if batch_queries else 1)
            first = int(full["offsets"][1])
            assert 3 < first < full["needed"]
            for cap in (first + 3, first, first - 3, 1):
                for flags in (0, EXACT):
                    r = pv.api.match_pairs(ctx, ds, [0, 0], [1, 1], 1.0, 1, flags, capacity=cap)
                    assert r["overflow"] and r["needed"] == full["needed"] and np.array_equal(r["offsets"], full["offsets"]) and np.array_equal(r["keep"], full["keep"])
                    assert len(r["matches"]) == cap and _same_records(r["matches"], full["matches"][:cap])
                    assert r["guard_intact"]
            # capacity 0 with no buffer at all
            keep = np.zeros(2, np.uint8); off = np.zeros(3, np.int64); needed = C.c_longlong(-1)
            src = np.array([0, 0], np.int32); tgt = np.array([1, 1], np.int32)
            rc = ctx.lib.pvlm_match_pairs(ctx._h, ds._h, C.c_int(2), src.ctypes.data_as(C.c_void_p), tgt.ctypes.data_as(C.c_void_p), C.c_float(1.0), C.c_int(1), C.c_uint(0),
                                          keep.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), None, C.c_longlong(0), C.byref(needed), None)
            assert rc == -5 and needed.value == full["needed"] and np.array_equal(off, full["offsets"]) and np.array_equal(keep, full["keep"])
    finally:
        ds.close()


def test_argument_checks(ctx):
    import panovlm_amd as pv
    A = np.ones((4, ref.DIM), np.float32)
    with pytest.raises(pv.api.PvlmError):
        pv.api.DescSet(ctx, [np.ones((4, 64), np.float32)])          # another width
    bad = A.copy(); bad[2, 100] = np.inf
    with pytest.raises(pv.api.PvlmError):
        pv.api.DescSet(ctx, [A, bad])
    bad[2, 100] = np.nan
    with pytest.raises(pv.api.PvlmError):
        pv.api.DescSet(ctx, [bad])
    ds = pv.api.DescSet(ctx, [A, A])
    try:
        with pytest.raises(pv.api.PvlmError):
            pv.api.match_pairs(ctx, ds, [0], [1], 0.8, -1)           # upstream would drop every pair
        with pytest.raises(pv.api.PvlmError):
            pv.api.match_pairs(ctx, ds, [0], [2], 0.8, 1)
        r = pv.api.match_pairs(ctx, ds, [], [], 0.8, 1)
        assert r["needed"] == 0 and len(r["keep"]) == 0
    finally:
        ds.close()


def test_chain_match_image_pairs_into_triangulate_tracks(tmp_path):
    """6 frames, about 230 keypoints each: every track has a descriptor of its own, its observations differ from it by +-1 on 8 components, so the true
    correspondences are the nearest neighbours by a wide margin.  Five more features seen in every frame carry noisy descriptors (+-12 on every component): they set
    every pair's dmax, so that the 0.8 filter keeps every clean match.  MatchImagePairs on all 15 pairs (threshold 1: the last frames share few tracks), then
    TriangulateTracks: the planted tracks come back with their points."""
    from panovlm_amd import build
    rng = np.random.default_rng(40)
    sc = ba_ref.trajectory_scene(rng, n_frames=6, n_tracks=300, noise_px=0.0, outlier_obs=0.0, rot_noise=0.0, trans_noise=0.0)
    F = 6
    kps = [np.rint(k).astype(np.float32) for k in sc["kps"]]
    desc = [np.zeros((len(k), ref.DIM), np.float32) for k in kps]
    for tr in sc["tracks"]:
        base = rng.integers(20, 236, size=ref.DIM)
        for f, k in tr:
            d = base.copy()
            d[rng.choice(ref.DIM, 8, replace=False)] += rng.choice([-1, 1], 8)
            desc[f][k] = d
    noisy_obs = set()
    for i in range(5):
        base = rng.integers(20, 236, size=ref.DIM)
        for f in range(F):
            noisy_obs.add((f, len(kps[f])))
            kps[f] = np.concatenate([kps[f], np.array([[100.0 + 40 * i + 3 * f, 300.0 + 25 * i]], np.float32)])
            desc[f] = np.concatenate([desc[f], (base + rng.integers(-12, 13, size=ref.DIM)).astype(np.float32)[None]])
    with open(tmp_path / "in.bin", "wb") as f:
        pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]
        f.write(np.array([F, sc["rows"], sc["cols"], len(pairs)], np.int32).tobytes())
        for i in range(F):
            f.write(np.array([1], np.int32).tobytes())
            f.write(np.asarray(sc["R_true"][i], np.float64).tobytes()); f.write(np.asarray(sc["t_true"][i], np.float64).tobytes())
            f.write(np.array([len(kps[i])], np.int32).tobytes()); f.write(kps[i].tobytes()); f.write(desc[i].tobytes())
        f.write(np.array(pairs, np.int32).tobytes())
    exe = build.MATCH_DRIVER
    assert os.path.exists(exe), "build() makes the driver"
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "0.8", "1"], check=True, timeout=300)
    raw = open(tmp_path / "out.bin", "rb").read()
    head = np.frombuffer(raw, np.int32, 3); at = 12
    assert head[0] == 1 and head[1] == 1                             # ok, and the host loop gives the same pairs and matches
    got = set()
    for _ in range(head[2]):
        a, b, n = np.frombuffer(raw, np.int32, 3, at); at += 12
        m = np.frombuffer(raw, np.int32, 2 * n, at).reshape(-1, 2); at += 8 * n
        got.update((int(a), int(q), int(b), int(t)) for q, t in m)
    clean = sc["tracks"]
    want = set((f0, k0, f1, k1) for tr in clean for i, (f0, k0) in enumerate(tr) for (f1, k1) in tr[i + 1:])
    assert want <= got                                               # every true correspondence of the clean tracks
    extra = got - want
    assert all((a, q) in noisy_obs and (b, t) in noisy_obs for a, q, b, t in extra)       # the rest are the noisy tracks' own
    nt = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
    found = {}
    for _ in range(nt):
        at += 4
        X = np.frombuffer(raw, np.float64, 3, at); at += 24
        nf = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
        feats = np.frombuffer(raw, np.uint32, 2 * nf, at).reshape(-1, 2); at += 8 * nf
        found[frozenset((int(f), int(k)) for f, k in feats)] = X
    hit = [t for t, tr in enumerate(sc["tracks"]) if frozenset((f, k) for f, k in tr) in found]
    assert len(hit) >= 0.9 * len(clean)                              # TriangulateTracks' own 25 deg filter may drop a few
    err = np.array([np.linalg.norm(found[frozenset((f, k) for f, k in sc["tracks"][t])] - sc["X_true"][t]) for t in hit])
    # keypoints rounded to pixels: up to 0.71 px = 2.3 mrad of bearing at 1920 columns; at the scene's middle depth of 7.5 m over the shortest track's 0.8 m of
    # baseline that is 7.5^2 * 2.3e-3 / 0.8 = 0.16 m.  The median is held to it; a track next to the line of its cameras has no finite bound (see K32), so no maximum.
    assert np.median(err) < 0.16
