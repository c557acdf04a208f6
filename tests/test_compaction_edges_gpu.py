"""The loops that the five users of panovlm_amd/csrc/pvlm_compact.h (K29, K30, the plane-run table, K33, K34) and K33's grid-stride kernel run once at the shapes
of the per-stage tests, driven into their second trip: items of more than one tile (td.p0 > 0) with kept and dropped points at the tile edge, more tiles than
one trip of k_tile_scan (the carry, the prefetched next chunk, per-item totals across the trip boundary), more items than one pass of k_match_exact's grid in
exact mode and on the fallback list.  Everything is compared exactly: with the host compiles of the cores, and with the numpy restatements where those are the
definition (tests/test_compaction_edges_cpu.py checks the two against each other at these shapes, and that the inputs reach the edges).  Sizes: tests/compact_edges.py."""
import numpy as np
import pytest

from tests import colorize_ref as cr
from tests import compact_edges as ce
from tests import essential_ref as er
from tests import fuse_ref
from tests import match_ref as mr
from tests import synth
from tests import test_colorize_gpu as tcg
from tests import test_essential_gpu as teg
from tests import test_fuse_gpu as tfg
from tests import test_plane_runs_gpu as tpr

pytestmark = pytest.mark.gpu

EXACT = 0x400
TILE, SCAN = ce.TILE, ce.SCAN


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mchk():
    return mr.build_check()


@pytest.fixture(scope="module")
def echk():
    return er.build_check()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_records(a, b):
    return len(a) == len(b) and np.array_equal(a["query"], b["query"]) and np.array_equal(a["train"], b["train"]) and np.array_equal(_bits(a["distance"]), _bits(b["distance"]))


# ---- K33 ---------------------------------------------------------------------------------------------------------------------------------------
def _match_against_host(ctx, chk, descs, src, tgt, ratio, thr, modes=(EXACT, 0), restatement=False):
    """match_knn2 and match_pairs of the pair list against the host compile (and the numpy restatement: integer descriptors only).  Returns (the last mode's
    stats, the host's keep, offsets, records)."""
    import panovlm_amd as pv
    ds = pv.api.DescSet(ctx, descs)
    try:
        knn = [mr.host_knn2(chk, descs[s], descs[t]) for s, t in zip(src, tgt)]
        hidx = np.concatenate([k[0] for k in knn] + [np.zeros((0, 2), np.int32)])
        hdist = np.concatenate([k[1] for k in knn] + [np.zeros((0, 2), np.float32)])
        rc, hkeep, hoff, hrec = mr.host_match_pairs(chk, descs, src, tgt, ratio, thr)
        assert rc == 0
        if restatement:
            at = 0
            for p, (s, t) in enumerate(zip(src, tgt)):
                ridx, rdist = mr.ref_knn2_int(descs[s], descs[t])
                assert np.array_equal(hidx[at:at + len(ridx)], ridx) and np.array_equal(_bits(hdist[at:at + len(ridx)]), _bits(rdist))
                rkeep, rgood = mr.ref_pair_filter(mr.ref_match_sift(ridx, rdist, ratio), thr)
                assert bool(hkeep[p]) == rkeep and _same_records(hrec[hoff[p]:hoff[p + 1]], rgood)
                at += len(ridx)
        stats = None
        for flags in modes:
            idx, dist, st = pv.api.match_knn2(ctx, ds, src, tgt, flags)
            assert np.array_equal(idx, hidx) and np.array_equal(_bits(dist), _bits(hdist)), flags
            r = pv.api.match_pairs(ctx, ds, src, tgt, ratio, thr, flags)
            assert not r["overflow"] and r["guard_intact"], flags
            assert np.array_equal(r["keep"], hkeep) and np.array_equal(r["offsets"], hoff) and _same_records(r["matches"], hrec), flags
            assert r["needed"] == hoff[-1] and r["stats"]["queries"] == len(hidx) == st["queries"]
            assert r["stats"]["batches"] == st["batches"]
            stats = r["stats"]
            if flags == EXACT:
                assert stats["fallback_queries"] == stats["queries"]
        return stats, hkeep, hoff, hrec
    finally:
        ds.close()


@pytest.mark.parametrize("n1", ce.MATCH_EDGE_N1)
def test_match_pair_of_more_than_one_tile(ctx, mchk, n1):
    """k_match_count / k_match_scatter with td.p0 = TILE (and 2 TILE): kept queries in the last round of a tile and the first of the next, on e - 1 and e, none on e - 2."""
    A, B = ce.match_edge_descriptors(n1)
    st, hkeep, hoff, hrec = _match_against_host(ctx, mchk, [A, B], [0], [1], 0.8, 5, restatement=True)
    assert st["batches"] == 1 and hkeep[0] == 1 and ce.match_edges_reached(hrec["query"], n1)
    assert (hrec["query"] >= TILE).any() == (n1 > TILE)              # records of a second tile: their places come from td.p0 and tile_base[1]


def test_match_capacity_cut_inside_the_second_tile(ctx, mchk):
    """the 2 TILE + 1 shape with capacities that end inside the second tile, on its first record and inside the first tile: the records that fit, `needed`, the guard"""
    import panovlm_amd as pv
    n1 = 2 * TILE + 1
    A, B = ce.match_edge_descriptors(n1)
    ds = pv.api.DescSet(ctx, [A, B])
    try:
        full = pv.api.match_pairs(ctx, ds, [0], [1], 0.8, 5)
        q = full["matches"]["query"]
        first = int((q < TILE).sum()); second = int((q < 2 * TILE).sum())
        assert not full["overflow"] and 3 < first < second - 3 and second < full["needed"] == len(q)     # every tile holds records
        for cap in (first + 3, first + 1, first, first - 3, second, full["needed"] - 1):
            for flags in (0, EXACT):
                r = pv.api.match_pairs(ctx, ds, [0], [1], 0.8, 5, flags, capacity=cap)
                assert r["overflow"] and r["needed"] == full["needed"] and np.array_equal(r["offsets"], full["offsets"]) and np.array_equal(r["keep"], full["keep"])
                assert len(r["matches"]) == cap and _same_records(r["matches"], full["matches"][:cap]) and r["guard_intact"]
    finally:
        ds.close()


def test_match_exact_mode_past_one_pass_of_the_grid(ctx, mchk):
    """EXACT_ITEMS + 5 queries in one batch: the capped grid of k_match_exact strides a second time; two pairs, so q0 is searched for"""
    n = ce.EXACT_ITEMS + 5
    rng = np.random.default_rng(77)
    A, B = mr.int_descriptors(rng, n, 66)
    for q in range(ce.EXACT_ITEMS - 2, n):                           # near neighbours for the queries around the end of the first trip: kept records there
        A[q] = B[int(rng.integers(2, 60))]
        A[q, rng.integers(0, mr.DIM, size=2)] = rng.integers(0, 256, size=2)
    cut = 20000
    assert 0 < cut < n and n <= ce.MATCH_BATCH_QUERIES
    st, hkeep, hoff, hrec = _match_against_host(ctx, mchk, [A[:cut], A[cut:], B], [0, 1], [2, 2], 0.8, 0, modes=(EXACT,), restatement=True)
    assert st["batches"] == 1 and st["queries"] == n > ce.EXACT_ITEMS
    assert hkeep.tolist() == [1, 1] and (hrec[hoff[1]:]["query"] >= ce.EXACT_ITEMS - cut).any()         # records of the queries of the second trip


def test_match_fallback_list_past_one_pass_of_the_grid(ctx, mchk):
    """FALLBACK_ITEMS + 8 queries whose screening bound exceeds every gap (offsets of 4096 on every component): all of them go to the fallback list, which the
    2048 workgroups of the fallback launch stride over twice"""
    n1 = ce.FALLBACK_ITEMS + 8
    rng = np.random.default_rng(6)
    base = np.float32(4096.0)
    B = (base + rng.integers(0, 8, size=(100, mr.DIM))).astype(np.float32)
    A = (base + rng.integers(0, 8, size=(n1, mr.DIM))).astype(np.float32)
    for q in (ce.FALLBACK_ITEMS - 1, ce.FALLBACK_ITEMS, n1 - 1):     # a train row with one component off by one: kept records on both sides of the first trip's end
        A[q] = B[int(rng.integers(0, 100))]
        A[q, 5] += 1
    st, hkeep, hoff, hrec = _match_against_host(ctx, mchk, [A, B], [0], [1], 0.9, 0)
    assert st["batches"] == 1 and st["fallback_queries"] == n1 == st["queries"]       # the fast mode's stats: the list really is that long
    assert hkeep[0] == 1 and (hrec["query"] >= ce.FALLBACK_ITEMS).any()


def _match_scan_frames():
    """six frames of 3 to 40 rows that share rows of one pool (real matches), and an empty one"""
    rng = np.random.default_rng(91)
    rows = [3, 7, 12, 25, 33, 40, 0]
    pool = rng.integers(0, 256, size=(40, mr.DIM)).astype(np.float32)
    descs = []
    for n in rows:
        d = rng.integers(0, 256, size=(n, mr.DIM)).astype(np.float32)
        k = (2 * n + 2) // 3                                         # two thirds of the rows are pool rows, two components off
        pick = rng.permutation(40)[:k]
        d[:k] = pool[pick]
        for i in range(k):
            d[i, rng.integers(0, mr.DIM, size=2)] = rng.integers(0, 256, size=2)
        descs.append(d)
    return descs


@pytest.mark.parametrize("n_tiles", [SCAN - 1, SCAN, SCAN + 1, 2 * SCAN + 1])
def test_match_scan_past_one_trip(ctx, mchk, n_tiles):
    """n_tiles pairs with queries (a tile each) and a few without (no tile: their per-pair total must be 0, their offsets those of the neighbours) in one batch"""
    import panovlm_amd as pv
    descs = _match_scan_frames()
    rng = np.random.default_rng(n_tiles)
    src = rng.integers(0, 6, size=n_tiles); tgt = rng.integers(0, 7, size=n_tiles)          # a target may be the empty frame
    for at in sorted(set([0, 5, SCAN - 1, SCAN, SCAN + 1, n_tiles, n_tiles + 3]) & set(range(n_tiles + 1)), reverse=True):
        src = np.insert(src, at, 6); tgt = np.insert(tgt, at, int(rng.integers(0, 6)))      # ... and these sources are
    tile_of = np.cumsum(src != 6) - 1                                                        # the tile of every pair with queries
    assert (src != 6).sum() == n_tiles and len(src) <= ce.MATCH_BATCH_PAIRS
    st, hkeep, hoff, hrec = _match_against_host(ctx, mchk, descs, src, tgt, 0.8, 2)
    assert st["batches"] == 1 and 0 < hkeep.sum() < len(src)
    trips = [b for b in range(SCAN, n_tiles, SCAN)]
    for b in trips:                                                  # kept records on both sides of every trip boundary
        p = int(np.flatnonzero((tile_of == b) & (src != 6))[0])
        assert 0 < hoff[p] < hoff[-1]
    assert len(trips) == (n_tiles - 1) // SCAN
    # ten pairs: those nearest to every trip boundary (between the tiles b - 1 and b; the end of the list where there is none), pairs without queries included
    marks = trips or [n_tiles]
    near_of = {b: sorted(range(len(src)), key=lambda p: abs(int(tile_of[p]) - b + 0.5))[:10 // len(marks)] for b in marks}
    near = [p for b in marks for p in near_of[b]]
    ds = pv.api.DescSet(ctx, descs)
    try:
        whole = pv.api.match_pairs(ctx, ds, src, tgt, 0.8, 2)
        for p in near:
            one = pv.api.match_pairs(ctx, ds, src[p:p + 1], tgt[p:p + 1], 0.8, 2)
            assert one["keep"][0] == whole["keep"][p] and _same_records(one["matches"], whole["matches"][whole["offsets"][p]:whole["offsets"][p + 1]])
    finally:
        ds.close()
    assert len(near) == 10 and (src[near] == 6).any()
    for b in trips:                                                  # single-pair calls on both sides of every trip boundary
        assert min(tile_of[near_of[b]]) < b <= max(tile_of[near_of[b]]) and (src[near_of[b]] != 6).sum() >= 2


# ---- K34 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ce.ESS_EDGE_N)
def test_essential_pair_of_more_than_one_tile(ctx, echk, n):
    """k_ess_count / k_ess_scatter / kept_point with td.p0 = TILE (and 2 TILE); global-scratch chains with a sort of 8192 or 16384 slots"""
    b1, b2, m = ce.essential_edge_scene(n)
    gr, gf = teg._both(ctx, echk, [b1, b2], [0], [1], [0, n], m, n_runs=ce.ESS_RUNS, max_iterations=ce.ESS_ITERS, tri=ce.ESS_TRI, seed=ce.ESS_SEED)
    rc, hf = er.host_filter(echk, [b1, b2], [0], [1], [0, n], m, ce.ESS_TRI, ce.ESS_RUNS, ce.ESS_ITERS, ce.ESS_SEED)
    assert rc == 0 and hf["keep"][0] == 1 and ce.essential_edges_reached(hf["inlier_idx"], n)           # the reference alone
    assert gf["stats"]["fallback_chains"] == ce.ESS_RUNS and gf["stats"]["lds_chains"] == 0
    assert (gf["inlier_idx"] >= TILE).any() == (n > TILE)


def test_essential_capacity_cut_inside_the_second_tile(ctx):
    import panovlm_amd as pv
    n = 2 * TILE + 1
    b1, b2, m = ce.essential_edge_scene(n)
    args = ([b1, b2], [0], [1], [0, n], m, ce.ESS_TRI, ce.ESS_RUNS, ce.ESS_ITERS, ce.ESS_SEED)
    full = pv.api.filter_image_pairs(ctx, *args)
    j = full["inlier_idx"]
    first = int((j < TILE).sum()); second = int((j < 2 * TILE).sum())
    assert not full["overflow"] and 3 < first < second - 3 and second < full["needed"] == len(j)
    for cap in (first + 3, first + 1, first, second, full["needed"] - 1):
        short = pv.api.filter_image_pairs(ctx, *args, capacity=cap)
        assert short["overflow"] and short["needed"] == full["needed"] and short["guard_intact"]
        assert np.array_equal(short["keep"], full["keep"]) and np.array_equal(short["offsets"], full["offsets"])
        assert np.array_equal(short["inlier_idx"], j[:cap]) and np.array_equal(_bits64(short["triangulated"]), _bits64(full["triangulated"][:cap]))


def test_essential_mixed_batch(ctx, echk):
    """0, 8, 9, 300 and TILE + 1 matches in one batch: LDS chains and global-scratch chains in one launch, pairs of no, one and two tiles in one scan"""
    big = TILE + 1
    b1, b2, m = teg._scene(300)
    c1, c2, mb = ce.essential_edge_scene(big)
    sizes = [9, big, 0, 300, 8]
    ms = [m[:9], mb, m[:0], m[:300], m[:8]]
    src = [0, 2, 0, 0, 0]; tgt = [1, 3, 1, 1, 1]
    off = np.concatenate([[0], np.cumsum(sizes)])
    gr, gf = teg._both(ctx, echk, [b1, b2, c1, c2], src, tgt, off, np.concatenate(ms), n_runs=ce.ESS_RUNS, max_iterations=ce.ESS_ITERS, tri=ce.ESS_TRI, seed=ce.ESS_SEED)
    st = gf["stats"]
    assert (st["chains"], st["lds_chains"], st["fallback_chains"]) == (3 * ce.ESS_RUNS, 2 * ce.ESS_RUNS, ce.ESS_RUNS)
    assert gf["keep"].tolist()[1:3] == [1, 0] and gf["keep"][4] == 0
    inl = gf["inlier_idx"][gf["offsets"][1]:gf["offsets"][2]]
    assert ce.essential_edges_reached(inl, big)
    assert np.array_equal(gf["offsets"][2:4], gf["offsets"][[2, 2]])                                     # the empty pair has no tile and no records


def _essential_scan_inputs(n_pairs):
    scenes = [er.two_view_scene(np.random.default_rng(60 + k), 12, outlier_fraction=0.0) for k in range(4)]
    bearings = [b for sc in scenes for b in sc[:2]]
    sizes = np.array([9 + (5 * p) % 4 for p in range(n_pairs)])
    sizes[[p for p in (3, SCAN - 1, SCAN + 2, n_pairs - 2) if p < n_pairs]] = 8      # no chain, no winner, a tile that keeps nothing
    which = np.arange(n_pairs) % 4
    ms = [scenes[k][2][:n] for k, n in zip(which, sizes)]
    off = np.concatenate([[0], np.cumsum(sizes)])
    return bearings, 2 * which, 2 * which + 1, off, ms, sizes


@pytest.mark.parametrize("n_pairs", [SCAN + 1, 2 * SCAN + 1])
def test_essential_scan_past_one_trip(ctx, echk, n_pairs):
    """n_pairs pairs of 8 to 12 exact matches (a tile each) in one batch"""
    import panovlm_amd as pv
    n_runs, maxit = 1, 3
    bearings, src, tgt, off, ms, sizes = _essential_scan_inputs(n_pairs)
    # make_batches: one batch holds at most kBatchChains / n_runs pairs and kBatchMatches / n_runs matches
    assert n_pairs <= ce.ESS_BATCH_CHAINS // n_runs and int(off[-1]) * n_runs <= ce.ESS_BATCH_MATCHES and n_pairs > SCAN
    gr, gf = teg._both(ctx, echk, bearings, src, tgt, off, np.concatenate(ms), n_runs=n_runs, max_iterations=maxit, tri=5, seed=ce.ESS_SEED)
    assert gf["stats"]["chains"] == int((sizes > 8).sum()) and not gf["keep"][sizes == 8].any()
    trips = list(range(SCAN, n_pairs, SCAN))
    for b in trips:
        assert 0 < gf["offsets"][b] < gf["offsets"][-1] and gf["keep"][b - 2:b].any() and gf["keep"][b:b + 2].any()
    for p in sorted(set(q for b in trips for q in range(b - 2, b + 2) if q < n_pairs) | {0, n_pairs - 1}):
        one = pv.api.filter_image_pairs(ctx, bearings, src[p:p + 1], tgt[p:p + 1], [0, sizes[p]], ms[p], 5, n_runs, maxit, ce.ESS_SEED)
        lo, hi = gf["offsets"][p], gf["offsets"][p + 1]
        assert one["keep"][0] == gf["keep"][p] and np.array_equal(_bits64(one["R_21"][0]), _bits64(gf["R_21"][p])) and np.array_equal(_bits64(one["t_21"][0]), _bits64(gf["t_21"][p]))
        assert np.array_equal(one["inlier_idx"], gf["inlier_idx"][lo:hi]) and np.array_equal(_bits64(one["triangulated"]), _bits64(gf["triangulated"][lo:hi]))


# ---- K29 ---------------------------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = [TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1]
FUSE_RANGE = (0.5, 40.0)


def _edge_pattern(n):
    """rows kept and rows dropped around every tile edge e inside n points and at the end: e - 1, e and n - 1 kept, e - 2, e + 1 and n - 2 dropped"""
    kept = {n - 1} | {r for e in range(TILE, n + 1, TILE) for r in (e - 1, e) if r < n}
    dropped = ({n - 2} | {r for e in range(TILE, n + 1, TILE) for r in (e - 2, e + 1) if r < n}) - kept
    return np.array(sorted(kept), np.int64), np.array(sorted(dropped), np.int64)


def _fuse_edge_clouds():
    rng = np.random.default_rng(43)
    sizes = list(tfg.SIZES) + EDGE_SIZES
    clouds = [tfg._cloud(rng, n) for n in sizes]
    for c in clouds[len(tfg.SIZES):]:
        kept, dropped = _edge_pattern(len(c))
        c[kept, :3] = (1.0, 2.0, 3.0)
        c[dropped[0::2], :3] = (50.0, 0.0, 0.0); c[dropped[1::2], :3] = (0.01, 0.0, 0.0)               # beyond max_range, inside min_range
        mask = fuse_ref.keep_mask(c, *FUSE_RANGE)
        assert mask[kept].all() and not mask[dropped].any() and 0.2 < mask.mean() < 0.8                  # by the restatement: a mix at every edge
    poses = [tfg._poses()[k % 3] for k in range(len(clouds))]
    return clouds, poses


def test_fuse_scans_of_more_than_one_tile(ctx):
    import torch
    from panovlm_amd import api
    clouds, poses = _fuse_edge_clouds()
    want, wper = fuse_ref.fuse(clouds, poses, *FUSE_RANGE)
    got, per = api.fuse_scans(ctx, clouds, poses, *FUSE_RANGE)
    assert np.array_equal(per, wper) and fuse_ref.same(got, want)
    dev = torch.device("cuda", 0)
    out, dper, n = api.fuse_scans_dev(ctx, [torch.from_numpy(c).to(dev) for c in clouds], poses, *FUSE_RANGE)
    m = int(n.item())
    assert m == len(want) and np.array_equal(dper.cpu().numpy(), wper) and fuse_ref.same(out[:m].cpu().numpy(), want)
    ctx.use_own_stream()


def _many_sizes(rng, count):
    sizes = rng.integers(0, 301, size=count)
    sizes[::37] = 0
    return sizes


def test_fuse_scan_past_one_trip(ctx):
    """2 SCAN + 1 scans of 0 to 300 points: one piece, a tile per non-empty scan, more tiles than one trip of k_tile_scan and three trips of its per-scan totals"""
    import torch
    import panovlm_amd as pv
    from panovlm_amd import api
    rng = np.random.default_rng(44)
    sizes = _many_sizes(rng, 2 * SCAN + 1)
    assert int(sizes.sum()) <= ce.PIECE_POINTS and len(sizes) <= ce.PIECE_SCANS and (sizes > 0).sum() > SCAN and (sizes == 0).sum() > 10      # one piece, two trips
    clouds = [tfg._cloud(rng, n) for n in sizes]
    poses = [tfg._poses()[k % 3] for k in range(len(clouds))]
    want, wper = fuse_ref.fuse(clouds, poses, *FUSE_RANGE)
    assert 0 < wper[:int(np.flatnonzero(np.cumsum(sizes > 0) == SCAN)[0]) + 1].sum() < len(want)         # records before and behind the second trip's first tile
    got, per = api.fuse_scans(ctx, clouds, poses, *FUSE_RANGE)
    assert np.array_equal(per, wper) and fuse_ref.same(got, want)
    with pytest.raises(pv.PvlmError, match="%d points kept" % len(want)):
        api.fuse_scans(ctx, clouds, poses, *FUSE_RANGE, capacity=len(want) - 1)
    dev = torch.device("cuda", 0)
    tens = [torch.from_numpy(c).to(dev) for c in clouds]
    m = len(want)
    sentinel = torch.full((m + 16, 4), 123.5, dtype=torch.float32, device=dev)
    out, dper, n = api.fuse_scans_dev(ctx, tens, poses, *FUSE_RANGE, out=sentinel, capacity=m - 1)
    res = out.cpu().numpy()
    assert int(n.item()) == m and np.array_equal(dper.cpu().numpy(), wper)
    assert fuse_ref.same(res[:m - 1], want[:m - 1]) and np.all(res[m - 1:] == 123.5)
    out, dper, n = api.fuse_scans_dev(ctx, tens, poses, *FUSE_RANGE)
    assert int(n.item()) == m and fuse_ref.same(out[:m].cpu().numpy(), want)
    ctx.use_own_stream()


# ---- K30 ---------------------------------------------------------------------------------------------------------------------------------------
COLOR_RANGE = (1.5, 35.0)
NOT_SKY = (10, 200, 30)


def _colour_kept(cloud, T, image):
    """per point: the restatement keeps it"""
    hit, px, py = cr.project(cloud[:, :3], T[:3].reshape(12), image.shape[0], image.shape[1], *COLOR_RANGE)
    word = np.zeros(len(cloud), np.uint32)
    word[hit] = cr.colour_word(image[py[hit], px[hit]])
    return word != 0


def _colorize_edge_pairs():
    rng = np.random.default_rng(35)
    sizes = list(tcg.SIZES) + EDGE_SIZES
    shapes = [(7, 13), (720, 1440), (33, 65)]
    plant = tcg._sky_edges()
    assert not cr.is_sky(cr.hsv_u8(np.array([NOT_SKY], np.uint8)))[0]
    clouds, Ts, images = [], [], []
    for k, n in enumerate(sizes):
        c = tcg._cloud(rng, n)
        T = None if k == 2 else tcg.POSES[k % 3]
        rows, cols = shapes[k % 3]
        kept, dropped = _edge_pattern(n) if n in EDGE_SIZES else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        c[kept, :3] = rng.uniform(2.0, 9.0, (len(kept), 3))
        c[dropped[0::2], :3] = (0.0, 0.0, 40.0); c[dropped[1::2], :3] = (np.nan, 1.0, 2.0)             # beyond max_dist, no position
        im = tcg._image(rng, rows, cols, c, T, plant)
        if len(kept):
            hit, px, py = cr.project(c[kept, :3], T[:3].reshape(12), rows, cols, *COLOR_RANGE)
            assert hit.all()
            im[py, px] = NOT_SKY
            mask = _colour_kept(c, T, im)
            assert mask[kept].all() and not mask[dropped].any() and 0.1 < mask.mean() < 0.9              # by the restatement: a mix at every edge
        clouds.append(c); Ts.append(T); images.append(im)
    return clouds, Ts, images


def test_colorize_scans_of_more_than_one_tile(ctx):
    import torch
    from panovlm_amd import api
    clouds, Ts, images = _colorize_edge_pairs()
    want, wper = tcg._want(clouds, Ts, images)
    got, per = api.colorize_scans(ctx, clouds, Ts, images, *COLOR_RANGE)
    assert np.array_equal(per, wper) and cr.same(got, want) and per[2] == 0
    dev = torch.device("cuda", ctx.device)
    out, dper, n = api.colorize_scans_dev(ctx, [torch.from_numpy(c).to(dev) for c in clouds], Ts, [torch.from_numpy(im).to(dev) for im in images], *COLOR_RANGE)
    torch.cuda.synchronize()
    m = int(n.item())
    assert m == len(want) and np.array_equal(dper.cpu().numpy(), wper) and cr.same(out[:m].cpu().numpy(), want)
    ctx.use_own_stream()


def test_colorize_scan_past_one_trip(ctx):
    """2 SCAN + 1 pairs of 0 to 300 points on two tiny images: one piece, more tiles than one trip of k_tile_scan"""
    import torch
    import panovlm_amd as pv
    from panovlm_amd import api
    rng = np.random.default_rng(36)
    sizes = _many_sizes(rng, 2 * SCAN + 1)
    plant = tcg._sky_edges()
    shared = []
    for rows, cols in ((7, 13), (33, 65)):
        im = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        sky = rng.random((rows, cols)) < 0.4
        im[sky] = plant[rng.integers(0, len(plant), int(sky.sum()))]
        shared.append(im)
    clouds = [tcg._cloud(rng, n) for n in sizes]
    Ts = [None if k % 101 == 7 else tcg.POSES[k % 3] for k in range(len(sizes))]
    images = [shared[k % 2] for k in range(len(sizes))]
    with_tile = np.array([n > 0 and T is not None for n, T in zip(sizes, Ts)])
    assert int(sizes.sum()) <= ce.PIECE_POINTS and len(sizes) <= ce.PIECE_PAIRS and with_tile.sum() > SCAN and (sizes == 0).sum() > 10
    want, wper = tcg._want(clouds, Ts, images)
    last_of_trip = int(np.flatnonzero(np.cumsum(with_tile) == SCAN)[0])                                  # the pair of tile SCAN - 1
    assert 0 < wper[:last_of_trip + 1].sum() < len(want) and (wper > 0).sum() > SCAN                     # records before and behind the second trip's first tile
    got, per = api.colorize_scans(ctx, clouds, Ts, images, *COLOR_RANGE)
    assert np.array_equal(per, wper) and cr.same(got, want)
    with pytest.raises(pv.PvlmError):
        api.colorize_scans(ctx, clouds, Ts, images, *COLOR_RANGE, capacity=len(want) - 1)
    dev = torch.device("cuda", ctx.device)
    tc = [torch.from_numpy(c).to(dev) for c in clouds]
    ts = [torch.from_numpy(im).to(dev) for im in shared]
    ti = [ts[k % 2] for k in range(len(sizes))]
    m = len(want)
    small = torch.full((m + 16, 4), 7.0, dtype=torch.float32, device=dev)
    _, dper, n = api.colorize_scans_dev(ctx, tc, Ts, ti, *COLOR_RANGE, out=small, capacity=m - 1)
    torch.cuda.synchronize()
    s = small.cpu().numpy()
    assert int(n.item()) == m and np.array_equal(dper.cpu().numpy(), wper) and cr.same(s[:m - 1], want[:m - 1]) and (s[m - 1:] == 7.0).all()
    out, dper, n = api.colorize_scans_dev(ctx, tc, Ts, ti, *COLOR_RANGE)
    torch.cuda.synchronize()
    assert int(n.item()) == m and cr.same(out[:m].cpu().numpy(), want)
    ctx.use_own_stream()


# ---- the plane-run table -------------------------------------------------------------------------------------------------------------------------
PLANE_CHUNK = 512
PLANE_ROWS = PLANE_CHUNK * (SCAN + 1) + 1                            # SCAN + 2 chunks: the scan of the chunks' run counts takes a second trip


@pytest.fixture(scope="module")
def plane_problem():
    """(rows, offsets, aa, t, starts): segments of 0, 1 and PLANE_ROWS rows, the "mixed" pattern of tests/test_plane_runs_gpu.py continued over the whole length:
    runs of 1 to 7 rows, and long runs over the chunk boundaries on both sides of the trip boundary"""
    rng = np.random.default_rng(47)
    aa, t = synth.random_poses(rng, tpr.F)
    n = 1 + PLANE_ROWS
    seg_of = np.concatenate([[1], np.full(PLANE_ROWS, 2)])
    P = rng.normal(size=(n, 3)) * 4.0
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o = rng.choice([1e-4, 5e-3, 0.05, 0.5], size=n) * rng.choice([-1.0, 1.0], size=n)
    d = np.empty(n)
    for s in (1, 2):
        r, k = tpr.REF[s], tpr.NEI[s]
        M = synth.rodrigues(aa[r]) @ synth.rodrigues(-aa[k])
        Pr = (P[seg_of == s] - t[k]) @ M.T + t[r]
        d[seg_of == s] = -(nrm[seg_of == s] * Pr).sum(1) + o[seg_of == s]
    rows = np.concatenate([P, nrm, d[:, None]], axis=1)
    off = np.array([0, 0, 1, n], np.int64)
    start = np.zeros(PLANE_ROWS, bool)
    at = np.cumsum(rng.integers(1, 8, size=PLANE_ROWS))
    start[0] = True; start[at[at < PLANE_ROWS]] = True
    for c in (1, SCAN - 1, SCAN, SCAN + 1):                          # one plane from 12 rows before the chunk boundary to 19 behind it
        start[c * PLANE_CHUNK - 12:c * PLANE_CHUNK + 19] = False; start[c * PLANE_CHUNK - 12] = True
    seg = rows[1:]
    first = np.maximum.accumulate(np.where(start, np.arange(PLANE_ROWS), 0))
    seg[:, 3:7] = seg[first, 3:7]
    return rows, off, aa, t, start


@pytest.mark.parametrize("wave", [0, 1])
def test_plane_runs_scan_past_one_trip(ctx, monkeypatch, plane_problem, wave):
    import panovlm_amd as pv
    rows, off, aa, t, start = plane_problem
    kind, flags, loss, loss_a = 1, 0, 1, 2 * np.pi / 180
    make = lambda: pv.ResidualSet.upload(ctx, kind, rows, off, tpr.REF, tpr.NEI, flags=flags, weight=1.3)
    a, _ = tpr._packed(ctx, monkeypatch, 0, wave, make, aa, t, loss, loss_a)
    b, state = tpr._packed(ctx, monkeypatch, 1, wave, make, aa, t, loss, loss_a)
    words = np.ascontiguousarray(rows[1:, 3:7]).view(np.uint64)
    starts = np.ones(PLANE_ROWS, bool)
    starts[1:] = np.any(words[1:] != words[:-1], axis=1) | (np.arange(1, PLANE_ROWS) % PLANE_CHUNK == 0)
    chunks = -(-PLANE_ROWS // PLANE_CHUNK)
    assert chunks == SCAN + 2 and starts[PLANE_CHUNK * SCAN] and not starts[PLANE_CHUNK * SCAN + 1:PLANE_CHUNK * SCAN + 19].any()
    assert state["runs"] == 1 + int(starts.sum()) and PLANE_ROWS > 1.25 * starts.sum()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
