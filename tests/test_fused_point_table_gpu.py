"""The point-table form of k_eval_fused (pvlm_resset::point_table) and its dispatch order against the streamed point columns of the same set.

Six synthetic scans of 2 048 points (synthetic.make_scan(k, cols=128, downsample_targets=0.2)), every scan against its +-2 neighbours, so every neighbour scan
is shared by up to four pairs; PVLM_FUSED_CHUNK=512.  The segment lengths at which the block form can go wrong are reached by truncating a neighbour's query
cloud to its first m points: queries are independent, so the rows a pair accepts under the truncated cloud are its accepted queries below m, and the largest m
that leaves exactly the wanted rows is found by bisection over the accepted query numbers of the full cloud (the cut cloud then ends in rejected queries
wherever the full one has some there).  Lengths and what each is there for:
  0, 1, 2      no rows; an odd last row whose pad row names run 0 and query 0; one full pair of rows
  511, 512     one chunk, with and without the pad row
  513          a second chunk of one row
  1025, 1537   a third and a fourth chunk of one row
One more neighbour is cut at both ends so that its first and its last query are rejected.  Every truncated cloud is a neighbour handle of its own and is used
by every reference scan of the scan it was cut from: the set has the 24 full pairs and the pairs of the nine cut clouds.

Same rows, same order, same lane-to-row mapping and reduction tree: the packed normal equations under PVLM_POINT_TABLE=0 and =1, and under
PVLM_DISPATCH_ORDER=0 and =1, must be the SAME BITS."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TARGETS = (0, 1, 2, 511, 512, 513, 1025, 1537)
F = 6
TOL, THR = 0.05, 1.0
KEEP = 0x100


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _env(monkeypatch, point_table, order, chunk=512, wave=0):
    monkeypatch.setenv("PVLM_POINT_TABLE", str(point_table))
    monkeypatch.setenv("PVLM_DISPATCH_ORDER", str(order))
    monkeypatch.setenv("PVLM_FUSED_CHUNK", str(chunk))
    monkeypatch.setenv("PVLM_WAVE_UNITS", str(wave))
    monkeypatch.setenv("PVLM_PLANE_RUNS", "1")


def _cut(scan, lo, hi):
    s = dict(scan)
    s["flat_xyz"] = np.ascontiguousarray(scan["flat_xyz"][lo:hi]); s["flat_tag"] = np.ascontiguousarray(scan["flat_tag"][lo:hi])
    return s


@pytest.fixture(scope="module")
def world(ctx):
    """The scans, the full pair list, the accepted query numbers of every full pair, and the pair list with the cut neighbours."""
    import panovlm_amd as pv
    from panovlm_amd import synthetic as sy
    mp = pytest.MonkeyPatch()
    _env(mp, 1, 1)
    host = [sy.make_scan(k, cols=128, downsample_targets=0.2) for k in range(F)]
    assert all(len(s["flat_xyz"]) == 2048 for s in host)
    dev = [pv.Scan(ctx, s) for s in host]
    ref, nei = sy.pair_list(F, 4)
    rs = ctx.assoc_point2plane([dev[r] for r in ref], [dev[n] for n in nei], TOL, THR, flags=1 | KEEP)
    off = rs.download()[0]
    qidx, _ = rs.assoc_debug()
    rs.close()
    accepted = [qidx[off[p]:off[p + 1]].astype(np.int64) for p in range(len(ref))]
    assert all(np.all(np.diff(a) > 0) for a in accepted)                       # rows are in query order
    # the pairs with the most rows take the longest targets; one neighbour scan per target
    by_rows = sorted(range(len(ref)), key=lambda p: -len(accepted[p]))
    cuts, used = [], set()
    for L in sorted(TARGETS, reverse=True):
        p = next(p for p in by_rows if int(nei[p]) not in used or len(used) >= F)
        used.add(int(nei[p]))
        a = accepted[p]
        assert len(a) >= L, "no pair accepts %d rows" % L
        # bisection: the largest m with exactly L accepted queries below it (the count is monotone in m)
        lo, hi = 0, 2048
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if np.searchsorted(a, mid) <= L:
                lo = mid
            else:
                hi = mid - 1
        assert np.searchsorted(a, lo) == L
        cuts.append((int(ref[p]), int(nei[p]), 0, lo, L))
    # both ends rejected: from the first to the last rejected query of the pair with the fewest rows
    p = by_rows[-1]
    rej = np.setdiff1d(np.arange(2048), accepted[p])
    assert len(rej) >= 2
    cuts.append((int(ref[p]), int(nei[p]), int(rej[0]), int(rej[-1]) + 1, int(np.sum((accepted[p] > rej[0]) & (accepted[p] < rej[-1])))))
    cut_dev = [pv.Scan(ctx, _cut(host[n], lo, hi)) for (_, n, lo, hi, _) in cuts]
    R, N, ids_r, ids_n, want, cut_pair = [dev[r] for r in ref], [dev[n] for n in nei], list(ref), list(nei), {}, []
    for c, (r0, n, lo, hi, L) in enumerate(cuts):
        for r in [int(a) for a, b in zip(ref, nei) if int(b) == n]:             # every reference scan of the cut neighbour
            if r == r0:
                want[len(R)] = L; cut_pair.append(len(R))
            R.append(dev[r]); N.append(cut_dev[c]); ids_r.append(r); ids_n.append(n)
    poses = [sy.pose_params(*sy.estimated_pose(k)) for k in range(F)]
    aa = np.array([p[0] for p in poses]); t = np.array([p[1] for p in poses])
    mp.undo()
    yield dict(R=R, N=N, ref=np.array(ids_r, np.int32), nei=np.array(ids_n, np.int32), want=want, aa=aa, t=t, cuts=cuts, cut_pair=cut_pair)
    for s in dev + cut_dev:
        s.close()


def _assoc(ctx, world, kind, flags):
    return ctx.assoc_point2plane(world["R"], world["N"], TOL, THR, kind=kind, flags=flags)


def _packed(ctx, world, rs, loss, kind):
    import panovlm_amd as pv
    from panovlm_amd import sharding
    ui, uj = sharding.unordered_pairs(world["ref"], world["nei"])
    ctx.set_poses(world["aa"], world["t"])
    neq = pv.NormalEq(ctx, F, ui, uj)
    packed = neq.accumulate(rs, loss, 0.2 if kind == 0 else 2 * np.pi / 180)
    neq.close()
    return packed


def test_segment_lengths_are_hit_and_numbers_and_points_match(ctx, monkeypatch, world):
    """(a), (b), (d): the lengths the set-up aimed at are there; the stored query numbers are the association's; the table entry they name is the row's point."""
    _env(monkeypatch, 1, 1)
    rs = _assoc(ctx, world, 1, 1 | KEEP)
    state = rs.point_table()
    assert state["in_use"] and rs.plane_runs()["in_use"]
    assert state["tables"] == F + len(world["cuts"])                            # one per distinct neighbour handle
    off, _, _, rows = rs.download()
    lengths = np.diff(off)
    for p, L in world["want"].items():
        assert lengths[p] == L, (p, L, lengths[p])
    assert set(TARGETS) <= set(int(x) for x in lengths)
    qidx, _ = rs.assoc_debug()
    qnum, pts = rs.point_table_debug()
    assert np.array_equal(qnum.astype(np.int64), qidx.astype(np.int64))
    cols = np.ascontiguousarray(np.asarray(rows).reshape(-1, 7)[:, :3])
    assert np.array_equal(cols.view(np.uint64), np.ascontiguousarray(pts).view(np.uint64))
    # (d): the neighbour cut at both ends: its first and last query have no row
    r0, n, lo, hi, L = world["cuts"][-1]
    p = world["cut_pair"][-1]
    seg = qnum[off[p]:off[p + 1]]
    assert len(seg) == L and (L == 0 or (seg[0] > 0 and seg[-1] < hi - lo - 1))
    # the grid covers every work-list entry; padding only makes it longer
    blocks = int(np.sum((lengths + 511) // 512))
    assert state["positions"] >= blocks
    rs.close()


@pytest.fixture(scope="module")
def packed_by_form(ctx, world):
    """(kind, flags, chunk) -> {(point_table, order): {loss: packed}}: every set is made once per form and linearised under both losses."""
    cache = {}

    def get(kind, flags, chunk):
        key = (kind, flags, chunk)
        if key not in cache:
            mp = pytest.MonkeyPatch()
            forms = {}
            for form in ((0, 1), (1, 1), (1, 0)):
                _env(mp, form[0], form[1], chunk)
                rs = _assoc(ctx, world, kind, flags)
                assert rs.point_table()["in_use"] == bool(form[0])
                forms[form] = {loss: _packed(ctx, world, rs, loss, kind) for loss in (0, 1)}
                rs.close()
            mp.undo()
            cache[key] = forms
        return cache[key]
    return get


@pytest.mark.parametrize("loss", [0, 1])
@pytest.mark.parametrize("kind,flags,chunk", [(1, 1, 512), (1, 0, 512), (0, 0, 512), (1, 1, 1024)])
def test_same_bits_with_and_without_table_and_order(packed_by_form, kind, flags, chunk, loss):
    """(c): Angle with and without normalize, Meter; Huber and trivial loss.  Chunk 1024: a second 512-row trip inside a chunk."""
    forms = packed_by_form(kind, flags, chunk)
    base = forms[(0, 1)][loss]
    assert np.isfinite(base).all() and np.any(base != 0.0)
    assert np.array_equal(base.view(np.uint64), forms[(1, 1)][loss].view(np.uint64))
    assert np.array_equal(forms[(1, 0)][loss].view(np.uint64), forms[(1, 1)][loss].view(np.uint64))


def test_wave_form_and_uploaded_sets_keep_the_old_form(ctx, monkeypatch, world):
    """(e): a wave-form set and an uploaded set do not take the form, whatever PVLM_POINT_TABLE says, and give what they gave."""
    import panovlm_amd as pv
    out = {}
    for pt in (0, 1):
        _env(monkeypatch, pt, 1, wave=1)
        rs = _assoc(ctx, world, 1, 1)
        assert not rs.point_table()["in_use"]
        out["wave", pt] = _packed(ctx, world, rs, 1, 1)
        off, pr, pn, rows = rs.download()
        rs.close()
        _env(monkeypatch, pt, 1, wave=0)
        up = pv.ResidualSet.upload(ctx, 1, rows, off, pr, pn, flags=1)
        assert not up.point_table()["in_use"] and up.plane_runs()["in_use"]
        with pytest.raises(pv.PvlmError):
            up.point_table_debug()
        out["up", pt] = _packed(ctx, world, up, 1, 1)
        up.close()
    for form in ("wave", "up"):
        assert np.isfinite(out[form, 0]).all() and np.any(out[form, 0] != 0.0)
        assert np.array_equal(out[form, 0].view(np.uint64), out[form, 1].view(np.uint64))
