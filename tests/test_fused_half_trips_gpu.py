"""The block form k_eval_fused on dense half-trips: lane t of a wave takes rows t and 64 + t of the wave's 128 (two halves of 64 consecutive rows, a half being
the slot of a ballot), and the plane-run forms have a second schedule that keeps one half's gather in flight behind the other half's arithmetic
(PVLM_HALF_ROTATE=1, csrc/pvlm_eval.hip; off by default, both schedules are in the library).

The set-up is that of test_fused_point_table_gpu.py: six synthetic scans of 2 048 points (synthetic.make_scan(k, cols=128, downsample_targets=0.2)), every scan
against its +-2 neighbours, and neighbours truncated by bisection over the accepted query numbers so that a pair has exactly the wanted rows.  PVLM_FUSED_CHUNK
is 512 (one trip of the workgroup per chunk) and 1024 (a second trip: the rotation crosses a trip boundary).  Segment lengths, the edges of
  a half                 0, 1, 63, 64, 65
  a wave's trip          127, 128, 129 (and 191, 192, 193: the second wave's first half)
  a workgroup's trip     511, 512, 513
  a chunk of two trips   1023, 1024, 1025; 1537: a chunk of one row behind full ones
Every form evaluates the same rows in the same order with the same lane-to-row mapping and the same reduction tree, so the packed normal equations are the
SAME BITS under every setting of PVLM_PLANE_RUNS, PVLM_POINT_TABLE, PVLM_DISPATCH_ORDER and PVLM_HALF_ROTATE; against the set's own materialised rows they
agree to the tolerance of the fused-against-materialised comparison of test_full_size_gpu.py (rtol 1e-9, atol 1e-12 of the largest entry)."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TARGETS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 511, 512, 513, 1023, 1024, 1025, 1537)
F = 6
TOL, THR = 0.05, 1.0
KEEP = 0x100
KINDS = [(1, 1), (1, 0), (0, 0)]          # (kind, flags): Angle with normalize, Angle, Meter
CHUNKS = (512, 1024)
# (plane runs, point table, dispatch order, rotation): every combination.  Without the plane runs there is no table, without the table no order: those
# settings are then ignored by the library, which is part of what is asserted.
FORMS = list(itertools.product((0, 1), repeat=4))


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _env(mp, form, chunk):
    runs, table, order, rotate = form
    mp.setenv("PVLM_PLANE_RUNS", str(runs))
    mp.setenv("PVLM_POINT_TABLE", str(table))
    mp.setenv("PVLM_DISPATCH_ORDER", str(order))
    mp.setenv("PVLM_HALF_ROTATE", str(rotate))
    mp.setenv("PVLM_FUSED_CHUNK", str(chunk))
    mp.setenv("PVLM_WAVE_UNITS", "0")


def _cut(scan, lo, hi):
    s = dict(scan)
    s["flat_xyz"] = np.ascontiguousarray(scan["flat_xyz"][lo:hi]); s["flat_tag"] = np.ascontiguousarray(scan["flat_tag"][lo:hi])
    return s


@pytest.fixture(scope="module")
def world(ctx):
    """The scans, the pair list with the cut neighbours, and the length every cut pair must have."""
    import panovlm_amd as pv
    from panovlm_amd import synthetic as sy
    mp = pytest.MonkeyPatch()
    _env(mp, (1, 1, 1, 1), 512)
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
    by_rows = sorted(range(len(ref)), key=lambda p: -len(accepted[p]))
    cuts, used = [], set()
    for L in sorted(TARGETS, reverse=True):                                    # the pairs with the most rows take the longest targets
        p = next(p for p in by_rows if int(nei[p]) not in used or len(used) >= F)
        used.add(int(nei[p]))
        a = accepted[p]
        assert len(a) >= L, "no pair accepts %d rows" % L
        lo, hi = 0, 2048                                                       # the largest m with exactly L accepted queries below it
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
    # every cut cloud is a neighbour handle of its own, used by every reference scan of the scan it was cut from
    R, N, ids_r, ids_n, want = [dev[r] for r in ref], [dev[n] for n in nei], list(ref), list(nei), {}
    for c, (r0, n, lo, hi, L) in enumerate(cuts):
        for r in [int(a) for a, b in zip(ref, nei) if int(b) == n]:
            if r == r0:
                want[len(R)] = L
            R.append(dev[r]); N.append(cut_dev[c]); ids_r.append(r); ids_n.append(n)
    poses = [sy.pose_params(*sy.estimated_pose(k)) for k in range(F)]
    aa = np.array([p[0] for p in poses]); t = np.array([p[1] for p in poses])
    mp.undo()
    yield dict(R=R, N=N, ref=np.array(ids_r, np.int32), nei=np.array(ids_n, np.int32), want=want, aa=aa, t=t)
    for s in dev + cut_dev:
        s.close()


def _loss_a(kind):
    return 0.2 if kind == 0 else 2 * np.pi / 180


def _packed(ctx, world, rs, loss, kind, twice=False):
    import panovlm_amd as pv
    from panovlm_amd import sharding
    ui, uj = sharding.unordered_pairs(world["ref"], world["nei"])
    ctx.set_poses(world["aa"], world["t"])
    neq = pv.NormalEq(ctx, F, ui, uj)
    packed = neq.accumulate(rs, loss, _loss_a(kind))
    again = neq.accumulate(rs, loss, _loss_a(kind)) if twice else None
    neq.close()
    return (packed, again) if twice else packed


def _from_rows(ctx, world, rs, loss, kind):
    """The packed system assembled in numpy from the set's own materialised r and J (pvlm_eval_dev into torch tensors)."""
    import torch
    from panovlm_amd import sharding
    from tests import synth
    ctx.set_poses(world["aa"], world["t"])
    dev = torch.device("cuda", 0)
    r = torch.empty(max(rs.n, 1), dtype=torch.float64, device=dev); J = torch.empty((max(rs.n, 1), 12), dtype=torch.float64, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    rs.eval_dev(r.data_ptr(), J.data_ptr())
    rh, Jh = r.cpu().numpy()[:rs.n], J.cpu().numpy()[:rs.n]
    ctx.use_own_stream()
    off = rs.download()[0]
    blocks = synth.pair_blocks_from_jacobian(rh, Jh, off, loss, _loss_a(kind))
    ui, uj = sharding.unordered_pairs(world["ref"], world["nei"])
    return sharding.pack_from_pair_blocks(blocks, world["ref"], world["nei"], F, ui, uj)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _close(got, want):
    return np.allclose(got, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())


def test_lengths_are_hit_and_the_debug_reader_returns_numbers_and_points(ctx, monkeypatch, world):
    """(c): one {run, query} word per row: the stored query numbers are the association's and the table entries they name are the rows' points, bit for bit."""
    _env(monkeypatch, (1, 1, 1, 1), 512)
    rs = ctx.assoc_point2plane(world["R"], world["N"], TOL, THR, kind=1, flags=1 | KEEP)
    assert rs.point_table()["in_use"] and rs.plane_runs()["in_use"]
    off, _, _, rows = rs.download()
    lengths = np.diff(off)
    for p, L in world["want"].items():
        assert lengths[p] == L, (p, L, lengths[p])
    assert set(TARGETS) <= set(int(x) for x in lengths)
    qidx, _ = rs.assoc_debug()
    qnum, pts = rs.point_table_debug()
    assert np.array_equal(qnum.astype(np.int64), qidx.astype(np.int64))
    cols = np.ascontiguousarray(np.asarray(rows).reshape(-1, 7)[:, :3])
    assert _same_bits(cols, pts)
    rs.close()


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind,flags", KINDS)
def test_every_form_gives_the_same_bits_and_agrees_with_the_rows(ctx, world, kind, flags, chunk):
    """(a), (b), (d) for the sets of the association: sixteen settings, trivial and Huber loss."""
    mp = pytest.MonkeyPatch()
    try:
        base = None
        for form in FORMS:
            _env(mp, form, chunk)
            rs = ctx.assoc_point2plane(world["R"], world["N"], TOL, THR, kind=kind, flags=flags)
            assert rs.plane_runs()["in_use"] == bool(form[0])
            assert rs.point_table()["in_use"] == bool(form[0] and form[1])
            got = {}
            for loss in (0, 1):
                got[loss], again = _packed(ctx, world, rs, loss, kind, twice=True)
                assert _same_bits(got[loss], again), (form, loss)                                   # (d)
            if base is None:
                base = got
                for loss in (0, 1):
                    assert np.isfinite(base[loss]).all() and np.any(base[loss] != 0.0)
                    assert _close(base[loss], _from_rows(ctx, world, rs, loss, kind)), loss         # (b)
            for loss in (0, 1):
                assert _same_bits(base[loss], got[loss]), (form, loss)                              # (a)
            rs.close()
    finally:
        mp.undo()


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("kind,flags", KINDS)
def test_uploaded_set_streamed_block_form(ctx, world, kind, flags, chunk):
    """(e): the same rows uploaded (no table): the streamed columns with and without the plane runs, rotation on and off."""
    import panovlm_amd as pv
    mp = pytest.MonkeyPatch()
    try:
        _env(mp, (1, 1, 1, 1), chunk)
        rs = ctx.assoc_point2plane(world["R"], world["N"], TOL, THR, kind=kind, flags=flags)
        off, pr, pn, rows = rs.download()
        rs.close()
        base = None
        for form in [f for f in FORMS if f[1] == 1 and f[2] == 1]:     # an uploaded set has no table and no order: plane runs and rotation
            _env(mp, form, chunk)
            up = pv.ResidualSet.upload(ctx, kind, rows, off, pr, pn, flags=flags)
            assert not up.point_table()["in_use"] and up.plane_runs()["in_use"] == bool(form[0])
            got = {}
            for loss in (0, 1):
                got[loss], again = _packed(ctx, world, up, loss, kind, twice=True)
                assert _same_bits(got[loss], again), (form, loss)
            if base is None:
                base = got
                for loss in (0, 1):
                    assert np.isfinite(base[loss]).all() and np.any(base[loss] != 0.0)
                    assert _close(base[loss], _from_rows(ctx, world, up, loss, kind)), loss
            for loss in (0, 1):
                assert _same_bits(base[loss], got[loss]), (form, loss)
            up.close()
    finally:
        mp.undo()
