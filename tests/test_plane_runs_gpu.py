"""The plane-run form of the fused point-to-plane evaluation (pvlm_resset::plane_runs) against the 7-column form: the same rows, visited in the
same order, with the same reduction tree — the packed normal equations must be the SAME BITS, NaN patterns included.  Each set is built once under
PVLM_PLANE_RUNS=0 and once under =1 (read at finalize) and linearised with NormalEq.accumulate.

Segments {0, 1, 1537}: with the 512-row chunk (the block form's minimum; PVLM_WAVE_CHUNK=512 for the wave form) the long one spans four chunks."""
import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 1537)
F = 4
REF = np.array([0, 1, 2], np.int32)
NEI = np.array([1, 2, 3], np.int32)
PATTERNS = ("distinct", "equal", "odd_pairs", "mixed", "nan")


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _run_starts(pattern, n):
    """start[i]: row i begins a new plane."""
    start = np.zeros(n, bool)
    start[0] = True
    if pattern == "distinct":
        start[:] = True
    elif pattern == "odd_pairs":            # [0] [1 2] [3 4] ...: every lane's two rows (2k, 2k + 1) straddle a run boundary
        start[1::2] = True
    elif pattern in ("mixed", "nan"):       # runs of 1..7 rows, and long runs over the chunk boundaries at 512 and 1024 (not over 1536)
        rng = np.random.default_rng(7)
        i = 0
        while i < n:
            start[i] = True
            i += int(rng.integers(1, 8))
        start[500:531] = False; start[500] = True
        start[1023:1026] = False; start[1023] = True
    return start


@pytest.fixture(scope="module")
def problems():
    """pattern -> (rows, offsets, aa, t); built once, never modified."""
    out = {}
    for k, pattern in enumerate(PATTERNS):
        rng = np.random.default_rng(40 + k)
        aa, t = synth.random_poses(rng, F)
        rows, off = synth.random_resset(rng, 1, aa, t, REF, NEI, COUNTS)
        lo, n = int(off[2]), COUNTS[2]
        seg = rows[lo:lo + n]
        first = np.maximum.accumulate(np.where(_run_starts(pattern, n), np.arange(n), 0))
        seg[:, 3:7] = seg[first, 3:7]                      # every row takes the plane of the first row of its run
        if pattern in ("mixed", "nan"):
            # two neighbouring single-row planes that differ only in the sign of a zero component
            seg[700, 3:7] = (0.0, 0.6, 0.8, -1.25); seg[701, 3:7] = (-0.0, 0.6, 0.8, -1.25); seg[702, 3:7] = (0.3, 0.4, 0.5, 0.1)
            assert seg[700, 3] == seg[701, 3] and np.signbit(seg[701, 3]) and not np.signbit(seg[700, 3])
        if pattern == "nan":
            # whatever a functor makes of a NaN plane (Meter: a NaN block), the two forms must agree bit for bit.  Rows 900 and 901 carry the SAME NaN
            # pattern (one run: a NaN equals its own bits, which no floating-point compare would say), row 902 a NaN with another payload (a new run)
            seg[900:902, 3:7] = np.nan
            seg[902:903, 3:7].view(np.uint64)[:] = np.array([np.nan]).view(np.uint64)[0] | np.uint64(1)
            assert np.isnan(seg[900:903, 3:7]).all()
        out[pattern] = (rows, off, aa, t)
    return out


def _packed(ctx, monkeypatch, plane_runs, wave, make_set, aa, t, loss, loss_a):
    import panovlm_amd as pv
    monkeypatch.setenv("PVLM_PLANE_RUNS", str(plane_runs))
    monkeypatch.setenv("PVLM_WAVE_UNITS", str(wave))
    monkeypatch.setenv("PVLM_WAVE_CHUNK", "512")
    rs = make_set()
    state = rs.plane_runs()
    assert state["in_use"] == bool(plane_runs)
    ctx.set_poses(aa, t)
    neq = pv.NormalEq(ctx, len(aa), [0, 1, 2], [1, 2, 3])
    packed = neq.accumulate(rs, loss, loss_a)
    neq.close(); rs.close()
    return packed, state


@pytest.mark.parametrize("wave", [0, 1])
@pytest.mark.parametrize("loss", [0, 1])
@pytest.mark.parametrize("kind,flags", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_plane_runs_same_bits(ctx, monkeypatch, problems, pattern, kind, flags, loss, wave):
    import panovlm_amd as pv
    rows, off, aa, t = problems[pattern]
    loss_a = 0.2 if kind == 0 else 2 * np.pi / 180
    make = lambda: pv.ResidualSet.upload(ctx, kind, rows, off, REF, NEI, flags=flags, weight=1.3)
    a, _ = _packed(ctx, monkeypatch, 0, wave, make, aa, t, loss, loss_a)
    b, state = _packed(ctx, monkeypatch, 1, wave, make, aa, t, loss, loss_a)
    # runs counted at finalize: one for the single-row segment + the long one's — a row starts a run when it is the first of its 512-row chunk or when its
    # plane differs from the previous row's in any bit
    seg = np.ascontiguousarray(rows[int(off[2]):, 3:7]).view(np.uint64)
    starts = np.ones(COUNTS[2], bool)
    starts[1:] = np.any(seg[1:] != seg[:-1], axis=1) | (np.arange(1, COUNTS[2]) % 512 == 0)
    assert state["runs"] == 1 + int(starts.sum())
    if pattern == "distinct":
        assert starts.all()
    if pattern == "equal":
        assert starts.sum() == 4
    if pattern == "odd_pairs":
        assert starts[1:511:2].all() and not starts[2:511:2].any()
    if pattern in ("mixed", "nan"):
        assert not starts[501:512].any() and starts[512] and not starts[513:531].any()       # the run over the chunk boundary is cut there
        assert starts[700] and starts[701] and starts[702]                                     # +0.0 / -0.0 are two planes
    if pattern == "nan":
        assert starts[900] and not starts[901] and starts[902] and starts[903]
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_plane_runs_same_bits_on_an_associated_set(ctx, monkeypatch):
    import panovlm_amd as pv
    from panovlm_amd import synthetic as sy
    scans = {k: sy.make_scan(k, cols=512, downsample_targets=0.2) for k in (0, 1)}
    dev = {k: pv.Scan(ctx, s) for k, s in scans.items()}
    aa, t = (np.array(x) for x in zip(*[sy.pose_params(*sy.estimated_pose(k)) for k in range(F)]))
    ui, uj = [0], [1]

    def linearise(plane_runs):
        monkeypatch.setenv("PVLM_PLANE_RUNS", str(plane_runs))
        rs = ctx.assoc_point2plane([dev[0], dev[1]], [dev[1], dev[0]], 0.05, 1.0, kind=pv.POINT2PLANE_ANGLE, flags=pv.FLAG_NORMALIZE_DISTANCE)
        state = rs.plane_runs()
        ctx.set_poses(aa[:2], t[:2])
        neq = pv.NormalEq(ctx, 2, ui, uj)
        packed = neq.accumulate(rs, pv.LOSS_HUBER, 2 * np.pi / 180)
        down = rs.download()
        neq.close(); rs.close()
        return packed, state, down

    a, sa, da = linearise(0)
    b, sb, db = linearise(1)
    assert not sa["in_use"] and sb["in_use"]
    n = len(da[3])
    assert n > 1000 and 0 < sb["runs"] < n               # neighbouring queries of a ring do share planes
    for x, y in zip(da, db):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    for d in dev.values():
        d.close()
