"""The run word of the plane-run form is fetched one trip ahead (k_eval_fused / k_eval_fused_wave on a plane-run table): every trip count and every last-trip
shape against the 7-column form of the same set.  As in tests/test_plane_runs_gpu.py each set is built once under PVLM_PLANE_RUNS=0 and once under =1 and
linearised with NormalEq.accumulate: same rows, same order, same reduction tree, so the packed normal equations must be the SAME BITS.

Block form: PVLM_FUSED_CHUNK=1536, a full chunk takes three 512-row trips.  Segment lengths and what each is there for:
  0, 1, 2      no rows; an odd last row whose pad row names entry 0; one full pair of rows
  511, 512     one trip, with and without the pad row
  513          a second trip of one row (it re-reads its own word)
  1025         a third trip of one row
  1535, 1536   three trips, the last one short by a row / full: the chunk boundary
  1537         a one-row last chunk
  3077         two full chunks and a third of five rows
Wave form: PVLM_WAVE_CHUNK=512, four 128-row trips per chunk: 1, 127, 128, 129, 257, 513.

Run patterns: every row its own plane, one plane for all, and runs of 1-7 rows with one run laid across every 128-row (so every 512-row) trip boundary."""
import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu

BLOCK_COUNTS = (0, 1, 2, 511, 512, 513, 1025, 1535, 1536, 1537, 3077)
WAVE_COUNTS = (1, 127, 128, 129, 257, 513)
BLOCK_CHUNK, WAVE_CHUNK = 1536, 512
PATTERNS = ("distinct", "equal", "runs")


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _run_starts(pattern, n):
    """start[i]: row i of an n-row segment begins a new plane."""
    start = np.zeros(n, bool)
    if n == 0:
        return start
    if pattern == "distinct":
        start[:] = True
    elif pattern == "runs":
        rng = np.random.default_rng(11 + n)
        i = 0
        while i < n:
            start[i] = True
            i += int(rng.integers(1, 8))
        for b in range(128, n, 128):                 # rows b - 2 .. b + 1 are one run: it crosses the trip boundary at b
            start[b - 1:min(b + 2, n)] = False
            start[b - 2] = True
    start[0] = True
    return start


def _chain(counts):
    """Segment p is the pair (p, p + 1) of a chain of len(counts) + 1 poses."""
    P = len(counts)
    return P + 1, np.arange(P, dtype=np.int32), np.arange(1, P + 1, dtype=np.int32)


def _problems(counts, seed):
    """pattern -> (rows, offsets, aa, t, starts): one draw of rows, the planes re-laid per pattern; starts[i] for every row of the set."""
    F, ref, nei = _chain(counts)
    rng = np.random.default_rng(seed)
    aa, t = synth.random_poses(rng, F)
    base, off = synth.random_resset(rng, 1, aa, t, ref, nei, counts)
    base = np.asarray(base, np.float64).reshape(-1, 7)
    out = {}
    for pattern in PATTERNS:
        rows = base.copy()
        starts = np.concatenate([_run_starts(pattern, c) for c in counts])
        for p, c in enumerate(counts):
            lo = int(off[p])
            seg = rows[lo:lo + c]
            first = np.maximum.accumulate(np.where(starts[lo:lo + c], np.arange(c), 0))
            seg[:, 3:7] = seg[first, 3:7]              # every row takes the plane of the first row of its run
            if pattern == "runs":
                for b in range(128, c, 128):
                    assert np.array_equal(seg[b - 2:b + 2, 3:7], np.broadcast_to(seg[b - 2, 3:7], (min(b + 2, c) - b + 2, 4)))
        rows.setflags(write=False)
        out[pattern] = (rows, off, aa, t, starts)
    return out


@pytest.fixture(scope="module")
def block_problems():
    return _problems(BLOCK_COUNTS, 60)


@pytest.fixture(scope="module")
def wave_problems():
    return _problems(WAVE_COUNTS, 61)


def _expected_runs(rows, off, counts, chunk):
    """Runs the finalize pass must count: a row starts one when it is the first of its chunk or its plane differs from the previous row's in any bit."""
    total = 0
    for p, c in enumerate(counts):
        if c == 0:
            continue
        seg = np.ascontiguousarray(rows[int(off[p]):int(off[p]) + c, 3:7]).view(np.uint64)
        s = np.ones(c, bool)
        s[1:] = np.any(seg[1:] != seg[:-1], axis=1) | (np.arange(1, c) % chunk == 0)
        total += int(s.sum())
    return total


def _packed(ctx, monkeypatch, plane_runs, wave, fused_chunk, problem, counts, kind, flags, loss):
    import panovlm_amd as pv
    rows, off, aa, t, _ = problem
    F, ref, nei = _chain(counts)
    monkeypatch.setenv("PVLM_PLANE_RUNS", str(plane_runs))
    monkeypatch.setenv("PVLM_WAVE_UNITS", str(wave))
    monkeypatch.setenv("PVLM_WAVE_CHUNK", str(WAVE_CHUNK))
    if fused_chunk is None:
        monkeypatch.delenv("PVLM_FUSED_CHUNK", raising=False)
    else:
        monkeypatch.setenv("PVLM_FUSED_CHUNK", str(fused_chunk))
    rs = pv.ResidualSet.upload(ctx, kind, rows, off, ref, nei, flags=flags, weight=1.3)
    state = rs.plane_runs()
    assert state["in_use"] == bool(plane_runs)
    ctx.set_poses(aa, t)
    neq = pv.NormalEq(ctx, F, ref, nei)
    packed = neq.accumulate(rs, loss, 0.2 if kind == 0 else 2 * np.pi / 180)
    neq.close(); rs.close()
    return packed, state


def _same_bits(ctx, monkeypatch, wave, fused_chunk, chunk, problem, counts, kind, flags, loss):
    a, _ = _packed(ctx, monkeypatch, 0, wave, fused_chunk, problem, counts, kind, flags, loss)
    b, state = _packed(ctx, monkeypatch, 1, wave, fused_chunk, problem, counts, kind, flags, loss)
    assert state["runs"] == _expected_runs(problem[0], problem[1], counts, chunk)       # the chunk asked for is the chunk in use
    assert np.isfinite(a).all() and np.any(a != 0.0)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("loss", [0, 1])
@pytest.mark.parametrize("kind,flags", [(0, 0), (1, 1)])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_block_form_three_trips_same_bits(ctx, monkeypatch, block_problems, pattern, kind, flags, loss):
    _same_bits(ctx, monkeypatch, 0, BLOCK_CHUNK, BLOCK_CHUNK, block_problems[pattern], BLOCK_COUNTS, kind, flags, loss)


@pytest.mark.parametrize("loss", [0, 1])
@pytest.mark.parametrize("kind,flags", [(0, 0), (1, 1)])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_wave_form_four_trips_same_bits(ctx, monkeypatch, wave_problems, pattern, kind, flags, loss):
    # PVLM_FUSED_CHUNK is set and must be ignored by a wave-form set: its chunk stays PVLM_WAVE_CHUNK
    _same_bits(ctx, monkeypatch, 1, BLOCK_CHUNK, WAVE_CHUNK, wave_problems[pattern], WAVE_COUNTS, kind, flags, loss)


def _one_segment(problems, counts, length):
    """The `length`-row segment of a problem as a set of its own (same rows, same poses)."""
    p = counts.index(length)
    rows, off, aa, t, starts = problems
    lo = int(off[p])
    return (rows[lo:lo + length], np.array([0, length], np.int64), aa[p:p + 2], t[p:p + 2], starts[lo:lo + length]), (length,)


def test_default_chunk_same_bits(ctx, monkeypatch, block_problems):
    """PVLM_FUSED_CHUNK unset: a 1 537-row set gets the 512-row chunk it always got (one trip per chunk)."""
    problem, counts = _one_segment(block_problems["runs"], BLOCK_COUNTS, 1537)
    _same_bits(ctx, monkeypatch, 0, None, 512, problem, counts, 1, 1, 1)


@pytest.mark.parametrize("value", ["0", "511", "1000", "66048", "131072", "junk"])
def test_fused_chunk_values_out_of_range_are_ignored(ctx, monkeypatch, block_problems, value):
    """Only a multiple of 512 from 512 to 65 536 is taken; anything else leaves the default (512 rows for a set this small)."""
    problem, counts = _one_segment(block_problems["runs"], BLOCK_COUNTS, 1537)
    _, state = _packed(ctx, monkeypatch, 1, 0, value, problem, counts, 1, 1, 1)
    assert state["runs"] == _expected_runs(problem[0], problem[1], counts, 512)


@pytest.mark.parametrize("value", [512, 1024, 65536])
def test_fused_chunk_ends_of_the_range_are_taken(ctx, monkeypatch, block_problems, value):
    problem, counts = _one_segment(block_problems["runs"], BLOCK_COUNTS, 1537)
    _same_bits(ctx, monkeypatch, 0, value, value, problem, counts, 1, 1, 1)
