"""Huber by slot in the fused evaluation (pvlm_eval.hip, accumulate_row): a slot — the 64 rows a wave evaluates together: the rows of equal parity out
of 128 consecutive rows of a unit of work, lane = (row % 128) // 2 — that holds no Huber outlier accumulates without the weights; a slot with one takes
the general arithmetic.  Both must give what the form before gave.

Point2Plane_Angle rows with normalize_distance (tests/angle_form_rows.py), uploaded as segments of 1, 2, 129 and 1025 rows (an odd tail, the two rows
of a lane, more than one wave, a last trip with idle lanes) and one CONSTRUCTED segment of 1061 rows = 8 x 128 + 37 in which every kind of slot occurs:
   rows    0 ..  127   inliers only                              rows  640 ..  767   even rows outliers, odd rows inliers
   rows  128 ..  255   outliers only                             rows  768 ..  895   inliers and dead rows (|sd| < 1e-3: r = 0)
   rows  256 ..  383   ONE outlier: lane 0, even row (256)       rows  896 .. 1023   outliers only
   rows  384 ..  511   ONE outlier: lane 63, odd row (511)       rows 1024 .. 1060   the partly filled last trip, ONE outlier: row 1044
   rows  512 ..  639   outliers only
The inliers of that segment lie below 0.1 degrees and its outliers above 3 degrees, so that it has these slots under the 2 degrees of width (c) as
under the median of width (b) — asserted from the oracle's residuals before any device call.

Every set is evaluated under both values of PVLM_PLANE_RUNS and of PVLM_WAVE_UNITS and with two chunkings: the library's own (512 rows per workgroup
at this size: one trip; 2048 per wave: up to 9 trips of 128) and PVLM_FUSED_CHUNK=1536, with which a workgroup takes the 1025 and the 1061 rows in
three trips, the last one partly filled.

Three loss widths.  (a) wider than every |r|: no outlier, and HUBER equals TRIVIAL bit for bit (it did before: this pins the path without weights).
(b) half the smallest non-zero |r|: every live row is an outlier.  (c) the median non-zero |r|.  (b), (c) and the fixed 2 degrees are compared with
the blocks assembled in numpy from the oracle's extended-precision r and J at the tolerance of tests/test_angle_form_gpu.py; (c) once more with the
rows of every segment in reverse order, which moves every row into another lane and most into another slot."""
import itertools

import numpy as np
import pytest

from tests import angle_form_rows as af
from tests import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-6                       # of the block's largest entry: tests/test_angle_form_gpu.py
DEG = np.pi / 180
A_FIXED = 2 * DEG                 # the benchmark's width
IN_MAX, OUT_MIN = 0.1 * DEG, 3 * DEG
COUNTS = (1, 2, 129, 1025, 8 * 128 + 37)
REF = np.array([2, 3, 1, 2, 3], np.int32)
NEI = np.array([3, 2, 2, 0, 1], np.int32)
CON = 4                           # the constructed segment
FORMS = list(itertools.product((0, 1), (0, 1)))            # (plane runs, wave units)
CHUNKS = ("own", "1536")


def constructed_kinds():
    """'in' / 'out' / 'dead' for every row of the constructed segment (module docstring)"""
    n = COUNTS[CON]
    kind = np.array(["in"] * n, dtype=object)
    kind[128:256] = "out"
    kind[256] = "out"
    kind[511] = "out"
    kind[512:640] = "out"
    kind[640:768:2] = "out"
    kind[768:896:3] = "dead"
    kind[896:1024] = "out"
    kind[1044] = "out"
    return kind


def _row_with_offset(rng, aa, t, r, n, o):
    p, nrm = rng.normal(size=3) * 4.0, af._unit(rng)
    return af._row(aa, t, r, n, p, nrm, lambda a: o - a)


def build_rows(oracle, seed=77):
    rng = np.random.default_rng(seed)
    aa, t = synth.random_poses(rng, af.F)
    rows = []
    for p, count in enumerate(COUNTS[:CON]):
        rows += [af.class_row(rng, "random", aa, t, REF[p], NEI[p]) for _ in range(count)]
    # the constructed segment: candidates at chosen distances from their planes, sorted by the oracle's residual into the three kinds
    offs = {"in": (1.5e-3, 2e-3, 3e-3), "out": (1.0, 2.0, 4.0), "dead": (1e-4, 5e-4)}
    kind = constructed_kinds()
    pool = {}
    for k, need in (("in", int((kind == "in").sum())), ("out", int((kind == "out").sum())), ("dead", int((kind == "dead").sum()))):
        cand = np.array([_row_with_offset(rng, aa, t, REF[CON], NEI[CON], rng.choice(offs[k]) * rng.choice([-1.0, 1.0])) for _ in range(4 * need + 8)])
        rid = np.full(len(cand), REF[CON], np.int32); nid = np.full(len(cand), NEI[CON], np.int32)
        ro, _ = oracle.evaluate(1, synth.oracle_rows(1, cand), rid, nid, aa, t, normalize=True, extended=True)
        ok = {"in": (np.abs(ro) > 0) & (np.abs(ro) < 0.8 * IN_MAX), "out": np.abs(ro) > 1.25 * OUT_MIN, "dead": ro == 0}[k]
        assert ok.sum() >= need, (k, int(ok.sum()), need)
        pool[k] = list(cand[ok][:need])
    rows += [pool[k].pop() for k in kind]
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    return aa, t, np.array(rows, np.float64), off


@pytest.fixture(scope="module")
def problem(oracle):
    aa, t, rows, off = build_rows(oracle)
    rid, nid = synth.expand_ids(off, REF, NEI)
    ro, Jo = oracle.evaluate(1, synth.oracle_rows(1, rows), rid, nid, aa, t, normalize=True, extended=True)
    live = np.abs(ro[ro != 0])
    widths = dict(none=4.0, all=0.5 * live.min(), median=float(np.median(live)), fixed=A_FIXED)      # |r| <= pi < 4
    rev = np.concatenate([np.arange(off[p + 1] - 1, off[p] - 1, -1) for p in range(len(COUNTS))])     # every segment back to front
    return dict(aa=aa, t=t, rows=rows, off=off, ro=ro, Jo=Jo, widths=widths, rev=rev)


def slot_census(r, a):
    """(outliers, live rows, rows) of every slot of a segment whose residuals are r: slot (g, h) = rows 128 g + 2 lane + h"""
    out = []
    for g in range((len(r) + 127) // 128):
        for h in (0, 1):
            s = r[128 * g + h:128 * (g + 1):2]
            out.append((int((s * s > a * a).sum()), int((s != 0).sum()), len(s)))
    return np.array(out).reshape(-1, 2, 3)


def test_the_constructed_segment_has_every_kind_of_slot(problem):
    """from the oracle's residuals alone; no device call"""
    ro, off, widths = problem["ro"], problem["off"], problem["widths"]
    r = ro[off[CON]:off[CON + 1]]
    kind = constructed_kinds()
    assert np.all(np.abs(r[kind == "in"]) < IN_MAX) and np.all(r[kind == "in"] != 0) and np.all(np.abs(r[kind == "out"]) > OUT_MIN) and np.all(r[kind == "dead"] == 0)
    assert IN_MAX < widths["median"] < OUT_MIN and IN_MAX < widths["fixed"] < OUT_MIN          # the same slots under both widths
    for a in (widths["median"], widths["fixed"]):
        c = slot_census(r, a)
        assert c.shape == (9, 2, 3) and np.all(c[:8, :, 2] == 64) and tuple(c[8, :, 2]) == (19, 18)      # 37 rows: lanes 0 .. 18, lane 18 its even row only
        outl = c[:, :, 0]
        assert np.array_equal(outl[0], [0, 0])                                                                               # inliers only
        assert np.array_equal(outl[1], [64, 64]) and np.array_equal(outl[4], [64, 64]) and np.array_equal(outl[7], [64, 64])   # outliers only
        assert np.array_equal(outl[5], [64, 0])                                                                              # one slot of each
        assert np.array_equal(outl[2], [1, 0]) and r[256] ** 2 > a * a                      # one outlier: lane 0, even row
        assert np.array_equal(outl[3], [0, 1]) and r[511] ** 2 > a * a                      # one outlier: lane 63, odd row
        assert np.array_equal(outl[6], [0, 0]) and c[6, 0, 1] < 64 and c[6, 1, 1] < 64      # inliers and dead rows
        assert np.array_equal(outl[8], [1, 0]) and r[1044] ** 2 > a * a                     # one outlier inside the partly filled last trip
    # the other two widths: no outlier anywhere / every live row
    allr = problem["ro"]
    assert not np.any(allr * allr > widths["none"] ** 2)
    assert np.all((allr * allr > widths["all"] ** 2) == (allr != 0)) and np.sum(allr == 0) > 100
    # reversed, the segment still has slots without an outlier and slots in which inliers and outliers sit side by side
    c = slot_census(r[::-1], widths["median"])
    assert np.any(c[:, :, 0] == 0) and np.any((c[:, :, 0] > 0) & (c[:, :, 0] < c[:, :, 1]))


@pytest.fixture(scope="module")
def device(problem):
    """(plane runs, wave units, chunking) -> {"trivial" | width | "median_reversed": pair blocks}; every set is uploaded once per setting."""
    import panovlm_amd as pv
    ctx = pv.Context(0)
    ctx.set_poses(problem["aa"], problem["t"])
    mp = pytest.MonkeyPatch()
    out = {}
    for (pr, wave), chunk in itertools.product(FORMS, CHUNKS):
        mp.setenv("PVLM_PLANE_RUNS", str(pr)); mp.setenv("PVLM_WAVE_UNITS", str(wave))
        mp.delenv("PVLM_FUSED_CHUNK", raising=False); mp.delenv("PVLM_WAVE_CHUNK", raising=False)
        if chunk != "own":
            mp.setenv("PVLM_FUSED_CHUNK", chunk)
        res = {}
        rs = pv.ResidualSet.upload(ctx, 1, problem["rows"], problem["off"], REF, NEI, flags=1)
        assert rs.plane_runs()["in_use"] == bool(pr)
        res["trivial"] = rs.pair_blocks(0, 0.0).copy()
        for name, a in problem["widths"].items():
            res[name] = rs.pair_blocks(1, a).copy()
        rs.close()
        rs = pv.ResidualSet.upload(ctx, 1, problem["rows"][problem["rev"]], problem["off"], REF, NEI, flags=1)
        res["median_reversed"] = rs.pair_blocks(1, problem["widths"]["median"]).copy()
        rs.close()
        out[(pr, wave, chunk)] = res
    mp.undo()
    yield out
    ctx.close()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


SETTINGS = list(itertools.product((0, 1), (0, 1), CHUNKS))


@pytest.mark.parametrize("setting", SETTINGS)
def test_without_outliers_huber_is_trivial_bit_for_bit(device, setting):
    res = device[setting]
    assert np.isfinite(res["trivial"]).all() and np.any(res["trivial"] != 0.0)
    assert np.array_equal(_bits(res["none"]), _bits(res["trivial"]))


@pytest.mark.parametrize("width", ["all", "median", "fixed", "median_reversed"])
@pytest.mark.parametrize("setting", SETTINGS)
def test_pair_blocks_match_the_reference(problem, device, setting, width):
    a = problem["widths"][width.split("_")[0]]
    expect = synth.pair_blocks_from_jacobian(problem["ro"], problem["Jo"], problem["off"], 1, a)       # a sum over the segment: the order of its rows is free
    blocks = device[setting][width]
    scale = np.maximum(np.abs(expect).max(axis=1, keepdims=True), 1e-12)
    worst = (np.abs(blocks - expect) / scale).max()
    print("%s %s: worst |block - reference| / largest entry %.3e" % (setting, width, worst))
    assert np.isfinite(blocks).all()
    assert np.all(np.abs(blocks - expect) <= RTOL * scale), worst


def test_the_weights_matter_at_this_tolerance(problem):
    """the check above would see a slot that took the wrong path: one outlier of the constructed segment weighted 1 moves its block by more than ten times RTOL"""
    ro, Jo, off = problem["ro"], problem["Jo"], problem["off"]
    a = problem["widths"]["median"]
    good = synth.pair_blocks_from_jacobian(ro, Jo, off, 1, a)[CON]
    for row in (256, 511, 1044):
        i = off[CON] + row
        rho1, _ = synth.huber_weights(ro[i:i + 1], 1, a)
        wrong = good.copy()
        wrong[72:108] += ((1.0 - rho1[0]) * np.outer(Jo[i, 6:], Jo[i, 6:])).reshape(-1)
        assert np.abs(wrong - good).max() > 10 * RTOL * np.abs(good).max(), row


def test_layout_switch_changes_no_bit(device):
    """plane runs on or off: the same rows in the same lanes, so the same bits within a unit of work and a chunking"""
    for wave, chunk in itertools.product((0, 1), CHUNKS):
        for name in device[(0, wave, chunk)]:
            assert np.array_equal(_bits(device[(0, wave, chunk)][name]), _bits(device[(1, wave, chunk)][name])), (wave, chunk, name)
    # the single-row segment: one term per sum, the same bits in every setting
    base = device[SETTINGS[0]]
    for setting in SETTINGS[1:]:
        for name in base:
            assert np.array_equal(_bits(base[name][0]), _bits(device[setting][name][0])), (setting, name)
