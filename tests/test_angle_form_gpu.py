"""The closed form of Point2Plane_Angle with normalize_distance on the device (pvlm_functors.h, residual_grad<POINT2PLANE_ANGLE, true>) on the edge
rows of tests/angle_form_rows.py, uploaded as segments of 1, 2, 129 and 1025 rows (an odd tail, the two rows of a lane, more than one wave, more than
one 512-row trip) and two segments of 1025 rows that differ in one row per wave (below).

Every kernel that evaluates the functor goes through the same device function, so the switches that select a kernel or a memory layout may not change
a bit: PVLM_PLANE_RUNS (7 columns / plane table), PVLM_POINT_TABLE (an uploaded set has no point table: the switch must change nothing), PVLM_WAVE_UNITS
(block / wave form of the fused kernel).  r and J (k_eval_materialise) are the same bits under all eight settings; the pair blocks are the same bits
under the four settings of a unit of work, and across the two units on the single-row segment, whose sums have one term (block and wave form add the
rows of a longer segment in different orders).

Segment 4 has exactly one row above pi/8 among the 64 rows a wave evaluates together (rows 10 mod 128: a wave covers 128 consecutive rows, a lane two
neighbours, one after the other), so its even rows take the octant path of atan2_pos_grad; segment 5 is the same segment with those rows replaced by
small-angle rows and takes the small-angle path throughout.  The rows common to both agree to 1e-14 relative: the two paths hand the same angle and the
same 1 / D' to the gradient."""
import itertools

import numpy as np
import pytest

from tests import angle_form_rows as af
from tests import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-6       # tests/test_eval_gpu.py
ATOL = 1e-13
LOSS_A = 2 * np.pi / 180
FORMS = list(itertools.product((0, 1), (0, 1), (0, 1)))          # (plane runs, point table, wave units)


@pytest.fixture(scope="module")
def problem(oracle):
    aa, t, rows, off, cls = af.build_problem()
    rid, nid = synth.expand_ids(off, af.REF, af.NEI)
    orows = synth.oracle_rows(1, rows)
    ro, Jo = oracle.evaluate(1, orows, rid, nid, aa, t, normalize=True, extended=True)
    rd, Jd = oracle.evaluate(1, orows, rid, nid, aa, t, normalize=True)
    dis = oracle.branch_distance(1, orows, rid, nid, aa, t)
    return dict(aa=aa, t=t, rows=rows, off=off, cls=cls, ro=ro, Jo=Jo, rd=rd, Jd=Jd, dis=dis)


@pytest.fixture(scope="module")
def device(problem):
    """form -> (r, J, {loss: pair blocks}); every set is uploaded once per form."""
    import panovlm_amd as pv
    ctx = pv.Context(0)
    mp = pytest.MonkeyPatch()
    out = {}
    for form in FORMS:
        mp.setenv("PVLM_PLANE_RUNS", str(form[0])); mp.setenv("PVLM_POINT_TABLE", str(form[1])); mp.setenv("PVLM_WAVE_UNITS", str(form[2]))
        mp.setenv("PVLM_FUSED_CHUNK", "512"); mp.setenv("PVLM_WAVE_CHUNK", "512")
        rs = pv.ResidualSet.upload(ctx, 1, problem["rows"], problem["off"], af.REF, af.NEI, flags=1)
        assert rs.plane_runs()["in_use"] == bool(form[0]) and not rs.point_table()["in_use"]
        ctx.set_poses(problem["aa"], problem["t"])
        r, J = rs.eval(jac=True)
        out[form] = (r.copy(), J.copy(), {loss: rs.pair_blocks(loss, LOSS_A).copy() for loss in (0, 1)})
        rs.close()
    mp.undo()
    yield out
    ctx.close()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def test_every_form_gives_the_same_bits(device):
    r0, J0, _ = device[FORMS[0]]
    assert np.isfinite(r0).all() and np.isfinite(J0).all() and np.any(J0 != 0.0)
    for form in FORMS[1:]:
        r, J, _ = device[form]
        assert np.array_equal(_bits(r0), _bits(r)) and np.array_equal(_bits(J0), _bits(J)), form
    for loss in (0, 1):
        for wave in (0, 1):
            base = device[(0, 0, wave)][2][loss]
            assert np.isfinite(base).all() and np.any(base != 0.0)
            for pr, pt in ((0, 1), (1, 0), (1, 1)):
                assert np.array_equal(_bits(base), _bits(device[(pr, pt, wave)][2][loss])), (pr, pt, wave, loss)
        assert np.array_equal(_bits(device[(1, 1, 0)][2][loss][0]), _bits(device[(1, 1, 1)][2][loss][0]))      # the single-row segment: one term


def test_residuals_and_jacobians_match_the_reference(problem, device):
    r, J, _ = device[(1, 1, 0)]
    ro, Jo, rd, Jd, dis, cls = (problem[k] for k in ("ro", "Jo", "rd", "Jd", "dis", "cls"))
    assert np.sum(np.abs(dis - 1e-3) <= 1e-15) == 0
    q0 = cls == "q_zero"                                  # parallel vectors: the reference clamps the cosine and returns 0 with a zero Jacobian
    assert q0.sum() >= 100
    assert np.array_equal(r == 0, (dis < 1e-3) | q0) and np.array_equal(ro == 0, r == 0) and np.array_equal(rd == 0, r == 0)
    assert np.all(J[r == 0] == 0.0)
    err_r = np.abs(r - ro) / (RTOL * np.abs(ro) + ATOL)
    scale = np.maximum(np.abs(Jo).max(axis=1, keepdims=True), 1e-9)
    err_J = np.abs(J - Jo) / (RTOL * scale)
    print("worst |r - ro| / tolerance %.3e, worst |J - Jo| / tolerance %.3e, |J - Jo|max %.3e, |Jd - Jo|max %.3e"
          % (err_r.max(), err_J.max(), np.abs(J - Jo).max(), np.abs(Jd - Jo).max()))
    assert np.all(err_r <= 1.0), err_r.max()
    assert np.all(err_J <= 1.0), err_J.max()
    # at least as close to the exact value as upstream's double arithmetic, up to rounding noise (tests/test_eval_gpu.py)
    assert np.abs(J - Jo).max() <= max(10 * np.abs(Jd - Jo).max(), 1e-10 * scale.max())


@pytest.mark.parametrize("loss", [0, 1])
@pytest.mark.parametrize("form", FORMS)
def test_pair_blocks_match_the_reference(problem, device, form, loss):
    expect = synth.pair_blocks_from_jacobian(problem["ro"], problem["Jo"], problem["off"], loss, LOSS_A)
    blocks = device[form][2][loss]
    scale = np.maximum(np.abs(expect).max(axis=1, keepdims=True), 1e-12)
    assert np.all(np.abs(blocks - expect) <= RTOL * scale), (np.abs(blocks - expect) / scale).max()


def test_octant_path_and_small_angle_path_agree(problem, device):
    r, J, _ = device[(1, 1, 0)]
    off, cls, ro = problem["off"], problem["cls"], problem["ro"]
    a, b = slice(off[4], off[5]), slice(off[5], off[6])
    big = np.arange(af.COUNTS[4]) % af.BIG_EVERY == af.BIG_AT
    assert np.all(ro[a][big] > np.pi / 8) and np.all(ro[a][~big] < np.pi / 16) and np.all(ro[b] < np.pi / 16)
    # exactly one such row among the 64 rows of equal parity of every 128 consecutive rows, none in the tail wave and none among the odd rows
    groups = big[:1024].reshape(-1, 64, 2)
    assert np.all(groups[:, :, 0].sum(1) == 1) and not groups[:, :, 1].any() and not big[1024:].any()
    assert np.array_equal(_bits(problem["rows"][a][~big]), _bits(problem["rows"][b][~big]))
    ra, rb, Ja, Jb = r[a][~big], r[b][~big], J[a][~big], J[b][~big]
    even = (np.arange(af.COUNTS[4]) % 2 == 0)[~big]
    assert np.any(ra[even] != rb[even]) or np.any(Ja[even] != Jb[even])          # the two paths really ran: somewhere they round differently
    dr = np.abs(ra - rb) / np.maximum(np.abs(rb), 1e-300)
    dJ = np.abs(Ja - Jb) / np.maximum(np.abs(Jb).max(axis=1, keepdims=True), 1e-300)
    live = rb != 0
    print("octant against small-angle path: worst relative difference r %.3e, J %.3e" % (dr[live].max(), dJ[live].max()))
    assert np.array_equal(ra == 0, rb == 0)
    assert np.all(dr[live] <= 1e-14) and np.all(dJ[live] <= 1e-14)
    assert np.all(Ja[~live] == 0.0) and np.all(Jb[~live] == 0.0)
