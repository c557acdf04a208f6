"""The closed form of Point2Plane_Angle with normalize_distance (pvlm_functors.h: X = nu - sd d, Y = |sd| q, one reciprocal for the quotient of the
angle and for 1 / D') restated in numpy (tests/angle_form_rows.py) against the reference's statements in extended precision, on the edge rows: random
rows, sd < 0, |sd| on both sides of 1e-3 at margins >= 1e-9, d = 0, q^2 = 0 exactly, angles above pi/8 and above pi/2 (X <= 0), |sd| ~ 1e-3 with the
plane 50 m away.  No device: this checks the algebra and its conditioning, the GPU file checks the kernels."""
import numpy as np
import pytest

from tests import angle_form_rows as af
from tests import synth

RTOL = 1e-6       # tests/test_eval_gpu.py
ATOL = 1e-13


@pytest.fixture(scope="module")
def problem(oracle):
    aa, t, rows, off, cls = af.build_problem()
    rid, nid = synth.expand_ids(off, af.REF, af.NEI)
    orows = synth.oracle_rows(1, rows)
    ro, Jo = oracle.evaluate(1, orows, rid, nid, aa, t, normalize=True, extended=True)
    dis = oracle.branch_distance(1, orows, rid, nid, aa, t)
    new = af.evaluate_form(af.form_new, rows, rid, nid, aa, t)
    old = af.evaluate_form(af.form_old, rows, rid, nid, aa, t)
    return dict(rows=rows, cls=cls, ro=ro, Jo=Jo, dis=dis, new=new, old=old, aa=aa, t=t, rid=rid, nid=nid)


def test_every_class_is_there(problem):
    cls, rows, dis, ro = problem["cls"], problem["rows"], problem["dis"], problem["ro"]
    for c in af.CLASSES:
        assert (cls == c).sum() >= 100, c
    assert np.all(dis[cls == "below_1e-3"] < 1e-3) and np.all(dis[cls == "above_1e-3"] >= 1e-3)
    margin = np.abs(dis[(cls == "below_1e-3") | (cls == "above_1e-3")] / 1e-3 - 1.0)
    assert margin.min() >= 0.9e-9 and margin.min() < 1e-8
    assert np.all(rows[cls == "d_zero", 6] == 0.0)
    P = rows[cls == "q_zero", :3]
    assert np.all(af.plane_terms(P, rows[cls == "q_zero", 3:6], rows[cls == "q_zero", 6])[2] == 0.0)      # zero-pose pair: P_r is the stored point
    assert np.all(ro[cls == "over_pi_8"] > np.pi / 8) and np.all(ro[cls == "over_pi_2"] > np.pi / 2)
    far = cls == "far_plane"
    assert np.all(np.abs(dis[far] - 1e-3) <= 0.6e-3) and np.all(np.linalg.norm(rows[far, :3], axis=1) == pytest.approx(50.0))


def test_new_form_matches_the_reference(problem):
    (r, J), ro, Jo, dis = problem["new"], problem["ro"], problem["Jo"], problem["dis"]
    assert np.isfinite(r).all() and np.isfinite(J).all()
    q0 = problem["cls"] == "q_zero"                      # parallel vectors: the reference clamps the cosine and returns 0 with a zero Jacobian
    assert np.array_equal(r == 0, (dis < 1e-3) | q0) and np.array_equal(ro == 0, r == 0)
    assert np.all(np.abs(r - ro) <= RTOL * np.abs(ro) + ATOL), (np.abs(r - ro) / (RTOL * np.abs(ro) + ATOL)).max()
    scale = np.maximum(np.abs(Jo).max(axis=1, keepdims=True), 1e-9)
    assert np.all(np.abs(J - Jo) <= RTOL * scale), (np.abs(J - Jo) / (RTOL * scale)).max()
    assert np.all(J[q0] == 0.0) and np.all(J[dis < 1e-3] == 0.0)


def test_new_form_is_no_less_accurate_than_the_form_it_replaces(problem):
    """Worst row error of each form against the extended-precision reference, on the same rows; the margin of 2 covers rounding noise between two
    equivalent orderings."""
    ro, Jo = problem["ro"], problem["Jo"]
    live = ro != 0
    scale = np.maximum(np.abs(Jo).max(axis=1, keepdims=True), 1e-9)
    err = {}
    for name in ("new", "old"):
        r, J = problem[name]
        err[name] = (np.max(np.abs(r - ro)[live] / np.abs(ro[live])), np.max(np.abs(J - Jo) / scale))
    print("worst relative error r: new %.3e old %.3e;  J: new %.3e old %.3e" % (err["new"][0], err["old"][0], err["new"][1], err["old"][1]))
    assert err["new"][0] <= 2 * err["old"][0]
    assert err["new"][1] <= 2 * err["old"][1]
    # and the two forms agree with each other at the rounding level
    (rn, Jn), (rl, Jl) = problem["new"], problem["old"]
    assert np.max(np.abs(rn - rl)[live] / np.abs(ro[live])) <= 1e-12
    assert np.max(np.abs(Jn - Jl) / scale) <= 1e-12
