"""Shared by tests/test_angle_form_cpu.py and tests/test_angle_form_gpu.py: the edge rows of Point2Plane_Angle with normalize_distance and numpy
restatements of the device's closed form (panovlm_amd/csrc/pvlm_functors.h, residual_grad<POINT2PLANE_ANGLE, true>), the present one and the one it replaced.

A restatement follows the device statement operation for operation with two exceptions numpy cannot express: the hardware reciprocal and reciprocal
square root estimates with their Newton step are an exact division and 1 / sqrt (both sit at the 1e-15 level, below what the tests resolve), and
fused multiply-adds are a multiplication and an addition."""
import numpy as np

from tests import synth

TAN_PI_8 = 0.41421356237309503
CLASSES = ("random", "negative_sd", "below_1e-3", "above_1e-3", "d_zero", "q_zero", "over_pi_8", "over_pi_2", "far_plane")


def _chain(aa, t, r, n, p):
    """P_r = R_rn (P_n - t_n) + t_r and the pieces of the pose chain the Jacobian row needs."""
    Rr, Rn = synth.rodrigues(aa[r]), synth.rodrigues(aa[n])
    Rrn = Rr @ Rn.T
    return Rrn @ (p - t[n]) + t[r], Rrn


def plane_terms(P, n, d):
    """sd, u, q^2, nu^2 exactly as the device forms them (shared by both forms; the decision dis >= 1e-3 is taken on these bits)."""
    sd = n[:, 0] * P[:, 0] + n[:, 1] * P[:, 1] + n[:, 2] * P[:, 2] + d
    u = P - (sd - d)[:, None] * n
    q2 = (u * u).sum(1)
    return sd, u, q2, q2 + d * d


def _atan2_pos(y, x):
    return np.arctan2(y, x)


def form_new(P, n, d):
    """X = nu - sd d, Y = |sd| q, r = atan2(Y, X), g = A n + B u with A = s q nu / D', B = |sd| d (d - sd nu) / (q nu D'), D' = X^2 + Y^2."""
    sd, u, q2, nu2 = plane_terms(P, n, d)
    dis = np.abs(sd)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_nu = 1.0 / np.sqrt(nu2)
        invq = np.where(q2 > 0.0, 1.0 / np.sqrt(q2), 0.0)
        q, nu = q2 * invq, nu2 * inv_nu
        X, Y = nu - sd * d, dis * q
        live = dis >= 1e-3
        h2 = X * X + Y * Y
        small = Y <= TAN_PI_8 * X
        R = 1.0 / (X * h2)
        invD = np.where(small, X * R, 1.0 / h2)
        t = Y * (h2 * R)
        r = np.where(live, np.where(small, np.arctan(t), _atan2_pos(Y, X)), 0.0)
        k0 = np.where(live, invD, 0.0)
        A = np.copysign(q * nu * k0, sd)
        B = dis * d * (d - sd * nu) * (invq * inv_nu) * k0
    return r, A[:, None] * n + B[:, None] * u


def form_old(P, n, d):
    """The statement this form replaced: x = 1 - sd d / nu, y = |sd| q / nu, r = atan2(y, x), g = fsd n + cu u."""
    sd, u, q2, nu2 = plane_terms(P, n, d)
    s = np.where(sd < 0.0, -1.0, 1.0)
    dis = s * sd
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_nu = 1.0 / np.sqrt(nu2)
        invq = np.where(q2 > 0.0, 1.0 / np.sqrt(q2), 0.0)
        q = q2 * invq
        x, y = 1.0 - sd * d * inv_nu, dis * q * inv_nu
        invD = 1.0 / (x * x + y * y)
        live = dis >= 1e-3
        r = np.where(live, _atan2_pos(y, x), 0.0)
        k0 = np.where(live, inv_nu * invD, 0.0)
        fsd = (x * s * q + y * d) * k0
        cu = (x * dis * d * d * invq - y * sd * d) * (inv_nu * inv_nu) * k0
    return r, fsd[:, None] * n + cu[:, None] * u


def evaluate_form(form, rows, rid, nid, aa, t):
    """r and the 1 x 12 AutoDiff rows [d aa_r | d t_r | d aa_n | d t_n] of a form, through the pose chain of the header of pvlm_functors.h."""
    tab = synth.pose_table(aa, t)
    N = len(rows)
    P = np.empty((N, 3)); Rrn = np.empty((N, 3, 3))
    for i in range(N):
        P[i], Rrn[i] = _chain(aa, t, rid[i], nid[i], rows[i, :3])
    r, g = form(P, rows[:, 3:6], rows[:, 6])
    c = np.cross(P - t[rid], g)
    Jl_r = tab[rid, 9:18].reshape(-1, 3, 3); Jl_n = tab[nid, 9:18].reshape(-1, 3, 3)
    J = np.empty((N, 12))
    J[:, 0:3] = np.einsum("ni,nij->nj", c, Jl_r)
    J[:, 3:6] = g
    J[:, 6:9] = -np.einsum("ni,nij,njk->nk", c, Rrn, Jl_n)
    J[:, 9:12] = -np.einsum("ni,nij->nj", g, Rrn)
    return r, J


def _row(aa, t, r, n, p, nrm, d_of):
    """A row whose plane offset is chosen from the point in the reference frame: d = d_of(n . P_r)."""
    Pr, _ = _chain(aa, t, r, n, p)
    return np.concatenate([p, nrm, [d_of(float(nrm @ Pr))]])


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _angle(aa, t, r, n, row):
    Pr, _ = _chain(aa, t, r, n, row[:3])
    return float(form_new(Pr[None], row[None, 3:6], row[None, 6:7].reshape(1))[0][0])


def class_row(rng, cls, aa, t, r, n):
    """One row of the class for the pair (r, n).  Offsets o are signed distances of P_r from the plane: n . P_r + d = o."""
    while True:
        p, nrm = rng.normal(size=3) * 4.0, _unit(rng)
        if cls == "random":
            o = rng.choice([1e-4, 5e-3, 0.05, 0.5]) * rng.choice([-1.0, 1.0])
            return _row(aa, t, r, n, p, nrm, lambda a: o - a)
        if cls == "negative_sd":
            o = -rng.choice([5e-3, 0.05, 0.5])
            return _row(aa, t, r, n, p, nrm, lambda a: o - a)
        if cls in ("below_1e-3", "above_1e-3"):
            # |sd| = 1e-3 (1 -+ margin), margin from 1e-9 up: the device's sd differs from this construction by a few ulp of |d| ~ 1e-15
            m = rng.choice([1e-9, 1e-8, 1e-6, 1e-3]) * (-1.0 if cls == "below_1e-3" else 1.0)
            o = 1e-3 * (1.0 + m) * rng.choice([-1.0, 1.0])
            row = _row(aa, t, r, n, p, nrm, lambda a: o - a)
            if abs(row[6]) < 20.0:            # keep the rounding of n . P + d three orders below the smallest margin (1e-12 absolute)
                return row
            continue
        if cls == "d_zero":
            # the plane passes through the reference origin; P_r is moved to a chosen distance o from it
            o = rng.choice([5e-3, 0.05, 0.5]) * rng.choice([-1.0, 1.0])
            Pr, Rrn = _chain(aa, t, r, n, p)
            Pr2 = Pr - (nrm @ Pr) * nrm + o * nrm
            p2 = Rrn.T @ (Pr2 - t[r]) + t[n]
            return np.concatenate([p2, nrm, [0.0]])
        if cls == "q_zero":
            # P_r on the normal through the origin.  q^2 = 0 EXACTLY needs u = P - (sd - d) n = 0 in floating point: an identity chain (the caller
            # gives both scans of the pair the zero pose), an axis normal, and binary fractions so that sd = h + d = o and sd - d = h are exact
            assert not aa[r].any() and not aa[n].any() and not t[r].any() and not t[n].any()
            axis = np.zeros(3); axis[rng.integers(0, 3)] = rng.choice([-1.0, 1.0])
            h = rng.choice([0.5, 2.0, 7.0])
            o = rng.choice([2.0 ** -8, 2.0 ** -5]) * rng.choice([-1.0, 1.0])
            return np.concatenate([h * axis, axis, [o - h]])
        if cls in ("over_pi_8", "over_pi_2"):
            o = rng.choice([2.0, 5.0, 20.0]) * rng.choice([-1.0, 1.0])
            row = _row(aa, t, r, n, p, nrm, lambda a: o - a)
            ang = _angle(aa, t, r, n, row)
            if (cls == "over_pi_8" and np.pi / 8 * 1.05 < ang < np.pi / 2) or (cls == "over_pi_2" and ang > np.pi / 2 * 1.05):
                return row
            continue
        if cls == "far_plane":
            # |sd| ~ 1e-3 with nu ~ 50 m
            p = _unit(rng) * 50.0
            o = 1e-3 * (1.0 + rng.choice([1e-6, 1e-3, 0.5])) * rng.choice([-1.0, 1.0])
            return _row(aa, t, r, n, p, nrm, lambda a: o - a)
        raise ValueError(cls)


def small_angle_row(rng, aa, t, r, n):
    while True:
        row = class_row(rng, "random", aa, t, r, n)
        if _angle(aa, t, r, n, row) < np.pi / 16:
            return row


F = 4
REF = np.array([2, 3, 1, 0, 2, 2], np.int32)
NEI = np.array([3, 2, 2, 1, 0, 0], np.int32)
COUNTS = (1, 2, 129, 1025, 1025, 1025)
BIG_EVERY, BIG_AT = 128, 10          # segment 4: rows BIG_AT (mod BIG_EVERY) lie above pi/8; a wave covers 128 consecutive rows, two per lane


def build_problem(seed=2024):
    """Poses (scans 0 and 1 at the zero pose), the six segments and the class of every row.
    Segments 0..3 (1, 2, 129, 1025 rows: an odd tail, the two rows of a lane, more than one wave, more than one 512-row trip) cycle through the edge
    classes; segment 3 lies on the zero-pose pair and is the only one with q^2 = 0 rows.  Segment 4 has exactly one row above pi/8 among the rows a wave
    evaluates together, segment 5 is the same segment with those rows replaced by small-angle rows: every other row takes the octant path in 4 and the
    small-angle path in 5."""
    rng = np.random.default_rng(seed)
    aa, t = synth.random_poses(rng, F)
    aa[:2] = 0.0; t[:2] = 0.0
    rows, cls = [], []
    for p, count in enumerate(COUNTS[:4]):
        names = [c for c in CLASSES if c != "q_zero" or p == 3]
        if p == 0:
            names = ["over_pi_2"]
        if p == 1:
            names = ["negative_sd", "over_pi_8"]
        for i in range(count):
            c = names[i % len(names)]
            rows.append(class_row(rng, c, aa, t, REF[p], NEI[p])); cls.append(c)
    seg5 = [small_angle_row(rng, aa, t, REF[5], NEI[5]) for _ in range(COUNTS[5])]
    seg4 = [class_row(rng, "over_pi_8", aa, t, REF[4], NEI[4]) if i % BIG_EVERY == BIG_AT else row for i, row in enumerate(seg5)]
    rows += seg4 + seg5
    cls += ["over_pi_8" if i % BIG_EVERY == BIG_AT else "random" for i in range(COUNTS[4])] + ["random"] * COUNTS[5]
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    return aa, t, np.array(rows, np.float64), off, np.array(cls)
