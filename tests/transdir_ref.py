"""K46 test helpers: synthetic camera graphs with known truth, an INDEPENDENT numpy float64 reference of the two problems of panovlm_amd/csrc/pvlm_transdir_core.h —
TranslationAveragingL2Chordal and one solve of TranslationAveragingLUD (sfm/TranslationAveraging.cpp:206-274, :553-626) — that builds the FULL dense system (for LUD
over 3 (F - 1) + P unknowns: the scales are explicit unknowns, nothing is eliminated, so it shares no reduction code with the core) with the same trust-region policy
and the same clamp, the knife-edge condition every scene of the K46 tests is held to, and the ctypes wrappers of the host compile of the core
(tests/cpp/transdir_core_check.cpp, built by panovlm_amd.build.build_transdir_check)."""
import ctypes as C

import numpy as np

from tests import transavg_ref as tr

MIN_RELATIVE_DECREASE, GRADIENT_TOL = 1e-3, 1e-10
INITIAL_RADIUS, MAX_RADIUS, MIN_RADIUS, MIN_LM_DIAG, MAX_LM_DIAG = 1e4, 1e16, 1e-32, 1e-6, 1e32
# function tolerance, parameter tolerance, max_num_iterations of the two problems (:254-257; :605 with Solver::Options' defaults)
POLICY = dict(chordal=(1e-7, 1e-8, 300), lud=(1e-6, 1e-8, 50))
G = 8   # pvlm_transdir_group_size(); tests assert it


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def scene(seed, pairs, n_cameras, origin=0, unscaled=0.0, noise_deg=0.0, outliers=0.0, size=8.0, wrong_length=None, start_off=0.3):
    """Camera centres uniform in a cube of `size` metres, the origin camera's at zero.  Pair (i, j): dir = (C_i - C_j) / |C_i - C_j| turned by noise_deg about a random
    axis; `outliers`: this fraction of the pairs gets a random direction (clean_dir: the directions before that); the start scale is |C_i - C_j|, times
    wrong_length[p] where given, or 1 for the `unscaled` fraction (upstream's pair without lower_scale / upper_scale).  start: the truth plus normal noise of start_off metres per coordinate, the origin kept."""
    rng = np.random.default_rng(seed)
    F = n_cameras; pairs = np.asarray(pairs, np.int32).reshape(-1, 2); P = len(pairs)
    Cw = rng.uniform(-size / 2, size / 2, (F, 3)); Cw -= Cw[origin]
    d = np.zeros((P, 3)); clean = np.zeros((P, 3)); scales = np.ones(P)
    bad = rng.permutation(P)[:int(round(outliers * P))] if outliers > 0 else []
    free = set(rng.permutation(P)[:int(round(unscaled * P))].tolist()) if unscaled > 0 else set()
    for p, (i, j) in enumerate(pairs):
        v = Cw[i] - Cw[j]
        if noise_deg > 0:
            a = np.cross(v, rng.normal(size=3)); a /= np.linalg.norm(a)
            v = tr.rodrigues(np.radians(noise_deg) * rng.normal() * a) @ v
        clean[p] = v / np.linalg.norm(v); clean[p] /= np.linalg.norm(clean[p])
        if p in bad:
            u = rng.normal(size=3); v = u / np.linalg.norm(u) * np.linalg.norm(v)
        n = np.linalg.norm(v)
        d[p] = v / n; d[p] /= np.linalg.norm(d[p])
        if p not in free:
            scales[p] = n * (wrong_length[p] if wrong_length and p in wrong_length else 1.0)
    off = rng.normal(size=(F, 3)) * start_off; off[origin] = 0.0
    return dict(F=F, P=P, first=pairs[:, 0].copy(), second=pairs[:, 1].copy(), dir=d, clean_dir=clean, scales=scales, origin=origin, truth=Cw, start=Cw + off, size=size)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def lud_bounds_of(s0, upper_ratio, lower_ratio):
    """per pair: ScaleFactor upper, lower, parameter lower, parameter upper.  An unscaled pair (s0 == 1 as written) has the parameter LOWER bound 1 and no upper"""
    s0 = np.asarray(s0, np.float64)
    scaled = s0 != 1
    return (np.where(scaled, s0 * upper_ratio, 2.0), np.where(scaled, s0 * lower_ratio, 1.0), np.where(scaled, s0 * 0.5, 1.0), np.where(scaled, s0 * 3.0, np.inf))


def solve_ref(problem, sc, c0=None, s0=None, weight=None, loss_a=0.5, upper_ratio=1.3, lower_ratio=0.9, max_num_iterations=None):
    """problem "chordal" or "lud" on the full system.  Returns dict(centres, scales, weight, sum_e, initial_cost, final_cost, successful, unsuccessful, termination,
    knife) — knife: the list of what came within the knife-edge condition's margins (empty: the scene is admitted).  For chordal scales, weight and sum_e are None."""
    lud = problem == "lud"
    FUNCTION_TOL, PARAMETER_TOL, default_iterations = POLICY[problem]
    if max_num_iterations is None:
        max_num_iterations = default_iterations
    F, P, origin = sc["F"], sc["P"], sc["origin"]
    first, second, d = sc["first"], sc["second"], sc["dir"]
    s0 = np.asarray(sc["scales"] if s0 is None else s0, np.float64).copy()
    w = np.ones(P) if weight is None else np.asarray(weight, np.float64).copy()
    U, L, lo, hi = lud_bounds_of(s0, upper_ratio, lower_ratio)
    cams = [c for c in range(F) if c != origin]
    col = {c: 3 * k for k, c in enumerate(cams)}
    nt = 3 * len(cams); nu = nt + (P if lud else 0)
    knife = []

    def near_bounds(s, clamped, where):
        for name, b in (("upper", U), ("lower", L), ("parameter lower", lo), ("parameter upper", hi)):
            fin = np.isfinite(b)
            close = fin & (np.abs(s - np.where(fin, b, 0.0)) <= 1e-9 * np.abs(s0)) & ~(clamped & (s == b))
            if close.any():
                knife.append("%s: scale of pair %d within 1e-9 s0 of its %s bound" % (where, int(np.argmax(close)), name))

    def evaluate(c, s, where):
        u = c[first] - c[second]
        if lud:
            e = u - s[:, None] * d
            m = np.linalg.norm(e, axis=1)
            f = w * np.sqrt(m)
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(m[:, None] > 0, (w * 0.5 * m ** -1.5)[:, None] * e, 0.0)
            f2 = np.where(s > U, s - U, np.where(s < L, L - s, 0.0)); jf = np.where(s > U, 1.0, np.where(s < L, -1.0, 0.0))
            J = np.zeros((2 * P, nu)); res = np.zeros(2 * P)
            for p in range(P):
                i, j = first[p], second[p]
                if i != origin:
                    J[p, col[i]:col[i] + 3] = q[p]
                if j != origin:
                    J[p, col[j]:col[j] + 3] -= q[p]
                J[p, nt + p] = -(q[p] @ d[p])
                J[P + p, nt + p] = jf[p]
            res[:P] = f; res[P:] = f2
            return float(0.5 * (f * f).sum() + 0.5 * (f2 * f2).sum()), J.T @ J, J.T @ res
        with np.errstate(divide="ignore", invalid="ignore"):
            n = np.linalg.norm(u, axis=1)
            un = u / n[:, None]
            r = un - d
            s2 = (r * r).sum(1)
            a2 = loss_a * loss_a
            if (np.abs(s2 - a2) <= 1e-9).any():
                knife.append("%s: Huber argument of pair %d within 1e-9 of a^2" % (where, int(np.argmax(np.abs(s2 - a2) <= 1e-9))))
            inl = s2 <= a2
            rho = np.where(inl, s2, 2 * loss_a * np.sqrt(s2) - a2); rw = np.where(inl, 1.0, loss_a / np.sqrt(s2))
        J = np.zeros((3 * P, nu)); res = np.zeros(3 * P)
        for p in range(P):
            i, j = first[p], second[p]
            A = np.sqrt(rw[p]) * (np.eye(3) - np.outer(un[p], un[p])) / n[p]
            if i != origin:
                J[3 * p:3 * p + 3, col[i]:col[i] + 3] = A
            if j != origin:
                J[3 * p:3 * p + 3, col[j]:col[j] + 3] -= A
            res[3 * p:3 * p + 3] = np.sqrt(rw[p]) * r[p]
        return float(0.5 * rho.sum()), J.T @ J, J.T @ res

    def pack(c):
        return c[cams].reshape(-1)

    c = np.asarray(sc["start"] if c0 is None else c0, np.float64).copy(); s = s0.copy()
    out = dict(successful=0, unsuccessful=0, termination=-1)
    if P == 0:
        out.update(termination=6, initial_cost=0.0, final_cost=0.0, centres=c, scales=s if lud else None, weight=None, sum_e=None, knife=knife)
        return out
    cost, H, g = evaluate(c, s, "start")
    out["initial_cost"] = cost
    radius, dec, it = INITIAL_RADIUS, 2.0, 0
    if not np.isfinite(cost):
        out["termination"] = 5
    else:
        scale = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(H), 0.0)))
        if max_num_iterations > 0:
            gm = np.abs(g).max()
            if 0.5 * GRADIENT_TOL <= gm <= 2 * GRADIENT_TOL:
                knife.append("start: gradient within a factor 2 of its tolerance")
            if gm <= GRADIENT_TOL:
                out["termination"] = 2
    while out["termination"] < 0 and it < max_num_iterations:
        it += 1
        Hs = H * scale[:, None] * scale[None, :]
        rhs = -g * scale
        D = np.clip(np.diag(Hs), MIN_LM_DIAG, MAX_LM_DIAG) / radius
        ok = True
        try:
            Lc = np.linalg.cholesky(Hs + np.diag(D))
            dy = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))
        except np.linalg.LinAlgError:
            ok = False
        accepted = False
        if ok:
            step = dy * scale
            c_s, clamped = s, np.zeros(P, bool)
            if lud:
                c_s = np.minimum(np.maximum(s + step[nt:], lo), hi)
                clamped = c_s != s + step[nt:]
                step[nt:] = c_s - s
            model = -(g @ step + 0.5 * step @ H @ step)
            ok = model > 0 and np.isfinite(model)
        if ok:
            c_c = c.copy(); c_c[cams] += step[:nt].reshape(-1, 3)
            if lud:
                near_bounds(c_s, clamped, "iteration %d" % it)
            c_cost, cH, cg = evaluate(c_c, c_s, "iteration %d" % it)
            rho = (cost - c_cost) / model
            if 0.5 * MIN_RELATIVE_DECREASE <= rho <= 2 * MIN_RELATIVE_DECREASE:
                knife.append("iteration %d: step quality %.3g within a factor 2 of min_relative_decrease" % (it, rho))
            if np.isfinite(c_cost) and rho > MIN_RELATIVE_DECREASE:
                accepted = True
                xn = np.sqrt((pack(c) ** 2).sum() + ((s ** 2).sum() if lud else 0.0))
                change = cost - c_cost; prev = cost
                c, s, cost, H, g = c_c, c_s, c_cost, cH, cg
                radius = min(MAX_RADIUS, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                dec = 2.0
                out["successful"] += 1
                tests = ((abs(change), FUNCTION_TOL * prev, "function"), (np.abs(g).max(), GRADIENT_TOL, "gradient"),
                         (np.linalg.norm(step), PARAMETER_TOL * (xn + PARAMETER_TOL), "parameter"))
                for code, (val, tol, name) in enumerate(tests, 1):
                    if 0.5 * tol <= val <= 2 * tol:
                        knife.append("iteration %d: %s test within a factor 2 of its tolerance" % (it, name))
                    if val <= tol:
                        out["termination"] = code
                        break
        if not accepted:
            out["unsuccessful"] += 1
            radius /= dec; dec *= 2.0
            if radius < MIN_RADIUS:
                out["termination"] = 4
    if out["termination"] < 0:
        out["termination"] = 0
    out.update(final_cost=cost, centres=c, scales=None, weight=None, sum_e=None, knife=knife)
    if lud:
        m = np.linalg.norm(c[first] - c[second] - s[:, None] * d, axis=1)
        out.update(scales=s, weight=(m + 1e-2) ** -0.5, sum_e=float(m.sum()))
    return out


def irls_ref(sc, solves, upper_ratio=1.3, lower_ratio=0.9):
    """`solves` LUD solves in a row as TranslationAveragingLUD's loop chains them (weights start at 1; scales, weights and centres carried over), without the stop
    rule.  Returns the list of the solves' results."""
    c, s, w, out = sc["start"], sc["scales"], np.ones(sc["P"]), []
    for _ in range(solves):
        r = solve_ref("lud", sc, c, s, w, upper_ratio=upper_ratio, lower_ratio=lower_ratio)
        out.append(r)
        c, s, w = r["centres"], r["scales"], r["weight"]
    return out


def scale_fit(c, truth):
    """the centres times the least-squares factor onto the truth (the chordal cost does not fix the scale)"""
    return c * float((c * truth).sum() / (c * c).sum())


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------
_CHECK = []


def check_lib():
    if not _CHECK:
        from panovlm_amd import build
        _CHECK.append(C.CDLL(build.build_transdir_check()))
    return _CHECK[0]


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _f64(a):
    return np.ascontiguousarray(a, np.float64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_group_size():
    return int(check_lib().chk_transdir_group_size())


def _summary(sm, rc):
    return dict(rc=int(rc), initial_cost=sm[0], final_cost=sm[1], successful=int(sm[2]), unsuccessful=int(sm[3]), termination=int(sm[4]))


def host_solve(problem, sc, c0=None, s0=None, weight=None, loss_a=0.5, upper_ratio=1.3, lower_ratio=0.9, max_num_iterations=None):
    """the host compile's solve: the same dict as solve_ref (without knife), plus rc.  On a refusal sm is -7 throughout and the outputs hold the inputs"""
    if max_num_iterations is None:
        max_num_iterations = POLICY[problem][2]
    first, second, d = _i32(sc["first"]), _i32(sc["second"]), _f64(sc["dir"])
    c = _f64(sc["start"] if c0 is None else c0).copy(); sm = np.full(5, -7.0)
    if problem == "chordal":
        rc = check_lib().chk_transdir_chordal(C.c_int(sc["F"]), C.c_int(sc["P"]), _p(first), _p(second), _p(d), C.c_int(sc["origin"]), _p(c), C.c_double(loss_a),
                                              C.c_int(max_num_iterations), _p(sm))
        return dict(_summary(sm, rc), centres=c, scales=None, weight=None, sum_e=None)
    s = _f64(sc["scales"] if s0 is None else s0).copy(); w = (np.ones(sc["P"]) if weight is None else _f64(weight).copy()); sum_e = C.c_double(-7.0)
    rc = check_lib().chk_transdir_lud(C.c_int(sc["F"]), C.c_int(sc["P"]), _p(first), _p(second), _p(d), _p(s), _p(w), C.c_int(sc["origin"]), _p(c), C.c_double(upper_ratio),
                                      C.c_double(lower_ratio), C.c_int(max_num_iterations), C.byref(sum_e), _p(sm))
    return dict(_summary(sm, rc), centres=c, scales=s, weight=w, sum_e=sum_e.value)


def host_irls(sc, solves, upper_ratio=1.3, lower_ratio=0.9):
    c, s, w, out = sc["start"], sc["scales"], np.ones(sc["P"]), []
    for _ in range(solves):
        r = host_solve("lud", sc, c, s, w, upper_ratio=upper_ratio, lower_ratio=lower_ratio)
        out.append(r)
        c, s, w = r["centres"], r["scales"], r["weight"]
    return out


# ---- the scenes of the K46 tests: every one is held to the knife-edge condition by tests/test_transdir_cpu.py ---------------------------------------------------
# How far a value comparison can go.  Both problems amplify a rounding difference along the LM path, measured here between the host compile and solve_ref:
#   lud:     |e|^(1/2) has unbounded curvature at e = 0, so a difference grows about tenfold every four iterations (hub8: 6e-15 m after 8 iterations, 3e-13 after
#            12, 2e-10 after 20, 5e-8 after 30, 1e-2 after the 50 of the default, still with equal step counts).  The comparison scenes therefore run 12 iterations
#            (3 to 6 accepted steps and 6 to 9 rejected ones: every path of the code is taken, the clamp scene's scales are on their bounds by then).
#   chordal: the cost does not see the overall scale, so with outlier pairs the centres drift along that gauge for tens of steps (P257 with 10 % outliers: the costs
#            agree to 9e-9 after 50 iterations, the centres differ by 0.25 m).  The comparison scenes use the directions before the outliers are put in (clean_dir)
#            and converge on the function tolerance in 4 to 12 steps.
# The tests that run the defaults (50 and 300 iterations, the LUD loop) assert what the methods have to achieve, not values.
COMPARE = dict(chordal={}, lud=dict(max_num_iterations=12))


def build_scenes():
    """name -> (problem, scene, keyword arguments of the solve).  Every graph is run under both problems ("chordal-<graph>", "lud-<graph>") but the graphs that only
    one of them can tell apart.  Seeds replaced because the scene failed the knife-edge condition are listed in SEEDS."""
    S = {}
    sd = lambda name, default: SEEDS.get(name, default)

    def add(graph, make, problems=("chordal", "lud"), **kw):
        for problem in problems:
            name = problem + "-" + graph
            sc = make(sd(name, None))
            if problem == "chordal":
                sc = dict(sc, dir=sc["clean_dir"])
            S[name] = (problem, sc, dict(COMPARE[problem], **kw))
    # pairs: a triangle, both sides of a wave, 4 * 64 + 1 (past one trip of a per-pair kernel whose grid is held to one workgroup of 256); shuffled lists with
    # first > second; the origin first, in the middle and last
    add("P3", lambda s: scene(3 if s is None else s, [(0, 1), (1, 2), (0, 2)], 3, noise_deg=1.0, unscaled=0.34))
    for P in (63, 64, 65, 257):
        F = 90 if P == 257 else 22
        add("P%d" % P, lambda s, P=P, F=F: scene(100 + P if s is None else s, tr.pairs_exactly(F, P, P), F, origin=(0, F // 2, F - 1, 3)[P % 4], unscaled=0.3, noise_deg=1.0,
                                                 outliers=0.1))
    # cameras: both sides of a wave (the triangle is P3); every camera with its next 3, shuffled
    for F in (64, 65):
        add("F%d" % F, lambda s, F=F: scene(300 + F if s is None else s, tr.pairs_exactly(F, len(tr.chain_pairs(F, 3)), F), F, origin=F - 1, unscaled=0.3, noise_deg=1.0,
                                            outliers=0.1))
    # a hub camera of degree G - 1, G, G + 1, 2 G + 1
    for deg in (G - 1, G, G + 1, 2 * G + 1):
        add("hub%d" % deg, lambda s, deg=deg: scene(200 + deg if s is None else s, tr.hub_pairs(24, deg, 11), 24, origin=5, unscaled=0.3, noise_deg=1.0))
    # a repeated pair (once in each orientation)
    add("repeat", lambda s: scene(31 if s is None else s, tr.chain_pairs(12, 3) + [(2, 4), (7, 6)], 12, origin=11, unscaled=0.3, noise_deg=1.0, outliers=0.1))
    # LUD alone: all-scaled, all-unscaled (the mixed lists are above), Room's ratios, and a scaled pair whose length is wrong tenfold each way: its scale ends
    # clamped at 3 s0 / 0.5 s0 (ScaleFactor bounds wide enough not to hold it back before)
    add("scaled", lambda s: scene(32 if s is None else s, tr.chain_pairs(16, 3), 16, noise_deg=1.0, outliers=0.1), ("lud",))
    add("unscaled", lambda s: scene(33 if s is None else s, tr.chain_pairs(16, 3), 16, unscaled=1.0, noise_deg=1.0), ("lud",))
    add("room_ratios", lambda s: scene(35 if s is None else s, tr.chain_pairs(20, 4), 20, unscaled=0.3, noise_deg=1.0, outliers=0.1), ("lud",), upper_ratio=1.3, lower_ratio=1.0)
    add("clamp", lambda s: scene(36 if s is None else s, tr.chain_pairs(14, 3), 14, origin=6, wrong_length={4: 0.1, 9: 10.0}), ("lud",), upper_ratio=5.0, lower_ratio=0.2)
    # chordal alone: a wide threshold (every pair an inlier of the Huber loss) and a narrow one (the outlier pairs past it)
    add("wide", lambda s: scene(41 if s is None else s, tr.chain_pairs(16, 3), 16, noise_deg=2.0), ("chordal",), loss_a=2.5)
    add("narrow", lambda s: scene(42 if s is None else s, tr.chain_pairs(16, 3), 16, noise_deg=2.0, outliers=0.1), ("chordal",), loss_a=0.05)
    # the issue's trial: 20 cameras in an 8 m box, every camera with its next 4 (70 pairs), 2 degrees of direction noise, a start 0.3 m off the truth
    add("trial", lambda s: scene(51 if s is None else s, tr.chain_pairs(20, 4), 20, noise_deg=2.0), ("chordal",))
    return S


# seeds replaced on the CPU because the scene failed the knife-edge condition (tests/test_transdir_cpu.py::test_knife_edge names the scene and the reason)
SEEDS = {'chordal-F64': 1011, 'chordal-hub7': 3012, 'chordal-trial': 1013}
# the LUD loop's scene of test_lud_irls_ends_closer: the trial's graph with 15 % outlier pairs, three solves
IRLS_SEED = 52
_SCENES = {}
_REF = {}


def scenes():
    if not _SCENES:
        _SCENES.update(build_scenes())
    return _SCENES


def reference(name):
    """solve_ref of a scene from its start, computed once and shared by the tests"""
    if name not in _REF:
        problem, sc, kw = scenes()[name]
        _REF[name] = solve_ref(problem, sc, **kw)
    return _REF[name]


def irls_scene():
    return scene(IRLS_SEED, tr.chain_pairs(20, 4), 20, noise_deg=2.0, outliers=0.15)


def irls_reference():
    if "irls" not in _REF:
        _REF["irls"] = irls_ref(irls_scene(), 3)
    return _REF["irls"]


# ---- tolerances ------------------------------------------------------------------------------------------------------------------------------
# The largest difference of the host compile against solve_ref over scenes() (tests/test_transdir_cpu.py::test_measured_is_the_maximum prints and bounds
# them): centres and scales in metres, weights, the final cost, sum_e.  With every decision held off its threshold
# only rounding through two different eliminations separates the two; the tolerance of the K46 tests is ten times that.
MEASURED = dict(c=2.1e-10, s=4.7e-9, w=3.2e-9, cost=1.7e-9, sum_e=3.4e-9)
TOL = {k: 10 * v for k, v in MEASURED.items()}


def differences(a, b):
    d = dict(c=float(np.abs(a["centres"] - b["centres"]).max()), cost=float(abs(a["final_cost"] - b["final_cost"])), s=0.0, w=0.0, sum_e=0.0)
    if b["scales"] is not None:
        d.update(s=float(np.abs(a["scales"] - b["scales"]).max()), w=float(np.abs(a["weight"] - b["weight"]).max()), sum_e=float(abs(a["sum_e"] - b["sum_e"])))
    return d


def bad_calls(sc):
    """(name, call, lud_only) for every argument the entry points refuse; the call is the scene with one thing wrong"""
    def mod(**kw):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
        c.update(kw)
        return c
    out = []
    first = sc["first"].copy(); first[1] = sc["F"]
    out.append(("camera index out of range", mod(first=first), False))
    first = sc["first"].copy(); first[1] = -1
    out.append(("negative camera index", mod(first=first), False))
    out.append(("first == second", mod(second=np.where(np.arange(sc["P"]) == 0, sc["first"], sc["second"]).astype(np.int32)), False))
    d = sc["dir"].copy(); d[1, 2] = np.nan
    out.append(("direction not finite", mod(dir=d), False))
    d = sc["dir"].copy(); d[2] *= 1.0 + 1e-8
    out.append(("direction not of unit length", mod(dir=d), False))
    d = sc["dir"].copy(); d[0] = 0.0
    out.append(("direction of zero length", mod(dir=d), False))
    out.append(("origin out of range", mod(origin=sc["F"]), False))
    out.append(("origin negative", mod(origin=-1), False))
    c0 = sc["start"].copy(); c0[sc["origin"], 1] = 1e-300
    out.append(("origin centre not zero", mod(start=c0), False))
    c0 = sc["start"].copy(); c0[(sc["origin"] + 1) % sc["F"], 0] = np.nan
    out.append(("centre not finite", mod(start=c0), False))
    out.append(("max_num_iterations < 0", mod(max_num_iterations=-1), False))
    s = sc["scales"].copy(); s[0] = np.nan
    out.append(("scale not finite", mod(scales=s), True))
    w = np.ones(sc["P"]); w[1] = 0.0
    out.append(("weight zero", mod(weight=w), True))
    w = np.ones(sc["P"]); w[2] = -1.0
    out.append(("weight negative", mod(weight=w), True))
    w = np.ones(sc["P"]); w[0] = np.inf
    out.append(("weight not finite", mod(weight=w), True))
    return out


# ---- the host mirror -------------------------------------------------------------------------------------------------------------------------
def lud_estimate_graph(seed=2):
    """The graph on which EstimateGlobalTranslation's method 6 is compared by value between its two routes: 4 frames, all 6 pairs, scaled, 1 degree of noise.  At
    its defaults (up to 10 solves of 50 iterations) LUD turns ONE ULP of one input into 6e-6 m on transavg_ref.mirror_scene() and into up to 3.5e-4 m on other seeds
    of this graph (COMPARE says why), so a value comparison means something only where the problem is well conditioned: this seed is admitted because a one-ulp
    change of one t_21 moves the host route's result by less than MEASURED["c"] (tests/test_transdir_cpu.py::test_estimate_lud_graph_is_well_conditioned)."""
    sc = tr.scene(seed, [(0, 1), (1, 2), (2, 3), (0, 2), (1, 3), (0, 3)], 4, noise_deg=1.0, size=4.0)
    return dict(F=4, R_wc=np.array([r.T for r in sc["R_cw"]]), t_wc=np.full((4, 3), np.inf), P=sc["P"], size=4.0,
                pairs=[dict(first=int(sc["first"][p]), second=int(sc["second"][p]), R_21=sc["R_21"][p], t_21=sc["t_21"][p].copy(), upper=0.0, lower=0.0) for p in range(sc["P"])])


def run_driver(g, mode, route, method=3, seed=1, num_iteration=3):
    """tests/cpp/pvlm_transdir_driver.cpp on the graph g (the format of transavg_ref.run_driver).  mode "estimate": EstimateGlobalTranslation with `method` and both
    flags set -> dict(ok, message, valid, t_wc, R_wc, pairs); "chordal" / "lud": the mirror function by hand from the DLT start -> dict(ok, iterations, n_pairs, t)."""
    import os
    import subprocess
    import tempfile
    from panovlm_amd import build
    if not os.path.exists(build.TRANSDIR_DRIVER):
        build.build_host()
    lines = [str(g["F"])]
    for i in range(g["F"]):
        lines.append(" ".join([str(i)] + [tr._num(v) for v in g["R_wc"][i].reshape(-1)] + [tr._num(v) for v in g["t_wc"][i]]))
    lines.append(str(len(g["pairs"])))
    for p in g["pairs"]:
        lines.append(" ".join([str(p["first"]), str(p["second"])] + [tr._num(v) for v in np.asarray(p["R_21"]).reshape(-1)] + [tr._num(v) for v in p["t_21"]] +
                              [tr._num(p["upper"]), tr._num(p["lower"])]))
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
        path = f.name
    try:
        args = [build.TRANSDIR_DRIVER, mode, route, path] + ([str(method), str(seed)] if mode == "estimate" else [str(num_iteration)])
        res = subprocess.run(args, capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(path)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    out = dict(ok=None, message="", valid={}, t_wc={}, R_wc={}, pairs=[], t={})
    for line in res.stdout.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "ok":
            out["ok"] = int(w[1])
        elif w[0] == "message":
            out["message"] = line[len("message "):]
        elif w[0] == "frame":
            i = int(w[1]); out["valid"][i] = int(w[2]); v = np.array([float(x) for x in w[3:]])
            out["t_wc"][i] = v[:3]; out["R_wc"][i] = v[3:].reshape(3, 3)
        elif w[0] == "pair":
            out["pairs"].append((int(w[1]), int(w[2])))
        elif w[0] == "iterations":
            out["iterations"] = int(w[1])
        elif w[0] == "pairs":
            out["n_pairs"] = int(w[1])
        elif w[0] == "t":
            out["t"][int(w[1])] = np.array([float(x) for x in w[2:]])
    return out
