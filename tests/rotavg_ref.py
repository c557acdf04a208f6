"""K40 test helpers: synthetic pair graphs with known rotations, an INDEPENDENT numpy float64 reference of RotationAveragingRefineL1 and RotationAveragingL2
(sfm/RotationAveraging.cpp:317-374, :428-582) that carries the FULL system — every pair twice, (i, j, R_21) and (j, i, R_21^T), in the order of upstream's map, a dense
A of 6 P x 3 (F - 1), dense numpy.linalg solves, a dense LM for the L2 stage with the Jacobians in their right-perturbation form — so it shares neither the halving
nor the dense inverse nor the Jacobian formulas with panovlm_amd/csrc/pvlm_rotavg_core.h; the scenes of the K40 tests, the knife-edge condition they are held to
(the same counts with every stopping threshold scaled by 1 +- 1e-6) and the ctypes wrappers of the host compile of the core (tests/cpp/rotavg_core_check.cpp)."""
import ctypes as C

import numpy as np

MIN_RELATIVE_DECREASE, FUNCTION_TOL, GRADIENT_TOL, PARAMETER_TOL = 1e-3, 1e-6, 1e-10, 1e-8
INITIAL_RADIUS, MAX_RADIUS, MIN_RADIUS, MIN_LM_DIAG, MAX_LM_DIAG = 1e4, 1e16, 1e-32, 1e-6, 1e32
ADMM_ABS, ADMM_REL, ADMM_MAX, OUTER_MAX, OUTER_E, OUTER_REL = 1e-4, 1e-2, 1000, 32, 1e-5, 1e-2


# ---- rotations -------------------------------------------------------------------------------------------------------------------------------
def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def exp_so3(w):
    """ceres::AngleAxisToRotationMatrix"""
    w = np.asarray(w, np.float64); th2 = float(w @ w)
    if th2 > np.finfo(np.float64).eps:
        th = np.sqrt(th2); k = w / th
        return np.cos(th) * np.eye(3) + np.sin(th) * hat(k) + (1 - np.cos(th)) * np.outer(k, k)
    return np.eye(3) + hat(w)


def log_so3(R):
    """ceres::RotationMatrixToAngleAxis: through the quaternion, the branch by the trace"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if tr >= 0:
        t = np.sqrt(tr + 1.0); q[0] = 0.5 * t; t = 0.5 / t
        q[1:] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = int(np.argmax(np.diag(R))); j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0); q[i + 1] = 0.5 * t; t = 0.5 / t
        q[0] = (R[k, j] - R[j, k]) * t; q[j + 1] = (R[j, i] + R[i, j]) * t; q[k + 1] = (R[k, i] + R[i, k]) * t
    s2 = float(q[1:] @ q[1:])
    if s2 > 0:
        s = np.sqrt(s2)
        two_theta = 2.0 * (np.arctan2(-s, -q[0]) if q[0] < 0 else np.arctan2(s, q[0]))
        return q[1:] * (two_theta / s)
    return q[1:] * 2.0


def angle_between(Ra, Rb):
    """the angle of Ra^T Rb, radians (through the skew part and the trace: accurate near zero)"""
    E = Ra.T @ Rb
    s = 0.5 * np.sqrt((E[2, 1] - E[1, 2]) ** 2 + (E[0, 2] - E[2, 0]) ** 2 + (E[1, 0] - E[0, 1]) ** 2)
    return float(np.arctan2(s, 0.5 * (np.trace(E) - 1.0)))


def right_jacobian(w):
    """J_r(w): exp(w + d) = exp(w) exp(J_r d) to first order, closed form (Taylor below 1e-4 rad)"""
    th = float(np.linalg.norm(w)); K = hat(w)
    if th < 1e-4:
        return np.eye(3) - 0.5 * K + K @ K / 6.0
    return np.eye(3) - (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K


def right_jacobian_inverse(w):
    th = float(np.linalg.norm(w)); K = hat(w)
    if th < 1e-4:
        return np.eye(3) + 0.5 * K + K @ K / 12.0
    return np.eye(3) + 0.5 * K + (1 / th ** 2 - (1 + np.cos(th)) / (2 * th * np.sin(th))) * K @ K


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def chain_pairs(F, reach):
    return [(i, i + k) for i in range(F) for k in range(1, reach + 1) if i + k < F]


def hub_pairs(F, degree, hub):
    """a chain (every camera with its next 2) plus a hub camera tied to `degree` cameras in all"""
    pairs = chain_pairs(F, 2)
    have = {tuple(sorted(p)) for p in pairs}
    deg = sum(1 for p in pairs if hub in p)
    c = 0
    while deg < degree and c < F:
        if c != hub and tuple(sorted((c, hub))) not in have:
            pairs.append((hub, c) if c % 2 else (c, hub)); have.add(tuple(sorted((c, hub)))); deg += 1
        c += 1
    assert deg == degree, (deg, degree)
    return pairs


def shuffled(pairs, seed):
    """the list in another order, three in ten with first > second"""
    rng = np.random.default_rng(seed)
    pairs = [pairs[k] for k in rng.permutation(len(pairs))]
    return [(j, i) if rng.random() < 0.3 else (i, j) for i, j in pairs]


def spanning_tree_start(F, first, second, R21, start):
    """The host mirror's RotationAveragingSpanningTree: Kruskal over the pairs in list order (all weights equal) by union-find, the tree walked breadth-first from
    start; a child's rotation is R_cp R_parent."""
    root = list(range(F))

    def find(c):
        while root[c] != c:
            root[c] = root[root[c]]; c = root[c]
        return c
    adj = {c: [] for c in range(F)}
    for p in range(len(first)):
        a, b = find(int(first[p])), find(int(second[p]))
        if a != b:
            root[a] = b
            adj[int(first[p])].append((int(second[p]), p, False)); adj[int(second[p])].append((int(first[p]), p, True))
    R = np.zeros((F, 3, 3)); R[start] = np.eye(3)
    seen = {start}; queue = [start]
    while queue:
        c = queue.pop(0)
        for d, p, child_is_first in adj[c]:
            if d in seen:
                continue
            R[d] = (R21[p].T if child_is_first else R21[p]) @ R[c]
            seen.add(d); queue.append(d)
    for c in range(F):
        if c not in seen:
            R[c] = np.eye(3)              # a camera the pairs do not reach (the refused calls)
    return R


def scene(seed, pairs, n_cameras, start=0, noise_deg=1.0, outliers=0.0):
    """A pair graph: random rotations R_cw, R_21 = R_2 R_1^T turned by noise_deg (normal) about a random axis; `outliers`: this fraction of the pairs gets a
    random rotation.  R0: the spanning-tree start (identity at start); truth: R_cw R_start^T."""
    rng = np.random.default_rng(seed)
    F = n_cameras; pairs = np.asarray(pairs, np.int32).reshape(-1, 2); P = len(pairs)
    Rc = np.array([exp_so3(rng.normal(size=3) * 0.6) for _ in range(F)])
    bad = set(rng.permutation(P)[:int(round(outliers * P))].tolist()) if outliers > 0 else set()
    R21 = np.zeros((P, 3, 3))
    for p, (i, j) in enumerate(pairs):
        R21[p] = Rc[j] @ Rc[i].T
        if noise_deg > 0:
            a = rng.normal(size=3); a /= np.linalg.norm(a)
            R21[p] = exp_so3(np.radians(noise_deg) * rng.normal() * a) @ R21[p]
        if p in bad:
            R21[p] = exp_so3(rng.normal(size=3) * 1.5)
    first, second = pairs[:, 0].copy(), pairs[:, 1].copy()
    return dict(F=F, P=P, first=first, second=second, R_21=R21, start=start, truth=np.array([R @ Rc[start].T for R in Rc]), bad=sorted(bad),
                R0=spanning_tree_start(F, first, second, R21, start))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def l1_ref(sc, R0=None, scale=1.0):
    """RotationAveragingRefineL1 on the full 2 P rows.  Returns dict(rotations, l1, admm, irls, info, knife); scale multiplies every stopping threshold.  knife: the
    decisions no threshold scales that rounding alone took — an IRLS system that is FINITE and still fails its factorisation (empty: nothing of the kind)."""
    F, start = sc["F"], sc["start"]
    rel = {}
    for p in range(sc["P"]):
        i, j = int(sc["first"][p]), int(sc["second"][p])
        rel[(i, j)] = sc["R_21"][p]; rel[(j, i)] = sc["R_21"][p].T
    keys = sorted(rel)
    m, n = 3 * len(keys), 3 * (F - 1)
    A = np.zeros((m, n))
    for r, (i, j) in enumerate(keys):
        for c, v in ((i, -1.0), (j, 1.0)):
            if c != start:
                q = 3 * (c - (c >= start))
                A[3 * r:3 * r + 3, q:q + 3] = v * np.eye(3)
    AtA_inv = np.linalg.inv(A.T @ A) if n else np.zeros((0, 0))       # once: the matrix never changes (six thousand ADMM iterations on the largest scenes)
    R = np.array(sc["R0"] if R0 is None else R0, np.float64).copy()
    out = dict(l1=0, admm=0, irls=0, info=0, knife=[])
    big = np.finfo(np.float64).max
    if F == 1:
        out["rotations"] = R
        return out

    def errors():
        return np.concatenate([log_so3(R[j].T @ rel[(i, j)] @ R[i]) for i, j in keys])

    def update(x):
        for c in range(F):
            if c != start:
                q = 3 * (c - (c >= start))
                R[c] = R[c] @ exp_so3(x[q:q + 3])

    shrink = lambda v, k: np.maximum(0.0, v - k) - np.maximum(0.0, -v - k)
    curr, it = big, 0
    while True:
        b = errors()
        z = np.zeros(m); u = np.zeros(m); x = np.zeros(n)
        b_norm = np.linalg.norm(b)
        for _ in range(ADMM_MAX):
            x = AtA_inv @ (A.T @ (b + z - u))
            ax = A @ x
            z_old = z
            z = shrink(ax - b + u, 1.0)
            u = u + (ax - z - b)
            out["admm"] += 1
            r_norm = np.linalg.norm(ax - z - b); s_norm = np.linalg.norm(A.T @ (z - z_old))
            primal = np.sqrt(m) * ADMM_ABS * scale + ADMM_REL * scale * max(np.linalg.norm(ax), np.linalg.norm(z), b_norm)
            dual = np.sqrt(n) * ADMM_ABS * scale + ADMM_REL * scale * np.linalg.norm(A.T @ u)
            if r_norm < primal and s_norm < dual:
                break
        last, curr = curr, np.linalg.norm(x)
        if (last if last == big else last * scale) < curr:
            break
        update(x)
        it += 1
        if not (it < OUTER_MAX and curr > OUTER_E * scale and (last == big or (last - curr) / curr > OUTER_REL * scale)):
            break
    out["l1"] = it
    x = np.zeros(n); curr, last, it = big, -1.0, 0
    while True:
        last_x = x
        b = errors()
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.abs(A @ x - b) ** -1.5
            M = A.T @ (w[:, None] * A); rhs = A.T @ (w * b)
        ok = bool(np.isfinite(M).all() and np.isfinite(rhs).all())
        if ok:
            try:
                Lc = np.linalg.cholesky(M)
                x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))
                ok = bool(np.isfinite(x).all())
            except np.linalg.LinAlgError:
                ok = False
                out["knife"].append("IRLS iteration %d: a finite system failed its factorisation (largest diagonal %.3g)" % (it, np.diag(M).max()))
        if not ok:
            out["info"] = 1
            break
        update(x)
        last, curr = curr, np.linalg.norm(last_x - x)
        it += 1
        if not (it < OUTER_MAX and curr > OUTER_E * scale and (last == big or (last - curr) / curr > OUTER_REL * scale)):
            break
    out["irls"] = it
    out["rotations"] = R
    return out


def l2_pair_ref(aa1, aa2, R21):
    """residual and Jacobians of PairWiseRotationResidual, right-perturbation form: with N = R_1^T R_21^T, d r / d aa_2 = J_r^-1(r) N^T J_r(aa_2) and
    d r / d aa_1 = -J_r^-1(r) N^T J_r(aa_1)"""
    R1, R2 = exp_so3(aa1), exp_so3(aa2)
    N = R1.T @ R21.T
    r = log_so3(R2 @ N)
    Ji = right_jacobian_inverse(r)
    return r, -Ji @ N.T @ right_jacobian(aa1), Ji @ N.T @ right_jacobian(aa2)


def l2_ref(sc, R_in, loss_a=0.07, max_num_iterations=50, scale=1.0):
    """RotationAveragingL2 as a dense LM over 3 F unknowns with ceres_like::Solve's policy.  Returns dict(rotations, initial_cost, final_cost, successful,
    unsuccessful, termination); scale multiplies every stopping threshold."""
    F, P, first, second, R21 = sc["F"], sc["P"], sc["first"], sc["second"], sc["R_21"]

    def evaluate(aa):
        J = np.zeros((3 * P, 3 * F)); res = np.zeros(3 * P); cost = 0.0
        for p in range(P):
            i, j = int(first[p]), int(second[p])
            r, J1, J2 = l2_pair_ref(aa[i], aa[j], R21[p])
            s2 = float(r @ r)
            if loss_a < 0:
                rho, rw = s2, 1.0
            else:
                b = loss_a * loss_a; q = np.sqrt(1 + s2 / b); rho, rw = 2 * b * (q - 1), 1 / q
            w = np.sqrt(rw)
            J[3 * p:3 * p + 3, 3 * i:3 * i + 3] = w * J1; J[3 * p:3 * p + 3, 3 * j:3 * j + 3] = w * J2; res[3 * p:3 * p + 3] = w * r
            cost += 0.5 * rho
        return cost, J.T @ J, J.T @ res

    aa = np.array([log_so3(R) for R in R_in])
    out = dict(successful=0, unsuccessful=0, termination=-1)
    if P == 0:
        out.update(initial_cost=0.0, final_cost=0.0, termination=6, rotations=np.array(R_in, np.float64).copy())
        return out
    cost, H, g = evaluate(aa)
    out["initial_cost"] = cost
    sig = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(H), 0.0)))
    radius, dec, it = INITIAL_RADIUS, 2.0, 0
    if not np.isfinite(cost):
        out["termination"] = 5
    elif max_num_iterations > 0 and np.abs(g).max() <= GRADIENT_TOL * scale:
        out["termination"] = 2
    while out["termination"] < 0 and it < max_num_iterations:
        it += 1
        Hs = H * sig[:, None] * sig[None, :]
        D = np.clip(np.diag(Hs), MIN_LM_DIAG, MAX_LM_DIAG) / radius
        ok = True
        try:
            Lc = np.linalg.cholesky(Hs + np.diag(D))
            step = sig * np.linalg.solve(Lc.T, np.linalg.solve(Lc, -g * sig))
        except np.linalg.LinAlgError:
            ok = False
        accepted = False
        if ok:
            model = -(g @ step + 0.5 * step @ H @ step)
            ok = model > 0 and np.isfinite(model)
        if ok:
            c_aa = aa + step.reshape(F, 3)
            c_cost, cH, cg = evaluate(c_aa)
            rho = (cost - c_cost) / model
            if np.isfinite(c_cost) and rho > MIN_RELATIVE_DECREASE * scale:
                accepted = True
                xn = np.linalg.norm(aa)
                change, prev = cost - c_cost, cost
                aa, cost, H, g = c_aa, c_cost, cH, cg
                radius = min(MAX_RADIUS, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                dec = 2.0
                out["successful"] += 1
                if abs(change) <= FUNCTION_TOL * scale * prev:
                    out["termination"] = 1
                elif np.abs(g).max() <= GRADIENT_TOL * scale:
                    out["termination"] = 2
                elif np.linalg.norm(step) <= PARAMETER_TOL * scale * (xn + PARAMETER_TOL * scale):
                    out["termination"] = 3
        if not accepted:
            out["unsuccessful"] += 1
            radius /= dec; dec *= 2.0
            if radius < MIN_RADIUS:
                out["termination"] = 4
    if out["termination"] < 0:
        out["termination"] = 0
    out.update(final_cost=cost, rotations=np.array([exp_so3(a) for a in aa]))
    return out


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------
_CHECK = []


def check_lib():
    if not _CHECK:
        from panovlm_amd import build
        _CHECK.append(C.CDLL(build.build_rotavg_check()))
    return _CHECK[0]


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _f64(a):
    return np.ascontiguousarray(a, np.float64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_group_size():
    return int(check_lib().chk_rotavg_group_size())


def host_tile():
    return int(check_lib().chk_rotavg_tile())


def host_l1(sc, R0=None):
    """the host compile's RotationAveragingRefineL1: the same dict as l1_ref, plus rc"""
    first, second, R21 = _i32(sc["first"]), _i32(sc["second"]), _f64(sc["R_21"])
    R = _f64(sc["R0"] if R0 is None else R0).copy(); sm = np.full(4, -7, np.int32)
    rc = check_lib().chk_rotavg_l1(C.c_int(sc["F"]), C.c_int(sc["P"]), _p(first), _p(second), _p(R21), C.c_int(sc["start"]), _p(R), _p(sm))
    return dict(rc=int(rc), rotations=R, l1=int(sm[0]), admm=int(sm[1]), irls=int(sm[2]), info=int(sm[3]))


def host_l2(sc, R_in, loss_a=0.07, max_num_iterations=50):
    """the host compile's RotationAveragingL2: the same dict as l2_ref, plus rc"""
    first, second, R21 = _i32(sc["first"]), _i32(sc["second"]), _f64(sc["R_21"])
    R = _f64(R_in).copy(); sm = np.zeros(5)
    rc = check_lib().chk_rotavg_l2(C.c_int(sc["F"]), C.c_int(sc["P"]), _p(first), _p(second), _p(R21), _p(R), C.c_double(loss_a), C.c_int(max_num_iterations), _p(sm))
    return dict(rc=int(rc), rotations=R, initial_cost=sm[0], final_cost=sm[1], successful=int(sm[2]), unsuccessful=int(sm[3]), termination=int(sm[4]))


def host_l2_pair(aa1, aa2, R21):
    aa1, aa2, R21 = _f64(aa1), _f64(aa2), _f64(R21)
    r = np.zeros(3); J1 = np.zeros((3, 3)); J2 = np.zeros((3, 3))
    check_lib().chk_rotavg_l2_pair(_p(aa1), _p(aa2), _p(R21), _p(r), _p(J1), _p(J2))
    return r, J1, J2


# ---- the scenes of the K40 tests: every one is held to the knife-edge condition by tests/test_rotavg_cpu.py -----------------------------------------------------
G = 8       # pvlm_rotavg_group_size(); tests assert it
TILE = 64   # the lanes across one row of the dense product; tests assert it


def build_scenes():
    """name -> scene.  The smallest that can still go wrong: a triangle; K4 with start_idx in the middle (the index shift); a 9-ring with chords; a hub camera of
    degree G - 1, G, G + 1, 2 G + 1; F - 1 = TILE - 1, TILE, TILE + 1 with reach 3 (F = 65: the per-camera groups pass one workgroup); noise-free; 10 % outliers."""
    S = {}
    sd = lambda name, default: SEEDS.get(name, default)
    S["tri"] = scene(sd("tri", 3), [(0, 1), (1, 2), (0, 2)], 3)
    S["K4"] = scene(sd("K4", 4), [(0, 1), (0, 2), (3, 0), (1, 2), (3, 1), (2, 3)], 4, start=2)
    S["ring9"] = scene(sd("ring9", 9), shuffled([(i, (i + 1) % 9) for i in range(9)] + [(0, 4), (2, 7), (3, 8)], 9), 9, start=8)
    for deg in (G - 1, G, G + 1, 2 * G + 1):
        name = "hub%d" % deg
        S[name] = scene(sd(name, 200 + deg), hub_pairs(24, deg, 11), 24, start=5)
    for F in (TILE, TILE + 1, TILE + 2):
        name = "F%d" % F
        S[name] = scene(sd(name, 300 + F), shuffled(chain_pairs(F, 3), F), F, start=(0, F // 2, F - 1)[F % 3])
    S["exact"] = scene(sd("exact", 37), chain_pairs(12, 3), 12, start=3, noise_deg=0.0)
    S["outlier10"] = scene(sd("outlier10", 38), shuffled(chain_pairs(40, 4), 40), 40, start=17, outliers=0.1)
    return S


# Candidate seeds replaced on the CPU because the scene failed the knife-edge condition (tests/test_rotavg_cpu.py::test_knife_edge): name -> seed in use.
# DROPPED records the candidates given up and why; at most one candidate in five may be.
SEEDS = {"F65": 1365}
DROPPED = {"F65 seed 365": "the first IRLS system is finite (largest diagonal 8.4e24: a pair error of 1e-17) and fails its factorisation in the reference by rounding: a "
                           "decision no threshold scales; the host compile passes that iteration and fails the next (1 of 13 candidates)"}
_SCENES = {}
_REF = {}


def scenes():
    if not _SCENES:
        _SCENES.update(build_scenes())
    return _SCENES


def reference(name):
    """(l1_ref, l2_ref from l1_ref's rotations) of a scene, computed once and shared by the tests"""
    if name not in _REF:
        sc = scenes()[name]
        a = l1_ref(sc)
        _REF[name] = (a, l2_ref(sc, a["rotations"]))
    return _REF[name]


def counts_l1(r):
    return (r["l1"], r["admm"], r["irls"], r["info"] > 0)


def counts_l2(r):
    return (r["successful"], r["unsuccessful"], r["termination"])


def largest_angle(Ra, Rb):
    return max(angle_between(Ra[c], Rb[c]) for c in range(len(Ra)))


# ---- tolerances ------------------------------------------------------------------------------------------------------------------------------
# The largest difference of the host compile against the reference over scenes() (tests/test_rotavg_cpu.py::test_measured_is_the_maximum prints and bounds them):
# rotation angle in radians after the L1 stages and after the L2 stage, the L2 final cost; x84: the X84 threshold of FilterPairs on the mirror scene, the host mirror
# against filter_pairs_ref on the same rotations (radians).  It covers the 2 P-versus-P rounding and the different solve orders; the
# tolerance of the K40 tests is ten times that.  The angle after the L1 stages is as large as it is because of the IRLS stage as upstream defines it: the L1 stage
# leaves pair errors of 1e-13 rad and less (least absolute deviations interpolates), their weights |e|^-1.5 reach 1e20 against 1e3 for an ordinary pair, and the
# weighted systems have condition numbers of 1e15 to 1e17 (hub7, F64, F66): rounding is amplified up to there.  The L2 stage, which starts from the same rotations on
# both sides, shows what rounding alone does.
MEASURED = dict(angle_l1=3.8e-5, angle_l2=1.2e-13, cost=8.9e-16, x84=2.5e-16)
TOL = {k: 10 * v for k, v in MEASURED.items()}


def bad_calls(sc):
    """(name, call) for every argument the entry points refuse; the call is the scene with one thing wrong"""
    def mod(**kw):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
        c.update(kw)
        return c
    out = []
    first = sc["first"].copy(); first[1] = sc["F"]
    out.append(("camera index out of range", mod(first=first)))
    first = sc["first"].copy(); first[1] = -1
    out.append(("negative camera index", mod(first=first)))
    out.append(("first == second", mod(second=np.where(np.arange(sc["P"]) == 0, sc["first"], sc["second"]).astype(np.int32))))
    first = sc["first"].copy(); second = sc["second"].copy(); first[1], second[1] = first[0], second[0]
    out.append(("the same pair twice", mod(first=first, second=second)))
    first = sc["first"].copy(); second = sc["second"].copy(); first[1], second[1] = second[0], first[0]
    out.append(("the same pair twice, turned round", mod(first=first, second=second)))
    R = sc["R_21"].copy(); R[1, 2, 0] = np.nan
    out.append(("relative rotation not finite", mod(R_21=R)))
    R0 = sc["R0"].copy(); R0[(sc["start"] + 1) % sc["F"], 0, 1] = np.inf
    out.append(("rotation not finite", mod(R0=R0)))
    out.append(("start_idx out of range", mod(start=sc["F"])))
    out.append(("start_idx negative", mod(start=-1)))
    R0 = sc["R0"].copy(); R0[sc["start"], 0, 1] = 1e-300
    out.append(("start rotation not the identity", mod(R0=R0)))
    out.append(("pair graph not connected", scene(1, [(0, 1), (1, 2), (0, 2), (3, 4)], 5)))
    return out


# ---- the host mirror's EstimateGlobalRotation: plain-Python restatements of its host-side pieces and the driver ------------------------------------------------
def find_triplet_ref(edges):
    """PoseGraph::FindTriplet (sfm/PoseGraph.cpp:195-226): per edge in sorted order the common neighbours of its ends, then the edge leaves the adjacency"""
    edges = sorted(set(edges))
    adj = {}
    for a, b in edges:
        adj.setdefault(a, set()).add(b); adj.setdefault(b, set()).add(a)
    out = []
    for a, b in edges:
        out += [tuple(sorted((n, a, b))) for n in sorted(adj[a] & adj[b])]
        adj[a].discard(b); adj[b].discard(a)
    return out


def triplet_angle_deg(R_21, R_32, R_31):
    """SfM::FilterByTriplet's measure as written (:739-742): acos of the trace of R_13 R_32 R_21 over 3, degrees"""
    return float(np.degrees(np.arccos(min(1.0, max(np.trace(R_31.T @ R_32 @ R_21) / 3.0, -1.0)))))


def filter_by_triplet_ref(pairs, angle_threshold):
    """(the pairs kept, in list order; the frames covered) of SfM::FilterByTriplet on a list of dict(first, second, R_21)"""
    from tests import transavg_ref as tr
    rot = {(p["first"], p["second"]): np.asarray(p["R_21"]) for p in pairs}
    keep = set()
    for i, j, k in find_triplet_ref(rot.keys()):
        if triplet_angle_deg(rot[(i, j)], rot[(j, k)], rot[(i, k)]) < angle_threshold:
            keep |= {(i, j), (j, k), (i, k)}
    left = [p for p in pairs if (p["first"], p["second"]) in keep]
    nodes = tr.largest_edge_biconnected([(p["first"], p["second"]) for p in left])
    return [p for p in left if p["first"] in nodes and p["second"] in nodes], sorted(nodes)


def filter_pairs_ref(pairs, R_cw):
    """FilterPairs (sfm/RotationAveraging.cpp:11-183) with the X84 threshold: (threshold in radians, the indices kept in ascending order, the errors)"""
    err = np.array([np.linalg.norm(log_so3(R_cw[p["second"]].T @ np.asarray(p["R_21"]) @ R_cw[p["first"]])) for p in pairs])
    mid = len(err) // 2
    median = np.sort(err)[mid]
    threshold = median + 5.2 * np.sort(np.abs(err - median))[mid]
    valid = {i for i in range(len(err)) if err[i] < threshold}; invalid = set(range(len(err))) - valid
    n = len(R_cw); before = [0] * n; after = [0] * n
    near = lambda p: 0 <= p["second"] - p["first"] <= 10
    for i in sorted(valid):
        if near(pairs[i]):
            after[pairs[i]["first"]] += 1; before[pairs[i]["second"]] += 1
    bad = {f: [] for f in range(n) if before[f] < 3 or after[f] < 3}
    for i in sorted(invalid):
        p = pairs[i]
        if near(p):
            if p["first"] in bad and after[p["first"]] < 3:
                bad[p["first"]].append(i)
            if p["second"] in bad and before[p["second"]] < 3:
                bad[p["second"]].append(i)
    for f in sorted(bad):
        if before[f] >= 3 and after[f] >= 3:
            continue
        order = sorted(bad[f], key=lambda i: (err[i], i))
        for side, count in (("second", before), ("first", after)):
            for i in order:
                if count[f] >= 3:
                    break
                if pairs[i][side] != f:
                    continue
                valid.add(i); invalid.discard(i)
                after[pairs[i]["first"]] += 1; before[pairs[i]["second"]] += 1
    return float(threshold), sorted(valid), err


def mirror_scene(seed=11, F=14, reach=4, noise_deg=0.01, triplet_bad=(8, 10), x84_bad=(5, 7), size=8.0):
    """F frames, every frame with its next `reach`; relative rotations with noise_deg of noise, relative translations exact and scaled.  One planted pair 5 degrees
    off, which no triplet survives with: the triplet test must drop it.  One planted pair 0.08 degrees off: its triplets pass 0.1 degrees (the measure as written
    reads 0.82 of the angle), the X84 threshold (a few hundredths of a degree at this noise) must drop it; both its frames keep three neighbours on each side, so
    the frame rule does not take it back.  No frame has a pose yet."""
    rng = np.random.default_rng(seed)
    Rc = np.array([exp_so3(rng.normal(size=3) * 0.6) for _ in range(F)])
    Cw = rng.uniform(-size / 2, size / 2, (F, 3))
    t = -np.einsum("cij,cj->ci", Rc, Cw)
    pairs = []
    for i, j in chain_pairs(F, reach):
        R21 = Rc[j] @ Rc[i].T
        tv = t[j] - R21 @ t[i]
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        deg = 5.0 if (i, j) == tuple(triplet_bad) else (0.08 if (i, j) == tuple(x84_bad) else noise_deg * rng.normal())
        pairs.append(dict(first=i, second=j, R_21=exp_so3(np.radians(deg) * a) @ R21, t_21=tv, upper=0.0, lower=0.0))
    return dict(F=F, R_wc=np.zeros((F, 3, 3)), t_wc=np.full((F, 3), np.inf), pairs=pairs, R_cw_true=Rc, centres=Cw, P=len(pairs), size=size)


def _num(v):
    return "inf" if v == np.inf else ("-inf" if v == -np.inf else repr(float(v)))


def run_driver(g, mode, route="host", *args):
    """tests/cpp/pvlm_rotavg_driver.cpp on the graph g.  Returns dict(ok, message, translation_ok, valid, t_wc, R_wc, pairs [(first, second)], R_21, triplets, covered,
    threshold, rotations)."""
    import os
    import subprocess
    import tempfile
    from panovlm_amd import build
    if not os.path.exists(build.ROTAVG_DRIVER):
        build.build_host()
    lines = [str(g["F"])]
    for i in range(g["F"]):
        lines.append(" ".join([str(i)] + [_num(v) for v in np.asarray(g["R_wc"][i]).reshape(-1)] + [_num(v) for v in g["t_wc"][i]]))
    lines.append(str(len(g["pairs"])))
    for p in g["pairs"]:
        lines.append(" ".join([str(p["first"]), str(p["second"])] + [_num(v) for v in np.asarray(p["R_21"]).reshape(-1)] + [_num(v) for v in p["t_21"]] +
                              [_num(p["upper"]), _num(p["lower"])]))
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
        path = f.name
    try:
        res = subprocess.run([build.ROTAVG_DRIVER, mode, route, path] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(path)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    out = dict(ok=None, message="", translation_ok=None, translation_message="", valid={}, t_wc={}, R_wc={}, pairs=[], R_21=[], triplets=[], covered=[], threshold=None, rotations={})
    for line in res.stdout.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] in ("ok", "translation_ok"):
            out[w[0]] = int(w[1])
        elif w[0] in ("message", "translation_message"):
            out[w[0]] = line[len(w[0]) + 1:]
        elif w[0] == "frame":
            i = int(w[1]); out["valid"][i] = int(w[2]); v = np.array([float(x) for x in w[3:]])
            out["t_wc"][i] = v[:3]; out["R_wc"][i] = v[3:].reshape(3, 3)
        elif w[0] == "pair":
            out["pairs"].append((int(w[1]), int(w[2]))); out["R_21"].append(np.array([float(x) for x in w[3:]]).reshape(3, 3))
        elif w[0] == "triplet":
            out["triplets"].append((int(w[1]), int(w[2]), int(w[3])))
        elif w[0] == "covered":
            out["covered"].append(int(w[1]))
        elif w[0] == "threshold":
            out["threshold"] = float(w[1])
        elif w[0] == "rotation":
            out["rotations"][int(w[1])] = np.array([float(x) for x in w[2:]]).reshape(3, 3)
    return out


def chain_error(g, c):
    """(the scale, the largest centre error in metres after taking the scale out) of a `chain` run c against the truth of the mirror scene g, in frame 0's gauge"""
    R0 = g["R_cw_true"][0]
    est = np.array([c["t_wc"][i] for i in range(g["F"])]); truth = np.array([R0 @ (g["centres"][i] - g["centres"][0]) for i in range(g["F"])])
    s = float((est * truth).sum() / (truth * truth).sum())
    return s, float(np.linalg.norm(est / s - truth, axis=1).max())


def estimate_ref(g):
    """EstimateGlobalRotation (sfm/SfM.cpp:811-905) for method 1 in Python around the host compile's two solves: the filters, the re-indexing, the spanning tree,
    FilterPairs.  Returns dict(pairs, R_cw {old frame: matrix}, threshold, after_triplet, errors, kept, l1_rotations: what
    FilterPairs was handed, by camera)."""
    from tests import transavg_ref as tr
    nodes = tr.largest_edge_biconnected([(p["first"], p["second"]) for p in g["pairs"]])
    pairs = [p for p in g["pairs"] if p["first"] in nodes and p["second"] in nodes]
    pairs, covered = filter_by_triplet_ref(pairs, 0.1)
    after_triplet = [(p["first"], p["second"]) for p in pairs]
    new = {old: k for k, old in enumerate(covered)}
    pairs = [dict(p, first=new[p["first"]], second=new[p["second"]]) for p in pairs]
    sc = dict(F=len(covered), P=len(pairs), first=np.array([p["first"] for p in pairs], np.int32), second=np.array([p["second"] for p in pairs], np.int32),
              R_21=np.array([p["R_21"] for p in pairs]), start=0)
    sc["R0"] = spanning_tree_start(sc["F"], sc["first"], sc["second"], sc["R_21"], 0)
    h1 = host_l1(sc)
    assert h1["rc"] == 0 and h1["info"] == 0
    threshold, kept, err = filter_pairs_ref(pairs, h1["rotations"])
    pairs = [pairs[i] for i in kept]
    sc2 = dict(F=sc["F"], P=len(pairs), first=np.array([p["first"] for p in pairs], np.int32), second=np.array([p["second"] for p in pairs], np.int32),
               R_21=np.array([p["R_21"] for p in pairs]))
    h2 = host_l2(sc2, h1["rotations"])
    assert h2["rc"] == 0
    return dict(pairs=[(covered[p["first"]], covered[p["second"]]) for p in pairs], R_cw={old: h2["rotations"][k] for old, k in new.items()}, threshold=threshold,
                after_triplet=after_triplet, errors=err, kept=kept, l1_rotations=h1["rotations"])
