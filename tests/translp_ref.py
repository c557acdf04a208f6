"""K47 test helpers: an INDEPENDENT numpy / scipy.sparse transcription of TranslationAveragingL1 (sfm/TranslationAveraging.cpp:277-417) that builds A, the bounds and
the cost literally — every row, the lambda and gamma columns, the origin's bounds — and hands them to scipy.optimize.linprog(method="highs"); it shares no code with
panovlm_amd/csrc/pvlm_translp_core.h (no elimination, no interior point).  Also: the triplets of a pair list (PoseGraph::FindTriplet), the certificate that needs no
reference (primal and dual feasibility and the gap, re-evaluated in numpy), the named scenes, the admission rule every scene is held to by tests/test_translp_cpu.py,
and the ctypes wrappers of the host compile of the core (tests/cpp/translp_core_check.cpp, built by panovlm_amd.build.build_translp_check)."""
import ctypes as C

import numpy as np

from tests import transavg_ref as tr

G = 8   # pvlm_translp_group_size(); tests assert it
ROWS = 19
GAP_TOL = FEAS_TOL = 1e-9
MAX_ITERATIONS = 60
TERMINATIONS = dict(converged=0, iteration_limit=1, factorisation_lost=2, not_finite=3, no_triplets=6)


# ---- the triplets ----------------------------------------------------------------------------------------------------------------------------
def find_triplets(first, second):
    """PoseGraph::FindTriplet (sfm/PoseGraph.cpp:195-226) over the pair list: per edge in ascending order, the nodes adjacent to both its ends, then the edge leaves
    the adjacency.  Returns (triplets T x 3 cameras i < j < k, triplet_pairs T x 3: the indices of (i,j), (j,k), (i,k); a repeated pair resolves to its last index)."""
    idx = {}
    for p, (a, b) in enumerate(zip(first, second)):
        idx[(int(a), int(b))] = p
    adj = {}
    for a, b in idx:
        adj.setdefault(a, set()).add(b); adj.setdefault(b, set()).add(a)
    trips = []
    for a, b in sorted(idx):
        for n in sorted(adj[a] & adj[b]):
            trips.append(tuple(sorted((n, a, b))))
        adj[a].discard(b); adj[b].discard(a)
    tp = [(idx[(i, j)], idx[(j, k)], idx[(i, k)]) for i, j, k in trips]
    return np.asarray(trips, np.int32).reshape(-1, 3), np.asarray(tp, np.int32).reshape(-1, 3)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def lower_bounds(sc):
    n = np.linalg.norm(sc["t_21"], axis=1)
    return 0.9 * n[sc["triplet_pairs"]].mean(axis=1) if len(sc["triplet_pairs"]) else np.zeros(0)


def lp_ref(sc):
    """:277-417 as written, solved by HiGHS.  Returns dict(gamma, t (F x 3), lam, status)."""
    import scipy.sparse as sp
    from scipy.optimize import linprog
    F, T = sc["F"], len(sc["triplets"])
    nv = 3 * F + T + 1
    lam0, gam = 3 * F, 3 * F + T
    rows, cols, vals, b_ub = [], [], [], []
    r = 0
    for ti, (trip, tp) in enumerate(zip(sc["triplets"], sc["triplet_pairs"])):
        i, j, k = (int(v) for v in trip)
        for (c1, c2), p in zip(((i, j), (j, k), (i, k)), tp):
            assert (sc["first"][p], sc["second"][p]) == (c1, c2)
            R21, t21 = sc["R_21"][p], sc["t_21"][p]
            for a in range(3):
                # e_a - gamma <= 0
                rows += [r] * 6; cols += [3 * c2 + a, 3 * c1, 3 * c1 + 1, 3 * c1 + 2, lam0 + ti, gam]; vals += [1.0, -R21[a, 0], -R21[a, 1], -R21[a, 2], -t21[a], -1.0]
                b_ub.append(0.0); r += 1
                # e_a + gamma >= 0, as -e_a - gamma <= 0
                rows += [r] * 6; cols += [3 * c2 + a, 3 * c1, 3 * c1 + 1, 3 * c1 + 2, lam0 + ti, gam]; vals += [-1.0, R21[a, 0], R21[a, 1], R21[a, 2], t21[a], -1.0]
                b_ub.append(0.0); r += 1
    A = sp.csr_matrix((vals, (rows, cols)), shape=(r, nv))
    bounds = [(None, None)] * nv
    for a in range(3):
        bounds[3 * sc["origin"] + a] = (0.0, 0.0)
    lo = lower_bounds(sc)
    for ti in range(T):
        bounds[lam0 + ti] = (float(lo[ti]), None)
    bounds[gam] = (0.0, None)
    cost = np.zeros(nv); cost[gam] = 1.0
    res = linprog(cost, A_ub=A, b_ub=np.asarray(b_ub), bounds=bounds, method="highs")
    return dict(gamma=float(res.x[gam]), t=res.x[:3 * F].reshape(F, 3), lam=res.x[lam0:gam], status=res.status)


# ---- the certificate -------------------------------------------------------------------------------------------------------------------------
def residuals(sc, t, lam):
    """e of every triplet's three pairs: T x 3 x 3"""
    tp = sc["triplet_pairs"]
    R = sc["R_21"][tp]; t21 = sc["t_21"][tp]
    a = t[sc["first"][tp]]; b = t[sc["second"][tp]]
    return b - np.einsum("tqij,tqj->tqi", R, a) - lam[:, None, None] * t21


def best_lambdas(sc, t):
    """Per triplet the lambda >= lo that minimises its max |e| at the translations t: the tightest primal certificate the translations admit.  (The ABI returns the
    translations, not the lambdas.)  max_c |v_c - lambda u_c| is convex and piecewise linear in lambda: its minimum over [lo, inf) is at lo or at a crossing of two
    of its lines."""
    tp = sc["triplet_pairs"]
    lo = lower_bounds(sc)
    v = residuals(sc, t, np.zeros(len(tp))).reshape(len(tp), 9); u = sc["t_21"][tp].reshape(len(tp), 9)
    out = np.zeros(len(tp))
    for k in range(len(tp)):
        lines = [(s * v[k, c], s * u[k, c]) for c in range(9) for s in (1.0, -1.0)]          # value = a - lambda b
        cand = [lo[k]]
        for x in range(len(lines)):
            for y in range(x + 1, len(lines)):
                d = lines[x][1] - lines[y][1]
                if d != 0.0:
                    c = (lines[x][0] - lines[y][0]) / d
                    if c > lo[k]:
                        cand.append(c)
        cand = np.asarray(cand)
        worst = np.max(np.abs(v[k][None, :] - cand[:, None] * u[k][None, :]), axis=1)
        out[k] = cand[int(np.argmin(worst))]
    return out


def certificate(sc, t, gamma, duals, lam=None):
    """What the stop rule promises, re-evaluated in numpy from what a call returns.  lam None: best_lambdas.  Returns dict(primal = max |e| - gamma, bound = max
    (lo - lambda), min_z, dual = |c + G^T z|_inf over the free unknowns, gap = s^T z, dual_objective = sum lo z_bound, pinned)."""
    T, F = len(sc["triplets"]), sc["F"]
    lo = lower_bounds(sc)
    lam = best_lambdas(sc, t) if lam is None else np.asarray(lam, np.float64)
    e = residuals(sc, t, lam)
    z = np.asarray(duals, np.float64).reshape(T, ROWS)
    zp, zm, zb = z[:, 0:18:2].reshape(T, 3, 3), z[:, 1:18:2].reshape(T, 3, 3), z[:, 18]
    d = zp - zm
    tp = sc["triplet_pairs"]
    g_t = np.zeros((F, 3))
    np.add.at(g_t, sc["second"][tp], d)
    np.add.at(g_t, sc["first"][tp], -np.einsum("tqij,tqi->tqj", sc["R_21"][tp], d))
    g_lam = -(d * sc["t_21"][tp]).sum(axis=(1, 2)) - zb
    g_gam = 1.0 - (zp + zm).sum()
    pinned = pinned_cameras(sc)
    free = np.ones(F, bool); free[pinned] = False
    used = np.zeros(F, bool); used[sc["triplets"].reshape(-1)] = True
    s = np.concatenate([(gamma - e).reshape(T, 9), (gamma + e).reshape(T, 9), (lam - lo)[:, None]], axis=1)
    zz = np.concatenate([zp.reshape(T, 9), zm.reshape(T, 9), zb[:, None]], axis=1)
    return dict(primal=float(np.abs(e).max() - gamma), bound=float((lo - lam).max()), min_z=float(z.min()),
                dual=float(max(np.abs(g_t[free & used]).max() if (free & used).any() else 0.0, np.abs(g_lam).max(), abs(g_gam))),
                gap=float((s * zz).sum()), dual_objective=float((lo * zb).sum()), pinned=pinned, fixed_zero=bool(np.all(t[~(free & used)] == 0.0)))


def check_certificate(sc, t, gamma, duals, lam=None):
    """assertion 1: every promise of the stop rule, re-evaluated in numpy, within twice its tolerance (the factor covers numpy's own rounding)"""
    c = certificate(sc, t, gamma, duals, lam)
    print("certificate", {k: v for k, v in c.items() if k != "pinned"})
    assert c["primal"] <= 2 * FEAS_TOL
    assert c["bound"] <= 2 * FEAS_TOL
    assert c["min_z"] >= -2 * FEAS_TOL
    assert c["dual"] <= 2 * FEAS_TOL
    assert c["gap"] <= 2 * GAP_TOL * max(1.0, abs(gamma))
    assert c["fixed_zero"]
    # weak duality: the dual objective bounds the optimum from below up to the dual residual, gamma from above
    assert gamma - c["dual_objective"] <= 2 * GAP_TOL * max(1.0, abs(gamma)) + 2 * FEAS_TOL * (1.0 + np.abs(t).sum())
    return c


def pinned_cameras(sc):
    """the gauge of the call: the origin for its own triplet component, the lowest-numbered camera of every other"""
    F = sc["F"]
    root = list(range(F))

    def find(c):
        while root[c] != c:
            c = root[c]
        return c
    for i, j, k in sc["triplets"]:
        for m in (j, k):
            a, b = find(int(i)), find(int(m))
            if a != b:
                root[max(a, b)] = min(a, b)
    used = set(int(c) for c in sc["triplets"].reshape(-1))
    comps = {}
    for c in sorted(used):
        comps.setdefault(find(c), []).append(c)
    return [sc["origin"] if sc["origin"] in cams else cams[0] for cams in comps.values()]


def n_components(sc):
    return len(pinned_cameras(sc))


def n_loose(sc):
    return sc["F"] - len(set(int(c) for c in sc["triplets"].reshape(-1)))


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------
_CHECK = []


def check_lib():
    if not _CHECK:
        from panovlm_amd import build
        _CHECK.append(C.CDLL(build.build_translp_check()))
    return _CHECK[0]


def host_group_size():
    return int(check_lib().chk_translp_group_size())


SUMMARY_KEYS = ("gamma", "dual_objective", "gap", "primal_residual", "dual_residual", "iterations", "bumps", "n_components", "n_loose", "termination")


def call_arrays(sc, mod=None):
    """the arrays of a call, contiguous, with the overrides of `mod`"""
    a = dict(F=sc["F"], first=tr._i32(sc["first"]), second=tr._i32(sc["second"]), R_21=tr._f64(sc["R_21"]), t_21=tr._f64(sc["t_21"]),
             triplet_pairs=tr._i32(sc["triplet_pairs"]), origin=sc["origin"], translations=np.zeros((sc["F"], 3)), max_iterations=MAX_ITERATIONS, gap_tol=GAP_TOL,
             feas_tol=FEAS_TOL)
    a.update(mod or {})
    return a


def host_l1(sc, mod=None):
    """the host compile's pvlm_transavg_l1: dict(rc, translations, duals, lam, gaps, the summary fields).  Outputs come back as they went in (-7 guard values in
    duals and lam) when the host compile wrote none."""
    a = call_arrays(sc, mod)
    P, T = len(a["first"]), len(a["triplet_pairs"])
    t = tr._f64(a["translations"]).copy(); duals = np.full((T, ROWS), -7.0); lam = np.full(T, -7.0); sm = np.full(10, -7.0); gaps = np.zeros(256); ng = C.c_int(0)
    rc = check_lib().chk_translp_l1(C.c_int(a["F"]), C.c_int(P), tr._p(a["first"]), tr._p(a["second"]), tr._p(a["R_21"]), tr._p(a["t_21"]), C.c_int(T), tr._p(a["triplet_pairs"]),
                                    C.c_int(a["origin"]), tr._p(t), tr._p(duals), tr._p(lam), C.c_int(a["max_iterations"]), C.c_double(a["gap_tol"]), C.c_double(a["feas_tol"]),
                                    tr._p(sm), tr._p(gaps), C.c_int(len(gaps)), C.byref(ng))
    out = dict(rc=int(rc), translations=t, duals=duals, lam=lam, gaps=gaps[:ng.value].copy())
    for k, v in zip(SUMMARY_KEYS, sm):
        out[k] = float(v) if k in SUMMARY_KEYS[:5] else int(v)
    return out


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------
def with_triplets(sc):
    sc["triplets"], sc["triplet_pairs"] = find_triplets(sc["first"], sc["second"])
    return sc


def fan_pairs(degree):
    """hub camera 0 and a rim 1 .. degree + 1: the hub lies in exactly `degree` triplets (0, k, k + 1)"""
    return [(0, k) for k in range(1, degree + 2)] + [(k, k + 1) for k in range(1, degree + 1)]


def book_pairs(pages):
    """the pair (0, 1) and `pages` further cameras tied to both: it lies in `pages` triplets"""
    return [(0, 1)] + [(0, c) for c in range(2, pages + 2)] + [(1, c) for c in range(2, pages + 2)]


K4 = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]

# name -> (pairs, cameras, keyword arguments of transavg_ref.scene).  `unit`: every t_21 normalised (unscaled = 1).  Seeds replaced at authoring time because the scene
# failed the admission rule (admitted(), below) are listed in SEEDS.
SCENE_LIST = {
    "one-triplet": ([(0, 1), (1, 2), (0, 2)], 3, dict(noise_deg=2.0)),
    "K4": (K4, 4, dict(noise_deg=2.0)),
    "K4-unit": (K4, 4, dict(noise_deg=2.0, unscaled=1.0)),
    "loose": (K4 + [(3, 4)], 6, dict(noise_deg=2.0)),                                             # (3, 4) in no triplet; cameras 4 and 5 in none
    "two-components": (K4 + [(a + 4, b + 4) for a, b in K4] + [(3, 4)], 8, dict(noise_deg=3.0)),      # joined by (3, 4) alone: a second pinned camera
    "hub-G-1": (fan_pairs(G - 1), G + 1, dict(noise_deg=1.0)),
    "hub-G": (fan_pairs(G), G + 2, dict(noise_deg=1.0)),
    "hub-G+1": (fan_pairs(G + 1), G + 3, dict(noise_deg=1.0)),
    "hub-3G": (fan_pairs(3 * G), 3 * G + 2, dict(noise_deg=1.0)),
    "book": (book_pairs(G + 3), G + 5, dict(noise_deg=1.0)),                                      # the pair (0, 1) in G + 3 triplets
    "metric": (tr.chain_pairs(14, 3), 14, dict(noise_deg=1.0, size=8.0)),                         # t_21 of several metres: lambda bounds active (lambda - lo down to 1e-13)
    "unit": (tr.chain_pairs(14, 3), 14, dict(noise_deg=1.0, unscaled=1.0)),
    "exact-small": (tr.chain_pairs(10, 3), 10, dict(size=0.8)),                                   # noise-free, baselines below a metre: gamma* = 0, no bound active
    "outliers": (tr.chain_pairs(24, 4), 24, dict(noise_deg=1.0, outliers=0.1)),
    "origin-5": (tr.chain_pairs(16, 3), 16, dict(noise_deg=1.0, origin=5)),
    "F40": (tr.chain_pairs(40, 5), 40, dict(noise_deg=1.0, outliers=0.05)),
}
SEEDS = {'K4': 4800, 'book': 4800, 'origin-5': 4800, 'exact-small': 4801}
ZERO_GAMMA = ("exact-small",)      # gamma* = 0: compared with HiGHS by |gamma| alone (there is no relative error of zero)
_SCENES = {}
_REF = {}
_HOST = {}


def build_scene(name):
    pairs, F, kw = SCENE_LIST[name]
    seed = SEEDS.get(name, 4700 + list(SCENE_LIST).index(name))
    return with_triplets(tr.scene(seed, sorted(pairs), F, **kw))


def scenes():
    if not _SCENES:
        for name in SCENE_LIST:
            _SCENES[name] = build_scene(name)
    return _SCENES


def reference(name):
    """HiGHS on the literal programme, computed once"""
    if name not in _REF:
        _REF[name] = lp_ref(scenes()[name])
    return _REF[name]


def host(name):
    """the host compile on the scene, computed once; callers do not modify it"""
    if name not in _HOST:
        _HOST[name] = host_l1(scenes()[name])
    return _HOST[name]


def admitted(h):
    """no knife-edge stop: the last gap is below half its tolerance and the one before it above twice the tolerance, so a device whose sums differ in the last bits
    stops at the same iteration"""
    tol = GAP_TOL * max(1.0, abs(h["gamma"]))
    return h["termination"] == 0 and len(h["gaps"]) >= 2 and h["gaps"][-1] < 0.5 * tol and h["gaps"][-2] > 2.0 * tol


# the largest |gamma_host - gamma_HiGHS| / gamma_HiGHS over the scenes (tests/test_translp_cpu.py::test_measured_is_the_maximum); the tolerance of the device
# against the host compile is ten times that: the device's sums run in another order
MEASURED = dict(gamma=2.1e-10)
TOL = {k: 10 * v for k, v in MEASURED.items()}


# ---- refused calls ---------------------------------------------------------------------------------------------------------------------------
def bad_calls(sc):
    """(what, overrides of call_arrays) of every PVLM_ERR_ARG case the header lists (the NULLs are the GPU test's own)"""
    P = sc["P"]
    out = []

    def arr(key, at, value):
        a = np.array(sc[key], copy=True); a[at] = value
        return {key: a}
    out.append(("camera index out of range", arr("second", 0, sc["F"])))
    out.append(("negative camera index", arr("first", 0, -1)))
    out.append(("first >= second", dict(first=tr._i32(sc["second"]), second=tr._i32(sc["first"]))))
    out.append(("first == second", arr("first", 0, int(sc["second"][0]))))
    rep = dict(first=np.append(sc["first"], sc["first"][0]), second=np.append(sc["second"], sc["second"][0]), R_21=np.concatenate([sc["R_21"], sc["R_21"][:1]]),
               t_21=np.concatenate([sc["t_21"], sc["t_21"][:1]]))
    out.append(("repeated pair", rep))
    out.append(("triplet pair index out of range", arr("triplet_pairs", (0, 0), P)))
    out.append(("triplet pairs in another order", dict(triplet_pairs=sc["triplet_pairs"][:, [1, 0, 2]])))
    out.append(("triplet of pairs that share no camera", arr("triplet_pairs", (0, 2), int(sc["triplet_pairs"][-1, 1]))))
    out.append(("R_21 not finite", arr("R_21", (0, 1, 1), np.nan)))
    out.append(("t_21 not finite", arr("t_21", (P - 1, 2), np.inf)))
    t = np.zeros((sc["F"], 3)); t[(sc["origin"] + 1) % sc["F"], 0] = np.nan
    out.append(("translation not finite", dict(translations=t)))
    t = np.zeros((sc["F"], 3)); t[sc["origin"], 2] = 1e-300
    out.append(("origin's translation not zero", dict(translations=t)))
    out.append(("origin out of range", dict(origin=sc["F"])))
    out.append(("origin negative", dict(origin=-1)))
    out.append(("max_iterations < 1", dict(max_iterations=0)))
    out.append(("gap tolerance zero", dict(gap_tol=0.0)))
    out.append(("feasibility tolerance negative", dict(feas_tol=-1e-9)))
    out.append(("tolerance not a number", dict(gap_tol=np.nan)))
    return out


# ---- the host mirror -------------------------------------------------------------------------------------------------------------------------
def run_driver(g, mode, route, enable=1, seed=1):
    """tests/cpp/pvlm_translp_driver.cpp on the graph g (the format of transavg_ref.run_driver).  mode "estimate": EstimateGlobalTranslation with method 2 and
    enable_l1 = `enable` -> dict(ok, message, valid, t_wc, R_wc, pairs); "l1": TranslationAveragingL1 by hand on the frames as cameras -> dict(ok, t)."""
    import os
    import subprocess
    import tempfile
    from panovlm_amd import build
    if not os.path.exists(build.TRANSLP_DRIVER):
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
        res = subprocess.run([build.TRANSLP_DRIVER, mode, route, path, str(enable), str(seed)], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(path)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    out = dict(ok=None, message="", valid={}, t_wc={}, R_wc={}, pairs=[], t={}, t_cw={})
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
        elif w[0] == "t":
            out["t"][int(w[1])] = np.array([float(x) for x in w[2:]])
    return out


def scene_graph(sc, duplicate=None):
    """a scene as a graph of the driver: the frames are the cameras.  duplicate: (pair, factor) puts a copy of that pair with its t_21 scaled by factor FIRST in the
    list, so that the map of :289 resolves the pair to its later, true copy"""
    pairs = [dict(first=int(sc["first"][p]), second=int(sc["second"][p]), R_21=sc["R_21"][p], t_21=sc["t_21"][p], upper=0.0, lower=0.0) for p in range(sc["P"])]
    if duplicate is not None:
        p, factor = duplicate
        pairs.insert(0, dict(pairs[p], t_21=pairs[p]["t_21"] * factor))
    return dict(F=sc["F"], R_wc=np.array([r.T for r in sc["R_cw"]]), t_wc=np.full((sc["F"], 3), np.inf), pairs=pairs)


def estimate_problem(g, out):
    """What EstimateGlobalTranslation's method 2 solved on the graph g, rebuilt from what the driver printed: the surviving pairs over the valid frames, re-indexed in
    ascending order, and the translations t_cw = -R_wc^T t_wc it left.  The rows of the programme do not change when every camera moves by R_cw c (the rotations of
    the graph are exact), so the origin the mirror chose does not matter to max |e|.  Returns (scene, t_cw)."""
    frames = sorted(i for i, v in out["valid"].items() if v)
    new = {f: k for k, f in enumerate(frames)}
    by_key = {(p["first"], p["second"]): p for p in g["pairs"]}
    keys = sorted(k for k in set(out["pairs"]) if k[0] in new and k[1] in new)
    sc = dict(F=len(frames), P=len(keys), first=np.array([new[a] for a, _ in keys], np.int32), second=np.array([new[b] for _, b in keys], np.int32),
              R_21=np.array([np.asarray(by_key[k]["R_21"]).reshape(3, 3) for k in keys]), t_21=np.array([by_key[k]["t_21"] for k in keys]), origin=0)
    t = np.array([-out["R_wc"][f].T @ out["t_wc"][f] for f in frames])
    return with_triplets(sc), t


def primal_gamma(sc, t):
    """the smallest gamma the translations t are feasible for: max |e| at each triplet's best lambda >= lo"""
    return float(np.abs(residuals(sc, t, best_lambdas(sc, t))).max())
