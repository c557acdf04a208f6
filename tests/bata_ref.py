"""K44 test helpers: synthetic camera graphs with known centres, an INDEPENDENT numpy float64 reference of BATA (sfm/BATA.cpp:36-237) that shares no formula text with
panovlm_amd/csrc/pvlm_bata_core.h — the LUD stage forms the full (3 F + 4) KKT matrix densely, as upstream writes it, and calls numpy.linalg.solve; the IRLS stage
forms A densely and solves its normal equations — the knife-edge condition every scene of the K44 tests is held to, and the ctypes wrappers of the host compile of the
core (tests/cpp/bata_core_check.cpp, built by panovlm_amd.build.build_bata_check)."""
import ctypes as C

import numpy as np

from tests import transavg_ref as tr

DEFAULTS = dict(delta=1e-6, init_iteration=10, inner_iteration=10, outer_iteration=10, robust_threshold=0.1)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def scene(seed, pairs, n_cameras, noise_deg=0.0, outliers=0.0, reverse=0.5, unscaled=0.0, size=8.0, id0=0):
    """Cameras with centres uniform in a cube of `size` metres.  Pair (i, j): the unit direction of centre[i] - centre[j] (At0 has +I at first, -I at second) turned
    by noise_deg about a random axis; `outliers`: this fraction of the pairs is wrong — the share `reverse` of them points the opposite way (their bilinear scale turns
    negative and the row drops out, BATA.cpp:156), the rest in a random direction.  `unscaled`: this fraction comes without a length and starts from a positive draw (the
    caller's part of BATA.cpp:64-68), the others from the true length.  id0: the smallest camera id."""
    rng = np.random.default_rng(seed)
    F = n_cameras; pairs = np.asarray(pairs, np.int32).reshape(-1, 2); P = len(pairs)
    Cw = rng.uniform(-size / 2, size / 2, (F, 3))
    d = np.zeros((P, 3)); s0 = np.zeros(P)
    bad = rng.permutation(P)[:int(round(outliers * P))] if outliers > 0 else np.zeros(0, int)
    rev = set(bad[:int(round(reverse * len(bad)))].tolist())
    free = set(rng.permutation(P)[:int(round(unscaled * P))].tolist()) if unscaled > 0 else set()
    for p, (i, j) in enumerate(pairs):
        v = Cw[i] - Cw[j]; n = np.linalg.norm(v); v = v / n
        if noise_deg > 0:
            a = np.cross(v, rng.normal(size=3)); a /= np.linalg.norm(a)
            v = tr.rodrigues(np.radians(noise_deg) * rng.normal() * a) @ v
        if p in rev:
            v = -v
        elif p in set(bad.tolist()):
            v = rng.normal(size=3)
        d[p] = v / np.linalg.norm(v)
        s0[p] = rng.uniform(0.05, 1.0) if p in free else n
    return dict(F=F, P=P, n_cameras=F + id0, first=(pairs[:, 0] + id0).astype(np.int32), second=(pairs[:, 1] + id0).astype(np.int32), dir=d, s0=s0, centres=Cw,
                bad=np.sort(bad), size=size)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def bata_ref(sc, delta=1e-6, init_iteration=10, inner_iteration=10, outer_iteration=10, robust_threshold=0.1):
    """BATA as sfm/BATA.cpp writes it, dense.  Returns dict(centres, lud_centres (F x 3, camera 0 zero), scales (P, the S of the last pass), wvec (one array per
    outer), knife (everything that came within margin of a decision))."""
    first = sc["first"].astype(int); second = sc["second"].astype(int); P = sc["P"]
    lo = min(first.min(), second.min()); F = max(first.max(), second.max()) - lo + 1
    first = first - lo; second = second - lo
    tij = sc["dir"]; flat = tij.reshape(-1)
    knife = []
    At0 = np.zeros((3 * P, 3 * F))
    for k in range(P):
        At0[3 * k:3 * k + 3, 3 * first[k]:3 * first[k] + 3] = np.eye(3)
        At0[3 * k:3 * k + 3, 3 * second[k]:3 * second[k] + 3] = -np.eye(3)
    inc = np.zeros((P, F)); inc[np.arange(P), first] = 1; inc[np.arange(P), second] = 1

    def starved(weights, where):
        per_cam = inc.T @ weights
        if per_cam.min() < 1e-9 * per_cam.max():
            knife.append("%s: camera %d is left with weight %.3e of %.3e" % (where, int(per_cam.argmin()), per_cam.min(), per_cam.max()))
    # LUDRevised
    Aeq1 = np.zeros((P, 3 * P))
    for k in range(P):
        Aeq1[k, 3 * k:3 * k + 3] = tij[k]
    Aeq = np.zeros((4, 3 * F)); Aeq[0] = (Aeq1 @ At0).sum(axis=0)
    for k in range(3 * F):
        Aeq[k % 3 + 1, k] = 1
    beq = np.zeros(4); beq[0] = P
    Svec = sc["s0"] * (P / sc["s0"].sum())
    W = np.sqrt(np.ones(3 * P))
    for it in range(init_iteration):
        A = W[:, None] * At0
        B = W * np.repeat(Svec, 3) * flat
        K = np.zeros((3 * F + 4, 3 * F + 4)); K[:3 * F, :3 * F] = 2 * A.T @ A; K[:3 * F, 3 * F:] = Aeq.T; K[3 * F:, :3 * F] = Aeq
        X = np.linalg.solve(K, np.concatenate([2 * A.T @ B, beq]))
        t = X[:3 * F]
        Aij = (At0 @ t).reshape(P, 3)
        Svec = (Aij * tij).sum(axis=1) / (tij ** 2).sum(axis=1)
        res = Aij - Svec[:, None] * tij
        Wvec = ((res ** 2).sum(axis=1) + delta) ** -0.5
        starved(Wvec, "LUD %d" % it)
        W = np.sqrt(np.repeat(Wvec, 3))
    pose = t.reshape(F, 3) - t[:3]
    lud = pose.copy()
    # IRLS
    A0 = At0[:, 3:]
    t = pose[1:].reshape(-1)
    wvecs = []
    for o in range(outer_iteration - 1):
        with np.errstate(divide="ignore"):
            A = (1.0 / np.repeat(Svec, 3))[:, None] * A0
        e = np.sqrt((((A @ t - flat).reshape(P, 3)) ** 2).sum(axis=1))
        near = np.abs(e - robust_threshold) <= 1e-9 * robust_threshold
        if near.any():
            knife.append("outer %d: pair %d has e = %.17g at the threshold" % (o, int(np.argmax(near)), e[np.argmax(near)]))
        Wvec = np.zeros(P); Wvec[e < robust_threshold] = 1.0
        big = e > robust_threshold; Wvec[big] = robust_threshold / e[big]
        wvecs.append(Wvec.copy())
        W = np.sqrt(np.repeat(Wvec, 3))
        for j in range(inner_iteration):
            Aij = (A0 @ t).reshape(P, 3)
            n2 = (Aij ** 2).sum(axis=1); dot = (Aij * tij).sum(axis=1)
            cos = dot / np.sqrt(n2)
            if (np.abs(cos) < 1e-6).any():
                knife.append("outer %d inner %d: pair %d has cos = %.3e" % (o, j, int(np.argmin(np.abs(cos))), cos[np.argmin(np.abs(cos))]))
            Svec = n2 / dot
            Svec[Svec < 0] = np.inf
            S3 = np.repeat(Svec, 3)
            starved(Wvec / Svec ** 2, "outer %d inner %d" % (o, j))
            A = (W / S3)[:, None] * A0
            B = W * flat
            t = np.linalg.solve(A.T @ A, A.T @ B)
    centres = np.vstack([np.zeros(3), t.reshape(F - 1, 3)])
    return dict(centres=centres, lud_centres=lud, scales=Svec, wvec=wvecs, knife=knife)


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------
_CHECK = []


def check_lib():
    if not _CHECK:
        from panovlm_amd import build
        _CHECK.append(C.CDLL(build.build_bata_check()))
    return _CHECK[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_group_size():
    return int(check_lib().chk_bata_group_size())


def host_solve(sc, n_cameras=None, delta=1e-6, init_iteration=10, inner_iteration=10, outer_iteration=10, robust_threshold=0.1):
    """the host compile's BATA: dict(rc, info, centres, lud_centres (F x 3), scales, untouched)"""
    first = np.ascontiguousarray(sc["first"], np.int32); second = np.ascontiguousarray(sc["second"], np.int32)
    d = np.ascontiguousarray(sc["dir"], np.float64); s0 = np.ascontiguousarray(sc["s0"], np.float64)
    P = len(first); F = sc["F"]; n = sc["n_cameras"] if n_cameras is None else n_cameras
    cen = np.full((max(n, F), 3), -7.0); lud = np.full((max(n, F), 3), -7.0); s = np.full(P, -7.0); info = C.c_int(-7)
    rc = check_lib().chk_bata_solve(C.c_int(n), C.c_int(P), _p(first), _p(second), _p(d), _p(s0), C.c_double(delta), C.c_int(init_iteration), C.c_int(inner_iteration),
                                    C.c_int(outer_iteration), C.c_double(robust_threshold), _p(cen), _p(lud), _p(s), C.byref(info))
    untouched = bool(np.all(cen == -7.0) and np.all(lud == -7.0) and np.all(s == -7.0))
    return dict(rc=int(rc), info=info.value, centres=cen[:F], lud_centres=lud[:F], scales=s, untouched=untouched)


# ---- the scenes of the K44 tests: every one is held to the knife-edge condition by tests/test_bata_cpu.py -------------------------------------------------------
G = 8   # pvlm_bata_group_size(); tests assert it


def build_scenes():
    """name -> (scene, keyword arguments of the solve).  Seeds replaced because the scene failed the knife-edge condition are listed in SEEDS."""
    S = {}

    def add(name, sc, **kw):
        S[name] = (sc, kw)
    sd = lambda name, default: SEEDS.get(name, default)
    # pairs: a triangle, both sides of a wave, 256 + 1 (past one trip of a per-pair kernel whose grid is held to one workgroup of 256); unsorted, some first > second
    add("P3", scene(sd("P3", 3), [(0, 1), (2, 1), (0, 2)], 3, noise_deg=1.0))
    for P in (63, 64, 65, 257):
        F = 90 if P == 257 else 22
        name = "P%d" % P
        add(name, scene(sd(name, 100 + P), tr.pairs_exactly(F, P, P), F, unscaled=0.3, noise_deg=1.0, outliers=0.1))
    # cameras: both sides of a wave (the triangle is P3); every camera with its next 3, shuffled
    for F in (64, 65):
        name = "F%d" % F
        add(name, scene(sd(name, 300 + F), tr.pairs_exactly(F, len(tr.chain_pairs(F, 3)), F), F, unscaled=0.3, noise_deg=1.0, outliers=0.1))
    # a hub camera of degree G - 1, G, G + 1, 2 G + 1
    for deg in (G - 1, G, G + 1, 2 * G + 1):
        name = "hub%d" % deg
        add(name, scene(sd(name, 200 + deg), tr.hub_pairs(24, deg, 11), 24, unscaled=0.3, noise_deg=1.0))
    # ids that start at 2, one repeated pair, all-scaled / all-unscaled / mixed
    add("id2", scene(sd("id2", 30), tr.pairs_exactly(14, 36, 14), 14, unscaled=0.3, noise_deg=1.0, id0=2))
    add("repeat", scene(sd("repeat", 31), tr.chain_pairs(12, 3) + [(2, 4)], 12, unscaled=0.3, noise_deg=1.0, outliers=0.1))
    add("scaled", scene(sd("scaled", 32), tr.chain_pairs(16, 3), 16, noise_deg=1.0, outliers=0.1))
    add("unscaled", scene(sd("unscaled", 33), tr.chain_pairs(16, 3), 16, unscaled=1.0, noise_deg=1.0))
    add("mixed", scene(sd("mixed", 34), tr.chain_pairs(16, 3), 16, unscaled=0.5, noise_deg=1.0))
    # noise-free: the truth up to a common factor; about 10 % gross outliers, half of them reversed
    add("exact", scene(sd("exact", 37), tr.chain_pairs(12, 3), 12))
    add("outlier", scene(sd("outlier", 38), tr.chain_pairs(40, 4), 40, noise_deg=0.5, outliers=0.1))
    # a short call: two LUD passes, one outer of three inners
    add("short", scene(sd("short", 39), tr.chain_pairs(10, 3), 10, noise_deg=1.0, unscaled=0.3), init_iteration=2, inner_iteration=3, outer_iteration=2)
    return S


# seeds replaced on the CPU because the scene failed the knife-edge condition (tests/test_bata_cpu.py::test_knife_edge names the scene and the reason)
SEEDS = {}
_SCENES = {}
_REF = {}


def scenes():
    if not _SCENES:
        _SCENES.update(build_scenes())
    return _SCENES


def reference(name):
    """bata_ref of a scene, computed once and shared by the tests"""
    if name not in _REF:
        sc, kw = scenes()[name]
        _REF[name] = bata_ref(sc, **kw)
    return _REF[name]


def disconnected():
    """two chains of 6 cameras with nothing between them"""
    pairs = tr.chain_pairs(6, 2) + [(i + 6, j + 6) for i, j in tr.chain_pairs(6, 2)]
    return scene(40, pairs, 12, noise_deg=1.0)


def align(centres, truth):
    """the truth in the gauge of `centres`: camera 0 at zero, one common factor (least squares); returns (factor, truth * factor)"""
    rel = truth - truth[0]
    f = float((centres * rel).sum() / (rel * rel).sum())
    return f, f * rel


# ---- tolerances ------------------------------------------------------------------------------------------------------------------------------
# The largest difference of the host compile against bata_ref over scenes() (tests/test_bata_cpu.py::test_measured_is_the_maximum prints and bounds them): centres and
# LUD centres in the solver's own unit (the mean start scale is 1, so pair lengths are of order 1), scales relative to max(1, |scale|) (a pair almost across its
# direction has a scale of |d| / cos).  With every decision held off its threshold only rounding separates the two — a KKT solve by LU against two Cholesky solves in
# the LUD stage, 90 re-weighted solves whose weights 1 / S^2 carry the rounding of the previous one in the IRLS stage; the tolerance of the K44 tests is ten times that.
MEASURED = dict(centres=8.7e-13, lud=3.5e-13, scales=4.5e-13)
TOL = {k: 10 * v for k, v in MEASURED.items()}
# what bata_ref itself reaches: the distance of its centres from the aligned truth on the noise-free scene `exact`, and the largest distance of a camera none of
# whose pairs is an outlier on the scene `outlier` (both in the solver's unit); the tests allow the host compile ten times these
REF_EXACT = 3.2e-15        # rounding alone: the noise-free scene is a fixed point of both stages
REF_OUTLIER = 6.5e-2       # 0.5 degrees of direction noise on pairs about one unit long, through chains of up to 39 cameras


def differences(a, b):
    """a against b (the reference side): centres, lud, scales; the scales must be infinite in the same places"""
    sa, sb = np.asarray(a["scales"]), np.asarray(b["scales"])
    fin = np.isfinite(sb)
    same_inf = bool(np.array_equal(np.isfinite(sa), fin) and np.array_equal(sa[~fin], sb[~fin]))
    ds = float((np.abs(sa[fin] - sb[fin]) / np.maximum(1.0, np.abs(sb[fin]))).max()) if same_inf and fin.any() else (0.0 if same_inf else np.inf)
    return dict(centres=float(np.abs(a["centres"] - b["centres"]).max()), lud=float(np.abs(a["lud_centres"] - b["lud_centres"]).max()), scales=ds)


def bad_calls(sc):
    """(name, call) for every argument the entry point refuses; the call is the scene with one thing wrong (and maybe keyword arguments under "kw")"""
    def mod(**kw):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
        c.update(kw)
        return c
    out = []
    first = sc["first"].copy(); first[1] = sc["n_cameras"]
    out.append(("camera index out of range", mod(first=first)))
    first = sc["first"].copy(); first[1] = -1
    out.append(("negative camera index", mod(first=first)))
    out.append(("first == second", mod(second=np.where(np.arange(sc["P"]) == 0, sc["first"], sc["second"]).astype(np.int32))))
    d = sc["dir"].copy(); d[1, 2] = np.nan
    out.append(("direction not finite", mod(dir=d)))
    d = sc["dir"].copy(); d[2] *= 1.0 + 1e-8
    out.append(("direction not of unit length", mod(dir=d)))
    d = sc["dir"].copy(); d[0] = 0.0
    out.append(("direction of zero length", mod(dir=d)))
    s = sc["s0"].copy(); s[0] = np.inf
    out.append(("scale not finite", mod(s0=s)))
    s = sc["s0"].copy(); s[1] = 0.0
    out.append(("scale zero", mod(s0=s)))
    s = sc["s0"].copy(); s[2] = -1.0
    out.append(("scale negative", mod(s0=s)))
    out.append(("init_iteration < 1", mod(kw=dict(init_iteration=0))))
    out.append(("inner_iteration < 1", mod(kw=dict(inner_iteration=0))))
    out.append(("outer_iteration < 1", mod(kw=dict(outer_iteration=0))))
    out.append(("n_cameras < 2", mod(n_cameras=1)))
    return out


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------------------
def mirror_graph(seed=5, F=9, size=8.0, unscaled=((2, 4), (3, 5), (6, 8))):
    """F frames with rotations, every frame with its next 3 (edge-biconnected); the pairs in `unscaled` carry a t_21 of unit length (BATA.cpp:192 then draws their start
    scale).  No frame has a translation yet (inf).  Noise-free.  The graph format of transavg_ref.run_driver."""
    rng = np.random.default_rng(seed)
    Rc = np.array([tr.rodrigues(rng.normal(size=3) * 0.6) for _ in range(F)])
    Cw = rng.uniform(-size / 2, size / 2, (F, 3))
    t = -np.einsum("cij,cj->ci", Rc, Cw)
    pairs = [tr._pair_of(Rc, t, i, i + k, scaled=(i, i + k) not in unscaled) for i in range(F) for k in (1, 2, 3) if i + k < F]
    for p in pairs:          # every pair keeps its place in the scaled / unscaled split of EstimateGlobalTranslation by its bounds; BATA looks at the length alone
        p["upper"] = p["lower"] = 0.0
    return dict(F=F, R_wc=np.array([Rc[i].T for i in range(F)]), t_wc=np.full((F, 3), np.inf), pairs=pairs, size=size, P=len(pairs))


def run_driver(g, mode, route, method=5, seed=1, use_all_pairs=1, init_dlt=0, enable_bata=1):
    """tests/cpp/pvlm_bata_driver.cpp on the graph g.  Returns dict(ok, message, valid, t_wc, R_wc, pairs) or, for bata, dict(ok, t, scale0)."""
    import os
    import subprocess
    import tempfile
    from panovlm_amd import build
    if not os.path.exists(build.BATA_DRIVER):
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
        args = [build.BATA_DRIVER, mode, route, path] + ([str(method), str(seed), str(use_all_pairs), str(init_dlt), str(enable_bata)] if mode == "estimate" else [str(seed)])
        res = subprocess.run(args, capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(path)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    out = dict(ok=None, message="", valid={}, t_wc={}, R_wc={}, pairs=[], t={}, scale0={})
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
            out["t"][int(w[1])] = np.array([float(x) for x in w[2:5]])
        elif w[0] == "scale0":
            out["scale0"][int(w[1])] = float(w[2])
    return out
