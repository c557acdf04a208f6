"""K45 test helpers: an INDEPENDENT numpy float64 restatement of RotationAveragingLeastSquare as upstream writes it (sfm/RotationAveraging.cpp:185-275) — the dense
A from the triplets, A^T A, numpy.linalg.eigh, a stable sort by |lambda|, numpy.linalg.svd per camera, the sign rule and the product with R_0^T — which shares no
code and no method with panovlm_amd/csrc/pvlm_rotstart_core.h (shift-and-invert subspace iteration); the scenes of the K45 tests; the ctypes wrapper of the host
compile of the core (tests/cpp/rotstart_core_check.cpp)."""
import ctypes as C

import numpy as np

from tests import rotavg_ref as rr

SHIFT_REL, TOL_REL, MAX_ITERATIONS = 1e-9, 1e-12, 100


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def dense_ata(sc):
    F, P = sc["F"], sc["P"]
    A = np.zeros((3 * P, 3 * F))
    for p in range(P):
        i, j = int(sc["first"][p]), int(sc["second"][p])
        A[3 * p:3 * p + 3, 3 * i:3 * i + 3] = -sc["R_21"][p]          # weight * (R_jw - R_ji R_iw) = 0 (:201-217)
        A[3 * p:3 * p + 3, 3 * j:3 * j + 3] = np.eye(3)
    return A.T @ A


def least_square_ref(sc):
    """dict(rotations (F x 3 x 3, R_cw with camera 0 the identity), eigenvalues: the six of smallest magnitude)"""
    F = sc["F"]
    lam, vec = np.linalg.eigh(dense_ata(sc))
    order = np.argsort(np.abs(lam), kind="stable")
    null = vec[:, order[:3]]
    rot = np.zeros((F, 3, 3))
    for c in range(F):
        U, _, Vt = np.linalg.svd(null[3 * c:3 * c + 3, :])
        R = U @ Vt
        rot[c] = -R if np.linalg.det(R) < 0 else R
    R0T = rot[0].T.copy()
    return dict(rotations=np.array([R @ R0T for R in rot]), eigenvalues=lam[order[:6]])


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------
_CHECK = []


def check_lib():
    if not _CHECK:
        from panovlm_amd import build
        _CHECK.append(C.CDLL(build.build_rotstart_check()))
    return _CHECK[0]


def host_least_square(sc, R0=None, shift_rel=SHIFT_REL, tol=TOL_REL, max_iterations=MAX_ITERATIONS, summary=True):
    """the host compile's pvlm_rotavg_least_square: dict(rc, rotations, iterations, solves, info, residual, theta); the summary arrays start at the sentinel -7"""
    first, second, R21 = rr._i32(sc["first"]), rr._i32(sc["second"]), rr._f64(sc["R_21"])
    R = rr._f64(sc["R0"] if R0 is None else R0).copy(); sm = np.full(3, -7, np.int32); val = np.full(4, -7.0)
    rc = check_lib().chk_rotstart_solve(C.c_int(sc["F"]), C.c_int(sc["P"]), rr._p(first), rr._p(second), rr._p(R21), rr._p(R), C.c_double(shift_rel), C.c_double(tol),
                                        C.c_int(max_iterations), rr._p(sm) if summary else None, rr._p(val))
    return dict(rc=int(rc), rotations=R.reshape(-1, 3, 3), iterations=int(sm[0]), solves=int(sm[1]), info=int(sm[2]), residual=float(val[0]), theta=val[1:].copy())


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------
def band_pairs(F, reach=3):
    return rr.chain_pairs(F, reach)


def random_pairs(F, seed):
    """a chain (so the graph is connected) plus random pairs up to 4 F in all"""
    rng = np.random.default_rng(seed)
    pairs = rr.chain_pairs(F, 1); have = set(pairs)
    most = min(4 * F, F * (F - 1) // 2)
    while len(pairs) < most:
        i, j = sorted(int(v) for v in rng.integers(0, F, 2))
        if i != j and (i, j) not in have:
            pairs.append((i, j)); have.add((i, j))
    return pairs


def flipped(sc, seed):
    """the pair list shuffled, half the pairs turned to first > second with R_21^T"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(sc["P"]); turn = rng.permutation(sc["P"]) < sc["P"] // 2
    first = np.where(turn, sc["second"][order], sc["first"][order]).astype(np.int32); second = np.where(turn, sc["first"][order], sc["second"][order]).astype(np.int32)
    R21 = np.array([sc["R_21"][p].T if t else sc["R_21"][p] for p, t in zip(order, turn)])
    return dict(sc, first=first, second=second, R_21=R21, R0=rr.spanning_tree_start(sc["F"], first, second, R21, 0))


def build_scenes():
    """name -> scene (rotavg_ref.scene: noise of 1 degree per pair unless it says otherwise, the spanning-tree start from camera 0).  F = 2: 3 F = 6 barely exceeds the
    width; the hub's row passes the 8 lanes of a gather group many times over; chain40 is a tree (exact zeros); band200 has the smallest gap; rand300 sends the
    camera tree past one 256-leaf chunk."""
    S = {}
    S["F2"] = rr.scene(452, [(0, 1)], 2)
    S["chain3"] = rr.scene(453, rr.chain_pairs(3, 1), 3)
    S["band5"] = rr.scene(455, band_pairs(5), 5)
    S["rand12"] = rr.scene(4512, random_pairs(12, 12), 12)
    S["hub64"] = rr.scene(4564, rr.hub_pairs(64, 63, 31), 64)
    S["chain40"] = rr.scene(4540, rr.chain_pairs(40, 1), 40)
    S["band200"] = rr.scene(45200, band_pairs(200), 200)
    S["rand300"] = rr.scene(45300, random_pairs(300, 300), 300)
    S["exact"] = rr.scene(4537, random_pairs(12, 37), 12, noise_deg=0.0)
    S["flipped"] = flipped(rr.scene(4541, band_pairs(40), 40), 41)
    return S


_SCENES = {}
_REF = {}
_HOST = {}


def scenes():
    if not _SCENES:
        _SCENES.update(build_scenes())
    return _SCENES


def reference(name):
    """least_square_ref of a scene, computed once and shared by the tests"""
    if name not in _REF:
        _REF[name] = least_square_ref(scenes()[name])
    return _REF[name]


def host(name):
    """the host compile's result on a scene from its spanning-tree start under the default parameters, computed once and shared by the tests"""
    if name not in _HOST:
        _HOST[name] = host_least_square(scenes()[name])
    return _HOST[name]


IMPROPER_Q = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) @ rr.exp_so3([0.3, -0.5, 0.2])      # orthogonal, determinant -1

# ---- the tolerance ---------------------------------------------------------------------------------------------------------------------------
# MEASURED: the largest rotation angle (radians) between the host compile and least_square_ref over scenes() (tests/test_rotstart_cpu.py::
# test_measured_is_the_maximum prints and bounds it).  The largest is band200, the scene of the smallest gap (lambda_2 = 4.5e-4, lambda_3 = 3.8e-3): the iteration
# stops at a residual of 2.0e-13 d_max = 1.2e-12, and a residual r leaves an angle of up to r / (lambda_3 - lambda_2) to the subspace, 3.6e-10 there.  So the
# figure is what the stopping rule tol = 1e-12 admits, not rounding: rand300 shows 8.7e-12, hub64 1.3e-12, the scenes that stop at 1e-16 show 1e-15.  The tolerance
# of the K45 tests is ten times MEASURED, the margin K40 and K44 use.
MEASURED = 2.7e-10
TOL = 10 * MEASURED


def run_driver(g, mode, route="host", *args):
    """tests/cpp/pvlm_rotstart_driver.cpp on the graph g (the dict of rotavg_ref.mirror_scene).  Returns dict(ok, message, translation_ok, translation_message, valid,
    t_wc, R_wc, pairs [(first, second)], R_21, rotations)."""
    import os
    import subprocess
    import tempfile
    from panovlm_amd import build
    if not os.path.exists(build.ROTSTART_DRIVER):
        build.build_host()
    lines = [str(g["F"])]
    for i in range(g["F"]):
        lines.append(" ".join([str(i)] + [rr._num(v) for v in np.asarray(g["R_wc"][i]).reshape(-1)] + [rr._num(v) for v in g["t_wc"][i]]))
    lines.append(str(len(g["pairs"])))
    for p in g["pairs"]:
        lines.append(" ".join([str(p["first"]), str(p["second"])] + [rr._num(v) for v in np.asarray(p["R_21"]).reshape(-1)] + [rr._num(v) for v in p["t_21"]] +
                              [rr._num(p["upper"]), rr._num(p["lower"])]))
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
        path = f.name
    try:
        res = subprocess.run([build.ROTSTART_DRIVER, mode, route, path] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(path)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    out = dict(ok=None, message="", translation_ok=None, translation_message="", valid={}, t_wc={}, R_wc={}, pairs=[], R_21=[], rotations={})
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
        elif w[0] == "rotation":
            out["rotations"][int(w[1])] = np.array([float(x) for x in w[2:]]).reshape(3, 3)
    return out


def bad_calls(sc):
    """(name, scene, params) for every argument the entry points refuse: rotavg_ref.bad_calls without those of start_idx, which this entry point does not have, plus
    the counts and the parameters"""
    out = [(n, c, {}) for n, c in rr.bad_calls(sc) if "start" not in n]
    one = dict(sc, F=1, P=0, first=sc["first"][:0], second=sc["second"][:0], R_21=sc["R_21"][:0], R0=sc["R0"][:1])
    out.append(("fewer than two cameras", one, {}))
    out.append(("no pair", dict(sc, P=0, first=sc["first"][:0], second=sc["second"][:0], R_21=sc["R_21"][:0]), {}))
    out.append(("shift_rel zero", sc, dict(shift_rel=0.0)))
    out.append(("shift_rel negative", sc, dict(shift_rel=-1e-9)))
    out.append(("tol zero", sc, dict(tol=0.0)))
    out.append(("tol not a number", sc, dict(tol=float("nan"))))
    out.append(("max_iterations zero", sc, dict(max_iterations=0)))
    return out
