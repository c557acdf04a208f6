"""Scenes, references and the host compile of K48 (pvlm_triplets_find / pvlm_triplets_filter) for tests/test_triplet_cpu.py and tests/test_triplet_gpu.py.
The references are tests/rotavg_ref.py's find_triplet_ref and triplet_angle_deg (what filter_by_triplet_ref does before its biconnected step); the admission checks
at the foot run when the module loads."""
import ctypes as C

import numpy as np

from tests import rotavg_ref as rr

BAND = 1e-12          # csrc/pvlm_triplet_core.h's kBand; the tests assert it
GROUP = 16            # pvlm_triplet_group_size(); the tests assert it
ADMIT = 1e-9          # no triplet of a scene meant to avoid the host fall-back lies this close to the cut in the reference's own numbers
PLANT = 1e-14         # how close to the cut the planted triplets lie


def _rotz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def graph_scene(F, pairs, seed, noise_deg, threshold):
    """camera rotations at random; R_21 = noise R_j R_i^T with a rotation of noise_deg * N(0, 1) degrees about a random axis per pair"""
    rng = np.random.default_rng(seed)
    Rc = np.array([rr.exp_so3(rng.normal(size=3) * 0.6) for _ in range(F)])
    R = np.zeros((len(pairs), 3, 3))
    for p, (i, j) in enumerate(pairs):
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        R[p] = rr.exp_so3(np.radians(noise_deg * rng.normal()) * a) @ Rc[j] @ Rc[i].T
    return dict(F=F, P=len(pairs), first=np.array([p[0] for p in pairs], np.int32), second=np.array([p[1] for p in pairs], np.int32), R_21=R, threshold=threshold, planted=False)


def shuffled(pairs, seed):
    """the list in another order, every pair still first < second"""
    rng = np.random.default_rng(seed)
    return [pairs[k] for k in rng.permutation(len(pairs))]


def complete_pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def planted_scene(threshold=2.0):
    """Four triangles that share no camera.  In three of them R_21 = R_32 = I and R_31 turns about z by the angle for which (1 + 2 cos) / 3 is the cut, and by that
    angle -+ 1e-13: c lies within PLANT of the cut (the products with the identity are exact).  The fourth is all identities (c = 1: kept by the device)."""
    cut = np.cos(threshold * np.pi / 180.0)
    theta = float(np.arccos((3.0 * cut - 1.0) / 2.0))
    pairs, R = [], []
    for t, d in enumerate((0.0, 1e-13, -1e-13, None)):
        i, j, k = 3 * t, 3 * t + 1, 3 * t + 2
        pairs += [(i, j), (j, k), (i, k)]
        R += [np.eye(3), np.eye(3), np.eye(3) if d is None else _rotz(theta + d)]
    sc = dict(F=12, P=len(pairs), first=np.array([p[0] for p in pairs], np.int32), second=np.array([p[1] for p in pairs], np.int32), R_21=np.array(R), threshold=threshold,
              planted=True)
    return sc


def build_scenes():
    """name -> scene: the smallest graphs at which the stage can still go wrong.  No pair; one pair; one triangle; K4 with its list shuffled (the caller-index contract
    of triplet_pairs); a star and a chain (no triangle); camera ids with gaps and a camera in no pair; K70 (a row of 69 is longer than a wave and than four groups:
    further rounds; 54 740 triplets cross the scan's chunks of 1024 pairs and 4096-wide tiles); the bench rule "next 19" at 300 cameras (49 020 triplets); the mirror
    scene of tests/rotavg_ref.py (46 pairs, 64 triplets, one pair planted 5 degrees off) at upstream's 0.1 degrees; a noisy scene whose loop errors lie on both sides
    of 2 degrees; the planted in-band scene."""
    S = {}
    S["no-pair"] = graph_scene(3, [], 1, 0.5, 1.0)
    S["one-pair"] = graph_scene(4, [(1, 3)], 2, 0.5, 1.0)
    S["triangle"] = graph_scene(3, [(0, 1), (1, 2), (0, 2)], 3, 0.5, 1.0)
    S["K4-shuffled"] = graph_scene(4, shuffled(complete_pairs(4), 4), 4, 0.5, 1.0)
    S["star"] = graph_scene(9, [(0, k) for k in range(1, 9)], 5, 0.5, 1.0)
    S["chain"] = graph_scene(20, [(i, i + 1) for i in range(19)], 6, 0.5, 1.0)
    ids = [0, 2, 5, 6, 9, 13, 14, 20]
    S["gaps"] = graph_scene(23, shuffled([(ids[a], ids[b]) for a in range(len(ids)) for b in range(a + 1, len(ids)) if (a + b) % 4], 7), 7, 0.5, 1.0)
    S["K70"] = graph_scene(70, shuffled(complete_pairs(70), 70), 8, 0.8, 2.0)
    S["next19-300"] = graph_scene(300, shuffled([(i, i + k) for i in range(300) for k in range(1, 20) if i + k < 300], 300), 9, 0.8, 2.0)
    g = rr.mirror_scene()
    S["mirror"] = dict(F=g["F"], P=g["P"], first=np.array([p["first"] for p in g["pairs"]], np.int32), second=np.array([p["second"] for p in g["pairs"]], np.int32),
                       R_21=np.array([p["R_21"] for p in g["pairs"]]), threshold=0.1, planted=False)
    S["noisy"] = graph_scene(40, shuffled(rr.chain_pairs(40, 5), 40), 10, 1.2, 2.0)
    S["planted"] = planted_scene()
    return S


_SCENES = {}
_REF = {}


def scenes():
    if not _SCENES:
        _SCENES.update(build_scenes())
    return _SCENES


def loop_cos(sc, tp):
    """the reference's own c of every triplet (numpy's products): trace(R_31^T R_32 R_21) / 3, by the triplet_pairs tp"""
    if len(tp) == 0:
        return np.zeros(0)
    R = sc["R_21"]
    return np.einsum("tji,tjk,tki->t", R[tp[:, 2]], R[tp[:, 1]], R[tp[:, 0]]) / 3.0


def reference(name):
    """dict(triplets (n x 3), triplet_pairs (n x 3, indices into the scene's list), pair_counts, c, keep (uint8 per pair), n_kept_triplets): find_triplet_ref's list
    and, per triplet, triplet_angle_deg < threshold.  Computed once per scene and shared; nobody writes into it."""
    if name not in _REF:
        sc = scenes()[name]
        edges = list(zip(sc["first"].tolist(), sc["second"].tolist()))
        place = {e: p for p, e in enumerate(edges)}
        trip = rr.find_triplet_ref(edges)
        t = np.array(trip, np.int32).reshape(-1, 3)
        tp = np.array([[place[(i, j)], place[(j, k)], place[(i, k)]] for i, j, k in trip], np.int32).reshape(-1, 3)
        counts = np.zeros(sc["P"], np.int64)
        np.add.at(counts, tp[:, 0], 1)
        keep = np.zeros(sc["P"], np.uint8)
        kept = np.array([rr.triplet_angle_deg(sc["R_21"][a], sc["R_21"][b], sc["R_21"][c]) < sc["threshold"] for a, b, c in tp], bool).reshape(-1)
        keep[np.unique(tp[kept].reshape(-1))] = 1
        _REF[name] = dict(triplets=t, triplet_pairs=tp, pair_counts=counts, c=loop_cos(sc, tp), keep=keep, n_kept_triplets=int(kept.sum()), kept=kept)
    return _REF[name]


def cut_of(threshold):
    return float(np.cos(threshold * np.pi / 180.0))


def admit():
    """Every scene but the planted one keeps its triplets ADMIT away from the cut in the reference's numbers, the planted triplets lie within PLANT of it, and the
    literal chain agrees with clamp(c) > cut on every triplet of every scene."""
    for name, sc in scenes().items():
        r = reference(name)
        c = np.minimum(1.0, np.maximum(r["c"], -1.0)); cut = cut_of(sc["threshold"])
        if sc["planted"]:
            assert int((np.abs(c - cut) < PLANT).sum()) == 3, (name, c - cut)
        else:
            assert not np.any(np.abs(c - cut) < ADMIT), (name, float(np.abs(c - cut).min()))
        literal = np.degrees(np.arccos(c)) < sc["threshold"]
        assert np.array_equal(literal, r["kept"]), name
        # the planted triplets are where the two may part (within an ulp of the cut): the reason the library hands them to the literal chain
        far = np.abs(c - cut) >= PLANT
        assert np.array_equal(literal[far], (c > cut)[far]), name


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------
_CHECK = []
GUARD = 8


def check_lib():
    if not _CHECK:
        from panovlm_amd import build
        lib = C.CDLL(build.build_triplet_check())
        lib.chk_triplet_band.restype = C.c_double
        _CHECK.append(lib)
    return _CHECK[0]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_find(F, first, second, want_triplets=True, want_pairs=True, capacity=None, want_counts=True, needed_ptr=True):
    """the host compile's pvlm_triplets_find: dict(rc, triplets, triplet_pairs, needed, pair_counts, guard_intact); capacity None: a sizing call first"""
    first = np.ascontiguousarray(first, np.int32); second = np.ascontiguousarray(second, np.int32); P = len(first)
    lib = check_lib()
    if capacity is None:
        n = C.c_longlong(-7)
        rc = lib.chk_triplets_find(C.c_int(F), C.c_int(P), _p(first), _p(second), None, None, C.c_longlong(0), C.byref(n), None)
        if rc:
            return dict(rc=int(rc), needed=n.value)
        capacity = n.value
    t = np.full((capacity + GUARD, 3), -7, np.int32) if want_triplets else None
    tp = np.full((capacity + GUARD, 3), -7, np.int32) if want_pairs else None
    pc = np.full(P + GUARD, -7, np.int64) if want_counts else None
    n = C.c_longlong(-7)
    rc = lib.chk_triplets_find(C.c_int(F), C.c_int(P), _p(first), _p(second), _p(t), _p(tp), C.c_longlong(capacity), C.byref(n) if needed_ptr else None, _p(pc))
    m = max(0, min(n.value, capacity))
    untouched = bool((t is None or np.all(t == -7)) and (tp is None or np.all(tp == -7)) and (pc is None or np.all(pc == -7)) and n.value == -7)
    intact = bool((t is None or np.all(t[max(capacity, 0):] == -7)) and (tp is None or np.all(tp[max(capacity, 0):] == -7)) and (pc is None or np.all(pc[P:] == -7)))
    return dict(rc=int(rc), triplets=None if t is None else t[:m], triplet_pairs=None if tp is None else tp[:m], needed=n.value, pair_counts=None if pc is None else pc[:P],
                guard_intact=intact, untouched=untouched)


def host_filter(F, first, second, R_21, threshold, null=()):
    """the host compile's pvlm_triplets_filter: dict(rc, keep, n_triplets, n_kept_triplets, n_uncertain, n_kept_pairs, guard_intact, untouched)"""
    first = np.ascontiguousarray(first, np.int32); second = np.ascontiguousarray(second, np.int32); P = len(first)
    R = np.ascontiguousarray(np.asarray(R_21, np.float64).reshape(-1, 9))
    keep = np.full(P + GUARD, 7, np.uint8); st = np.full(4, -7, np.int64)
    rc = check_lib().chk_triplets_filter(C.c_int(F), C.c_int(P), _p(first), _p(second), None if "R" in null else _p(R), C.c_double(threshold), None if "keep" in null else _p(keep),
                                         None if "stats" in null else _p(st))
    return dict(rc=int(rc), keep=keep[:P], n_triplets=int(st[0]), n_kept_triplets=int(st[1]), n_uncertain=int(st[2]), n_kept_pairs=int(st[3]),
                guard_intact=bool(np.all(keep[P:] == 7)), untouched=bool(np.all(keep == 7) and np.all(st == -7)))


def bad_calls(sc):
    """(name, first, second, threshold) for every argument both entries refuse; the call is the scene with one thing wrong"""
    out = []
    f = sc["first"].copy(); f[1] = sc["F"]
    out.append(("camera index out of range", f, sc["second"], sc["threshold"]))
    s = sc["second"].copy(); s[2] = sc["F"]
    out.append(("second camera index out of range", sc["first"], s, sc["threshold"]))
    f = sc["first"].copy(); f[1] = -1
    out.append(("negative camera index", f, sc["second"], sc["threshold"]))
    s = sc["second"].copy(); s[0] = sc["first"][0]
    out.append(("first == second", sc["first"], s, sc["threshold"]))
    f = sc["first"].copy(); s = sc["second"].copy(); f[0], s[0] = s[0], f[0]
    out.append(("first > second", f, s, sc["threshold"]))
    f = sc["first"].copy(); s = sc["second"].copy(); f[3], s[3] = f[0], s[0]
    out.append(("the same pair twice", f, s, sc["threshold"]))
    return out


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
def scene_graph(sc, duplicate=None, t_21=None):
    """the graph form tests/rotavg_ref.py's run_driver writes; duplicate = (p, R): pair p named once more at the end of the list with rotation R"""
    pairs = [dict(first=int(sc["first"][p]), second=int(sc["second"][p]), R_21=sc["R_21"][p], t_21=np.zeros(3) if t_21 is None else t_21[p], upper=0.0, lower=0.0)
             for p in range(sc["P"])]
    if duplicate is not None:
        p, R = duplicate
        pairs.append(dict(pairs[p], R_21=R))
    return dict(F=sc["F"], R_wc=np.zeros((sc["F"], 3, 3)), t_wc=np.full((sc["F"], 3), np.inf), pairs=pairs)


def run_driver(g, mode, route, *args):
    """tests/cpp/pvlm_triplet_driver.cpp on the graph g: dict(ok, message, lines {keyword: [the rest of every such line, as text]})"""
    import os
    import subprocess
    import tempfile
    from panovlm_amd import build
    if not os.path.exists(build.TRIPLET_DRIVER):
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
        res = subprocess.run([build.TRIPLET_DRIVER, mode, route, path] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(path)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    out = dict(ok=None, message="", lines={})
    for line in res.stdout.splitlines():
        w = line.split(" ", 1)
        if w[0] == "ok":
            out["ok"] = int(w[1])
        elif w[0] == "message":
            out["message"] = w[1] if len(w) > 1 else ""
        else:
            out["lines"].setdefault(w[0], []).append(w[1] if len(w) > 1 else "")
    return out


admit()
