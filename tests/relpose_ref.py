"""K36 test helpers: the synthetic two-view scenes of the relative-pose refinement, an independent numpy twin of one pair's SfMLocalBA (residuals and Jacobians by
tests/sfm_ba_ref.eval_jet, the FULL damped system over 6 + 3 N unknowns solved densely, the trust-region policy of tests/lm_twin.py with Solver::Options' defaults)
and the ctypes wrappers of the host compile (tests/cpp/relpose_core_check.cpp, built with -ffp-contract=off and with -ffp-contract=fast)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import essential_ref as er
from tests import sfm_ba_ref as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH_DTYPE = er.MATCH_DTYPE
ROWS, COLS = 720, 1440
KIND = {"angle2": 1, "pixel": 2}


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def pixels_of(b, rows=ROWS, cols=COLS):
    """float32 pixels of bearings (N x 3) in a rows x cols panorama."""
    b = np.asarray(b, np.float64)
    lon = np.arctan2(b[:, 0], b[:, 2]); lat = -np.arcsin(b[:, 1] / np.linalg.norm(b, axis=1))
    return np.stack([cols * (0.5 + lon / (2 * np.pi)), rows * (0.5 - lat / np.pi)], 1).astype(np.float32)


def perturbed(rng, R, t, rot_deg=0.5, dir_deg=2.0):
    """R turned by rot_deg about a random axis; t / |t| turned by dir_deg about a random axis orthogonal to it."""
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    Rp = er.rodrigues(np.radians(rot_deg) * a) @ R
    d = t / np.linalg.norm(t)
    b = np.cross(d, rng.normal(size=3)); b /= np.linalg.norm(b)
    return Rp, er.rodrigues(np.radians(dir_deg) * b) @ d


def pair_scene(seed, n, planted=0.0, pole=False, keep=None):
    """One pair: n matches without outliers (er.two_view_scene), the keypoints its bearings project to, the true pose, a start pose 0.5 degrees / 2 degrees off and the
    points triangulated there.  planted: this fraction of the inliers gets a 20-pixel error in frame 2.  pole: the start rotation is the identity and the first point
    starts on camera 2's pole axis (p0 = p2 = 0 exactly).  keep: hand only every keep-th match to the refinement (the others stay in the match list)."""
    rng = np.random.default_rng(seed)
    w = (0.004, -0.006, 0.003) if pole else (0.05, -0.2, 0.1)
    b1, b2, m, _, R, t = er.two_view_scene(rng, n, outlier_fraction=0.0, w=w)
    kp1 = pixels_of(b1); kp2 = pixels_of(b2)
    idx = np.arange(n, dtype=np.int32) if not keep else np.arange(0, n, keep, dtype=np.int32)
    if planted > 0 and len(idx):
        bad = idx[rng.permutation(len(idx))[:max(1, int(round(planted * len(idx))))]]
        ang = rng.uniform(0, 2 * np.pi, len(bad))
        kp2[m["train"][bad]] += (20.0 * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
    R0, t0 = perturbed(rng, R, t)
    if pole:
        R0 = np.eye(3)
    p1 = b1[m["query"][idx]]; p2 = b2[m["train"][idx]]
    X0 = er.triangulate_2view(R0, t0, p1, p2) if len(idx) else np.zeros((0, 3))
    if pole and len(idx):
        X0[0] = [-t0[0], 1.7, -t0[2]]
    assert np.isfinite(X0).all()
    return dict(kp1=kp1, kp2=kp2, matches=m, idx=idx, R0=R0, t0=t0, X0=X0, R_true=R, t_true=t / np.linalg.norm(t), n=len(idx))


SIZES = (0, 1, 2, 8, 63, 64, 65, 257, 300)      # every inlier count a K36 test uses: the twin's sizes, both sides of the workgroup (64 lanes), 4 W + 1, the ragged batch


# seeds replaced on the CPU because the scene failed the knife-edge condition (tests/test_relpose_cpu.py): n = 8 (108), n = 257 (357), the pole scene (7)
SEEDS = {8: 1108, 257: 1357}


def size_scene(n):
    return pair_scene(SEEDS.get(n, 100 + n), n)


def outlier_scene(n=120):
    """10 % of the points carry a 20-pixel error in frame 2: the Huber branch, rejected steps"""
    return pair_scene(7, n, planted=0.1)


def pole_scene():
    return pair_scene(8, 40, pole=True)


def all_scenes():
    """(name, scene) of every scene the CPU and GPU tests hand to the refinement; test_relpose_cpu.py holds each to the knife-edge condition"""
    return [("n%d" % n, size_scene(n)) for n in SIZES] + [("outlier", outlier_scene()), ("outlier40", outlier_scene(40)), ("pole", pole_scene())]


def assemble(scenes, frames=None):
    """The arrays of one call from a list of pair scenes.  frames: per scene its (src frame, tgt frame); default (2 p, 2 p + 1).  A frame named by several scenes holds
    their keypoints one block after the other (the matches are renumbered)."""
    frames = frames or [(2 * p, 2 * p + 1) for p in range(len(scenes))]
    nf = max([max(f) for f in frames], default=-1) + 1
    kps = [np.zeros((0, 2), np.float32) for _ in range(nf)]
    src, tgt, ms, idxs, moff, ioff = [], [], [], [], [0], [0]
    for sc, (f1, f2) in zip(scenes, frames):
        m = sc["matches"].copy()
        m["query"] += len(kps[f1]); kps[f1] = np.concatenate([kps[f1], sc["kp1"]])
        m["train"] += len(kps[f2]); kps[f2] = np.concatenate([kps[f2], sc["kp2"]])
        src.append(f1); tgt.append(f2); ms.append(m); idxs.append(sc["idx"])
        moff.append(moff[-1] + len(m)); ioff.append(ioff[-1] + len(sc["idx"]))
    cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)
    return dict(keypoints=kps, img_rows=np.full(nf, ROWS, np.int32), img_cols=np.full(nf, COLS, np.int32), src=np.array(src, np.int32), tgt=np.array(tgt, np.int32),
                match_offsets=np.array(moff, np.int64), matches=np.concatenate(ms) if ms else np.zeros(0, MATCH_DTYPE), inlier_offsets=np.array(ioff, np.int64),
                inlier_idx=cat(idxs, 0, np.int32), R_21=np.array([s["R0"] for s in scenes]).reshape(-1, 3, 3), t_21=np.array([s["t0"] for s in scenes]).reshape(-1, 3),
                triangulated=cat([s["X0"] for s in scenes], (0, 3), np.float64).reshape(-1, 3))


def subset(call, pairs):
    """The call restricted to the listed pairs, in the listed order (frames untouched)."""
    mo, io = call["match_offsets"], call["inlier_offsets"]
    out = dict(call)
    out["src"] = call["src"][pairs]; out["tgt"] = call["tgt"][pairs]
    out["matches"] = np.concatenate([call["matches"][mo[p]:mo[p + 1]] for p in pairs]) if len(pairs) else call["matches"][:0]
    out["inlier_idx"] = np.concatenate([call["inlier_idx"][io[p]:io[p + 1]] for p in pairs]) if len(pairs) else call["inlier_idx"][:0]
    out["triangulated"] = np.concatenate([call["triangulated"][io[p]:io[p + 1]] for p in pairs]) if len(pairs) else call["triangulated"][:0]
    out["match_offsets"] = np.concatenate([[0], np.cumsum([mo[p + 1] - mo[p] for p in pairs])]).astype(np.int64)
    out["inlier_offsets"] = np.concatenate([[0], np.cumsum([io[p + 1] - io[p] for p in pairs])]).astype(np.int64)
    out["R_21"] = call["R_21"][pairs]; out["t_21"] = call["t_21"][pairs]
    return out


def split_points(res, call):
    io = call["inlier_offsets"]
    return [res["triangulated"][io[p]:io[p + 1]] for p in range(len(call["src"]))]


# ---- the twin --------------------------------------------------------------------------------------------------------------------------------
class Options:
    max_num_iterations = 50
    initial_radius = 1e4
    max_radius = 1e16
    min_radius = 1e-32
    min_relative_decrease = 1e-3
    function_tolerance = 1e-6
    gradient_tolerance = 1e-10
    parameter_tolerance = 1e-8
    min_lm_diagonal = 1e-6
    max_lm_diagonal = 1e32


def observations(kind, kp, rows=ROWS, cols=COLS):
    """What a block is created with: the float pixel widened (pixel), eq.ImageToSphere of the widened pixel in double (angle2; eval_jet applies the constructor's wrap)."""
    kp = np.asarray(kp, np.float32).astype(np.float64).reshape(-1, 2)
    return kp if kind == sb.PIXEL else np.stack([(2 * kp[:, 0] / cols - 1) * np.pi, (0.5 - kp[:, 1] / rows) * np.pi], 1)


def twin_refine(sc, kind, opt=None):
    """One pair's SfMLocalBA on the full system.  Returns dict(R_21, t_21, triangulated, ok, initial_cost, final_cost, successful (accepted steps), unsuccessful,
    termination)."""
    opt = opt or Options()
    k = KIND[kind]; a = 4.0 if k == sb.PIXEL else 4.0 * np.pi / 180.0
    n = sc["n"]
    if n == 0:
        return dict(R_21=sc["R0"].copy(), t_21=sc["t0"].copy(), triangulated=sc["X0"].copy(), ok=1, initial_cost=0.0, final_cost=0.0, successful=0, unsuccessful=0,
                    termination=6)
    m = sc["matches"][sc["idx"]]
    o1 = observations(k, sc["kp1"][m["query"]]); o2 = observations(k, sc["kp2"][m["train"]])
    aa0 = np.zeros(3)
    aa = matrix_to_angle_axis(sc["R0"]); t = sc["t0"].astype(np.float64).copy(); X = sc["X0"].astype(np.float64).copy()
    nu = 6 + 3 * n
    z = np.zeros((n, 3))

    def evaluate(aa_, t_, X_):
        r1, J1 = sb.eval_jet(k, np.broadcast_to(aa0, (n, 3)), z, X_, o1, 1.0, ROWS, COLS)
        r2, J2 = sb.eval_jet(k, np.broadcast_to(aa_, (n, 3)), np.broadcast_to(t_, (n, 3)), X_, o2, 1.0, ROWS, COLS)
        for J in (J1, J2):          # the zero-derivative convention at the poles (Jet arithmetic gives inf / NaN there)
            J[~np.isfinite(J).all(axis=(1, 2))] = 0.0
        w1, h1 = sb.huber_block(r1, 1, a); w2, h2 = sb.huber_block(r2, 1, a)
        Jf = np.zeros((4 * n, nu)); rf = np.zeros(4 * n)
        for i in range(n):
            s1, s2 = np.sqrt(w1[i]), np.sqrt(w2[i])
            Jf[4 * i:4 * i + 2, 6 + 3 * i:9 + 3 * i] = s1 * J1[i, :, 6:]
            Jf[4 * i + 2:4 * i + 4, :6] = s2 * J2[i, :, :6]
            Jf[4 * i + 2:4 * i + 4, 6 + 3 * i:9 + 3 * i] = s2 * J2[i, :, 6:]
            rf[4 * i:4 * i + 2] = s1 * r1[i]; rf[4 * i + 2:4 * i + 4] = s2 * r2[i]
        return float(h1.sum() + h2.sum()), Jf.T @ Jf, Jf.T @ rf

    with np.errstate(all="ignore"):
        cost, H, g = evaluate(aa, t, X)
        out = dict(initial_cost=cost, successful=0, unsuccessful=0, termination=-1)
        scale = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(H), 0.0)))
        radius, dec, it = opt.initial_radius, 2.0, 0
        if not np.isfinite(cost):
            out["termination"] = 5
        elif np.abs(g).max() <= opt.gradient_tolerance:
            out["termination"] = 2
        while out["termination"] < 0 and it < opt.max_num_iterations:
            it += 1
            Hs = H * scale[:, None] * scale[None, :]
            rhs = -g * scale
            D = np.clip(np.diag(Hs), opt.min_lm_diagonal, opt.max_lm_diagonal) / radius
            ok = True
            try:
                L = np.linalg.cholesky(Hs + np.diag(D))
                dy = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
            except np.linalg.LinAlgError:
                ok = False
            accepted = False
            if ok:
                model = -((-rhs) @ dy + 0.5 * dy @ Hs @ dy)
                ok = model > 0 and np.isfinite(model)
            if ok:
                step = dy * scale
                c_aa = aa + step[:3]; c_t = t + step[3:6]; c_X = X + step[6:].reshape(n, 3)
                c_cost, cH, cg = evaluate(c_aa, c_t, c_X)
                rho = (cost - c_cost) / model
                if np.isfinite(c_cost) and rho > opt.min_relative_decrease:
                    accepted = True
                    xn = np.sqrt((aa ** 2).sum() + (t ** 2).sum() + (X ** 2).sum())
                    change = cost - c_cost; prev = cost
                    aa, t, X, cost, H, g = c_aa, c_t, c_X, c_cost, cH, cg
                    radius = min(opt.max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                    dec = 2.0
                    out["successful"] += 1
                    if abs(change) <= opt.function_tolerance * prev:
                        out["termination"] = 1
                    elif np.abs(g).max() <= opt.gradient_tolerance:
                        out["termination"] = 2
                    elif np.linalg.norm(step) <= opt.parameter_tolerance * (xn + opt.parameter_tolerance):
                        out["termination"] = 3
            if not accepted:
                out["unsuccessful"] += 1
                radius /= dec; dec *= 2.0
                if radius < opt.min_radius:
                    out["termination"] = 4
    if out["termination"] < 0:
        out["termination"] = 0
    s = np.linalg.norm(t)
    out.update(final_cost=cost, R_21=er.rodrigues(aa), t_21=t / s, triangulated=X / s, ok=int(np.isfinite(cost)))
    return out


def outer_blocks(sc, kind, R, t, X):
    """how many of the pair's 2 N blocks lie in Huber's outer region at (R, t, X): residuals by eval_jet"""
    k = KIND[kind]; a = 4.0 if k == sb.PIXEL else 4.0 * np.pi / 180.0
    n = sc["n"]; m = sc["matches"][sc["idx"]]
    o1 = observations(k, sc["kp1"][m["query"]]); o2 = observations(k, sc["kp2"][m["train"]])
    z = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        r1, _ = sb.eval_jet(k, z, z, X, o1, 1.0, ROWS, COLS)
        r2, _ = sb.eval_jet(k, np.broadcast_to(matrix_to_angle_axis(R), (n, 3)), np.broadcast_to(t, (n, 3)), X, o2, 1.0, ROWS, COLS)
    return int(((r1 * r1).sum(1) > a * a).sum() + ((r2 * r2).sum(1) > a * a).sum())


def matrix_to_angle_axis(R):
    """log of a rotation matrix away from pi (the scenes' rotations are small)."""
    c = np.clip((np.trace(R) - 1) / 2, -1, 1); th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return v * (0.5 if th < 1e-12 else th / (2 * np.sin(th)))


# ---- the host compile ------------------------------------------------------------------------------------------------------------------------
_CHECKS = {}


def build_check(contract="off"):
    """build/librelpose_check_<contract>.so: tests/cpp/relpose_core_check.cpp with -ffp-contract=off or fast."""
    if contract in _CHECKS:
        return _CHECKS[contract]
    out = os.path.join(ROOT, "build", "librelpose_check_%s.so" % contract)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=" + contract] + (["-march=native"] if contract == "fast" else []) +
                          ["-fPIC", "-shared", "-pthread", "-o", out, os.path.join(ROOT, "tests", "cpp", "relpose_core_check.cpp")])
    _CHECKS[contract] = C.CDLL(out)
    return _CHECKS[contract]


def build_check_main(sanitize=True):
    """The stand-alone program of the same file (its own main), with the host sanitizers."""
    out = os.path.join(ROOT, "build", "relpose_check_main")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-DRELPOSE_CHECK_MAIN"] + san +
                          ["-o", out, os.path.join(ROOT, "tests", "cpp", "relpose_core_check.cpp")])
    return out


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def host_refine(chk, call, kind="pixel", max_num_iterations=50, threads=8):
    """The host loop on the arrays of `assemble`.  Returns (rc, dict like api.refine_relative_poses plus accept_masks); the inputs are not modified."""
    arrs = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in call["keypoints"]]
    rows_kp = np.array([len(a) for a in arrs], np.int32)
    flat = np.ascontiguousarray(np.concatenate(arrs + [np.zeros((1, 2), np.float32)]))
    src = np.ascontiguousarray(call["src"], np.int32); tgt = np.ascontiguousarray(call["tgt"], np.int32)
    moff = np.ascontiguousarray(call["match_offsets"], np.int64); ioff = np.ascontiguousarray(call["inlier_offsets"], np.int64)
    m = np.ascontiguousarray(call["matches"], MATCH_DTYPE); idx = np.ascontiguousarray(call["inlier_idx"], np.int32)
    ir = np.ascontiguousarray(call["img_rows"], np.int32); ic = np.ascontiguousarray(call["img_cols"], np.int32)
    npairs = len(src)
    R = np.array(call["R_21"], np.float64).reshape(npairs, 3, 3).copy(); t = np.array(call["t_21"], np.float64).reshape(npairs, 3).copy()
    tri = np.array(call["triangulated"], np.float64).reshape(-1, 3).copy()
    if len(tri) == 0:
        tri = np.zeros((0, 3))
    ok = np.zeros(max(npairs, 1), np.uint8); sm = np.zeros((max(npairs, 1), 5)); masks = np.zeros(max(npairs, 1), np.uint64)
    tri_buf = tri if len(tri) else np.zeros((1, 3))
    rc = chk.chk_relpose_refine(C.c_int(len(arrs)), _ptr(rows_kp), _ptr(flat), _ptr(ir), _ptr(ic), C.c_int(npairs), _ptr(src), _ptr(tgt), _ptr(moff), _ptr(m), _ptr(ioff),
                                _ptr(idx if len(idx) else np.zeros(1, np.int32)), _ptr(R if npairs else np.zeros(9)), _ptr(t if npairs else np.zeros(3)), _ptr(tri_buf),
                                C.c_int(KIND[kind] if isinstance(kind, str) else kind), C.c_int(max_num_iterations), C.c_int(threads), _ptr(ok), _ptr(sm), _ptr(masks))
    summ = np.zeros(npairs, np.dtype([("initial_cost", np.float64), ("final_cost", np.float64), ("successful_steps", np.int32), ("unsuccessful_steps", np.int32),
                                      ("termination", np.int32)]))
    for j, name in enumerate(summ.dtype.names):
        summ[name] = sm[:npairs, j]
    return rc, dict(R_21=R, t_21=t, triangulated=tri, ok=ok[:npairs], summaries=summ, accept_masks=masks[:npairs])


def same_decisions(call, kind, max_num_iterations=50):
    """The knife-edge condition: both host builds take the same accept / reject sequence and end for the same reason, pair by pair.  Returns (bool, result of the
    -ffp-contract=off build)."""
    rc_a, a = host_refine(build_check("off"), call, kind, max_num_iterations)
    rc_b, b = host_refine(build_check("fast"), call, kind, max_num_iterations)
    assert rc_a == 0 and rc_b == 0
    same = (np.array_equal(a["accept_masks"], b["accept_masks"]) and np.array_equal(a["summaries"]["termination"], b["summaries"]["termination"]) and
            np.array_equal(a["summaries"]["successful_steps"], b["summaries"]["successful_steps"]) and
            np.array_equal(a["summaries"]["unsuccessful_steps"], b["summaries"]["unsuccessful_steps"]))
    return same, a


# ---- the host tail: SetTranslationScaleDepthMap, LargestBiconnectedGraph, the final sort -----------------------------------------------------------
def _round_half_away(x):
    return int(np.sign(x) * np.floor(abs(x) + 0.5))


def _cam_to_image(rows, cols, p):
    lon = float(sb.fast_atan2(np.float64(p[0]), np.float64(p[2])))
    lat = -float(sb.fast_atan2(np.float64(p[1]), np.sqrt(np.float64(p[0]) * p[0] + np.float64(p[2]) * p[2])))
    return cols * (0.5 + lon / (2.0 * np.pi)), rows * (0.5 - lat / np.pi)


def scale_ref(eq_rows, eq_cols, rows1, d1, d2, R, t, tri):
    """SfM::SetTranslationScaleDepthMap(eq, pair) line by line.  d1 / d2: uint16 arrays (or None).  Returns (ok, t, tri, points_with_depth, upper, lower)."""
    t = np.array(t, np.float64); tri = np.array(tri, np.float64).reshape(-1, 3)
    if d1 is None or d2 is None:
        return False, t, tri, 0, -1.0, -1.0
    half = 1.0 if d1.shape[0] == (rows1 + 1) // 2 else 0.0
    scale = []
    for p in tri:
        x, y = _cam_to_image(eq_rows, eq_cols, p)
        row, col = _round_half_away(y / (1.0 + half)), _round_half_away(x / (1.0 + half))
        if not (col >= 0 and row >= 0 and col + 1 <= eq_cols and row + 1 <= eq_rows) or row >= d1.shape[0] or col >= d1.shape[1]:
            continue
        depth1 = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
        real1 = np.float32(d1[row, col] / 256.0)
        if real1 <= 0:
            continue
        s1 = np.float64(real1) / depth1
        q = np.array([(R[r, 0] * p[0] + R[r, 1] * p[1] + R[r, 2] * p[2]) + t[r] for r in range(3)])
        x, y = _cam_to_image(eq_rows, eq_cols, q)
        row, col = _round_half_away(y / (1.0 + half)), _round_half_away(x / (1.0 + half))
        if not (col >= 0 and row >= 0 and col + 1 <= eq_cols and row + 1 <= eq_rows) or row >= d2.shape[0] or col >= d2.shape[1]:
            continue
        depth2 = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
        real2 = np.float32(d2[row, col] / 256.0)
        if real2 <= 0:
            continue
        s2 = np.float64(real2) / depth2
        if abs(s1 - s2) / min(s1, s2) > 0.2:
            continue
        scale += [s1, s2]
    if len(scale) < 10:
        return False, t, tri, 0, -1.0, -1.0
    good = True
    preserve = list(scale)
    for _ in range(2):
        num = len(scale)
        if num < 10:
            good = False
            break
        mx, mn = max(scale), min(scale)
        if mx / mn < 1.2:
            break
        interval = (mx - mn) / 10
        histo = [[] for _ in range(10)]
        for s in scale:
            b = int((s - mn - 1e-8) / interval)
            histo[max(0, min(b, 9))].append(s)
        scale = [s for bin_ in histo if len(bin_) > 0.1 * num for s in bin_]
    if good:
        final = 0.0
        for s in scale:
            final += s
        final /= len(scale)
        pwd, up, lo = len(scale) // 2, max(scale), min(scale)
    else:
        final = sorted(preserve)[len(preserve) // 2]
        pwd, up, lo = len(preserve) // 2, 0.0, 0.0
    return True, t * final, tri * final, pwd, up, lo


def host_scale(chk, eq_rows, eq_cols, rows1, d1, d2, R, t, tri):
    z = np.zeros((1, 1), np.uint16)
    a = np.ascontiguousarray(d1 if d1 is not None else z, np.uint16); b = np.ascontiguousarray(d2 if d2 is not None else z, np.uint16)
    R = np.ascontiguousarray(R, np.float64); t = np.array(t, np.float64); tri = np.array(tri, np.float64).reshape(-1, 3).copy(); out = np.zeros(3)
    ok = chk.chk_relpose_scale(C.c_int(eq_rows), C.c_int(eq_cols), C.c_int(rows1), _ptr(a), C.c_int(a.shape[0] if d1 is not None else 0), C.c_int(a.shape[1]), _ptr(b),
                               C.c_int(b.shape[0] if d2 is not None else 0), C.c_int(b.shape[1]), _ptr(R), _ptr(t), _ptr(tri), C.c_int(len(tri)), _ptr(out))
    return bool(ok), t, tri, int(out[0]), out[1], out[2]


def host_graph(chk, pairs):
    """LargestBiconnectedGraph: (keep per pair, surviving frames)"""
    n = len(pairs)
    a = np.array([p[0] for p in pairs] + [0], np.int64); b = np.array([p[1] for p in pairs] + [0], np.int64)
    keep = np.zeros(n + 1, np.uint8); nodes = np.zeros(2 * n + 2, np.int64)
    k = chk.chk_relpose_graph(C.c_int(n), _ptr(a), _ptr(b), _ptr(keep), _ptr(nodes))
    return keep[:n].tolist(), nodes[:k].tolist()


def host_sort(chk, pairs):
    n = len(pairs)
    a = np.array([p[0] for p in pairs] + [0], np.int64); b = np.array([p[1] for p in pairs] + [0], np.int64); order = np.zeros(n + 1, np.int32)
    chk.chk_relpose_sort(C.c_int(n), _ptr(a), _ptr(b), _ptr(order))
    return [pairs[i] for i in order[:n]]


def sort_ref(pairs):
    """the insertion sort std::sort runs on a short range, with upstream's comparator as written"""
    less = lambda a, b: True if a[0] < b[0] else a[1] < b[1]
    v = list(pairs)
    for i in range(1, len(v)):
        val = v[i]
        if less(val, v[0]):
            v[1:i + 1] = v[0:i]; v[0] = val
        else:
            j = i
            while j > 0 and less(val, v[j - 1]):
                v[j] = v[j - 1]; j -= 1
            v[j] = val
    return v


# ---- the comparison every K36 test makes --------------------------------------------------------------------------------------------------------------
def cost_floor(n, kind, cost):
    """How far two correct evaluations of the same cost may lie apart because of the rounding of its residuals.  A residual is the difference of a projected coordinate
    of magnitude up to M (the image width for the pixel kind, 2 pi for the angle kind) and an observation; the projection passes through four roundings of a value of
    that magnitude (atan2 or asin, the division by pi, the scaling, the subtraction), so it carries an absolute error of up to d = 4 eps M.  With m = 4 n residuals and
    cost = sum r^2 / 2:  |cost(r + e) - cost(r)| <= |r| |e| + |e|^2 / 2 <= sqrt(2 cost) sqrt(m) d + m d^2 / 2."""
    M = float(COLS) if KIND[kind] == sb.PIXEL else 2 * np.pi
    d = 4 * np.finfo(np.float64).eps * M
    m = 4 * n
    return np.sqrt(2 * abs(cost)) * np.sqrt(m) * d + 0.5 * m * d * d


def check_against(res, p, ref, pts, kind):
    """one pair of a result against a reference dict(R_21, t_21, triangulated, initial_cost, final_cost, successful, unsuccessful, termination, ok): initial cost 1e-9
    relative, final cost 1e-6 relative, pose and points 1e-6, equal step counts and termination (the tolerances of tests/test_sfm_ba_gpu.py::_check_against_twin).
    One addition, for pairs with fewer residuals than unknowns only (4 N < 6 + 3 N, N <= 5): their minimum is ZERO, so both final costs are the square of what the
    stopping rule left of the rounding errors (1e-21 .. 1e-28) and differ in the first digit between any two correct programs; there the bound on the final cost is
    1e-6 relative PLUS cost_floor, the rounding of the residuals themselves (about 1e-25 for the pixel kind, 1e-26 for the angle kind at these costs)."""
    s = res["summaries"][p]
    n = len(pts)
    assert abs(s["initial_cost"] - ref["initial_cost"]) <= 1e-9 * abs(ref["initial_cost"]), (s["initial_cost"], ref["initial_cost"])
    tol = 1e-6 * abs(ref["final_cost"]) + (cost_floor(n, kind, ref["final_cost"]) if 0 < 4 * n < 6 + 3 * n else 0.0)
    print("final cost", s["final_cost"], ref["final_cost"], "difference", abs(s["final_cost"] - ref["final_cost"]), "bound", tol)
    assert abs(s["final_cost"] - ref["final_cost"]) <= tol, (s["final_cost"], ref["final_cost"], tol)
    assert (s["successful_steps"], s["unsuccessful_steps"]) == (ref["successful"], ref["unsuccessful"])
    assert s["termination"] == ref["termination"]
    assert np.abs(res["R_21"][p] - ref["R_21"]).max() <= 1e-6
    assert np.abs(res["t_21"][p] - ref["t_21"]).max() <= 1e-6
    X = np.asarray(ref["triangulated"]).reshape(-1, 3)
    assert pts.shape == X.shape
    if len(X):
        assert (np.abs(pts - X) / np.maximum(1.0, np.linalg.norm(X, axis=1, keepdims=True))).max() <= 1e-6
    assert res["ok"][p] == ref["ok"]
