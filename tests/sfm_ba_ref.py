"""numpy restatements for K31 (SfMGlobalBA's two-row reprojection kinds and the track filters of SfM::GlobalBundleAdjustment).

- `eval_jet`: PanoramaReprojResidual_2Angle / _Pixel (base/CostFunction.h:178-214, :249-288) through a vectorised dual number
  Jet<9> and a restated ceres::AngleAxisRotatePoint (small-angle branch included) — independent of the closed form on the device.
- `bundle_reference2`: the Schur complement of the point blocks from materialised two-row r, J, with the loss on the block's
  squared norm.
- `filter_ref`: FilterTracksPixelResidual / FilterTracksAngleResidual (sfm/Structure.cpp:121-193) restated operation by operation,
  for bit-for-bit comparison with the per-track core (csrc/pvlm_sfm_filter_core.h).
"""
import numpy as np

from tests import synth

ANGLE2, PIXEL = 1, 2
EPS = np.finfo(np.float64).eps


# ---- Jet<9>: value v (N,), derivative d (N, 9) ----------------------------------------------------------------------------------------
class Jet:
    def __init__(self, v, d):
        self.v = np.asarray(v, np.float64); self.d = np.asarray(d, np.float64)

    @staticmethod
    def const(c, n):
        return Jet(np.broadcast_to(np.asarray(c, np.float64), (n,)).copy(), np.zeros((n, 9)))

    def __add__(self, o):
        o = _j(o, self); return Jet(self.v + o.v, self.d + o.d)

    __radd__ = __add__

    def __sub__(self, o):
        o = _j(o, self); return Jet(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return _j(o, self) - self

    def __neg__(self):
        return Jet(-self.v, -self.d)

    def __mul__(self, o):
        o = _j(o, self); return Jet(self.v * o.v, self.d * o.v[:, None] + o.d * self.v[:, None])

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _j(o, self)
        q = self.v / o.v
        return Jet(q, (self.d - q[:, None] * o.d) / o.v[:, None])

    def __rtruediv__(self, o):
        return _j(o, self) / self


def _j(o, like):
    return o if isinstance(o, Jet) else Jet.const(o, like.v.shape[0])


def jsqrt(a):
    s = np.sqrt(a.v)
    return Jet(s, a.d / (2.0 * s)[:, None])


def jsin(a):
    return Jet(np.sin(a.v), a.d * np.cos(a.v)[:, None])


def jcos(a):
    return Jet(np.cos(a.v), -a.d * np.sin(a.v)[:, None])


def jatan2(y, x):
    t = 1.0 / (x.v * x.v + y.v * y.v)
    return Jet(np.arctan2(y.v, x.v), (x.v[:, None] * y.d - y.v[:, None] * x.d) * t[:, None])


def jasin(a):
    return Jet(np.arcsin(a.v), a.d / np.sqrt(1.0 - a.v * a.v)[:, None])


def _where(m, a, b):
    return Jet(np.where(m, a.v, b.v), np.where(m[:, None], a.d, b.d))


def angle_axis_rotate_point(aa, pt):
    """ceres::AngleAxisRotatePoint on Jets (rotation.h): Rodrigues when theta^2 > eps, else pt + aa x pt."""
    n = aa[0].v.shape[0]
    theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]
    big = theta2.v > EPS
    # the large-angle branch on safe inputs where it is not taken (keeps inf / NaN out of the other lanes)
    one = Jet.const(1.0, n)
    th2s = _where(big, theta2, one)
    theta = jsqrt(th2s)
    c, s = jcos(theta), jsin(theta)
    inv = 1.0 / theta
    w = [aa[k] * inv for k in range(3)]
    wx = [w[1] * pt[2] - w[2] * pt[1], w[2] * pt[0] - w[0] * pt[2], w[0] * pt[1] - w[1] * pt[0]]
    tmp = (w[0] * pt[0] + w[1] * pt[1] + w[2] * pt[2]) * (1.0 - c)
    r_big = [pt[k] * c + wx[k] * s + w[k] * tmp for k in range(3)]
    ax = [aa[1] * pt[2] - aa[2] * pt[1], aa[2] * pt[0] - aa[0] * pt[2], aa[0] * pt[1] - aa[1] * pt[0]]
    r_small = [pt[k] + ax[k] for k in range(3)]
    return [_where(big, r_big[k], r_small[k]) for k in range(3)]


def eval_jet(kind, aa, t, X, o, w, rows=0, cols=0):
    """Residuals (N, 2) and Jacobians (N, 2, 9) [d/daa_cw | d/dt_cw | d/dX] of the functors, per observation (aa, t, X, o: N rows).
    kind ANGLE2: o = sphere angles before the constructor's wrap (applied here); kind PIXEL: o = pixels."""
    aa, t, X, o = (np.asarray(a, np.float64) for a in (aa, t, X, o))
    n = aa.shape[0]
    eye = np.eye(9)

    def seed(a, c0):
        return [Jet(a[:, k], np.broadcast_to(eye[c0 + k], (n, 9)).copy()) for k in range(3)]

    A, T, P = seed(aa, 0), seed(t, 3), seed(X, 6)
    pc = angle_axis_rotate_point(A, P)
    pc = [pc[k] + T[k] for k in range(3)]
    norm = jsqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2])
    lon = jatan2(pc[0], pc[2])
    lat = -jasin(pc[1] / norm)
    if kind == PIXEL:
        px = float(cols) * (0.5 + lon / (2.0 * np.pi))
        py = float(rows) * (0.5 - lat / np.pi)
        r0 = w * (px - o[:, 0]); r1 = w * (py - o[:, 1])
    else:
        x = np.where(o[:, 0] < 0, o[:, 0] + 2 * np.pi, o[:, 0])
        lon = _where(lon.v < 0.0, lon + 2 * np.pi, lon)
        r0 = w * (lon - x); r1 = w * (lat - o[:, 1])
    return np.stack([r0.v, r1.v], 1), np.stack([r0.d, r1.d], 1)


def project(kind, tab_rows, X, rows=0, cols=0):
    """Exact projection of X through pose-table rows (N x 21): pixels (PIXEL) or wrapped sphere angles (ANGLE2), N x 2."""
    R = tab_rows[:, :9].reshape(-1, 3, 3); p = np.einsum("nij,nj->ni", R, X) + tab_rows[:, 18:]
    lon = np.arctan2(p[:, 0], p[:, 2]); lat = -np.arcsin(p[:, 1] / np.linalg.norm(p, axis=1))
    if kind == PIXEL:
        return np.stack([cols * (0.5 + lon / (2 * np.pi)), rows * (0.5 - lat / np.pi)], 1)
    return np.stack([np.where(lon < 0, lon + 2 * np.pi, lon), lat], 1)


def huber_block(r, loss, a):
    """rho' and rho / 2 per observation of two-row residuals r (N, 2): the loss acts on s = r0^2 + r1^2."""
    s = (r * r).sum(1)
    if loss == 1:
        outer = s > a * a
        rr = np.sqrt(np.where(outer, s, 1.0))
        return np.where(outer, a / rr, 1.0), 0.5 * np.where(outer, 2 * a * rr - a * a, s)
    return np.ones_like(s), 0.5 * s


def bundle_reference2(r, J, off, cam, n_cams, loss, a, scale, radius, min_diag, max_diag, frozen=None):
    """Two-row version of synth.bundle_reference: r (n, 2), J (n, 2, 9).  Returns dict(S 6F x 6F, g, cost, Udiag F x 6, gcam 6F,
    Vinv, gp, scale, gmax).  Frozen points are not eliminated (Vinv = 0)."""
    rho1, half = huber_block(r, loss, a)
    F = n_cams; M = len(off) - 1
    S = np.zeros((6 * F, 6 * F)); gc = np.zeros(6 * F); Ud = np.zeros((F, 6))
    Vinv = np.zeros((M, 3, 3)); gp = np.zeros((M, 3)); sc = np.zeros((M, 3)) if scale is None else np.array(scale, np.float64)
    for i in range(len(r)):
        c = cam[i]; Jc = J[i, :, :6]
        S[6 * c:6 * c + 6, 6 * c:6 * c + 6] += rho1[i] * Jc.T @ Jc
        gc[6 * c:6 * c + 6] += rho1[i] * Jc.T @ r[i]
        Ud[c] += rho1[i] * (Jc * Jc).sum(0)
    g = gc.copy()
    gmax = 0.0
    for p in range(M):
        V = np.zeros((3, 3)); W = np.zeros((6 * F, 3))
        for i in range(off[p], off[p + 1]):
            Jp = J[i, :, 6:]; c = cam[i]
            V += rho1[i] * Jp.T @ Jp; gp[p] += rho1[i] * Jp.T @ r[i]
            W[6 * c:6 * c + 6] += rho1[i] * J[i, :, :6].T @ Jp
        if scale is None:
            sc[p] = 1.0 / (1.0 + np.sqrt(np.diag(V)))
        if frozen is not None and frozen[p]:
            continue
        gmax = max(gmax, float(np.abs(gp[p]).max()))
        lam = np.clip(np.diag(V) * sc[p] ** 2, min_diag, max_diag) / (radius * sc[p] ** 2)
        Vinv[p] = np.linalg.inv(V + np.diag(lam))
        S -= W @ Vinv[p] @ W.T
        g -= W @ Vinv[p] @ gp[p]
    return dict(S=S, g=g, cost=float(half.sum()), Udiag=Ud, gcam=gc, Vinv=Vinv, gp=gp, scale=sc, gmax=gmax)


def step_reference2(ref, r, J, off, cam, X, dcam, loss, a, frozen=None):
    """Back-substitution of the points for camera steps dcam (F x 6): (candidate points, [model decrease, |dX|^2, |X|^2 of free points])."""
    rho1, _ = huber_block(r, loss, a)
    Xc = X.copy(); model = 0.0; dx2 = 0.0; x2 = 0.0
    for p in range(len(off) - 1):
        b = ref["gp"][p].copy()
        for i in range(off[p], off[p + 1]):
            b += rho1[i] * J[i, :, 6:].T @ (J[i, :, :6] @ dcam[cam[i]])
        dp = -ref["Vinv"][p] @ b
        for i in range(off[p], off[p + 1]):
            d = J[i, :, :6] @ dcam[cam[i]] + J[i, :, 6:] @ dp
            model -= rho1[i] * (r[i] @ d + 0.5 * d @ d)
        Xc[p] = X[p] + dp; dx2 += dp @ dp
        if frozen is None or not frozen[p]:
            x2 += X[p] @ X[p]
    return Xc, np.array([model, dx2, x2])


def random_bundle2(rng, kind, rows=960, cols=1920, n_cams=5, n_points=30, noise_px=0.5, outliers=0.1, seam=0.2):
    """synth.random_bundle's geometry with two-row observations: keypoint pixels (PIXEL) or sphere angles in (-pi, pi] before the
    2Angle constructor's wrap (ANGLE2).  A share `seam` of the points sits near the lon = +-pi seam of some camera; `outliers` of the
    observations move by 40 px (outside Huber's inner region).  Returns dict(aa, t, X, off, cam, obs)."""
    b = synth.random_bundle(rng, n_cams=n_cams, n_points=n_points, noise=0.0, outliers=0.0)
    tab = synth.pose_table(b["aa"], b["t"])
    M = len(b["off"]) - 1
    # move some points behind a camera of their track (lon near +-pi)
    X = b["X"].copy()
    for p in range(M):
        if b["off"][p + 1] > b["off"][p] and rng.uniform() < seam:
            c = b["cam"][b["off"][p]]
            R = tab[c, :9].reshape(3, 3); tc = tab[c, 18:]
            pc = np.array([rng.uniform(-1e-3, 1e-3), rng.uniform(-1, 1), -rng.uniform(2, 5)])
            X[p] = R.T @ (pc - tc)
    pt = np.repeat(np.arange(M), np.diff(b["off"]))
    px = project(PIXEL, tab[b["cam"]], X[pt], rows, cols)
    px += rng.normal(size=px.shape) * noise_px
    bad = rng.uniform(size=len(px)) < outliers
    px[bad] += rng.choice([-40.0, 40.0], size=(bad.sum(), 2))
    if kind == PIXEL:
        obs = px
    else:   # eq.ImageToSphere in float (Equirectangular.h:99-105), widened to double
        p32 = px.astype(np.float32)
        sx = ((np.float32(2) * p32[:, 0] / np.float32(cols) - np.float32(1)).astype(np.float64) * np.pi).astype(np.float32)
        sy = ((0.5 - (p32[:, 1] / np.float32(rows)).astype(np.float64)) * np.pi).astype(np.float32)
        obs = np.stack([sx, sy], 1).astype(np.float64)
    Xp = X + rng.normal(size=X.shape) * 0.02
    return dict(aa=b["aa"], t=b["t"], X=Xp, off=b["off"], cam=b["cam"], obs=obs, rows=rows, cols=cols)


# ---- track filters -----------------------------------------------------------------------------------------------------------------
def fast_atan2(y, x):
    """FastAtan2 (base/Math.h:15-29) in double, operation by operation."""
    ax = np.abs(x); ay = np.abs(y)
    mn = np.minimum(ax, ay); mx = np.maximum(ax, ay)
    a = mn / (mx + EPS)
    s = a * a
    r = ((-0.04432655554792128 * s + 0.1555786518463281) * s - 0.3258083974640975) * s * a + 0.9997878412794807 * a
    r = np.where(ay > ax, 1.57079632679489661923 - r, r)
    r = np.where(x < 0, 3.14159265358979323846 - r, r)
    return np.where(y < 0, -r, r)


def image_to_cam_point2i(rows, cols, kp):
    """eq.ImageToCam(kp.pt) through the cv::Point2i overload: round half to even, un-project in float (sin / cos in double)."""
    kp = np.asarray(kp, np.float32)
    px = np.rint(kp[:, 0]).astype(np.float32); py = np.rint(kp[:, 1]).astype(np.float32)
    sx = ((np.float32(2) * px / np.float32(cols) - np.float32(1)).astype(np.float64) * np.pi).astype(np.float32)
    sy = ((0.5 - (py / np.float32(rows)).astype(np.float64)) * np.pi).astype(np.float32)
    cy = np.cos(sy.astype(np.float64)).astype(np.float32)
    return np.stack([np.float32(1) * cy * np.sin(sx.astype(np.float64)).astype(np.float32),
                     np.float32(-1) * np.sin(sy.astype(np.float64)).astype(np.float32),
                     np.float32(1) * cy * np.cos(sx.astype(np.float64)).astype(np.float32)], 1)


def filter_threshold(mode, threshold):
    """The per-mode threshold the core compares with: threshold^2 (pixel; +inf when threshold < 0: nothing is filtered) or
    cos(threshold pi / 180) (angle)."""
    if mode == 0:
        return np.inf if threshold < 0 else threshold * threshold
    return float(np.cos(threshold * np.pi / 180.0))


def filter_ref(mode, rows, cols, off, frame_ids, kp, X, T_cw, thr):
    """keep mask (uint8) of the tracks; thr as filter_threshold gives it.  T_cw: frames x 3 x 4 (zeros = invalid frame)."""
    off = np.asarray(off, np.int64); fid = np.asarray(frame_ids); kp = np.asarray(kp, np.float32); X = np.asarray(X, np.float64)
    T = np.asarray(T_cw, np.float64).reshape(-1, 3, 4)
    n = len(off) - 1
    pt = np.repeat(np.arange(n), np.diff(off))
    Tn = T[fid]; Xo = X[pt]
    p = [Tn[:, r, 0] * Xo[:, 0] + Tn[:, r, 1] * Xo[:, 1] + Tn[:, r, 2] * Xo[:, 2] + Tn[:, r, 3] for r in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == 0:
            lon = fast_atan2(p[0], p[2]); lat = -fast_atan2(p[1], np.sqrt(p[0] * p[0] + p[2] * p[2]))
            u = cols * (0.5 + lon / (2.0 * np.pi)); v = rows * (0.5 - lat / np.pi)
            dx = kp[:, 0].astype(np.float64) - u; dy = kp[:, 1].astype(np.float64) - v
            reject = (dx * dx + dy * dy) > thr
        else:
            ray = image_to_cam_point2i(rows, cols, kp).astype(np.float64)
            dot = p[0] * ray[:, 0] + p[1] * ray[:, 1] + p[2] * ray[:, 2]
            npn = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
            nr = np.sqrt(ray[:, 0] * ray[:, 0] + ray[:, 1] * ray[:, 1] + ray[:, 2] * ray[:, 2])
            reject = (dot / npn / nr) < thr
    bad = np.zeros(n, bool)
    np.logical_or.at(bad, pt, reject)
    return (~bad).astype(np.uint8)


def rigid_inverse_3x4(R_wc, t_wc):
    """T_cw = [R^T | -R^T t] of a camera-to-world pose (the mirror's rigid inverse), 3 x 4."""
    R = np.asarray(R_wc, np.float64); t = np.asarray(t_wc, np.float64)
    return np.concatenate([R.T, (-R.T @ t)[:, None]], 1)


# ---- scenes for the host mirror's driver (tests/cpp/pvlm_sfm_driver.cpp) -----------------------------------------------------------
def rot(aa):
    return synth.pose_table(np.asarray(aa, np.float64)[None], np.zeros((1, 3)))[0, :9].reshape(3, 3)


def trajectory_scene(rng, n_frames=60, n_tracks=20000, rows=960, cols=1920, noise_px=0.5, outlier_obs=0.05, min_track=3, max_track=6,
                     rot_noise=np.deg2rad(1.5), trans_noise=0.1, outlier_tracks=0, outlier_px=80.0, seam_margin=0.3):
    """Panoramas on a gently curving trajectory and triangulated tracks seen by windows of consecutive frames.  Returns dict with the true
    poses (R_wc, t_wc), the perturbed starting poses (frame 0 exact), keypoints per frame (float32), tracks (list of (frame, kp) lists),
    true and perturbed points, and the indices of the planted outlier tracks (one observation moved by outlier_px).  No observation lies
    within seam_margin rad of the lon = +-pi seam: the pixel residual and the pixel filter jump by `cols` there (upstream's trap, kept), so a
    track next to the seam may be dropped whatever its noise."""
    R_true, t_true = [], []
    for i in range(n_frames):
        R_true.append(rot([0.0, 0.02 * i, 0.0]) @ rot(rng.normal(size=3) * 0.02))
        t_true.append(np.array([0.4 * i, 0.0, 0.1 * np.sin(0.2 * i)]))
    kps = [[] for _ in range(n_frames)]
    tracks, X_true = [], []
    for tr in range(n_tracks):
        k = int(rng.integers(min_track, max_track + 1))
        f0 = int(rng.integers(0, max(n_frames - k, 1)))
        fs = list(range(f0, min(f0 + k, n_frames)))
        c = t_true[fs[len(fs) // 2]]
        while True:
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            X = c + d * rng.uniform(3.0, 12.0)
            ps = [R_true[f].T @ (X - t_true[f]) for f in fs]
            if abs(d[1]) < 0.9 and all(abs(np.arctan2(p[0], p[2])) < np.pi - seam_margin for p in ps):
                break
        X_true.append(X)
        obs = []
        for f in fs:
            p = R_true[f].T @ (X - t_true[f])
            lon = np.arctan2(p[0], p[2]); lat = -np.arcsin(p[1] / np.linalg.norm(p))
            u = np.array([cols * (0.5 + lon / (2 * np.pi)), rows * (0.5 - lat / np.pi)]) + rng.normal(size=2) * noise_px
            if rng.uniform() < outlier_obs:
                u += rng.normal(size=2) * 20.0
            obs.append([f, len(kps[f])]); kps[f].append(u)
        tracks.append(obs)
    planted = np.sort(rng.choice(n_tracks, size=outlier_tracks, replace=False)) if outlier_tracks else np.zeros(0, np.int64)
    for tr in planted:
        f, k = tracks[tr][len(tracks[tr]) // 2]
        ang = rng.uniform(0, 2 * np.pi)
        kps[f][k] = kps[f][k] + outlier_px * np.array([np.cos(ang), np.sin(ang)])
    R0 = [R_true[0]] + [R_true[i] @ rot(rng.normal(size=3) * rot_noise) for i in range(1, n_frames)]
    t0 = [t_true[0]] + [t_true[i] + rng.normal(size=3) * trans_noise for i in range(1, n_frames)]
    X_true = np.array(X_true)
    X0 = X_true + rng.normal(size=X_true.shape) * 0.02
    return dict(rows=rows, cols=cols, R_true=np.array(R_true), t_true=np.array(t_true), R0=np.array(R0), t0=np.array(t0),
                kps=[np.array(k, np.float32).reshape(-1, 2) for k in kps], tracks=tracks, X_true=X_true, X0=X0, planted=planted)


def write_scene(path, sc, lidars=None, valid=None):
    """The driver's input file (layout in tests/cpp/pvlm_sfm_driver.cpp).  lidars: list of (R_wl, t_wl)."""
    F = len(sc["R0"]); lidars = lidars or []
    with open(path, "wb") as f:
        f.write(np.array([F, sc["rows"], sc["cols"], len(sc["tracks"]), len(lidars)], np.int32).tobytes())
        for i in range(F):
            f.write(np.array([1 if valid is None else int(valid[i])], np.int32).tobytes())
            f.write(np.asarray(sc["R0"][i], np.float64).tobytes()); f.write(np.asarray(sc["t0"][i], np.float64).tobytes())
            f.write(np.array([len(sc["kps"][i])], np.int32).tobytes()); f.write(np.ascontiguousarray(sc["kps"][i], np.float32).tobytes())
        for t, obs in enumerate(sc["tracks"]):
            f.write(np.array([len(obs)], np.int32).tobytes()); f.write(np.array(obs, np.uint32).tobytes())
            f.write(np.asarray(sc["X0"][t], np.float64).tobytes())
        for R, t in lidars:
            f.write(np.asarray(R, np.float64).tobytes()); f.write(np.asarray(t, np.float64).tobytes())


def read_result(path, n_frames, n_lidars=0):
    b = open(path, "rb").read()
    o = 0
    ok = int(np.frombuffer(b, np.int32, 1, o)[0]); o += 4
    costs = np.frombuffer(b, np.float64, 2, o); o += 16
    steps = np.frombuffer(b, np.int32, 3, o); o += 12
    poses = np.frombuffer(b, np.float64, 12 * n_frames, o).reshape(n_frames, 12); o += 96 * n_frames
    nt = int(np.frombuffer(b, np.int32, 1, o)[0]); o += 4
    rec = np.frombuffer(b, np.dtype([("id", np.uint32), ("X", np.float64, 3)]), nt, o); o += 28 * nt
    lid = np.frombuffer(b, np.float64, 12 * n_lidars, o).reshape(n_lidars, 12)
    return dict(ok=ok, initial_cost=costs[0], final_cost=costs[1], steps=int(steps[0]), unsuccessful=int(steps[1]), blocks=int(steps[2]), R=poses[:, :9].reshape(-1, 3, 3),
                t=poses[:, 9:].copy(), ids=rec["id"].astype(np.int64), X=rec["X"].copy(), lidar_R=lid[:, :9].reshape(-1, 3, 3), lidar_t=lid[:, 9:].copy(), raw=b)


# ---- CPU LM twin of SfMGlobalBA with the two-row functors ----------------------------------------------------------------------------
def sphere_of_keypoints(kp, rows, cols):
    """eq.ImageToSphere(kp.pt) in float (Equirectangular.h:99-105), widened to double: what AddCameraResidual hands _2Angle."""
    p32 = np.asarray(kp, np.float32).reshape(-1, 2)
    sx = ((np.float32(2) * p32[:, 0] / np.float32(cols) - np.float32(1)).astype(np.float64) * np.pi).astype(np.float32)
    sy = ((0.5 - (p32[:, 1] / np.float32(rows)).astype(np.float64)) * np.pi).astype(np.float32)
    return np.stack([sx, sy], 1).astype(np.float64)


def scene_groups(sc, kind_of_track):
    """Reprojection groups of a trajectory scene as AddCameraResidual builds them: kind_of_track(t) -> PIXEL (HuberLoss(4.0)) or ANGLE2
    (HuberLoss(4 deg)); one group per kind, observations in (frame, keypoint) order per track."""
    groups = {}
    for ti, obs in enumerate(sc["tracks"]):
        k = kind_of_track(ti)
        g = groups.setdefault(k, dict(kind=k, cam=[], pt=[], obs=[], w=1.0, a=4.0 if k == PIXEL else 4.0 * np.pi / 180.0, rows=sc["rows"], cols=sc["cols"]))
        for f, kp in sorted(tuple(o) for o in obs):
            g["cam"].append(f); g["pt"].append(ti); g["obs"].append(sc["kps"][f][kp])
    out = []
    for g in groups.values():
        g["cam"] = np.array(g["cam"]); g["pt"] = np.array(g["pt"]); kp = np.array(g["obs"], np.float32)
        g["obs"] = kp.astype(np.float64) if g["kind"] == PIXEL else sphere_of_keypoints(kp, g["rows"], g["cols"])
        out.append(g)
    return out


def lm_twin_solve(groups, aa, t, X, const_poses, opt):
    """tests/lm_twin.py's trust-region policy (dense full system: pose and point columns) for two-row reprojection groups with the loss
    on each block's squared norm.  aa, t (F x 3) and X (M x 3) are updated in place.  Returns dict(initial_cost, final_cost, successful,
    unsuccessful, message, outer_blocks_at_start)."""
    F, M = aa.shape[0], X.shape[0]
    used = sorted(set(np.concatenate([g["cam"] for g in groups]).tolist()))
    free = [p for p in used if p not in const_poses]
    col = {p: 6 * i for i, p in enumerate(free)}
    n_pose = 6 * len(free)
    n = n_pose + 3 * M

    def evaluate(a_, t_, X_):
        H = np.zeros((n, n)); g = np.zeros(n); cost = 0.0; outer = 0
        for gr in groups:
            r, J = eval_jet(gr["kind"], a_[gr["cam"]], t_[gr["cam"]], X_[gr["pt"]], gr["obs"], gr["w"], gr["rows"], gr["cols"])
            w, half = huber_block(r, 1, gr["a"])
            cost += half.sum(); outer += int((w < 1).sum())
            for i in range(len(r)):
                cols = []
                c = col.get(int(gr["cam"][i]))
                if c is not None:
                    cols.append((c, J[i, :, :6]))
                cols.append((n_pose + 3 * int(gr["pt"][i]), J[i, :, 6:]))
                for ci, Ji in cols:
                    g[ci:ci + Ji.shape[1]] += w[i] * Ji.T @ r[i]
                    for cj, Jj in cols:
                        H[ci:ci + Ji.shape[1], cj:cj + Jj.shape[1]] += w[i] * Ji.T @ Jj
        return cost, H, g, outer

    x_aa, x_t, x_X = aa.copy(), t.copy(), X.copy()
    cost, H, g, outer0 = evaluate(x_aa, x_t, x_X)
    out = dict(initial_cost=cost, successful=1, unsuccessful=0, message="", outer_blocks_at_start=outer0)
    scale = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(H), 0.0)))
    radius, dec = opt.initial_radius, 2.0
    it = 0
    if np.abs(g).max() <= opt.gradient_tolerance:
        out["message"] = "gradient tolerance reached"
    while not out["message"] and it < opt.max_num_iterations:
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
            c_aa, c_t = x_aa.copy(), x_t.copy()
            for p in free:
                c_aa[p] += step[col[p]:col[p] + 3]; c_t[p] += step[col[p] + 3:col[p] + 6]
            c_X = x_X + step[n_pose:].reshape(M, 3)
            c_cost, cH, cg, _ = evaluate(c_aa, c_t, c_X)
            rho = (cost - c_cost) / model
            if np.isfinite(c_cost) and rho > opt.min_relative_decrease:
                accepted = True
                xn = np.sqrt(sum((x_aa[p] ** 2).sum() + (x_t[p] ** 2).sum() for p in free) + (x_X ** 2).sum())
                change = cost - c_cost
                prev = cost
                x_aa, x_t, x_X, cost, H, g = c_aa, c_t, c_X, c_cost, cH, cg
                radius = min(opt.max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                dec = 2.0
                out["successful"] += 1
                if abs(change) <= opt.function_tolerance * prev:
                    out["message"] = "function tolerance reached"
                elif np.abs(g).max() <= opt.gradient_tolerance:
                    out["message"] = "gradient tolerance reached"
                elif np.linalg.norm(step) <= opt.parameter_tolerance * (xn + opt.parameter_tolerance):
                    out["message"] = "parameter tolerance reached"
        if not accepted:
            out["unsuccessful"] += 1
            radius /= dec
            dec *= 2.0
            if radius < opt.min_radius:
                out["message"] = "trust region collapsed"
    aa[:] = x_aa; t[:] = x_t; X[:] = x_X
    out["final_cost"] = cost
    return out
