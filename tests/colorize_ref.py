"""numpy restatement of the colour stage of Texture::ColorizeLidarPointCloud (mvs/Texture.cpp:46-76), of FuseCloud (:82-97), of OpenCV's 8-bit
cv::cvtColor(CV_BGR2HSV) (RGB2HSV_b, recalled from OpenCV's color_hsv sources: hsv_shift 12, the sdiv / hdiv180 tables) and of the XYZRGB PCD file —
what K30 (csrc/pvlm_texture.hip, per-point statement csrc/pvlm_texture_core.h) and the host mirror's Texture are compared with, bit for bit."""
import numpy as np

INT_MIN = -2147483648
SKY = ((100, 124), (43, 200), (150, 255))


def hsv_u8(bgr):
    """OpenCV's RGB2HSV_b (hrange 180) of an n x 3 uint8 BGR array -> n x 3 int64 (h, s, v)."""
    bgr = np.asarray(bgr, np.uint8).reshape(-1, 3).astype(np.int64)
    b, g, r = bgr[:, 0], bgr[:, 1], bgr[:, 2]
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    idx = np.arange(256, dtype=np.float64)
    with np.errstate(divide="ignore"):
        sdiv = np.where(idx > 0, np.rint((255 << 12) / idx), 0).astype(np.int64)
        hdiv = np.where(idx > 0, np.rint((180 << 12) / (6.0 * idx)), 0).astype(np.int64)
    vr = np.where(v == r, -1, 0)
    vg = np.where(v == g, -1, 0)
    s = (diff * sdiv[v] + (1 << 11)) >> 12
    h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + (~vg & (r - g + 4 * diff))))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return np.stack([h, s, v], axis=1)


def is_sky(hsv):
    hsv = np.asarray(hsv).reshape(-1, 3)
    ok = np.ones(len(hsv), bool)
    for c, (lo, hi) in enumerate(SKY):
        ok &= (hsv[:, c] >= lo) & (hsv[:, c] <= hi)
    return ok


def colour_word(bgr):
    """b | g << 8 | r << 16 | 255 << 24 as uint32, 0 where the pixel's HSV is sky."""
    bgr = np.asarray(bgr, np.uint8).reshape(-1, 3)
    w = bgr[:, 0].astype(np.uint32) | (bgr[:, 1].astype(np.uint32) << 8) | (bgr[:, 2].astype(np.uint32) << 16) | np.uint32(255 << 24)
    return np.where(is_sky(hsv_u8(bgr)), np.uint32(0), w).astype(np.uint32)


def in_range(xyz, min_dist, max_dist):
    xyz = np.asarray(xyz, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        xx, yy, zz = xyz[:, 0] * xyz[:, 0], xyz[:, 1] * xyz[:, 1], xyz[:, 2] * xyz[:, 2]
        d = ((xx + yy) + zz).astype(np.float64)
    sq_min, sq_max = float(min_dist) * float(min_dist), float(max_dist) * float(max_dist)
    return ~((d < sq_min) | (d > sq_max))


def to_camera(xyz, T12):
    T = np.asarray(T12, np.float64).reshape(-1)
    X, Y, Z = (np.asarray(xyz, np.float32)[:, k].astype(np.float64) for k in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        w = ((0.0 * X + 0.0 * Y) + 0.0 * Z) + 1.0
        return np.stack([(((T[4 * r] * X + T[4 * r + 1] * Y) + T[4 * r + 2] * Z) + T[4 * r + 3]) / w for r in range(3)], axis=1)


def fast_atan2(y, x):
    """FastAtan2<double> (base/Math.h:15-29)."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        mn = np.where(ay < ax, ay, ax); mx = np.where(ax < ay, ay, ax)
        a = mn / (mx + np.finfo(np.float64).eps)
        s = a * a
        r = ((-0.04432655554792128 * s + 0.1555786518463281) * s - 0.3258083974640975) * s * a + 0.9997878412794807 * a
        r = np.where(ay > ax, 1.57079632679489661923 - r, r)
        r = np.where(x < 0, 3.14159265358979323846 - r, r)
        return np.where(y < 0, -r, r)


def cam_to_image(p, rows, cols):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        lon = fast_atan2(x, z)
        lat = -fast_atan2(y, np.sqrt(x * x + z * z))
        return cols * (0.5 + lon / (2.0 * np.pi)), rows * (0.5 - lat / np.pi)


def round_to_int(v):
    """int(std::round(v)) on x86-64: half away from zero; NaN and values outside int become INT_MIN."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(v)
        r = np.where(np.abs(v - t) >= 0.5, t + np.sign(v), t)
        ok = (r >= -2147483648.0) & (r < 2147483648.0)
        return np.where(ok, np.nan_to_num(r), INT_MIN).astype(np.int64)


def project(xyz, T12, rows, cols, min_dist, max_dist):
    """(hit, px, py) per point: the range test, the transform, CamToImage, round and IsInside."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    keep = in_range(xyz, min_dist, max_dist)
    u, v = cam_to_image(to_camera(xyz, T12), rows, cols)
    px, py = round_to_int(u), round_to_int(v)
    inside = (px >= 0) & (py >= 0) & (px + 1 <= cols) & (py + 1 <= rows)
    return keep & inside, px, py


def colorize_pair(xyz, T12, image, min_dist, max_dist):
    """One pair: the kept records (m x 4 float32, the fourth the bits of the colour word) in point order."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz) == 0 or T12 is None:
        return np.zeros((0, 4), np.float32)
    image = np.asarray(image, np.uint8)
    rows, cols = image.shape[:2]
    hit, px, py = project(xyz, T12, rows, cols, min_dist, max_dist)
    word = np.zeros(len(xyz), np.uint32)
    word[hit] = colour_word(image[py[hit], px[hit]])
    keep = word != 0
    out = np.zeros((int(keep.sum()), 4), np.float32)
    out[:, :3] = xyz[keep]
    out[:, 3] = word[keep].view(np.float32)
    return out


def colorize(clouds, T_cls, images, min_dist, max_dist):
    """All pairs (T_cl None = a pair left out): records in pair order, per-pair counts."""
    parts = [colorize_pair(np.asarray(c, np.float32)[:, :3], T, im, min_dist, max_dist) for c, T, im in zip(clouds, T_cls, images)]
    per = np.array([len(p) for p in parts], np.int64)
    return (np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)), per


def same(a, b):
    """Bit-for-bit equality of record arrays (NaN never survives K30, so plain bytes)."""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def camera_from_lidar(R_wc, t_wc, T_wl):
    """T_cl = T_wc^-1 T_wl with the rigid inverse, rows 0..2 as 12 doubles — every sum in index order, as the host mirror forms it."""
    R = np.asarray(R_wc, np.float64).reshape(9); t = np.asarray(t_wc, np.float64).reshape(3); B = np.asarray(T_wl, np.float64).reshape(16)
    inv = np.zeros(16)
    for r in range(3):
        for c in range(3):
            inv[4 * r + c] = R[3 * c + r]
        inv[4 * r + 3] = -(((R[r] * t[0]) + R[3 + r] * t[1]) + R[6 + r] * t[2])
    inv[15] = 1.0
    T = np.zeros(12)
    for r in range(3):
        for c in range(4):
            acc = inv[4 * r] * B[c]
            for k in range(1, 4):
                acc = acc + inv[4 * r + k] * B[4 * k + c]
            T[4 * r + c] = acc
    return T


def fuse(colored, poses, skip):
    """Texture::FuseCloud: pairs 0, skip + 1, ... with a pose (None = invalid), float(((m0 x + m1 y) + m2 z) + m3) in double; the colour word kept."""
    out = []
    for i in range(0, len(colored), skip + 1):
        if poses[i] is None or len(colored[i]) == 0:
            continue
        T = np.asarray(poses[i], np.float64).reshape(-1)
        c = np.asarray(colored[i], np.float32)
        X, Y, Z = (c[:, k].astype(np.float64) for k in range(3))
        o = c.copy()
        for r in range(3):
            o[:, r] = ((((T[4 * r] * X + T[4 * r + 1] * Y) + T[4 * r + 2] * Z) + T[4 * r + 3])).astype(np.float32)
        out.append(o)
    return np.concatenate(out) if out else np.zeros((0, 4), np.float32)


def pcd_bytes(records):
    """pcl::io::savePCDFileBinary<pcl::PointXYZRGB> as recalled from PCL 1.x (not pinned)."""
    records = np.ascontiguousarray(records, np.float32)
    n = len(records)
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\n"
            "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA binary\n" % (n, n)).encode()
    return head + records.tobytes()
