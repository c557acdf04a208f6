"""The coloured LiDAR map without a GPU: K30's per-point statement (csrc/pvlm_texture_core.h, compiled for the host by tests/cpp/texture_core_check.cpp)
against the numpy restatement of Texture::ColorizeLidarPointCloud's loop body and OpenCV's 8-bit HSV (tests/colorize_ref.py) bit for bit, the recalled HSV
against its rational definition, the XYZRGB PCD writer byte for byte and Texture's two deliberate divergences."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from tests import colorize_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("texture_core") / "texture_core_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "texture_core_check.cpp")])
    return ctypes.CDLL(out)


def P(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def core_hsv(lib, bgr):
    bgr = np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3)
    hsv = np.zeros_like(bgr)
    lib.chk_hsv(P(bgr, ctypes.c_ubyte), ctypes.c_longlong(len(bgr)), P(hsv, ctypes.c_ubyte))
    return hsv


def core_colorize(lib, pts, T12, image, min_dist, max_dist):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3); T = np.ascontiguousarray(T12, np.float64).reshape(12)
    image = np.ascontiguousarray(image, np.uint8)
    rows, cols = image.shape[:2]
    n = len(pts)
    px = np.zeros(n, np.int32); py = np.zeros(n, np.int32); hit = np.zeros(n, np.uint8); word = np.zeros(n, np.uint32)
    lib.chk_colorize(P(pts, ctypes.c_float), ctypes.c_longlong(n), P(T, ctypes.c_double), P(image, ctypes.c_ubyte), ctypes.c_int(rows), ctypes.c_int(cols),
                     ctypes.c_double(min_dist), ctypes.c_double(max_dist), P(px, ctypes.c_int), P(py, ctypes.c_int), P(hit, ctypes.c_ubyte), P(word, ctypes.c_uint))
    return hit.astype(bool), px.astype(np.int64), py.astype(np.int64), word


def all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(c & 255), (c >> 8) & 255, (c >> 16) & 255], axis=1).astype(np.uint8)


def test_hsv_of_every_colour_matches_numpy_and_the_rational_definition(chk):
    bgr = all_colours()
    got = core_hsv(chk, bgr).astype(np.int64)
    want = cr.hsv_u8(bgr)
    assert np.array_equal(got, want)
    # the recall against the definition: V = max, S = 255 diff / V, H = the hue in 0..180 units (degrees / 2), each within one step of rounding
    b, g, r = (bgr[:, k].astype(np.float64) for k in range(3))
    v = np.maximum(np.maximum(b, g), r); mn = np.minimum(np.minimum(b, g), r); d = v - mn
    assert np.array_equal(got[:, 2], v.astype(np.int64))
    with np.errstate(invalid="ignore", divide="ignore"):
        s_exact = np.where(v > 0, 255.0 * d / v, 0.0)
        h = np.where(v == r, (g - b) / d, np.where(v == g, 2.0 + (b - r) / d, 4.0 + (r - g) / d)) * 30.0
    h = np.where(d > 0, np.where(h < 0, h + 180.0, h), 0.0)
    assert np.abs(got[:, 1] - s_exact).max() <= 1.0
    dh = np.abs(got[:, 0] - h)
    dh = np.minimum(dh, 180.0 - dh)                       # 179.6 rounds to 180 = 0 around the circle
    assert dh.max() <= 1.0
    assert got[:, 0].max() <= 179
    sky = cr.is_sky(got)
    print("colours inside the sky box: %d of %d" % (int(sky.sum()), len(sky)))
    assert 0 < sky.sum() < len(sky)


def _hsv_edges():
    """BGR colours whose HSV sits on each edge of the sky box (h 99/100/124/125, s 42/43/200/201, v 149/150), found in the full table."""
    bgr = all_colours()
    hsv = cr.hsv_u8(bgr)
    picks = {}
    base = (hsv[:, 0] >= 100) & (hsv[:, 0] <= 124) & (hsv[:, 1] >= 43) & (hsv[:, 1] <= 200) & (hsv[:, 2] >= 150)
    for c, vals in ((0, (99, 100, 124, 125)), (1, (42, 43, 200, 201)), (2, (149, 150, 255))):
        others = np.ones(len(hsv), bool)
        for o, (lo, hi) in enumerate(cr.SKY):
            if o != c:
                others &= (hsv[:, o] >= lo) & (hsv[:, o] <= hi)
        for val in vals:
            idx = np.flatnonzero(others & (hsv[:, c] == val))
            assert len(idx), (c, val)
            picks[(c, val)] = idx[len(idx) // 2]
    return bgr, hsv, picks, base


def test_sky_box_edges(chk):
    bgr, hsv, picks, _ = _hsv_edges()
    idx = np.array(list(picks.values()))
    word = cr.colour_word(bgr[idx])
    inside = {(0, 100), (0, 124), (1, 43), (1, 200), (2, 150), (2, 255)}
    for (c, val), w in zip(picks.keys(), word):
        assert (w == 0) == ((c, val) in inside), (c, val, hsv[picks[(c, val)]])
    assert np.array_equal(core_hsv(chk, bgr[idx]).astype(np.int64), hsv[idx])


def planted_points():
    """Points that pin each quirk of the statement (rows: x, y, z)."""
    f = np.float32
    pts = []
    for r in (1.5, 35.0):                                        # 0-11: distances exactly at 1.5^2 and 35^2 after float rounding, one ulp either side
        z = f(r)
        for zz in (np.nextafter(z, f(0)), z, np.nextafter(z, f(np.inf))):
            pts.append([0, 0, zz]); pts.append([0, 0, -zz])
    pts += [[np.nan, 1, 2], [1, np.nan, 2], [0, 0, np.nan], [np.inf, 0, 0], [0, -np.inf, 3], [np.nan, np.nan, np.nan]]   # 12-17
    pts += [[0, 5, 0], [0, -5, 0], [0, 0, -10], [-0.0, 0, -10], [0, 20, 1e-30], [1e-30, -20, 0]]   # 18-23: the poles, lon = pi (x = cols)
    return np.array(pts, np.float32)


def _pose(rotvec, t):
    T = np.eye(4); T[:3, :3] = Rotation.from_rotvec(rotvec).as_matrix(); T[:3, 3] = t
    return T


@pytest.mark.parametrize("shape", [(10, 21), (720, 1440), (33, 64)])
def test_per_point_statement_matches_numpy_bit_for_bit(chk, shape):
    rows, cols = shape
    rng = np.random.default_rng(30 + rows)
    image = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    bgr, hsv, picks, base = _hsv_edges()
    sky = bgr[np.flatnonzero(base)[:: 997]]
    mask = rng.random((rows, cols)) < 0.33                        # sky-box colours at a third of the pixels
    image[mask] = sky[rng.integers(0, len(sky), int(mask.sum()))]
    image[:, -1] = image[-1, :] = (10, 200, 30)                  # the last row and column: kept colours
    sp = planted_points()
    # points aimed at the last column and the last row (pixel centres) and at the image's corners
    lon = 2 * np.pi * ((np.array([cols - 1.0, cols - 1.0, 0.0, 0.3])) / cols - 0.5)
    lat = np.pi * (0.5 - np.array([rows - 1.0, 0.0, rows - 1.0, rows - 0.7]) / rows)
    aim = np.stack([10 * np.cos(lat) * np.sin(lon), -10 * np.sin(lat), 10 * np.cos(lat) * np.cos(lon)], axis=1).astype(np.float32)
    rnd = rng.normal(0, 15, (20000, 3)).astype(np.float32)
    pts = np.concatenate([sp, aim, rnd])
    poses = [np.eye(4), _pose([0.3, -2.0, 0.9], [1.25, -3.5, 0.75]), _pose([2.5, 0.1, -0.4], [250.0, -1e3, 33.0])]
    kept_any = 0
    for T in poses:
        T12 = T[:3].reshape(12)
        for min_d, max_d in ((1.5, 35.0), (0.0, 1000.0), (0.0, np.inf), (np.nan, 35.0)):
            hit, px, py, word = core_colorize(chk, pts, T12, image, min_d, max_d)
            want_hit, wpx, wpy = cr.project(pts, T12, rows, cols, min_d, max_d)
            assert np.array_equal(px, wpx) and np.array_equal(py, wpy)
            assert np.array_equal(hit, want_hit)
            rec = cr.colorize_pair(pts, T12, image, min_d, max_d)
            assert cr.same(np.concatenate([pts[word != 0], word[word != 0].view(np.float32)[:, None]], axis=1), rec)
            kept_any += len(rec)
    assert kept_any > 0
    # the quirks under the identity pose, 1.5 .. 35
    hit, px, py, word = core_colorize(chk, pts, np.eye(4)[:3].reshape(12), image, 1.5, 35.0)
    assert cr.in_range(pts[:12], 1.5, 35.0).tolist() == [False, False, True, True, True, True, True, True, True, True, False, False]
    assert hit[0:12:2].tolist() == [False, True, True, True, True, False]      # +z: the distance decides
    assert not hit[1:12:2].any() and (px[1:12:2] == cols).all()              # -z: lon = pi, u = cols
    for k in range(12, 18):                                       # NaN / inf: dropped, never coloured from pixel (0, 0)
        assert not hit[k] and word[k] == 0
    assert px[12] == cr.INT_MIN and py[12] == cr.INT_MIN          # a NaN pixel is INT_MIN, as the x86-64 conversion gives, not 0
    assert py[18] == rows and not hit[18]                         # (0, 5, 0): lat = -pi/2, v = rows: dropped
    assert py[19] == 0 and hit[19]                                # (0, -5, 0): the top row
    assert px[20] == cols and px[21] == cols and not hit[20] and not hit[21]   # lon = pi: u = cols rounds to cols, dropped, not wrapped
    a = len(sp)
    assert px[a] == cols - 1 and py[a] == rows - 1 and hit[a]     # the last column and row
    assert px[a + 1] == cols - 1 and py[a + 1] == 0 and hit[a + 1]
    assert px[a + 2] == 0 and py[a + 2] == rows - 1 and hit[a + 2]
    assert py[a + 3] == rows - 1 and hit[a + 3]                   # v = rows - 0.7 rounds down into the last row


def test_round_and_is_inside(chk):
    """int(std::round(v)): half away from zero; NaN / inf / out of int's range -> INT_MIN.  IsInside(Point2i): x + 1 <= cols, y + 1 <= rows."""
    v = np.array([-0.5, -0.49, 0.49, 0.5, 1.5, 2.5, -1.5, np.nan, np.inf, -np.inf, 3e9, -3e9, 2147483647.4, -2147483648.4, 5759.5, 5759.49], np.float64)
    want = [-1, 0, 0, 1, 2, 3, -2, cr.INT_MIN, cr.INT_MIN, cr.INT_MIN, cr.INT_MIN, cr.INT_MIN, 2147483647, -2147483648, 5760, 5759]
    out = np.zeros(len(v), np.int32)
    chk.chk_round(P(v, ctypes.c_double), ctypes.c_longlong(len(v)), P(out, ctypes.c_int))
    assert out.tolist() == want and cr.round_to_int(v).tolist() == want
    rows, cols = 2880, 5760
    xy = np.array([[-1, 0], [0, 0], [cols - 1, rows - 1], [cols, 0], [0, rows], [0, -1], [cr.INT_MIN, cr.INT_MIN], [2147483647, 0], [5759, 2879]], np.int32)
    x, y = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
    ins = np.zeros(len(xy), np.uint8)
    chk.chk_inside(P(x, ctypes.c_int), P(y, ctypes.c_int), ctypes.c_longlong(len(xy)), ctypes.c_int(rows), ctypes.c_int(cols), P(ins, ctypes.c_ubyte))
    assert ins.astype(bool).tolist() == [False, True, True, False, False, False, False, False, True]


def test_exact_distance_bounds(chk):
    """The distance is (x*x + y*y) + z*z in float, compared in double against min^2 / max^2: exactly 1.5^2 and 35^2 kept, one float ulp beyond dropped."""
    f = np.float32
    pts, want = [], []
    for r, inside in ((1.5, (False, True, True)), (35.0, (True, True, False))):
        z = f(r)
        for zz, w in zip((np.nextafter(z, f(0)), z, np.nextafter(z, f(np.inf))), inside):
            pts.append([0, 0, zz]); want.append(w)
    pts = np.array(pts, np.float32)
    assert cr.in_range(pts, 1.5, 35.0).tolist() == want
    image = np.full((8, 16, 3), 40, np.uint8)
    hit, _, _, word = core_colorize(chk, pts, np.eye(4)[:3].reshape(12), image, 1.5, 35.0)
    assert hit.tolist() == want and ((word != 0) == np.array(want)).all()


def _driver():
    from panovlm_amd import build
    build.build_host()
    return build.TEXTURE_DRIVER


def test_pcd_writer_xyzrgb_byte_for_byte(tmp_path):
    rng = np.random.default_rng(7)
    n = 3000
    rec = np.zeros((n, 4), np.float32)
    rec[:, :3] = rng.normal(0, 10, (n, 3))
    bgr = rng.integers(0, 256, (n, 3), dtype=np.uint32)
    rec[:, 3] = (bgr[:, 0] | (bgr[:, 1] << 8) | (bgr[:, 2] << 16) | np.uint32(255 << 24)).astype(np.uint32).view(np.float32)
    src, pcd = str(tmp_path / "rec.bin"), str(tmp_path / "map.pcd")
    with open(src, "wb") as f:
        f.write(np.int64(n).tobytes()); f.write(rec.tobytes())
    out = subprocess.run([_driver(), "savepcd", src, pcd], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["saved", "1"], out.stderr
    raw = open(pcd, "rb").read()
    assert raw == cr.pcd_bytes(rec)
    body = np.frombuffer(raw[-16 * n:], np.uint8).reshape(n, 16)
    assert np.array_equal(body[:, 12:15], bgr.astype(np.uint8)) and (body[:, 15] == 255).all()   # bytes b g r 255
    with open(src, "wb") as f:
        f.write(np.int64(0).tobytes())
    out = subprocess.run([_driver(), "savepcd", src, str(tmp_path / "empty.pcd")], capture_output=True, text=True, timeout=120)
    assert out.stdout.split() == ["saved", "0"] and not os.path.exists(str(tmp_path / "empty.pcd"))


def test_the_two_divergences_throw():
    """Upstream asserts lidars.size() == frames.size() and skip >= 0; the mirror throws std::invalid_argument before it touches a scan (no device needed)."""
    out = subprocess.run([_driver(), "diverge"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["size_mismatch_throws", "1", "negative_skip_throws", "1"]
