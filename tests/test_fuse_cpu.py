"""The fused LiDAR map without a GPU: K29's per-point statement (csrc/pvlm_fuse_core.h, compiled for the host by tests/cpp/fuse_core_check.cpp) against the numpy
restatement of LidarOdometry::FuseLidar's loop body bit for bit — upstream's quirks included —, the PCD writer of the host mirror (SavePCDFileBinary) byte
for byte and through Velodyne::LoadLidar, and FuseLidar's one deliberate divergence (skip < 0 throws)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import fuse_ref, host_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def chk(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuse_core") / "fuse_core_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "fuse_core_check.cpp")])
    return ctypes.CDLL(out)


def core(lib, pts, T, min_range, max_range):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4); T = np.ascontiguousarray(T, np.float64).reshape(16)
    keep = np.zeros(len(pts), np.uint8); out = np.zeros((len(pts), 3), np.float32)
    P = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    lib.chk_fuse(P(pts, ctypes.c_float), ctypes.c_longlong(len(pts)), P(T, ctypes.c_double), ctypes.c_double(min_range), ctypes.c_double(max_range),
                 P(keep, ctypes.c_ubyte), P(out, ctypes.c_float))
    return keep.astype(bool), out


def special_points():
    """Points that pin each quirk of the range test (rows: x, y, z, intensity)."""
    nan, inf = np.nan, np.inf
    p = [
        [3, 0, 0, 1], [40, 0, 0, 2], [0, 0, 40, 3], [0, 3, 0, 4],              # exactly at 3^2 / 40^2; (0, 3, 0): y*y is not in the range at all
        [1, 30, -30, 5], [1, -30, 30, 6],                                      # y = -z: range = x^2, a far point kept by a small max
        [10, 2, 3, 7], [10, -2, 3, 8], [35, 25, 25, 9], [35, -25, 25, 10],     # the y*z term alone decides against max 40
        [nan, 1, 2, 11], [1, nan, 2, 12], [0, 0, nan, 13],                     # NaN range: kept, transformed to NaN
        [inf, 0, 0, 14], [0, 0, -inf, 15], [0, -1, inf, 16], [0, inf, -1, 17],  # inf ranges dropped (unless max is inf); (0, -1, inf): -inf + inf = NaN, kept
        [0, 5, -1, 18], [0, 7, -2, 19],                                        # negative ranges: dropped by min 0 (-4 < 0)
        [1e20, 0, 0, 20], [0, 2e19, 2e19, 21],                                 # float overflow to inf
        [1e-20, 0, 0, 22], [1.5e-20, 0, 0, 23], [0.7e-20, 0, 0, 24],          # subnormal ranges around min 1e-20
        [1e-22, 0, 0, 25], [3e-23, 1e-23, 2e-23, 26], [0, 0, 0, 27],
        [1e-19, -1e-19, 1e-19, 28], [2e-20, 3e-20, -1e-20, 29],
    ]
    return np.array(p, np.float32)


CASES = [(0.0, 40.0), (3.0, 40.0), (1e-20, 100.0), (1.2e-20, 1.0), (0.0, np.inf), (10.0, 5.0), (0.5, 0.5), (0.0, 0.0), (np.nan, 40.0), (-3.0, -40.0)]


def test_core_matches_numpy_bit_for_bit(chk):
    rng = np.random.default_rng(29)
    sp = special_points()
    rnd = np.concatenate([rng.normal(0, 25, (4000, 3)), rng.uniform(0, 255, (4000, 1))], axis=1).astype(np.float32)
    tiny = np.concatenate([rng.normal(0, 1, (1000, 3)) * 10.0 ** rng.uniform(-24, -18, (1000, 1)), np.ones((1000, 1))], axis=1).astype(np.float32)
    pts = np.concatenate([sp, rnd, tiny])
    ang = 2.5
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    poses = [np.eye(4), fuse_ref.pose4((Rz, [0.0, 0.0, 0.0])), fuse_ref.pose4((Rz @ Rz.T @ Rz, [1e6, -3e5, 12.5])), fuse_ref.pose4((np.eye(3), [1e-30, 0, 0]))]
    decided = {}
    for min_r, max_r in CASES:
        for T in poses:
            keep, out = core(chk, pts, T, min_r, max_r)
            want_keep = fuse_ref.keep_mask(pts, min_r, max_r)
            assert np.array_equal(keep, want_keep), (min_r, max_r)
            assert fuse_ref.same(np.concatenate([out, pts[:, 3:]], axis=1), fuse_ref.transform(pts, T)), (min_r, max_r)
        decided[(min_r, max_r)] = keep[:len(sp)]
    # rows of special_points(): 0 (3,0,0)  1 (40,0,0)  2 (0,0,40)  3 (0,3,0)  4 (1,30,-30)  5 (1,-30,30)  8 (35,25,25)  9 (35,-25,25)  10-12 NaN coordinates
    # 13 (inf,0,0)  14 (0,0,-inf)  15 (0,-1,inf)  16 (0,inf,-1)  17-18 negative ranges  19-20 float overflow  21-28 tiny / subnormal ranges
    k = decided[(0.0, 40.0)]
    assert k[1] and k[2] and k[4] and k[5] and k[3]                  # on the 40 m sphere: kept; y = -z keeps a point 42 m away; (0, 3, 0) has range 0
    assert not k[8] and k[9]                                          # (35, 25, 25): 35^2 + 2 * 625 > 1600; (35, -25, 25): range 35^2
    assert k[10] and k[11] and k[12]                                  # NaN ranges are kept ...
    assert k[14] and k[15]                                            # ... also those of 0 * -inf and -inf + inf
    assert not k[13] and not k[16] and not k[17] and not k[18] and not k[19] and not k[20]   # inf, -inf, negative, overflowed
    assert np.all(k[21:])                                             # min 0: every tiny range is >= 0
    k3 = decided[(3.0, 40.0)]
    assert k3[0] and not k3[3]                                        # exactly 3^2: kept; (0, 3, 0): range 0 < 9
    ki = decided[(0.0, np.inf)]
    assert ki[13] and ki[19] and ki[20] and not ki[16] and not ki[17]   # max inf keeps the inf ranges, not -inf or the negative ones
    assert np.flatnonzero(decided[(10.0, 5.0)]).tolist() == [10, 11, 12, 14, 15]   # min > max: only the NaN ranges survive
    assert np.flatnonzero(decided[(0.0, 0.0)]).tolist() == [3, 10, 11, 12, 14, 15, 26]
    # subnormal float ranges decide against min 1e-20 (1e-40 in double): a flush to zero would drop rows 22, 27 and 28
    ks = decided[(1e-20, 100.0)]
    assert ks[22] and ks[27] and ks[28] and not ks[21] and not ks[23] and not ks[26]
    kn = decided[(np.nan, 40.0)]
    assert kn[17] and kn[18] and kn[16] and not kn[13]                # NaN min: the lower comparison is always false
    assert np.array_equal(decided[(-3.0, -40.0)], k3)                 # the bounds enter squared

def test_pcd_writer_layout_and_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    n = 5000
    pts = np.concatenate([rng.normal(0, 8, (n, 3)), rng.uniform(0, 255, (n, 1))], axis=1).astype(np.float32)
    pts[10] = [0.1, 0.1, 0.1, 7.0]                                     # closer than 0.5 m: LoadLidar drops it
    pts[20] = [np.nan, 1.0, 2.0, 8.0]                                  # non-finite: LoadLidar drops it
    src, pcd = str(tmp_path / "cloud.bin"), str(tmp_path / "map.pcd")
    with open(src, "wb") as f:
        f.write(np.int64(n).tobytes()); f.write(pts.tobytes())
    out = fuse_ref.run("savepcd", src, pcd)
    assert out.stdout.split() == ["saved", "1"]
    lines, data = fuse_ref.read_pcd(pcd)
    assert tuple(lines[:6]) == fuse_ref.HEADER
    assert lines[6:] == ["WIDTH %d" % n, "HEIGHT 1", "VIEWPOINT 0 0 0 1 0 0 0", "POINTS %d" % n, "DATA binary"]
    assert data.tobytes() == pts.tobytes()
    raw = open(pcd, "rb").read()
    assert raw == ("\n".join(fuse_ref.HEADER + tuple(lines[6:])) + "\n").encode() + pts.tobytes()
    # the file is one Velodyne::LoadLidar reads: NaN / near points dropped, axes swapped (x, y, z) -> (x, -z, y)
    log = host_io.run("loadpcd", pcd)
    head = log[0].split()
    got = np.array([[float.fromhex(v) for v in l.split()[1:]] for l in log[1:] if l.startswith("p ")], np.float32).reshape(-1, 4)
    want = fuse_ref.load_lidar(pcd)
    assert int(head[1]) == 1 and int(head[5]) == len(want) == n - 2
    assert np.array_equal(got, want)


def test_pcd_writer_refuses_an_empty_cloud(tmp_path):
    src, pcd = str(tmp_path / "empty.bin"), str(tmp_path / "empty.pcd")
    with open(src, "wb") as f:
        f.write(np.int64(0).tobytes())
    out = fuse_ref.run("savepcd", src, pcd)
    assert out.stdout.split() == ["saved", "0"]
    assert not os.path.exists(pcd)


@pytest.mark.parametrize("which", ["odometry", "joint"])
def test_negative_skip_throws(tmp_path, which):
    """Upstream's `i += skip + 1` never ends for skip < 0; the mirror throws std::invalid_argument before it touches a scan (no device needed)."""
    scans = [dict(R=np.eye(3), t=np.zeros(3), cloud=np.ones((4, 4), np.float32))]
    fuse_ref.write_scans(str(tmp_path / "s.bin"), scans)
    out = fuse_ref.run("fuse", str(tmp_path / "s.bin"), str(tmp_path / "m.bin"), which, -1, 0.0, 40.0, check=False)
    assert out.returncode == 3 and "skip < 0" in out.stderr
    assert not os.path.exists(str(tmp_path / "m.bin"))
