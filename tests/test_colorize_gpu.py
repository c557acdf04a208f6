"""K30 (pvlm_colorize_scans / pvlm_colorize_scans_dev / pvlm_colorize_debug_hsv: the colour stage of Texture::ColorizeLidarPointCloud), Velodyne::SegmentBatch
and the host mirror's Texture end to end, against the numpy restatement (tests/colorize_ref.py) bit for bit."""
import struct
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import panovlm_amd as pv
from panovlm_amd import api
from panovlm_amd import synthetic as sy
from tests import colorize_ref as cr
from tests import fuse_ref
from tests import ring_cases

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 28800, 40000]


@pytest.fixture(scope="module")
def ctx():
    c = pv.Context()
    yield c
    c.close()


def _T(rotvec, t):
    T = np.eye(4); T[:3, :3] = Rotation.from_rotvec(rotvec).as_matrix(); T[:3, 3] = t
    return T


POSES = [np.eye(4), _T([0.3, -2.0, 0.9], [1.25, -3.5, 0.75]), _T([0.05, 0.1, -0.02], [-2.0, 0.5, 4.0])]


def _cloud(rng, n):
    """n x 8 float32 in pcl::PointXYZI's layout (x y z pad intensity pad pad pad), quirks sprinkled."""
    c = np.full((n, 8), -3.75, np.float32)
    c[:, :3] = rng.normal(0, 12, (n, 3))
    if n > 40:
        c[3, :3] = [np.nan, 1, 2]; c[7, :3] = [0, -1, np.inf]; c[11, :3] = [0, 0, 1.5]; c[19, :3] = [0, 0, 35.0]; c[23, :3] = [0, 0, -10.0]
        c[29, :3] = [0, 5, 0]; c[31, :3] = [0, -5, 0]; c[37, :3] = [np.inf, 0, 0]
    return c


def _sky_edges():
    bgr = np.stack(np.meshgrid(np.arange(256), np.arange(0, 256, 3), np.arange(0, 256, 5), indexing="ij"), -1).reshape(-1, 3).astype(np.uint8)
    hsv = cr.hsv_u8(bgr)
    near = np.zeros(len(bgr), bool)
    for c, vals in ((0, (99, 100, 124, 125)), (1, (42, 43, 200, 201)), (2, (149, 150))):
        near |= np.isin(hsv[:, c], vals)
    box = (hsv[:, 0] >= 98) & (hsv[:, 0] <= 126) & (hsv[:, 1] >= 40) & (hsv[:, 1] <= 203) & (hsv[:, 2] >= 147)
    return bgr[near & box]


def _image(rng, rows, cols, cloud, T, plant):
    """A random BGR image with sky-box and box-edge colours planted at half of the pixels the cloud's points hit."""
    im = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    if T is not None and len(cloud):
        hit, px, py = cr.project(cloud[:, :3], T[:3].reshape(12), rows, cols, 1.5, 35.0)
        sel = np.flatnonzero(hit)[::2]
        im[py[sel], px[sel]] = plant[rng.integers(0, len(plant), len(sel))]
    return im


def _pairs(rng, sizes, shapes, invalid=()):
    plant = _sky_edges()
    clouds, Ts, images = [], [], []
    for k, n in enumerate(sizes):
        c = _cloud(rng, n)
        T = None if k in invalid else POSES[k % 3]
        rows, cols = shapes[k % len(shapes)]
        clouds.append(c); Ts.append(T); images.append(_image(rng, rows, cols, c, T, plant))
    return clouds, Ts, images


def _want(clouds, Ts, images, lo=1.5, hi=35.0):
    return cr.colorize([c[:, :3] for c in clouds], [None if T is None else T[:3].reshape(12) for T in Ts], images, lo, hi)


def test_colorize_scans_matches_numpy(ctx):
    rng = np.random.default_rng(30)
    clouds, Ts, images = _pairs(rng, SIZES, [(7, 13), (720, 1440), (33, 65)], invalid=(2, 8))
    clouds.append(_cloud(rng, 40000)); Ts.append(POSES[1]); images.append(_image(rng, 2880, 5760, clouds[-1], POSES[1], _sky_edges()))
    for lo, hi in ((1.5, 35.0), (0.0, 1000.0)):
        got, per = api.colorize_scans(ctx, clouds, Ts, images, lo, hi)
        want, wper = _want(clouds, Ts, images, lo, hi)
        assert np.array_equal(per, wper), (lo, hi)
        assert cr.same(got, want), (lo, hi)
        assert per[2] == 0 and per[8] == 0 and len(got) > 1000
    words = got[:, 3].view(np.uint32)
    assert not np.isnan(got[:, :3]).any() and (words >> 24 == 255).all()


def test_batch_over_several_pieces_and_determinism(ctx):
    """120 pairs of 40000 points (4.8 M): three pieces of at most 2 M points through the pinned window; two calls give the same bytes."""
    rng = np.random.default_rng(31)
    base, Tb, ib = _pairs(rng, [40000] * 6, [(720, 1440), (361, 723)])
    clouds = [base[k % 6] for k in range(120)]; Ts = [Tb[k % 6] for k in range(120)]; images = [ib[k % 6] for k in range(120)]
    Ts[17] = None
    a, pa = api.colorize_scans(ctx, clouds, Ts, images, 1.5, 35.0)
    b, pb = api.colorize_scans(ctx, clouds, Ts, images, 1.5, 35.0)
    assert a.tobytes() == b.tobytes() and np.array_equal(pa, pb)
    want, wper = _want(clouds, Ts, images)
    assert np.array_equal(pa, wper) and cr.same(a, want)
    with pytest.raises(pv.PvlmError):
        api.colorize_scans(ctx, clouds, Ts, images, 1.5, 35.0, capacity=len(want) - 1)


def test_colorize_scans_dev_on_torch_tensors(ctx):
    import torch
    rng = np.random.default_rng(32)
    clouds, Ts, images = _pairs(rng, SIZES, [(720, 1440), (7, 13)], invalid=(4,))
    dev = torch.device("cuda", ctx.device)
    tc = [torch.from_numpy(c).to(dev) for c in clouds]
    ti = [torch.from_numpy(im).to(dev) for im in images]
    out, per, n = api.colorize_scans_dev(ctx, tc, Ts, ti, 1.5, 35.0)
    torch.cuda.synchronize()
    m = int(n.item())
    host, hper = api.colorize_scans(ctx, clouds, Ts, images, 1.5, 35.0)
    want, wper = _want(clouds, Ts, images)
    assert m == len(want) and np.array_equal(per.cpu().numpy(), wper) and np.array_equal(hper, wper)
    got = out[:m].cpu().numpy()
    assert cr.same(got, want) and cr.same(host, want)
    # a capacity below the count: the full count, nothing past capacity written
    small = torch.full((m // 2 + 1, 4), 7.0, dtype=torch.float32, device=dev)
    _, _, n2 = api.colorize_scans_dev(ctx, tc, Ts, ti, 1.5, 35.0, out=small, capacity=m // 2)
    torch.cuda.synchronize()
    assert int(n2.item()) == m
    s = small.cpu().numpy()
    assert cr.same(s[:m // 2], want[:m // 2]) and (s[m // 2] == 7.0).all()


def test_colorize_scans_dev_binds_the_stream_once(ctx, monkeypatch):
    """The context is bound to torch's current stream only when it is not already; another stream rebinds."""
    import torch
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(34)
    clouds, Ts, images = _pairs(rng, [5000], [(720, 1440)])
    tc = [torch.from_numpy(clouds[0]).to(dev)]; ti = [torch.from_numpy(images[0]).to(dev)]
    binds = []
    real = ctx.set_stream
    monkeypatch.setattr(ctx, "set_stream", lambda h: (binds.append(h), real(h)))
    ctx.use_own_stream()
    a = api.colorize_scans_dev(ctx, tc, Ts, ti, 1.5, 35.0)
    b = api.colorize_scans_dev(ctx, tc, Ts, ti, 1.5, 35.0)
    assert len(binds) == 1 and ctx._bound_stream == int(torch.cuda.current_stream(dev).cuda_stream or 0)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = api.colorize_scans_dev(ctx, tc, Ts, ti, 1.5, 35.0)
        m = int(c[2].item())
    assert len(binds) == 2 and ctx._bound_stream == int(side.cuda_stream)
    torch.cuda.synchronize()
    want, _ = _want(clouds, Ts, images)
    assert m == int(a[2].item()) == int(b[2].item()) == len(want) and cr.same(c[0][:m].cpu().numpy(), want)
    ctx.use_own_stream()


def test_debug_hsv_of_every_colour(ctx):
    c = np.arange(1 << 24, dtype=np.uint32)
    bgr = np.stack([(c & 255), (c >> 8) & 255, (c >> 16) & 255], axis=1).astype(np.uint8)
    got = api.colorize_debug_hsv(ctx, bgr).astype(np.int64)
    assert np.array_equal(got, cr.hsv_u8(bgr))


def _driver():
    from panovlm_amd import build
    build.build_host()
    return build.TEXTURE_DRIVER


def _run(*args):
    out = subprocess.run([_driver()] + [str(a) for a in args], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    return out


def _read_clouds(f, cols):
    n = struct.unpack("<q", f.read(8))[0]
    return np.frombuffer(f.read(4 * cols * n), np.float32).reshape(n, cols).copy()


def test_segment_batch_matches_per_scan_host(tmp_path):
    """Velodyne::SegmentBatch against ReOrderVLP() + Segmentation() scan by scan on the ring cases, one invalid and one already re-ordered scan included."""
    scans = []
    for k, case in enumerate(ring_cases.CASES):
        raw, n_scans, cols, _ = ring_cases.raw_of(case)
        mode = 1 if k == 3 else (2 if k == 5 else 0)
        scans.append((mode, n_scans, cols, raw))
    src, dst = str(tmp_path / "scans.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(scans)))
        for mode, n_scans, cols, raw in scans:
            f.write(struct.pack("<iiii", mode, n_scans, cols, len(raw))); f.write(np.ascontiguousarray(raw, np.float32).tobytes())
    _run("segment", src, dst, 16)
    with open(dst, "rb") as f:
        for k, (mode, *_rest) in enumerate(scans):
            a, b = _read_clouds(f, 4), _read_clouds(f, 4)
            assert a.tobytes() == b.tobytes(), k
            if mode == 1:
                assert len(b) == 0
            else:
                assert len(b) > 0


def _write_pairs(path, pairs):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(pairs)))
        for p in pairs:
            f.write(struct.pack("<i", 1 if p["T_wl"] is not None else 0))
            T = p["T_wl"] if p["T_wl"] is not None else np.eye(4)
            f.write(np.ascontiguousarray(T[:3, :3], np.float64).tobytes()); f.write(np.ascontiguousarray(T[:3, 3], np.float64).tobytes())
            name = p["name"].encode()
            f.write(struct.pack("<i", len(name))); f.write(name)
            f.write(struct.pack("<i", 1 if p["T_wc"] is not None else 0))
            T = p["T_wc"] if p["T_wc"] is not None else np.eye(4)
            f.write(np.ascontiguousarray(T[:3, :3], np.float64).tobytes()); f.write(np.ascontiguousarray(T[:3, 3], np.float64).tobytes())
            im = np.ascontiguousarray(p["image"], np.uint8)
            f.write(struct.pack("<ii", im.shape[0], im.shape[1])); f.write(im.tobytes())


def test_texture_end_to_end(tmp_path):
    """main.cpp:524-552: Texture(lidars, frames).ColorizeLidarPointCloud(1.5, 35), then savePCDFileBinary(FuseCloud(4)) — from scans written as PCD files."""
    rng = np.random.default_rng(33)
    rows, cols = 720, 1440
    pairs = []
    for k in range(14):
        raw = sy.raw_vlp16_scan(k % 5, cols=900, clutter=20)
        name = str(tmp_path / ("scan%02d.pcd" % k))
        # LoadLidar swaps (x, y, z) -> (x, -z, y): the file holds (x, z, -y) of the camera-style scan
        fuse_ref.write_pcd(name, np.stack([raw[:, 0], raw[:, 2], -raw[:, 1], raw[:, 3]], axis=1))
        T_wl = _T(rng.normal(0, 0.3, 3), rng.normal(0, 3, 3))
        T_wc = T_wl @ _T([0.02, -0.01, 0.03], [0.1, -0.05, 0.2])
        im = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        im[: rows // 3] = (235, 180, 120)                                       # a sky band: h 104, s 125, v 235
        pairs.append(dict(name=name, T_wl=T_wl, T_wc=T_wc, image=im))
    pairs[3]["T_wl"] = None                                                        # scan pose invalid
    pairs[6]["T_wc"] = None                                                        # frame pose invalid
    pairs[8]["T_wc"] = None
    src, dst, pcd = str(tmp_path / "pairs.bin"), str(tmp_path / "out.bin"), str(tmp_path / "lidar_colored_fuse.pcd")
    _write_pairs(src, pairs)
    log = _run("texture", src, dst, 1.5, 35.0, 4, pcd).stdout
    assert "saved 1" in log
    colored, poses = [], []
    with open(dst, "rb") as f:
        for k, p in enumerate(pairs):
            scan = _read_clouds(f, 4)
            got = _read_clouds(f, 4)
            T_cl = None
            if p["T_wl"] is not None and p["T_wc"] is not None:
                T_cl = cr.camera_from_lidar(p["T_wc"][:3, :3], p["T_wc"][:3, 3], p["T_wl"])
                assert len(scan) > 1000
            want = cr.colorize_pair(scan[:, :3], T_cl, p["image"], 1.5, 35.0)
            assert cr.same(got, want), k
            colored.append(want); poses.append(None if p["T_wl"] is None else p["T_wl"])
        fused = _read_clouds(f, 4)
    want_fused = cr.fuse(colored, poses, 4)
    assert cr.same(fused, want_fused) and len(want_fused) > 1000
    assert open(pcd, "rb").read() == cr.pcd_bytes(want_fused)
    assert sum(len(c) for c in colored) > 5000
