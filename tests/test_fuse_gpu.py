"""K29 (pvlm_fuse_scans / pvlm_fuse_scans_dev: the fused LiDAR map of LidarOdometry::FuseLidar) and the host mirror's FuseLidar / SavePCDFileBinary against the
numpy restatement (tests/fuse_ref.py): bit for bit, NaN positions compared with isnan (payloads differ between the GPU and x86)."""
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import panovlm_amd as pv
from panovlm_amd import api
from panovlm_amd import synthetic as sy
from tests import fuse_ref

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 28800, 40000]


@pytest.fixture(scope="module")
def ctx():
    c = pv.Context()
    yield c
    c.close()


def _poses():
    big = Rotation.from_rotvec([2.1, -1.3, 0.7]).as_matrix()
    return [(np.eye(3), np.zeros(3)), (big, np.array([0.3, -1.2, 2.0])), (Rotation.from_rotvec([0.1, 0.2, -0.05]).as_matrix(), np.array([4.5e5, -2.25e6, 1234.5]))]


def _cloud(rng, n):
    c = np.concatenate([rng.normal(0, 25, (n, 3)), rng.uniform(0, 255, (n, 1))], axis=1).astype(np.float32)
    if n > 40:                                                         # the quirks, sprinkled
        c[3] = [np.nan, 1, 2, 5]; c[7] = [0, -1, np.inf, 6]; c[11] = [1, 30, -30, 7]; c[19] = [np.inf, 0, 0, 8]; c[23] = [0, 5, -1, 9]
        c[29] = [1.5e-20, 0, 0, 10]; c[31] = [40, 0, 0, 11]; c[37] = [0, 0, -np.inf, 12]
    return c


def _layout(c, stride, at):
    """The n x 4 cloud stored n x stride with intensity at float `at` (the other floats garbage)."""
    out = np.full((len(c), stride), -7.25, np.float32)
    out[:, :3] = c[:, :3]; out[:, at] = c[:, 3]
    return out


def test_fuse_scans_matches_numpy(ctx):
    rng = np.random.default_rng(41)
    clouds = [_cloud(rng, n) for n in SIZES]
    poses = [_poses()[k % 3] for k in range(len(clouds))]
    for (stride, at) in ((4, 3), (8, 3), (8, 4)):
        for min_r, max_r in ((0.0, 40.0), (1e-20, np.inf), (20.0, 10.0)):
            got, per = api.fuse_scans(ctx, [_layout(c, stride, at) for c in clouds], poses, min_r, max_r, intensity_at=at)
            want, wper = fuse_ref.fuse(clouds, poses, min_r, max_r)
            assert np.array_equal(per, wper), (stride, at, min_r, max_r)
            assert fuse_ref.same(got, want), (stride, at, min_r, max_r)
    assert np.isnan(got).any() and len(got) == int(per.sum())


def test_batch_above_one_piece_and_determinism(ctx):
    """4.3 M points: three pieces of at most 2 M points through the pinned window — the third reuses the buffer set of the first (the upload's wait for the
    kernels of piece q - 2) —, the output order across pieces; batch == scan by scan; two calls, the same bits."""
    rng = np.random.default_rng(7)
    sizes = [28800] * 146 + [40000, 0, 70000, 1]
    base = [_cloud(rng, 28800) for _ in range(4)]
    clouds = [base[k % 4] if n == 28800 else _cloud(rng, n) for k, n in enumerate(sizes)]
    poses = [(Rotation.from_rotvec(rng.normal(0, 1.0, 3)).as_matrix(), rng.normal(0, 30, 3)) for _ in sizes]
    got, per = api.fuse_scans(ctx, clouds, poses, 2.0, 35.0)
    want, wper = fuse_ref.fuse(clouds, poses, 2.0, 35.0)
    assert sum(sizes) > 2 * (2 << 20) and np.array_equal(per, wper) and fuse_ref.same(got, want)
    again, _ = api.fuse_scans(ctx, clouds, poses, 2.0, 35.0)
    assert again.tobytes() == got.tobytes()
    pick = (0, 1, 72, 145, 146, 147, 148, 149)
    alone = np.concatenate([api.fuse_scans(ctx, [clouds[k]], [poses[k]], 2.0, 35.0)[0] for k in pick])
    off = np.concatenate([[0], np.cumsum(per)])
    assert alone.tobytes() == np.concatenate([got[off[k]:off[k + 1]] for k in pick]).tobytes()
    with pytest.raises(pv.PvlmError, match="%d points kept" % int(per[:3].sum())):
        api.fuse_scans(ctx, clouds[:3], poses[:3], 2.0, 35.0, capacity=int(per[:3].sum()) - 1)


def test_fuse_scans_dev_on_torch_tensors(ctx):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(13)
    clouds = [_cloud(rng, n) for n in SIZES]
    poses = [_poses()[k % 3] for k in range(len(clouds))]
    for stride, at in ((4, 3), (8, 4)):
        host = [_layout(c, stride, at) for c in clouds]
        want, wper = api.fuse_scans(ctx, host, poses, 0.5, 40.0, intensity_at=at)
        tens = [torch.from_numpy(h).to(dev) for h in host]
        out, per, n = api.fuse_scans_dev(ctx, tens, poses, 0.5, 40.0, intensity_at=at)
        m = int(n.item())
        assert m == len(want) and np.array_equal(per.cpu().numpy(), wper)
        assert out[:m].cpu().numpy().tobytes() == want.tobytes()         # the same kernels: NaN payloads included
        # capacity = kept - 1: the full count is reported, nothing is written past capacity
        sentinel = torch.full((m + 16, 4), 123.5, dtype=torch.float32, device=dev)
        out2, per2, n2 = api.fuse_scans_dev(ctx, tens, poses, 0.5, 40.0, intensity_at=at, out=sentinel, capacity=m - 1)
        got = out2.cpu().numpy()
        assert int(n2.item()) == m and np.array_equal(per2.cpu().numpy(), wper)
        assert got[:m - 1].tobytes() == want[:m - 1].tobytes() and np.all(got[m - 1:] == 123.5)
    # layouts the float4 load cannot serve (the kernels' scalar loads): a stride of 5 floats, and clouds 4 bytes off a 16-byte boundary
    host5 = [_layout(c, 5, 4) for c in clouds]
    want5, wper5 = api.fuse_scans(ctx, host5, poses, 0.5, 40.0, intensity_at=4)
    out5, per5, n5 = api.fuse_scans_dev(ctx, [torch.from_numpy(h).to(dev) for h in host5], poses, 0.5, 40.0, intensity_at=4)
    assert int(n5.item()) == len(want5) and np.array_equal(per5.cpu().numpy(), wper5) and out5[:len(want5)].cpu().numpy().tobytes() == want5.tobytes()
    off = []
    for c in clouds:
        flat = torch.zeros(4 * len(c) + 1, dtype=torch.float32, device=dev)
        off.append(flat[1:].view(len(c), 4)); off[-1].copy_(torch.from_numpy(c))
    assert all(t.data_ptr() % 16 == 4 for t in off if len(t))
    want4, _ = api.fuse_scans(ctx, clouds, poses, 0.5, 40.0)
    out4, _, n4 = api.fuse_scans_dev(ctx, off, poses, 0.5, 40.0)
    assert out4[:int(n4.item())].cpu().numpy().tobytes() == want4.tobytes()
    with pytest.raises(ValueError, match="16-byte aligned"):
        api.fuse_scans_dev(ctx, off, poses, 0.5, 40.0, out=torch.zeros(4 * len(want4) + 1, dtype=torch.float32, device=dev)[1:].view(-1, 4))
    ctx.use_own_stream()


def test_fuse_scans_dev_binds_the_stream_once(ctx, monkeypatch):
    """The context is bound to torch's current stream only when it is not already (pvlm_set_stream waits for the stream bound before): a second call on the
    same stream queues without that wait; another stream rebinds."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17)
    tens = [torch.from_numpy(_cloud(rng, 5000)).to(dev)]
    poses = [_poses()[1]]
    binds = []
    real = ctx.set_stream
    monkeypatch.setattr(ctx, "set_stream", lambda h: (binds.append(h), real(h)))
    ctx.use_own_stream()
    a = api.fuse_scans_dev(ctx, tens, poses, 0.5, 40.0)
    b = api.fuse_scans_dev(ctx, tens, poses, 0.5, 40.0)
    assert len(binds) == 1 and ctx._bound_stream == int(torch.cuda.current_stream(dev).cuda_stream or 0)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = api.fuse_scans_dev(ctx, tens, poses, 0.5, 40.0)
        m = int(c[2].item())
    assert len(binds) == 2 and ctx._bound_stream == int(side.cuda_stream)
    torch.cuda.synchronize()
    assert m == int(a[2].item()) == int(b[2].item()) and c[0][:m].cpu().numpy().tobytes() == a[0][:m].cpu().numpy().tobytes()
    ctx.use_own_stream()


def _scan(R, t, cloud=None, scan=None, valid=True, name=""):
    return dict(R=R, t=t, valid=valid, name=name, cloud=np.zeros((0, 4), np.float32) if cloud is None else cloud,
                cloud_scan=np.zeros((0, 4), np.float32) if scan is None else scan)


@pytest.mark.parametrize("which", ["odometry", "joint"])
def test_fuse_lidar_selection(tmp_path, which):
    """Which scans FuseLidar(skip, ..) fuses: stride from 0 without re-syncing after a skipped scan, valid flags, pose validity (zero rotation, inf
    translation), the reload of an empty cloud (a .pcd on disk; one that leaves the scan invalid still contributes), cloud_scan over cloud, a failed reload."""
    rng = np.random.default_rng(3)
    d = str(tmp_path)
    ok_pcd = os.path.join(d, "reload.pcd")
    fuse_ref.write_pcd(ok_pcd, np.concatenate([rng.normal(0, 9, (700, 3)), rng.uniform(0, 99, (700, 1))], axis=1))
    scans = []
    for i in range(31):
        R, t = Rotation.from_rotvec(rng.normal(0, 1, 3)).as_matrix(), rng.normal(0, 20, 3)
        scans.append(_scan(R, t, cloud=_cloud(rng, int(rng.integers(100, 600)))))
    scans[3]["valid"] = False                                            # visited by skips 0 and 2 ...
    scans[4]["t"] = np.array([np.inf, 0, 0])                             # ... and right after it an invalid pose: skip 2 goes on to 6, not 4
    scans[5]["valid"] = False
    scans[6]["R"] = np.zeros((3, 3))                                     # zero rotation: no pose
    for i in (9, 20):                                                    # empty cloud, reloaded from disk (700 points < 4000: the scan turns invalid, still fused)
        scans[i]["cloud"] = np.zeros((0, 4), np.float32); scans[i]["name"] = ok_pcd
    scans[10]["cloud_scan"] = _cloud(rng, 300)                           # cloud_scan wins over cloud
    scans[15]["cloud"] = np.zeros((0, 4), np.float32); scans[15]["name"] = ok_pcd; scans[15]["cloud_scan"] = _cloud(rng, 200)
    scans[12]["cloud"] = np.zeros((0, 4), np.float32); scans[12]["name"] = os.path.join(d, "missing.pcd")   # reload fails: nothing
    scans[25]["cloud"] = np.zeros((0, 4), np.float32); scans[25]["name"] = os.path.join(d, "missing.pcd")
    for skip in (0, 2, 4):
        got, log = fuse_ref.fuse_lidar(d, scans, which, skip, 0.5, 30.0)
        want, per = fuse_ref.select_and_fuse(scans, skip, 0.5, 30.0)
        assert fuse_ref.same(got, want), (which, skip)
        assert len(got) > 0
    # the cases were reached: skip 2 fuses the reloaded 9 and the cloud_scan of 15, skip 4 the reloaded 20 and the cloud_scan of 10
    visited = lambda skip: list(range(0, 31, skip + 1))
    assert {3, 9, 12, 15} <= set(visited(2)) and {5, 10, 15, 20, 25} <= set(visited(4)) and 4 not in visited(2)
    out = fuse_ref.run("fuse", os.path.join(d, "scans.bin"), os.path.join(d, "neg.bin"), which, -1, 0.0, 40.0, check=False)
    assert out.returncode == 3 and "skip < 0" in out.stderr


def test_fuse_lidar_to_pcd_end_to_end(tmp_path):
    """main.cpp:408: savePCDFileBinary(path, FuseLidar(4, 0, 40)) on a 64-scan Room-like set of raw VLP-16 scans; the file's points equal the restatement."""
    base = [sy.raw_vlp16_scan(k, cols=900, clutter=20) for k in range(4)]
    scans = []
    for k in range(64):
        R, t = sy.estimated_pose(k % 16)
        scans.append(_scan(R, t, cloud=base[k % 4]))
    scans[20]["valid"] = False
    pcd = str(tmp_path / "lidar_fuse_refined.pcd")
    got, log = fuse_ref.fuse_lidar(str(tmp_path), scans, "odometry", 4, 0, 40, pcd=pcd)
    want, _ = fuse_ref.select_and_fuse(scans, 4, 0, 40)
    assert "saved 1" in log
    lines, data = fuse_ref.read_pcd(pcd)
    assert lines[6] == "WIDTH %d" % len(want) and lines[9] == "POINTS %d" % len(want)
    assert fuse_ref.same(data, want) and fuse_ref.same(got, want)
    assert len(want) > 10 * 14400
