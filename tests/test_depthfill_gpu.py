"""GPU checks of K37 through the C ABI: pvlm_depth_completion and pvlm_compute_depth_images against the host compile of the same core
(tests/cpp/depthfill_core_check.cpp) bit for bit, as fp32 and as uint16, on the shapes and contents where a tiled stencil goes wrong: tile edges, halos, the column
scans across tiles, fill rounds that cross two tiles, batches; the point-cloud chain against project_lidar_depth + depth_completion; the host mirror's
ComputeDepthImage into FilterImagePairsFull through tests/cpp/pvlm_depthfill_driver.cpp; one 720 x 1440 frame."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import depthfill_ref as ref

pytestmark = pytest.mark.gpu

M = ref.MAX_DEPTH
_SRC = open(os.path.join(ref.ROOT, "panovlm_amd", "csrc", "pvlm_depthfill.hip")).read()
TH = int(re.search(r"constexpr int kTileH = (\d+);", _SRC).group(1))
TW = int(re.search(r"constexpr int kTileW = (\d+);", _SRC).group(1))


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(ctx, sparse, max_depth=M):
    """device == host compile, fp32 and uint16, and the statistics; returns the device's fp32 result"""
    rc, hd, hu, hstats = ref.host_completion(sparse, max_depth)
    assert rc == 0
    d, u, st = ctx.depth_completion(sparse, max_depth, want_f32=True, want_u16=True)
    bad = np.argwhere(_bits(d) != _bits(hd))
    assert len(bad) == 0, (sparse.shape, len(bad), bad[:4].tolist())
    assert np.array_equal(u, hu)
    assert (st["valid_in"], st["valid_out"]) == hstats and st["images"] == (1 if sparse.ndim == 2 else len(sparse))
    return d


@pytest.mark.parametrize("rows,cols,p", [(TH, TW, 0.02), (TH + 1, TW + 1, 0.02), (2 * TH + 1, 2 * TW + 1, 0.01), (TH + 7, TW + 6, 0.02), (5, 7, 0.3), (1, 9, 0.5), (9, 1, 0.5),
                                         (1, 1, 1.0)])
def test_tile_edges(ctx, rows, cols, p):
    _same(ctx, ref.recipe(rows, cols, p))
    _same(ctx, ref.as_f32(ref.recipe(rows, cols, p, seed=11)))


def test_halos_and_corners(ctx):
    """valid pixels in the last row / column of a tile and the first of the next, and at the four image corners: the ignored border of the morphology, the replicated one
    of the medians and the reflected one of the bilateral"""
    rows, cols = 2 * TH + 5, 2 * TW + 5
    img = np.zeros((rows, cols), np.uint16)
    for r, c, d in ((0, 0, 2), (0, cols - 1, 20), (rows - 1, 0, 33), (rows - 1, cols - 1, 8), (TH - 1, TW - 1, 15), (TH, TW, 30), (TH - 1, TW, 33), (TH, TW - 1, 2),
                    (2 * TH - 1, 5, 20), (2 * TH, 6, 8), (7, 2 * TW - 1, 2), (8, 2 * TW, 39.99)):
        img[r, c] = int(round(d * 256))
    want = ref.complete(ref.as_f32(img), M)
    d = _same(ctx, img)
    assert np.array_equal(_bits(d), _bits(want["out"])) and want["valid_out"] > 12


def test_top_masks_across_tiles(ctx):
    """the empty stripe covers the boundary between two tiles, the column that is valid in its last row only is the last column of a tile, the one valid in row 0 the
    first of the next"""
    rows, cols = 2 * TH + 6, 2 * TW + 12
    img = ref.recipe(rows, cols, 0.01, empty_col=TW - 1, bottom_col=2 * TW - 1, top_col=2 * TW)
    assert not img[:, TW - 1:TW + 2].any() and img[rows - 1, 2 * TW - 1] and not img[:rows - 1, 2 * TW - 1].any() and img[0, 2 * TW]
    want = ref.complete(ref.as_f32(img), M)
    assert want["cut_top"] > 0
    _same(ctx, img)


def test_fill_rounds_across_two_tiles(ctx):
    """a hole 2.5 tiles wide between two valid bands: the six fills advance 12 pixels from either side, across tile boundaries, and by the restatement alone leave
    unfilled pixels under the top mask"""
    rows, cols = TH + 9, 3 * TW + 20
    img = ref.recipe(rows, cols, 0.05, empty_col=0)
    img[rows // 5 + 1:, TW - 20:3 * TW + 12] = 0
    img[rows // 5, :] = 2 * 256                                   # a valid row on top: the top mask covers the hole
    want = ref.complete(ref.as_f32(img), M)
    assert want["unfilled"] > 0 and min(want["round_work"]) > 0
    d = _same(ctx, img)
    assert np.array_equal(_bits(d), _bits(want["out"]))


def test_batches(ctx, monkeypatch):
    imgs = np.stack([ref.recipe(TH + 3, TW + 9, 0.02, seed=s) for s in (1, 2, 3)])
    single = [ctx.depth_completion(imgs[k], M, want_u16=True) for k in range(3)]
    assert single[0][2]["batches"] == 1
    d, u, st = ctx.depth_completion(imgs, M, want_u16=True)
    assert st["images"] == 3 and st["batches"] == 1
    for k in range(3):
        assert np.array_equal(_bits(d[k]), _bits(single[k][0])) and np.array_equal(u[k], single[k][1])
    _same(ctx, imgs)
    monkeypatch.setenv("PVLM_DEPTHFILL_BATCH_IMAGES", "2")
    d2, u2, st2 = ctx.depth_completion(imgs, M, want_u16=True)
    assert st2["batches"] == 2 and st2["images"] == 3 and st2["valid_out"] == st["valid_out"]
    assert np.array_equal(_bits(d2), _bits(d)) and np.array_equal(u2, u)
    only16 = ctx.depth_completion(imgs, M, want_f32=False, want_u16=True)
    assert only16[0] is None and np.array_equal(only16[1], u)


def test_point_clouds(ctx, monkeypatch):
    """compute_depth_images == project_lidar_depth per scan, then depth_completion == the host loop; a scan without points gives zeros"""
    clouds = [ref.synthetic_cloud(900, 1), np.zeros((0, 3), np.float32), ref.synthetic_cloud(400, 3, radius=(0.5, 48.0))]
    for max_depth in (5.0, M):
        got, st = ctx.compute_depth_images(90, 180, clouds, ref.T_CL, 4, max_depth)
        assert st["images"] == 3 and st["batches"] == 1 and not got[1].any()
        rc, host = ref.host_depth_images(90, 180, clouds, ref.T_CL, 4, max_depth)
        assert rc == 0 and np.array_equal(got, host)
        for k, c in enumerate(clouds):
            sparse = ctx.project_lidar_depth(90, 180, c, ref.T_CL, 4)
            assert np.array_equal(ctx.depth_completion(sparse, max_depth, want_f32=False, want_u16=True)[1], got[k])
    monkeypatch.setenv("PVLM_DEPTHFILL_BATCH_IMAGES", "1")
    again, st = ctx.compute_depth_images(90, 180, clouds, ref.T_CL, 4, M)
    assert st["batches"] == 3 and np.array_equal(again, got)


def test_refusals(ctx):
    import panovlm_amd as pv
    img = ref.recipe(9, 11, 0.2); f = ref.as_f32(img)
    C = pv.api.C
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    dense = np.zeros((9, 11), np.float32); u16 = np.zeros((9, 11), np.uint16)
    call = lambda a16, a32, d, u: ctx.lib.pvlm_depth_completion(ctx._h, C.c_int(9), C.c_int(11), C.c_int(1), p(a16, C.c_uint16), p(a32, C.c_float), C.c_float(M),
                                                                  p(d, C.c_float), p(u, C.c_uint16), None)
    assert call(img, None, dense, u16) == 0
    arg = call(img, f, dense, u16)
    assert arg != 0 and call(None, None, dense, u16) == arg and call(img, None, None, None) == arg
    for bad in (np.nan, np.inf, -1.0):
        g = f.copy(); g[4, 5] = bad
        with pytest.raises(pv.PvlmError):
            ctx.depth_completion(g, M)
    clouds = [ref.synthetic_cloud(50, 1), ref.synthetic_cloud(20, 2)]
    xyz = np.concatenate(clouds)
    with pytest.raises(pv.PvlmError):
        ctx.compute_depth_images_flat(30, 60, [0, 50, 40], xyz, ref.T_CL, 4, M)
    assert ctx.compute_depth_images_flat(30, 60, [0, 50, 70], xyz, ref.T_CL, 4, M)[0].shape == (2, 30, 60)


def test_compute_depth_image_into_filter_image_pairs_full():
    """pvlm::ComputeDepthImage (device) == ComputeDepthImageHost, then MatchImagePairs -> FilterImagePairsFull with those maps, through the driver"""
    from panovlm_amd import build
    out = subprocess.run([build.DEPTHFILL_DRIVER], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "device maps equal host maps" in out.stdout and out.stdout.count("pair (") == 3


def test_one_full_size_frame(ctx):
    img = ref.recipe(720, 1440, 0.01)
    _same(ctx, img)
