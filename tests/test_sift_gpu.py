"""GPU checks of K41 (pvlm_sift_extract, pvlm_sift_pyramid_debug): the device against the host compile of csrc/pvlm_sift_core.h (tests/sift_ref.py) bit for bit --
layers, candidates, keypoints, their order, descriptors --, the capacity protocol and the refusals, the chain into pvlm_descset_create and pvlm_match_pairs, and
bit-reproducibility.  The host compile is itself pinned to the numpy restatement by tests/test_sift_cpu.py."""
import numpy as np
import pytest

from tests import match_ref as mr
from tests import sift_ref as sr

pytestmark = pytest.mark.gpu

SIZES = ((17, 33, 1), (64, 96, 7), (119, 161, 3), (260, 520, 5))      # rows, cols, seed; 520 x 260: past one blur tile both ways, past one 4096-pixel compaction tile
CHAIN_SEED, SHIFT, RATIO = 11, (16, 8), 0.8


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def api():
    from panovlm_amd import api
    return api


@pytest.fixture(scope="module")
def images():
    return {(r, c): sr.blob_image(r, c, s) for r, c, s in SIZES}


@pytest.fixture(scope="module")
def host_pre(images):
    """the host compile's candidates and keypoints before the selection, once per image"""
    return {k: sr.host_detect(img) for k, img in images.items()}


def _half_mask(rows, cols):
    m = np.zeros((rows, cols), np.uint8); m[:, :cols // 2] = 1
    return m


@pytest.mark.parametrize("rows,cols,seed", SIZES)
def test_layers_and_candidates_equal_the_host_compile(ctx, api, images, host_pre, rows, cols, seed):
    img = images[(rows, cols)]
    hc, hk, _ = host_pre[(rows, cols)]
    sizes = sr.host_sizes(rows, cols)
    for o in range(len(sizes)):
        d = api.sift_pyramid_debug(ctx, img, o)
        g, dg = sr.host_pyramid(img, o)
        assert d["n_octaves"] == len(sizes) and d["gauss"].shape[1:] == sizes[o]
        assert np.array_equal(d["gauss"].view(np.uint32), g.view(np.uint32)), "Gaussian layers of octave %d" % o
        assert np.array_equal(d["dog"].view(np.uint32), dg.view(np.uint32)), "difference layers of octave %d" % o
        assert d["candidates"].tobytes() == hc[hc["octave"] == o].tobytes(), "candidates of octave %d, in order" % o
        assert d["keypoints"].tobytes() == hk.tobytes()


def test_a_second_520_x_260_image_past_one_trip_of_the_scan(ctx, api):
    """k_tile_scan walks its counts 1024 at a time.  The tile counts of a 520 x 260 image stay below that (3 x 133 tiles in the first octave: only the bench's
    panoramas cross it there), but the scan also places the keypoints behind the per-candidate peak counts: the dot pattern gives the first octave more than 2048
    candidates, two trips and their carry, and the peaks of every candidate must land in order."""
    img = sr.dot_image(260, 520, 5)
    hc, hk, _ = sr.host_detect(img)
    assert int((hc["octave"] == 0).sum()) > 2048
    d = api.sift_pyramid_debug(ctx, img, 0)
    assert d["candidates"].tobytes() == hc[hc["octave"] == 0].tobytes() and d["keypoints"].tobytes() == hk.tobytes()
    for nf, root in ((len(hk) + 10, False), (1000, True)):
        r = api.sift_extract(ctx, [img], nf, flags=api.FLAG_SIFT_ROOT if root else 0)
        k, dd = sr.host_extract(img, nf, None, root)
        assert r["keypoints"].tobytes() == k.tobytes() and r["descriptors"].tobytes() == dd.tobytes() and r["calls"] == 1


@pytest.mark.parametrize("rows,cols,seed", SIZES)
@pytest.mark.parametrize("root", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_extract_equals_the_host_compile(ctx, api, images, host_pre, rows, cols, seed, root, masked):
    img = images[(rows, cols)]
    n_pre = len(host_pre[(rows, cols)][1])
    mask = _half_mask(rows, cols) if masked else None
    for nf in (n_pre + 100, max(1, n_pre // 3)):                                   # above and below the candidate count
        r = api.sift_extract(ctx, [img], nf, mask=mask, flags=api.FLAG_SIFT_ROOT if root else 0)
        k, d = sr.host_extract(img, nf, mask, root)
        assert r["needed"] == len(k) and not r["overflow"] and r["guard_intact"]
        assert r["keypoints"].tobytes() == k.tobytes(), "keypoints and their order"
        assert r["descriptors"].view(np.uint32).tobytes() == d.view(np.uint32).tobytes()
        if nf < n_pre and not masked:
            assert len(k) >= nf


def test_batch_equals_single_calls_in_any_order(ctx, api):
    imgs = [sr.blob_image(64, 96, s) for s in (20, 21, 22, 23, 24)]
    mask = _half_mask(64, 96)
    single = [api.sift_extract(ctx, [im], 30, mask=mask, flags=api.FLAG_SIFT_ROOT) for im in imgs]
    for order in ((0, 1, 2, 3, 4), (3, 0, 4, 2, 1)):
        r = api.sift_extract(ctx, [imgs[i] for i in order], 30, mask=mask, flags=api.FLAG_SIFT_ROOT)
        assert r["stats"]["images"] == 5 and len(r["offsets"]) == 6 and r["offsets"][-1] == r["needed"]
        for pos, i in enumerate(order):
            a, b = r["offsets"][pos], r["offsets"][pos + 1]
            assert r["keypoints"][a:b].tobytes() == single[i]["keypoints"].tobytes()
            assert r["descriptors"][a:b].tobytes() == single[i]["descriptors"].tobytes()
    assert sum(len(s["keypoints"]) for s in single) > 20


def test_capacity_protocol(ctx, api):
    imgs = [sr.blob_image(64, 96, s) for s in (20, 21)]
    full = api.sift_extract(ctx, imgs, 1000)
    n = full["needed"]
    assert n > 10 and not full["overflow"] and full["calls"] == 1, "an open capacity is served by ONE device call"
    lib_calls = []
    real = ctx.lib.pvlm_sift_extract
    try:
        ctx.lib.pvlm_sift_extract = lambda *a: (lib_calls.append(1), real(*a))[1]
        again = api.sift_extract(ctx, imgs, 5)                       # nfeatures below the count: still one call, ties included
    finally:
        ctx.lib.pvlm_sift_extract = real
    assert len(lib_calls) == 1 and again["calls"] == 1 and not again["overflow"] and again["offsets"][-1] >= 10
    only_kp = np.zeros(n, api.SIFT_KEYPOINT_DTYPE); off = np.zeros(3, np.int64); needed = api.C.c_longlong(0)
    ptrs = (api.C.POINTER(api.C.c_ubyte) * 2)(*[api._p(im, api.C.c_ubyte) for im in imgs])
    rc = real(ctx._h, api.C.c_int(2), api.C.c_int(64), api.C.c_int(96), ptrs, None, api.C.c_int(1000), api.C.c_uint(0), api._p(off, api.C.c_longlong),
              only_kp.ctypes.data_as(api.C.c_void_p), None, api.C.c_longlong(n), api.C.byref(needed), None)
    assert rc == 0 and needed.value == n and only_kp.tobytes() == full["keypoints"].tobytes(), "descriptors == NULL: the keypoints alone"
    zero = api.sift_extract(ctx, imgs, 1000, capacity=0)
    assert zero["overflow"] and zero["needed"] == n and zero["guard_intact"] and np.array_equal(zero["offsets"], full["offsets"])
    part = api.sift_extract(ctx, imgs, 1000, capacity=int(full["offsets"][1]) + 3)              # the second image fits in part
    assert part["overflow"] and part["needed"] == n and part["guard_intact"]
    assert part["keypoints"].tobytes() == full["keypoints"][:len(part["keypoints"])].tobytes()
    assert part["descriptors"].tobytes() == full["descriptors"][:len(part["keypoints"])].tobytes()
    exact = api.sift_extract(ctx, imgs, 1000, capacity=n)
    assert not exact["overflow"] and exact["guard_intact"] and exact["keypoints"].tobytes() == full["keypoints"].tobytes()
    assert exact["descriptors"].tobytes() == full["descriptors"].tobytes()


def test_refusals(ctx, api):
    import panovlm_amd as pv
    ok = sr.blob_image(64, 96, 20)
    for bad in (np.zeros((7, 40), np.uint8), np.zeros((40, 7), np.uint8)):
        with pytest.raises(pv.PvlmError, match="below 8"):
            api.sift_extract(ctx, [bad], 10)
        with pytest.raises(pv.PvlmError, match="below 8"):
            api.sift_pyramid_debug(ctx, bad, 0)
    with pytest.raises(pv.PvlmError, match="one size"):
        api.sift_extract(ctx, [ok, ok[:, :90]], 10)
    for nf in (0, -3):
        with pytest.raises(pv.PvlmError, match="nfeatures"):
            api.sift_extract(ctx, [ok], nf)
    with pytest.raises(pv.PvlmError, match="flag"):
        api.sift_extract(ctx, [ok], 10, flags=0x2000)
    with pytest.raises(pv.PvlmError, match="octave"):
        api.sift_pyramid_debug(ctx, ok, 6)
    assert len(api.sift_extract(ctx, [np.zeros((8, 8), np.uint8)], 10)["keypoints"]) == 0      # the smallest image is served


def test_a_set_from_another_context_is_refused_down_the_chain(ctx, api):
    import panovlm_amd as pv
    r = api.sift_extract(ctx, [sr.blob_image(64, 96, 20), sr.blob_image(64, 96, 21)], 100, flags=api.FLAG_SIFT_ROOT)
    descs = [r["descriptors"][r["offsets"][i]:r["offsets"][i + 1]] for i in range(2)]
    other = pv.Context(0)
    try:
        ds = api.DescSet(other, descs)
        with pytest.raises(pv.PvlmError):
            api.match_pairs(ctx, ds, [0], [1], RATIO, 0)
        ds.close()
    finally:
        other.close()


def test_a_graph_capture_is_refused(ctx, api):
    import torch
    import panovlm_amd as pv
    img = sr.blob_image(64, 96, 20)
    before = api.sift_extract(ctx, [img], 100)
    dev = torch.device("cuda", 0)
    cam = torch.randn((64, 3), dtype=torch.float32).to(dev); px = torch.empty((64, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.graph_begin()
    try:
        ctx.cam_to_image_f32_dev(720, 1440, 64, cam.data_ptr(), px.data_ptr())             # so that the capture is not empty
        with pytest.raises(pv.PvlmError, match="capture"):
            api.sift_extract(ctx, [img], 100)
        with pytest.raises(pv.PvlmError, match="capture"):
            api.sift_pyramid_debug(ctx, img, 0)
    finally:
        g = ctx.graph_end()
    g.close()
    after = api.sift_extract(ctx, [img], 100)
    assert after["keypoints"].tobytes() == before["keypoints"].tobytes() and after["descriptors"].tobytes() == before["descriptors"].tobytes()


def _share(ka, kb, m):
    dx = ka["x"][m["query"]] - kb["x"][m["train"]]; dy = ka["y"][m["query"]] - kb["y"][m["train"]]
    return float((np.hypot(dx - SHIFT[0], dy - SHIFT[1]) <= 0.5).mean())


def test_the_chain_into_matching(ctx, api):
    """two 256 x 192 crops of one texture, shifted by (16, 8): pvlm_sift_extract (RootSIFT) -> pvlm_descset_create -> pvlm_match_pairs gives the match list of
    ExtractSIFTHost + MatchSIFT, and the share of matches displaced by the shift within 0.5 px is the restatement's, at least 0.8 for this seed"""
    a, b = sr.texture_crops(CHAIN_SEED, 192, 256, SHIFT)
    r = api.sift_extract(ctx, [a, b], 2000, flags=api.FLAG_SIFT_ROOT)
    off = r["offsets"]
    kd = [(r["keypoints"][off[i]:off[i + 1]], r["descriptors"][off[i]:off[i + 1]]) for i in range(2)]
    host = [sr.host_extract(im, 2000, None, True) for im in (a, b)]
    for (k, d), (hk, hd) in zip(kd, host):
        assert k.tobytes() == hk.tobytes() and d.tobytes() == hd.tobytes()
    ds = api.DescSet(ctx, [kd[0][1], kd[1][1]])
    try:
        got = api.match_pairs(ctx, ds, [0], [1], RATIO, 0)
    finally:
        ds.close()
    chk = mr.build_check()
    keep, want = mr.ref_pair_filter(mr.host_match_sift(chk, host[0][1], host[1][1], RATIO), 0)
    assert keep and got["keep"][0] == 1 and got["matches"].tobytes() == want.tobytes(), "the match lists are equal"
    share_dev = _share(kd[0][0], kd[1][0], got["matches"]); share_host = _share(host[0][0], host[1][0], want)
    # the restatement, once: its keypoints and descriptors, matched by the same MatchSIFT
    rest = [sr.Restatement(im).extract(2000, None, True) for im in (a, b)]
    rk = [sr.kp_array(k) for k, _ in rest]
    keep_r, mrest = mr.ref_pair_filter(mr.host_match_sift(chk, rest[0][1], rest[1][1], RATIO), 0)
    share_rest = _share(rk[0], rk[1], mrest)
    print("matches %d, share within 0.5 px of the shift: device %.4f host %.4f restatement %.4f" % (len(want), share_dev, share_host, share_rest))
    assert share_rest >= 0.8 and len(mrest) >= 50
    assert share_dev >= share_host - 0 and share_dev == share_rest


def test_driver_read_images_into_matching_equals_the_api(ctx, api, tmp_path):
    """tests/cpp/pvlm_sift_driver.cpp: ReadImages (three frames per call, frames handed over out of order) -> InitImagePairs (CONTIGUOUS) -> MatchImagePairs against
    pvlm_sift_extract -> pvlm_descset_create -> pvlm_match_pairs on the driver's pair list; the driver itself compares ExtractSIFTHost, Frame::ExtractKeyPoints /
    ComputeDescriptor and RootSIFT with what ReadImages filled"""
    import subprocess
    from panovlm_amd import build
    build.build_host()
    big = sr.blob_image(192, 256 + 3 * 12, CHAIN_SEED, blobs=260, noise=2)
    imgs = [np.ascontiguousarray(big[:, 12 * i:12 * i + 256]) for i in range(4)]
    src = tmp_path / "images.bin"; out = tmp_path / "out.bin"
    src.write_bytes(b"".join(im.tobytes() for im in imgs))
    threshold = 20
    run = subprocess.run([build.SIFT_DRIVER, str(src), "4", "192", "256", "300", "1", repr(RATIO), str(threshold), str(out)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = out.read_bytes()
    pos = 0
    r = api.sift_extract(ctx, imgs, 300, flags=api.FLAG_SIFT_ROOT)
    descs = []
    for i in range(4):
        m = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
        a, b = r["offsets"][i], r["offsets"][i + 1]
        assert m == b - a and m >= 50
        assert raw[pos:pos + 24 * m] == r["keypoints"][a:b].tobytes(); pos += 24 * m
        assert raw[pos:pos + 512 * m] == r["descriptors"][a:b].tobytes(); pos += 512 * m
        descs.append(r["descriptors"][a:b])
    n_pairs = int(np.frombuffer(raw, np.int64, 1, pos)[0]); pos += 8
    listed = [(i, j) for i in range(4) for j in range(i + 1, 4)]                       # CONTIGUOUS with a window of 20: every pair of four frames
    ds = api.DescSet(ctx, descs)
    try:
        want = api.match_pairs(ctx, ds, [p[0] for p in listed], [p[1] for p in listed], RATIO, threshold)
    finally:
        ds.close()
    kept = [p for p, k in zip(range(len(listed)), want["keep"]) if k]
    assert n_pairs == len(kept) >= 3
    got = {}
    for _ in range(n_pairs):
        a, b, m = (int(v) for v in np.frombuffer(raw, np.int64, 3, pos)); pos += 24
        got[(a, b)] = np.frombuffer(raw, np.int32, 2 * m, pos).reshape(m, 2); pos += 8 * m
    assert pos == len(raw)
    for p in kept:
        rec = want["matches"][want["offsets"][p]:want["offsets"][p + 1]]
        assert np.array_equal(got[listed[p]], np.stack([rec["query"], rec["train"]], 1))


def test_two_calls_give_identical_bytes(ctx, api, images):
    imgs = [images[(119, 161)], sr.blob_image(119, 161, 9)]
    a = api.sift_extract(ctx, imgs, 40, mask=_half_mask(119, 161), flags=api.FLAG_SIFT_ROOT)
    b = api.sift_extract(ctx, imgs, 40, mask=_half_mask(119, 161), flags=api.FLAG_SIFT_ROOT)
    assert a["keypoints"].tobytes() == b["keypoints"].tobytes() and a["descriptors"].tobytes() == b["descriptors"].tobytes() and np.array_equal(a["offsets"], b["offsets"])
    d1 = api.sift_pyramid_debug(ctx, imgs[0], 1); d2 = api.sift_pyramid_debug(ctx, imgs[0], 1)
    assert d1["gauss"].tobytes() == d2["gauss"].tobytes() and d1["dog"].tobytes() == d2["dog"].tobytes() and d1["candidates"].tobytes() == d2["candidates"].tobytes()
