"""CPU checks of K37: the host compile of panovlm_amd/csrc/pvlm_depthfill_core.h (tests/cpp/depthfill_core_check.cpp) against the numpy restatement of
tests/depthfill_ref.py bit for bit; the restatement's own morphology and medians against scipy.ndimage; sel against upstream's multiply-add blend; exp_neg against
math.exp; what the entry points refuse; and the chain ComputeDepthImageHost -> SetTranslationScaleDepthMap."""
import math
import subprocess
from decimal import Decimal, getcontext

import numpy as np
import pytest

from tests import depthfill_ref as ref

M = ref.MAX_DEPTH
SHAPES = [(96, 160, 0.01), (67, 131, 0.004), (5, 7, 0.3), (1, 9, 0.5), (9, 1, 0.5)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def completed():
    """the restatement on the recipe shapes, computed once"""
    out = {}
    for rows, cols, p in SHAPES:
        img = ref.recipe(rows, cols, p)
        out[(rows, cols)] = (img, ref.complete(ref.as_f32(img), M))
    return out


@pytest.mark.parametrize("rows,cols,p", SHAPES)
def test_host_equals_restatement(completed, rows, cols, p):
    img, want = completed[(rows, cols)]
    rc, dense, u16, stats = ref.host_completion(img, M)
    assert rc == 0
    assert np.array_equal(_bits(dense), _bits(want["out"])) and np.array_equal(u16, want["u16"])
    assert stats == (want["valid_in"], want["valid_out"])


def test_recipe_reaches_every_branch(completed):
    """by the restatement alone: all three bands, both top masks cut, every fill round has work and unfilled pixels remain"""
    for key in ((96, 160), (67, 131)):
        w = completed[key][1]
        assert min(w["bands"]) > 0 and w["cut_top"] > 0 and min(w["round_work"]) > 0 and w["unfilled"] > 0, (key, w["bands"], w["round_work"])
    img = completed[(96, 160)][0]
    assert {int(round(d * 256)) for d in ref.DEPTHS} <= set(np.unique(img).tolist())


def test_all_zero_image_and_fp32_input_and_a_batch():
    zero = np.zeros((13, 21), np.uint16)
    rc, dense, u16, stats = ref.host_completion(zero, M)
    assert rc == 0 and not dense.any() and not u16.any() and stats == (0, 0)
    assert not ref.complete(ref.as_f32(zero), M)["out"].any()
    rng = np.random.default_rng(3)
    f = np.where(rng.random((40, 70)) < 0.02, rng.uniform(0.05, 45.0, (40, 70)), 0.0).astype(np.float32)   # depths that are no multiple of 1 / 256
    f[:8] = 0
    want = ref.complete(f, M)
    rc, dense, u16, _ = ref.host_completion(f, M)
    assert rc == 0 and np.array_equal(_bits(dense), _bits(want["out"])) and np.array_equal(u16, want["u16"])
    imgs = np.stack([ref.recipe(33, 65, 0.02, seed=s) for s in (1, 2, 3)])
    rc, dense, u16, _ = ref.host_completion(imgs, M, n_threads=3)
    for k in range(3):
        w = ref.complete(ref.as_f32(imgs[k]), M)
        assert np.array_equal(_bits(dense[k]), _bits(w["out"])) and np.array_equal(u16[k], w["u16"])


def test_max_depth_5_uses_the_near_band_only():
    img = ref.recipe(40, 50, 0.03)
    w = ref.complete(ref.as_f32(img), 5.0)
    assert w["bands"][0] > 0 and w["bands"][1:] == (0, 0)
    rc, dense, u16, _ = ref.host_completion(img, 5.0)
    assert rc == 0 and np.array_equal(_bits(dense), _bits(w["out"])) and np.array_equal(u16, w["u16"])


def test_restatement_morphology_and_medians_against_scipy():
    from scipy import ndimage
    rng = np.random.default_rng(5)
    for shape in ((31, 47), (5, 7), (1, 9), (9, 1)):
        img = np.where(rng.random(shape) < 0.3, rng.uniform(0, 40, shape), 0).astype(np.float32)
        for fp in (ref.cross(3), ref.cross(5), ref.cross(7), ref.full(5), ref.full(9)):
            assert np.array_equal(ref.dilate(img, fp), ndimage.grey_dilation(img, footprint=fp, mode="constant", cval=-np.inf))
            assert np.array_equal(ref.erode(img, fp), ndimage.grey_erosion(img, footprint=fp, mode="constant", cval=np.inf))
        assert np.array_equal(ref.median5(img), ndimage.median_filter(img, size=5, mode="nearest"))


def test_median_network_of_the_core():
    chk = ref.build_check()
    rng = np.random.default_rng(6)
    for _ in range(300):
        v = rng.integers(0, 6, 25).astype(np.float32) if rng.random() < 0.5 else rng.uniform(0, 40, 25).astype(np.float32)
        assert chk.chk_median25(v.ctypes.data_as(ref.C.c_void_p)) == np.sort(v)[12]


def test_sel_equals_the_multiply_add_blend(completed):
    for key in ((96, 160), (67, 131), (5, 7)):
        img, want = completed[key]
        got = ref.complete(ref.as_f32(img), M, blend=ref.muladd)
        assert np.array_equal(_bits(got["out"]), _bits(want["out"])), key


def test_u16_conversion_half_to_even_and_saturation():
    x = np.array([0.0, 0.5 / 256, 1.5 / 256, 2.5 / 256, 0.49 / 256, 39.99, 255.998, 256.0, 300.0, 65535.0 / 256, 65534.5 / 256, 0.1], np.float32)
    got = np.zeros(len(x), np.uint16)
    ref.build_check().chk_to_u16(ref.C.c_longlong(len(x)), x.ctypes.data_as(ref.C.c_void_p), got.ctypes.data_as(ref.C.c_void_p))
    assert np.array_equal(got, ref.to_u16(x)) and got[1] == 0 and got[2] == 2 and got[3] == 2 and got[7] == 65535 and got[8] == 65535


def test_exp_neg_against_math_exp(completed):
    """relative error <= 2^-50: with |r| <= ln2 / 2 the degree-13 Taylor polynomial truncates below 2^-57, and the handful of roundings of the reduction, the last Horner
    steps and the scaling stay within four ulp.  The measured maximum is printed (records it)."""
    rng = np.random.default_rng(8)
    sweep = np.concatenate([np.linspace(0.0, 708.0, 400_001)[:-1], rng.uniform(0, 708, 100_000), rng.uniform(0, 2, 100_000), np.nextafter(708.0, 0.0).reshape(1),
                            (np.arange(0, 1022) + 0.5) * math.log(2.0), np.nextafter((np.arange(0, 1022) + 0.5) * math.log(2.0), 0.0)])
    sweep = sweep[sweep < 708.0]
    recipe_args = np.concatenate([ref.bilateral_args(completed[k][1]["s7b"]) for k in ((96, 160), (67, 131), (5, 7), (1, 9))])
    x = np.concatenate([sweep, recipe_args[recipe_args < 708.0]])
    got = ref.exp_neg(x)
    want = np.array([math.exp(-v) for v in x])
    rel = np.abs(got - want) / want
    print("exp_neg: %d arguments, largest relative error %.3g = 2^%.2f" % (len(x), rel.max(), math.log2(rel.max())))
    assert rel.max() <= 2.0 ** -50
    assert np.array_equal(ref.host_exp_neg(x).view(np.uint64), got.view(np.uint64)), "the host compile and numpy give the same bits"
    big = np.array([708.0, 709.0, 3200.0, 1e300])
    assert not ref.exp_neg(big).any() and not ref.host_exp_neg(big).any() and (recipe_args >= 708.0).any()
    assert ref.exp_neg(np.array([0.0]))[0] == 1.0


def test_space_weights_are_exp_correctly_rounded():
    getcontext().prec = 60
    for d2, x in ((1, "0.125"), (2, "0.25"), (4, "0.5")):
        assert ref.WS[d2] == float((-Decimal(x)).exp()) == math.exp(-float(x))
    assert ref.WS[0] == 1.0


def test_reflect101_of_the_core():
    chk = ref.build_check()
    for n in (1, 2, 3, 4, 9):
        for i in range(-2, n + 2):
            assert chk.chk_reflect101(i, n) == ref.reflect101(i, n) and 0 <= ref.reflect101(i, n) < n
    assert [ref.reflect101(i, 5) for i in (-2, -1, 5, 6)] == [2, 1, 3, 2]


def test_refusals():
    chk = ref.build_check()
    C = ref.C
    img = ref.recipe(9, 11, 0.2); f = ref.as_f32(img)
    dense = np.zeros((9, 11), np.float32); u16 = np.zeros((9, 11), np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    call = lambda a16, a32, d, u, md=M: chk.chk_depth_completion(C.c_int(9), C.c_int(11), C.c_int(1), p(a16), p(a32), C.c_float(md), p(d), p(u), C.c_int(1), None)
    assert call(img, None, dense, u16) == 0 and call(None, f, dense, None) == 0
    assert call(img, f, dense, u16) == -1 and call(None, None, dense, u16) == -1            # both inputs, neither
    assert call(img, None, None, None) == -1                                                # no output
    for bad in (np.nan, np.inf, -1.0, -0.0):
        g = f.copy(); g[4, 5] = bad
        assert call(None, g, dense, None) == -1, bad
    assert call(img, None, dense, None, md=0.0) == -1 and call(img, None, dense, None, md=float("nan")) == -1
    clouds = [ref.synthetic_cloud(50, 1), ref.synthetic_cloud(20, 2)]
    assert ref.host_depth_images(30, 60, clouds, ref.T_CL, 4, M)[0] == 0
    assert ref.host_depth_images(30, 60, clouds, ref.T_CL, 4, M, first_point=[0, 50, 40])[0] == -1        # not ascending
    assert ref.host_depth_images(30, 60, clouds, ref.T_CL, 4, M, first_point=[1, 50, 70])[0] == -1        # does not start at 0


def test_compute_depth_image_host_is_splat_then_completion(oracle):
    """the host chain equals the oracle's ProjectLidar2PanoramaDepth followed by the restatement; a scan without points gives an all-zero image"""
    clouds = [ref.synthetic_cloud(900, 1), np.zeros((0, 3), np.float32), ref.synthetic_cloud(400, 3, radius=(0.5, 48.0))]
    for max_depth in (5.0, M):
        rc, got = ref.host_depth_images(90, 180, clouds, ref.T_CL, 4, max_depth)
        assert rc == 0 and not got[1].any()
        for k, c in enumerate(clouds):
            sparse = oracle.project_lidar_depth(90, 180, c, ref.T_CL, 4)
            assert k == 1 or sparse.any()
            assert np.array_equal(got[k], ref.complete(ref.as_f32(sparse), max_depth)["u16"]), (max_depth, k)


def test_depth_maps_of_the_host_mirror_give_the_pairs_their_scale():
    """pvlm::ComputeDepthImageHost -> MatchImagePairsHost -> FilterImagePairsFullHost through the driver, no device: the DepthMaps are what
    SetTranslationScaleDepthMap takes, and every surviving pair gets its baseline from them (the driver checks it)"""
    from panovlm_amd import build
    build.build_host()
    out = subprocess.run([build.DEPTHFILL_DRIVER, "host"], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host route only" in out.stdout and out.stdout.count("pair (") == 3
