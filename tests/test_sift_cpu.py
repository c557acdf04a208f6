"""CPU checks of K41's definition: the host compile of csrc/pvlm_sift_core.h (tests/cpp/sift_core_check.cpp) against tests/sift_ref.py, the numpy restatement (a
second implementation that shares the core's coefficients and operation orders, see its docstring; the checks independent of the core are the blur against scipy,
the elementary functions against numpy / math and the single blob).  In float32 the restatement performs the same IEEE operations in the same order, so layers, candidates, keypoints and
descriptors are compared bit for bit; the refined fields are also compared with the same formulas evaluated in float64, within 4 x the deviation the float32
restatement itself shows against float64 on these images (figures next to the assertions and in profiles/HISTORY.md, K41)."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest
from scipy.ndimage import correlate1d

from tests import sift_ref as sr

SIZES = ((17, 33, 1), (64, 96, 7), (119, 161, 3))        # rows, cols, seed: 33 x 17, 96 x 64, 161 x 119 as width x height
MAIN = (119, 161, 3)                                      # the image of the candidate, field and selection tests


@pytest.fixture(scope="module")
def pyramids():
    out = {}
    for rows, cols, seed in SIZES:
        img = sr.blob_image(rows, cols, seed)
        out[(rows, cols)] = (img, sr.pyramid(img))
    return out


@pytest.fixture(scope="module")
def main(pyramids):
    img, p32 = pyramids[MAIN[:2]]
    A = sr.Restatement(img, np.float32, pyr=p32)
    cands, kps = A.detect()
    B = sr.Restatement(img, np.float64, pyr=[(g.astype(np.float64), d.astype(np.float64)) for g, d in p32])
    cands64, kps64 = B.detect()
    hc, hk, hct = sr.host_detect(img)
    return dict(img=img, A=A, B=B, cands=cands, kps=kps, cands64=cands64, kps64=kps64, hc=hc, hk=hk, hct=hct)


# ---- 1. pyramid and differences ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,seed", SIZES)
def test_pyramid_equals_the_restatement_bit_for_bit(pyramids, rows, cols, seed):
    img, pyr = pyramids[(rows, cols)]
    sizes = sr.host_sizes(rows, cols)
    m = min(2 * rows, 2 * cols)
    assert len(sizes) == int(np.rint(math.log2(m) - 2)) + 1 == len(pyr)                       # the formula
    assert sizes == sr.octave_sizes(rows, cols) and sizes[0] == (2 * rows, 2 * cols)
    for o in range(len(sizes)):
        g, d = sr.host_pyramid(img, o)
        assert g.shape[1:] == sizes[o]
        assert np.array_equal(g.view(np.uint32), pyr[o][0].view(np.uint32)), "Gaussian layers of octave %d" % o
        assert np.array_equal(d.view(np.uint32), pyr[o][1].view(np.uint32)), "difference layers of octave %d" % o
    if (rows, cols) == (17, 33):
        assert min(sizes[-1]) < 13, "the smallest octave is narrower than the radius of the widest kernel: the border folds more than once"


def test_kernels():
    K, HK = sr.kernels(), sr.host_kernels()
    assert [len(k) for k in K] == [11, 11, 13, 17, 21, 27]
    for a, b in zip(K, HK):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert abs(float(a.astype(np.float64).sum()) - 1.0) < 1e-6 and np.array_equal(a, a[::-1])


def test_blur_against_scipy(pyramids):
    K = sr.kernels()
    worst = 0.0
    for (rows, cols), (img, pyr) in pyramids.items():
        k0 = K[0].astype(np.float64)
        ref = correlate1d(correlate1d(sr.doubled(img).astype(np.float64), k0, axis=1, mode="mirror"), k0, axis=0, mode="mirror")
        worst = max(worst, float(np.abs(pyr[0][0][0] - ref).max()))
        for o, (g, d) in enumerate(pyr):
            hg, _ = sr.host_pyramid(img, o)
            for l in range(1, 6):
                k = K[l].astype(np.float64)
                ref = correlate1d(correlate1d(hg[l - 1].astype(np.float64), k, axis=1, mode="mirror"), k, axis=0, mode="mirror")
                worst = max(worst, float(np.abs(hg[l] - ref).max()))
    print("largest deviation of a float32 layer from the float64 correlation of its source layer: %.3g grey levels" % worst)
    # the restatement shows 6.84e-05 on these three images (it equals the host compile bit for bit); 4 x that
    assert worst <= 4 * 6.84e-05


def test_doubling_is_exact(pyramids):
    """the core's doubled_at (host compile) against the weights written out, and against the restatement in both float types"""
    img, _ = pyramids[(17, 33)]
    d = sr.host_doubled(img)
    assert np.array_equal(d.view(np.uint32), sr.doubled(img).view(np.uint32))
    assert d.shape == (34, 66) and d[0, 0] == img[0, 0] and d[-1, -1] == img[-1, -1]
    assert d[1, 1] == np.float32(0.75 * 0.75 * img[0, 0] + 0.75 * 0.25 * (float(img[0, 1]) + img[1, 0]) + 0.0625 * img[1, 1])
    assert np.array_equal(d, sr.doubled(img, np.float64).astype(np.float32))


# ---- 2. candidates -------------------------------------------------------------------------------------------------------------------------------------------
def test_candidates_equal_as_integer_sets(main):
    ct = main["A"].counters
    print(ct)
    assert ct["keypoints"] >= 50 and ct["multi_peak"] >= 1 and ct["moved"] >= 1
    assert ct["reject_moves"] >= 1 and ct["reject_contrast"] >= 1 and ct["reject_edge"] >= 1
    assert ct == main["hct"]
    want = {(c["octave"], c["layer"], c["r"], c["c"]) for c in main["cands"]}
    hc = main["hc"]
    got = {(int(c["octave"]), int(c["layer"]), int(c["r"]), int(c["c"])) for c in hc}
    assert got == want and len(hc) == len(main["cands"])
    # and in the defined order: octave, layer, row, column of the detection
    order = [(int(c["octave"]), int(c["det_layer"]), int(c["det_r"]), int(c["det_c"])) for c in hc]
    assert order == sorted(order) and order == [(c["octave"],) + c["det"] for c in main["cands"]]
    assert any((int(c["layer"]), int(c["r"]), int(c["c"])) != (int(c["det_layer"]), int(c["det_r"]), int(c["det_c"])) for c in hc), "a kept candidate that moved"


def test_keypoints_before_selection_bit_for_bit(main):
    assert sr.kp_array(main["kps"]).tobytes() == main["hk"].tobytes()


# ---- 3. refined fields, angles, descriptors against float64 ----------------------------------------------------------------------------------------------------
def test_fields_against_float64(main):
    c64, k64, hc, hk = main["cands64"], main["kps64"], main["hc"], main["hk"]
    assert [(c["octave"],) + c["det"] for c in c64] == [(int(c["octave"]), int(c["det_layer"]), int(c["det_r"]), int(c["det_c"])) for c in hc]
    assert [c["word"] for c in c64] == [int(c["word"]) for c in hc] and len(k64) == len(hk)
    dev = {n: max(abs(float(h[n]) - float(c[n])) for h, c in zip(hc, c64)) for n in ("x", "y", "size", "response")}
    dev["angle"] = max(abs(float(h["angle"]) - float(k["angle"])) for h, k in zip(hk, k64))
    print("host compile against float64:", dev)
    # float32 restatement against float64 on this image: x 1.33e-05, y 7.08e-06, size 2.11e-06, response 7.47e-09, angle 2.59e-05; 4 x each
    assert dev["x"] <= 4 * 1.33e-05 and dev["y"] <= 4 * 7.08e-06 and dev["size"] <= 4 * 2.11e-06 and dev["response"] <= 4 * 7.47e-09 and dev["angle"] <= 4 * 2.59e-05


def test_descriptors_against_float64(main):
    A, B, img = main["A"], main["B"], main["img"]
    sel64 = B.select(main["kps64"], 100000)
    ones = twos = 0
    worst_root = 0.0
    for root in (False, True):
        hk, hd = sr.host_extract(img, 100000, None, root)
        assert len(hk) == len(sel64) == len(A.select(main["kps"], 100000))
        for i, k in enumerate(sel64):
            d64 = B.descriptor(k, root)
            if root:
                worst_root = max(worst_root, float(np.abs(hd[i] - d64).max()))
            else:
                df = np.abs(hd[i] - d64)
                ones += int((df == 1).sum()); twos += int((df >= 2).sum())
                assert np.array_equal(hd[i], np.rint(hd[i])) and hd[i].min() >= 0 and hd[i].max() <= 255
    print("descriptor entries %d: differ by 1: %d, by 2 or more: %d; RootSIFT deviation %.3g" % (len(sel64) * 128, ones, twos, worst_root))
    # float32 restatement against float64: 0 of 9856 entries differ by 1, none by 2; RootSIFT entries deviate by 6.25e-06 at most
    assert twos == 0 and ones <= 4 * 0 and worst_root <= 4 * 6.25e-06


def test_descriptors_equal_the_restatement_bit_for_bit(main):
    A, img = main["A"], main["img"]
    sel = A.select(main["kps"], 100000)
    for root in (False, True):
        hk, hd = sr.host_extract(img, 100000, None, root)
        assert sr.kp_array(sel).tobytes() == hk.tobytes()
        d = np.stack([A.descriptor(k, root) for k in sel])
        assert d.view(np.uint32).tobytes() == hd.view(np.uint32).tobytes()


def test_elementary_functions():
    lib = sr.build_check()
    s, c = C.c_double(), C.c_double()
    worst = 0.0
    for a in np.linspace(0, 360, 1441).astype(np.float32):
        lib.chk_sift_sincos_deg(C.c_float(a), C.byref(s), C.byref(c))
        worst = max(worst, abs(s.value - math.sin(math.radians(float(a)))), abs(c.value - math.cos(math.radians(float(a)))))
        assert (s.value, c.value) == sr.sincos_deg(a) or abs(s.value - sr.sincos_deg(a)[0]) < 1e-15
    assert worst < 2e-15                                    # Taylor to x^23 on [0, pi / 2): truncation 1e-19, the rest is rounding
    rng = np.random.default_rng(5)
    yx = rng.normal(size=(4000, 2)).astype(np.float32)
    got = np.array([lib.chk_sift_atan2_deg(float(y), float(x)) for y, x in yx], np.float32)
    assert np.array_equal(got, sr.atan2_deg_v(yx[:, 0], yx[:, 1]))
    want = np.degrees(np.arctan2(yx[:, 0].astype(np.float64), yx[:, 1])) % 360.0
    err = np.abs(got - want); err = np.minimum(err, 360 - err)
    assert err.max() < 1.5e-3                               # the polynomial's 1.1e-5 rad = 6e-4 degrees, plus float32 rounding of values up to 360
    for t in (0.17, 0.5, 1.0, 1.16):
        assert abs(lib.chk_sift_pow2(t) / 2.0 ** float(np.float32(t)) - 1) < 2e-7 and lib.chk_sift_pow2(t) == sr.pow2(np.float32(t))


# ---- 4. independent of any restatement -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amp,bg", [(150, 40), (-100, 200)])
def test_single_blob_position_and_scale(amp, bg):
    """A Gaussian blob A exp(-r^2 / 2 s^2), s = 4 px, centred at (64.7, 63.3).  Blurred to scale sigma its centre value is A s^2 / (s^2 + sigma^2), so the difference
    of the layers k sigma and sigma is A s^2 (1 / (s^2 + k^2 sigma^2) - 1 / (s^2 + sigma^2)), extremal in sigma at sigma^2 = s^2 / k: the keypoint's size / 2, the
    sigma of the lower layer of the pair, is predicted at s / sqrt(k) = 3.564 (not s sqrt 2 = 5.657, the figure of a disc's radius under the Laplacian).  The
    quadratic fit through three layers a factor k apart locates the extremum within half a layer: the band is [k^-1/2, k^1/2] around the prediction.  The position
    carries the 0.25 px of the doubling's (d + 0.5) / 2 - 0.5 followed by a plain * 0.5; the 0.5 px bound holds with it."""
    s, cy, cx = 4.0, 63.3, 64.7
    yy, xx = np.mgrid[0:128, 0:128].astype(np.float64)
    img = np.clip(np.rint(bg + amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))), 0, 255).astype(np.uint8)
    kps, _ = sr.host_extract(img, 1000)
    assert len(kps) >= 1
    pos = {(float(k["x"]), float(k["y"]), float(k["size"])) for k in kps}
    assert len(pos) == 1, "one extremum, possibly several orientations"
    x, y, size = pos.pop()
    pred = s / math.sqrt(sr.K3)
    print("blob: x %.3f y %.3f size / 2 %.4f predicted %.4f ratio %.4f" % (x, y, size / 2, pred, size / 2 / pred))
    assert math.hypot(x - cx, y - cy) <= 0.5
    assert sr.K3 ** -0.5 <= (size / 2) / pred <= sr.K3 ** 0.5


# ---- 5. selection and RootSIFT ---------------------------------------------------------------------------------------------------------------------------------
def _records(n, seed):
    rng = np.random.default_rng(seed)
    k = np.zeros(n, sr.KP)
    k["x"] = rng.uniform(0, 300, n).astype(np.float32); k["y"] = rng.uniform(0, 200, n).astype(np.float32); k["size"] = rng.uniform(2, 9, n).astype(np.float32)
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32); k["response"] = rng.uniform(0.02, 0.2, n).astype(np.float32); k["octave"] = 1 + (2 << 8)
    return k


def _as_dicts(k):
    return [dict(x=r["x"], y=r["y"], size=r["size"], angle=r["angle"], response=r["response"], octave=int(r["octave"])) for r in k]


def test_retain_best_keeps_ties_and_order():
    k = _records(200, 1)
    thr = np.sort(k["response"])[::-1][49]
    k["response"][np.sort(np.argsort(k["response"])[:3])] = thr                  # the three weakest records now tie with the 50th largest response
    got = sr.host_select(k, 50, 100, 150)
    keep = k["response"] >= thr
    assert keep.sum() == 53 and len(got) == 53
    want = k[keep].copy()
    assert np.array_equal(got["response"], want["response"]), "a stable filter of the input order"
    assert np.array_equal(got["x"], want["x"] * np.float32(0.5)) and np.array_equal(got["size"], want["size"] * np.float32(0.5))
    assert np.all(got["octave"] == ((1 + (2 << 8)) & ~255 | 0))
    assert sr.kp_array(sr.Restatement(np.zeros((100, 150), np.uint8), pyr=[]).select(_as_dicts(k), 50)).tobytes() == got.tobytes()
    assert len(sr.host_select(k, 200, 100, 150)) == 200 and len(sr.host_select(k, 100000, 100, 150)) == 200


def test_duplicates_are_removed_first():
    k = _records(40, 2)
    k[7] = k[30]; k[12] = k[30]                       # equal x, y, size, angle
    k["response"][12] = 0.9                           # a duplicate with another response is still a duplicate: the first in order stays
    k[20]["angle"] = k[5]["angle"]; k[20]["x"] = k[5]["x"]          # three of the four fields equal: kept
    got = sr.host_select(k, 1000, 100, 150)
    assert len(got) == 38
    want = np.delete(k, [12, 30])
    assert np.array_equal(got["angle"], want["angle"]) and np.array_equal(got["response"], want["response"])
    assert sr.kp_array(sr.Restatement(np.zeros((100, 150), np.uint8), pyr=[]).select(_as_dicts(k), 1000)).tobytes() == got.tobytes()
    # the octave -1: octave 0 of the pyramid becomes byte 255
    z = _records(3, 3); z["octave"] = 0 + (1 << 8) + (77 << 16)
    assert np.all(sr.host_select(z, 10, 100, 150)["octave"] == 255 + (1 << 8) + (77 << 16))


def test_mask_is_applied_after_the_selection(main):
    img = main["img"]
    rows, cols = img.shape
    mask = np.zeros((rows, cols), np.uint8); mask[:, :cols // 2] = 1
    n = 20
    free, _ = sr.host_extract(img, n)
    got, _ = sr.host_extract(img, n, mask)
    assert len(free) >= n and 0 < len(got) < n, "the mask takes from the best n, it does not refill them"
    inside = mask[np.clip(np.rint(free["y"]).astype(int), 0, rows - 1), np.clip(np.rint(free["x"]).astype(int), 0, cols - 1)] != 0
    assert got.tobytes() == free[inside].tobytes() and np.all(np.rint(got["x"]) < cols // 2)
    sel = main["A"].select(main["kps"], n, mask)
    assert sr.kp_array(sel).tobytes() == got.tobytes()


def test_rootsift_rows():
    img = sr.blob_image(64, 96, 7)
    _, plain = sr.host_extract(img, 1000, None, False)
    _, root = sr.host_extract(img, 1000, None, True)
    assert len(root) >= 10
    assert np.abs(np.sqrt((root.astype(np.float64) ** 2).sum(1)) - 512.0).max() <= 1e-3
    l1 = plain.astype(np.float64).sum(1, keepdims=True)
    assert np.abs(root - np.sqrt(plain / l1) * 512).max() < 1e-4
    zero = sr.host_desc_finish(np.zeros(128, np.float32), True)
    assert not zero.any(), "a zero row stays zero"
    assert np.array_equal(zero, sr.Restatement(img, pyr=[]).desc_finish(np.zeros(128, np.float32), True))


# ---- 6. the stand-alone program --------------------------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_under_the_host_sanitizers():
    """tests/cpp/sift_core_check.cpp with its own main under -fsanitize=address,undefined: six sizes down to 8 x 8, with and without mask, RootSIFT and a small
    nfeatures"""
    exe = sr.build_check_main()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "MISMATCH" not in out.stdout and out.stdout.count(" ok") == 18
