"""GPU checks of K34 through the C ABI: pvlm_essential_acransac and pvlm_filter_image_pairs against the host compile of the same core
(tests/cpp/essential_core_check.cpp) bit for bit: E, nfa, the inlier lists and their order, keep, R_21, t_21, the triangulated points.  Small n_runs x
max_iterations (3 x 40) except for one case with the full parameters."""
import os
import subprocess

import numpy as np
import pytest

from tests import essential_ref as er

pytestmark = pytest.mark.gpu

SEED = 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import panovlm_amd as pv
    c = pv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chk():
    return er.build_check()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _scene(n, seed=3):
    """n matches of a two-view scene with 30 % outliers (n >= 9; below that the pose cannot matter)"""
    b1, b2, m, inl, R, t = er.two_view_scene(np.random.default_rng(seed + n), max(n, 1))
    return b1, b2, m[:n]


def _same_raw(g, h):
    assert np.array_equal(_bits(g["E"]), _bits(h["E"])), "E"
    assert np.array_equal(_bits(g["nfa"]), _bits(h["nfa"])), "nfa"
    assert np.array_equal(g["offsets"], h["offsets"]) and np.array_equal(g["inliers"], h["inliers"]), "inlier lists"


def _same_filter(g, h):
    assert np.array_equal(g["keep"], h["keep"]), "keep"
    assert np.array_equal(_bits(g["R_21"]), _bits(h["R_21"])) and np.array_equal(_bits(g["t_21"]), _bits(h["t_21"])), "pose"
    assert np.array_equal(g["offsets"], h["offsets"]) and np.array_equal(g["inlier_idx"], h["inlier_idx"]), "inlier_idx"
    assert np.array_equal(_bits(g["triangulated"]), _bits(h["triangulated"])), "triangulated"


def _both(ctx, chk, bearings, src, tgt, off, m, n_runs=3, max_iterations=40, tri=5, seed=SEED, flags=0):
    """Both entry points against the host compile; returns (raw, filter) of the device."""
    import panovlm_amd as pv
    rc, hr = er.host_acransac(chk, bearings, src, tgt, off, m, n_runs, max_iterations, seed, flags)
    assert rc == 0
    gr = pv.api.essential_acransac(ctx, bearings, src, tgt, off, m, n_runs, max_iterations, seed, flags)
    assert not gr["overflow"] and gr["guard_intact"]
    _same_raw(gr, hr)
    assert gr["stats"]["chains"] == hr["chains"] and gr["stats"]["hypotheses"] == hr["hypotheses"]
    rc, hf = er.host_filter(chk, bearings, src, tgt, off, m, tri, n_runs, max_iterations, seed, flags)
    assert rc == 0
    gf = pv.api.filter_image_pairs(ctx, bearings, src, tgt, off, m, tri, n_runs, max_iterations, seed, flags)
    assert not gf["overflow"] and gf["guard_intact"]
    _same_filter(gf, hf)
    assert gf["stats"]["hypotheses"] == hf["hypotheses"]
    return gr, gf


@pytest.mark.parametrize("n", [9, 10, 63, 64, 65, 257, er.N_LDS, er.N_LDS + 1])
def test_match_counts_against_the_host_compile(ctx, chk, n):
    """the smallest legal size, the wave boundaries, a sort that is no power of two, both sides of the fall-back"""
    b1, b2, m = _scene(n)
    gr, gf = _both(ctx, chk, [b1, b2], [0], [1], [0, n], m)
    st = gf["stats"]
    assert st["chains"] == 3
    assert (st["lds_chains"], st["fallback_chains"]) == ((3, 0) if n <= er.N_LDS else (0, 3))
    if n >= 63:
        assert gf["keep"][0] == 1 and gr["nfa"].min() < 0           # the checks above compared something


@pytest.mark.parametrize("n", [9, 10, 12])
def test_smallest_sizes_with_a_model(ctx, chk, n):
    """n exact matches and no outlier: at the smallest legal sizes a model is found, so the tail (DecomposeEssential, CheckRT, selection, scatter) runs on the device
    and the comparison is of non-zero E, non-empty inlier lists, a kept pair and its points"""
    b1, b2, m, inl, R, t = er.two_view_scene(np.random.default_rng(40 + n), n, outlier_fraction=0.0)
    gr, gf = _both(ctx, chk, [b1, b2], [0], [1], [0, n], m, tri=5)
    assert gr["nfa"].min() < 0 and gr["E"].any() and gr["offsets"][-1] >= 9
    assert gf["keep"][0] == 1 and len(gf["inlier_idx"]) >= 5 and np.isfinite(gf["triangulated"]).all()


def _ragged():
    """0, 8, 9, 65 and 300 matches; frame 1 is the target of one pair and the source of others"""
    sizes = [0, 8, 9, 65, 300]
    b1, b2, m = _scene(300)
    bearings = [b1, b2, b1[::-1].copy()]
    ms, src, tgt = [], [], []
    for i, n in enumerate(sizes):
        mm = m[:n].copy()
        if i % 2 == 0:
            src.append(0); tgt.append(1)
        else:                                                       # the same geometry seen from frame 1: query and train swapped
            mm["query"], mm["train"] = m[:n]["train"].copy(), m[:n]["query"].copy()
            src.append(1); tgt.append(0)
        ms.append(mm)
    off = np.concatenate([[0], np.cumsum(sizes)])
    return bearings, np.array(src), np.array(tgt), off, np.concatenate(ms), ms


def test_ragged_batch_equals_per_pair_calls_and_many_batches(ctx, chk, monkeypatch):
    import panovlm_amd as pv
    bearings, src, tgt, off, m, ms = _ragged()
    gr, gf = _both(ctx, chk, bearings, src, tgt, off, m)
    assert gf["keep"].tolist()[:2] == [0, 0] and gf["keep"][4] == 1
    for p in range(len(src)):                                      # per-pair calls
        one = pv.api.filter_image_pairs(ctx, bearings, src[p:p + 1], tgt[p:p + 1], [0, len(ms[p])], ms[p], 5, 3, 40, SEED)
        assert one["keep"][0] == gf["keep"][p] and np.array_equal(_bits(one["R_21"][0]), _bits(gf["R_21"][p])) and np.array_equal(_bits(one["t_21"][0]), _bits(gf["t_21"][p]))
        assert np.array_equal(one["inlier_idx"], gf["inlier_idx"][gf["offsets"][p]:gf["offsets"][p + 1]])
        assert np.array_equal(_bits(one["triangulated"]), _bits(gf["triangulated"][gf["offsets"][p]:gf["offsets"][p + 1]]))
        raw = pv.api.essential_acransac(ctx, bearings, src[p:p + 1], tgt[p:p + 1], [0, len(ms[p])], ms[p], 3, 40, SEED)
        assert np.array_equal(_bits(raw["E"][0]), _bits(gr["E"][p])) and np.array_equal(raw["inliers"], gr["inliers"][gr["offsets"][3 * p]:gr["offsets"][3 * p + 3]])
    monkeypatch.setenv("PVLM_ESSENTIAL_BATCH_PAIRS", "2")          # the same list cut into three batches
    gr2 = pv.api.essential_acransac(ctx, bearings, src, tgt, off, m, 3, 40, SEED)
    gf2 = pv.api.filter_image_pairs(ctx, bearings, src, tgt, off, m, 5, 3, 40, SEED)
    _same_raw(gr2, gr); _same_filter(gf2, gf)
    assert gf2["stats"] == gf["stats"]


def test_flags_and_seeds(ctx, chk):
    b1, b2, m = _scene(120)
    a, _ = _both(ctx, chk, [b1, b2], [0], [1], [0, 120], m, seed=1)
    b, _ = _both(ctx, chk, [b1, b2], [0], [1], [0, 120], m, seed=2)
    c, _ = _both(ctx, chk, [b1, b2], [0], [1], [0, 120], m, seed=1, flags=er.FRESH)
    assert not np.array_equal(a["E"], b["E"]) and not np.array_equal(a["E"], c["E"])


def test_full_parameters_on_two_pairs(ctx, chk):
    b1, b2, m = _scene(120)
    c1, c2, m2 = _scene(120, seed=9)
    gr, gf = _both(ctx, chk, [b1, b2, c1, c2], [0, 2], [1, 3], [0, 120, 240], np.concatenate([m, m2]), n_runs=40, max_iterations=300, tri=20)
    assert gf["keep"].tolist() == [1, 1] and gf["stats"]["chains"] == 80


def test_capacity_too_small(ctx, chk):
    import panovlm_amd as pv
    b1, b2, m = _scene(120)
    full = pv.api.filter_image_pairs(ctx, [b1, b2], [0, 0], [1, 1], [0, 120, 240], np.concatenate([m, m]), 5, 3, 40, SEED)
    assert full["needed"] > 12 and not full["overflow"]
    for cap in (0, 11, full["needed"] - 1):
        short = pv.api.filter_image_pairs(ctx, [b1, b2], [0, 0], [1, 1], [0, 120, 240], np.concatenate([m, m]), 5, 3, 40, SEED, capacity=cap)
        assert short["overflow"] and short["needed"] == full["needed"] and short["guard_intact"]
        assert np.array_equal(short["keep"], full["keep"]) and np.array_equal(short["offsets"], full["offsets"])
        assert np.array_equal(short["inlier_idx"], full["inlier_idx"][:cap]) and np.array_equal(_bits(short["triangulated"]), _bits(full["triangulated"][:cap]))
    again = pv.api.filter_image_pairs(ctx, [b1, b2], [0, 0], [1, 1], [0, 120, 240], np.concatenate([m, m]), 5, 3, 40, SEED, capacity=full["needed"])
    _same_filter(again, full)
    raw = pv.api.essential_acransac(ctx, [b1, b2], [0], [1], [0, 120], m, 3, 40, SEED)
    short = pv.api.essential_acransac(ctx, [b1, b2], [0], [1], [0, 120], m, 3, 40, SEED, capacity=10)
    assert short["overflow"] and short["needed"] == raw["needed"] and short["guard_intact"] and np.array_equal(short["inliers"], raw["inliers"][:10])
    assert np.array_equal(_bits(short["E"]), _bits(raw["E"]))


def test_argument_checks(ctx):
    import panovlm_amd as pv
    b1, b2, m = _scene(20)
    ok = dict(src=[0], tgt=[1], match_offsets=[0, 20], matches=m)
    def bad(**kw):
        a = dict(ok); a.update({k: v for k, v in kw.items() if k in a}); extra = {k: v for k, v in kw.items() if k not in a}
        with pytest.raises(pv.PvlmError):
            pv.api.filter_image_pairs(ctx, [b1, b2], a["src"], a["tgt"], a["match_offsets"], a["matches"], 5, extra.get("n_runs", 3), extra.get("max_iterations", 40), SEED)
    bad(tgt=[2]); bad(src=[-1]); bad(n_runs=0); bad(max_iterations=0); bad(match_offsets=[1, 20]); bad(match_offsets=[0, -1])
    mm = m.copy(); mm["query"][3] = len(b1)
    bad(matches=mm)
    with pytest.raises(pv.PvlmError):
        pv.api.essential_acransac(ctx, [b1, b2], [0], [5], [0, 20], m, 3, 40, SEED)
    empty = pv.api.filter_image_pairs(ctx, [b1, b2], [], [], [0], m[:0], 5, 3, 40, SEED)
    assert empty["needed"] == 0 and len(empty["keep"]) == 0


def test_driver_chain_match_then_filter():
    """MatchImagePairs -> FilterImagePairs of the host mirror on a synthetic scene: exits 0 with the kept pair's pose within the CPU test's bound (the driver checks it)"""
    from panovlm_amd import build
    build.build_host()
    out = subprocess.run([build.ESSENTIAL_DRIVER], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
