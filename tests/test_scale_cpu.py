"""CPU checks of K39's definition: the host compile of csrc/pvlm_scale_core.h (tests/cpp/scale_core_check.cpp, the lanes of the wave one after the other) against
both references of SetTranslationScaleDepthMap(eq, pair) -- rr.scale_ref, the numpy restatement, and rr.host_scale, relpose_detail::SetScaleOne -- bit for bit: ok,
t_21, every triangulated coordinate, points_with_depth, upper_scale, lower_scale.  Both sides run the same IEEE fp64 operations in the same order with contraction
off, so there is no tolerance.  Every scene states the exit it must take (read from the reference's outputs): a scene that drifts into another exit fails."""
import subprocess

import numpy as np
import pytest

from tests import relpose_ref as rr
from tests import scale_ref as sr

NO_START = (0, -1.0, -1.0)          # what a fresh TailPair holds: the references start from it


@pytest.fixture(scope="module")
def chk():
    return sr.build_check()


@pytest.fixture(scope="module")
def parent():
    return rr.build_check("off")


def _all_three(chk, parent, sc):
    """the core == the numpy restatement == SetScaleOne; returns (the reference's result, the survivor list, the core's own exit and count)"""
    ref = sr.reference(sc)
    host = rr.host_scale(parent, sc["eq_rows"], sc["eq_cols"], sc["rows1"], sc["d1"], sc["d2"], sc["R"], sc["t"], sc["X"])
    got = sr.host_core(chk, sc, NO_START)
    sr.same(host, ref)
    sr.same(got, ref)
    sr.same(got, host)
    return ref, sr.survivors(sc), got


_SCENES = sr.all_scenes()


@pytest.mark.parametrize("name,sc,want", _SCENES, ids=[s[0] for s in _SCENES])
def test_core_equals_both_references(chk, parent, name, sc, want):
    ref, scale, got = _all_three(chk, parent, sc)
    consistent = 0 if scale is None else len(scale) // 2
    took = sr.exit_of(ref, consistent)
    print(name, "points", len(sc["X"]), "consistent", consistent, "exit", took, "with depth", ref[3], "upper", ref[4], "lower", ref[5])
    if want is not None:
        assert took == want, (name, took, want)
    assert got[7] == consistent and got[6] == {"none": "none", "early": "mean", "histogram": "mean", "median": "median"}[took]


def test_every_exit_below_and_above_one_wave():
    """the early break, two histogram passes and the median fall-back, each at a size below and above 64 points (counted in points that gave a scale pair)"""
    seen = {}
    for name, sc, _ in _SCENES:
        scale = sr.survivors(sc)
        if not scale:
            continue
        took = sr.exit_of(sr.reference(sc), len(scale) // 2)
        if took == "histogram" and sr.passes(scale)[0] != 2:
            continue
        seen.setdefault(took, set()).add(len(scale) // 2 > 64)
    assert seen.get("early") == {False, True} and seen.get("histogram") == {False, True} and seen.get("median") == {False, True}, seen


def test_sizes_are_the_ones_stated():
    got = {len(sc["X"]) for name, sc, _ in _SCENES if name.startswith("true")}
    assert got == set(sr.SIZES)
    four = sr.survivors(dict(_S)["true4"]); five = sr.survivors(dict(_S)["true5"])
    assert len(four) == 8 and len(five) == 10                                   # 8 scales: not scaled; exactly 10: scaled


_S = [(n, s) for n, s, _ in _SCENES]


def test_special_cases_are_what_they_claim():
    by = dict(_S)
    # the maximum lands in bin index 10 (clamped), the minimum's quotient is negative (truncated to 0)
    scale = sr.survivors(by["clamp"])
    mx, mn = max(scale), min(scale)
    assert len(scale) >= 10 and mx / mn >= 1.2
    interval = (mx - mn) / 10
    assert int((mx - mn - 1e-8) / interval) == 10 and (mn - mn - 1e-8) / interval < 0
    # a bin holding exactly a tenth is dropped
    scale = sr.survivors(by["tenth"])
    assert len(scale) == 20
    ran, sizes = sr.passes(scale)
    assert sizes[0] == 18
    # ties at the median rank, even and odd point counts
    for name, n in (("median20", 20), ("median22", 22), ("median140", 140)):
        scale = sr.survivors(by[name])
        assert len(scale) == n
        srt = sorted(scale); k = n // 2
        assert srt[k] == srt[k + 1] or srt[k] == srt[k - 1]
    assert sr.passes(sr.survivors(by["median20"]))[1] == [0] and sr.passes(sr.survivors(by["median140"]))[1] == [0]
    # the seam: a point that rounds to column eq_cols is skipped; one pole is inside (row 0), the other rounds to row eq_rows
    X = by["seam_pole_full"]["X"]
    x_hi, _ = rr._cam_to_image(sr.ROWS, sr.COLS, X[-4])
    assert rr._round_half_away(x_hi) == sr.COLS
    assert rr._round_half_away(rr._cam_to_image(sr.ROWS, sr.COLS, X[-1])[1]) == 0 and rr._round_half_away(rr._cam_to_image(sr.ROWS, sr.COLS, X[-2])[1]) == sr.ROWS
    # the skip rule: points inside the image but outside the smaller map
    small = by["map2_smaller"]
    full = dict(small); full["d2"] = sr.depth_scene(9, 120)["d2"]
    assert 10 <= len(sr.survivors(small)) < len(sr.survivors(full))
    assert by["zero_and_65535"]["d1"].max() == 65535 and by["full_and_half"]["d1"].shape == (sr.ROWS, sr.COLS)


def test_start_values_stay_where_the_step_does_not_write(chk):
    by = dict(_S)
    got = sr.host_core(chk, by["empty_map1"])
    assert not got[0] and (got[3], got[4], got[5]) == sr.START                  # a map is missing: nothing is touched
    got = sr.host_core(chk, by["inconsistent"])
    assert not got[0] and (got[3], got[4], got[5]) == (0, sr.START[1], sr.START[2])   # both maps there: points_with_depth = 0, the bounds untouched
    assert np.array_equal(got[1], by["inconsistent"]["t"]) and np.array_equal(got[2], by["inconsistent"]["X"])


def test_stand_alone_program_under_the_host_sanitizers():
    """tests/cpp/scale_core_check.cpp with its own main under -fsanitize=address,undefined: 0 .. 700 points, three kinds of scene, half- and full-size maps, each
    compared with SetScaleOne inside the program"""
    exe = sr.build_check_main()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "MISMATCH" not in out.stdout and out.stdout.count("equal") == 60
