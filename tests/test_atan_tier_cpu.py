"""The short small-angle tier of atan_small (pvlm_functors.h: on a slot whose lanes all have tan r <= 1/32 the Horner chain is entered at a later one of
its ten coefficients) restated in numpy, every fma rounded once through np.longdouble, against np.arctan in np.longdouble.  The condition for the
entry point: the short chain's worst relative error on (0, 1/32] is not above the full chain's worst on (0, tan pi/8], both measured here, on the same
machine by the same code.  The coefficients and the entry point are read out of the header, so the test follows the code.  No device."""
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "panovlm_amd", "csrc", "pvlm_functors.h")
TAN_PI_8 = 0.41421356237309503       # the bound of atan_small in the header
TIER = 1.0 / 32.0
LD = np.longdouble

pytestmark = pytest.mark.skipif(np.finfo(LD).nmant < 63, reason="np.longdouble is no wider than double here: nothing to round through")


def header_chain():
    """(the ten coefficients of atan_small in the order of the chain, the index at which the short tier enters it)"""
    text = open(HEADER).read()
    body = text[text.index("double atan_small("):]
    body = body[:body.index("\n}\n")]
    coef = [float(x) for x in re.findall(r"-?\d\.\d+e-\d+", body)]
    assert len(coef) == 10, coef
    entry = int(re.search(r"#define PVLM_ATAN_TIER_ENTRY (\d+)", text).group(1))
    return coef, entry


def fma(a, b, c):
    return (LD(a) * LD(b) + LD(c)).astype(np.float64)


def atan_chain(t, coef, entry):
    """atan_small with the chain entered at coef[entry]: u = t * t, p = coef[entry], p = fma(p, u, c) for the coefficients behind it and 1.0, t * p"""
    u = t * t
    p = np.full_like(t, coef[entry])
    for c in coef[entry + 1:] + [1.0]:
        p = fma(p, u, np.full_like(t, c))
    return t * p


def arguments(hi, seed):
    """a dense grid of (0, hi], random arguments uniform in t and uniform in log t, hi itself and the next double above 0"""
    rng = np.random.default_rng(seed)
    grid = np.linspace(0.0, hi, 1_000_001)[1:]
    uni = rng.uniform(0.0, hi, 500_000)
    log = hi * np.exp2(-rng.uniform(0.0, 60.0, 500_000))
    t = np.concatenate([grid, uni, log, [hi, np.nextafter(0.0, 1.0)]])
    t = t[(t > 0) & (t <= hi)]
    assert t[-2] == hi and t[-1] == 5e-324
    return t


def worst_relative_error(t, approx):
    ref = np.arctan(t.astype(LD))
    return float(np.max(np.abs(approx.astype(LD) - ref) / ref))


@pytest.fixture(scope="module")
def figures():
    coef, entry = header_chain()
    t_full, t_tier = arguments(TAN_PI_8, 1), arguments(TIER, 2)
    full = atan_chain(t_tier, coef, 0)
    out = dict(coef=coef, entry=entry, full_wide=worst_relative_error(t_full, atan_chain(t_full, coef, 0)), full_tier=worst_relative_error(t_tier, full))
    for e in range(4, 8):
        short = atan_chain(t_tier, coef, e)
        out[e] = (worst_relative_error(t_tier, short), int(np.count_nonzero(short != full)))
    return out


def test_short_chain_is_no_worse_than_the_full_chain(figures):
    entry = figures["entry"]
    print("full chain: worst relative error %.3e on (0, tan pi/8], %.3e on (0, 1/32]" % (figures["full_wide"], figures["full_tier"]))
    for e in range(4, 8):
        print("entered at coefficient %d (%d steps shorter): worst relative error %.3e on (0, 1/32], differs from the full chain on %d arguments%s"
              % (e + 1, e, figures[e][0], figures[e][1], "   <- the header's tier" if e == entry else ""))
    assert 4 <= entry <= 6
    assert figures[entry][0] <= figures["full_wide"]


def test_header_takes_the_shortest_chain_that_passes(figures):
    """one step shorter than the header's tier must miss the condition, else the header leaves instructions on the table (entries 6 and 7 — the 6th and
    7th coefficient — are the candidates; the 8th drops a term of 1.1e-1 * 2^-40 and is far off)"""
    entry = figures["entry"]
    assert figures[entry + 1][0] > figures["full_wide"]


def test_edges(figures):
    coef, entry = figures["coef"], figures["entry"]
    t = np.array([TIER, np.nextafter(TIER, 0.0), np.nextafter(0.0, 1.0), 2.2250738585072014e-308, 1e-160])
    r = atan_chain(t, coef, entry)
    assert np.all(np.isfinite(r)) and np.all(r > 0) and np.all(r <= t)
    assert r[2] == t[2] and r[3] == t[3] and r[4] == t[4]              # u underflows or is negligible: atan t = t
    assert abs(r[0] - float(np.arctan(LD(TIER)))) <= np.spacing(r[0])
