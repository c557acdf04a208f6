"""The sizes at which the loops of panovlm_amd/csrc/pvlm_compact.h and pvlm_match.hip take their second trip, read from the sources (a changed constant
moves the shapes of tests/test_compaction_edges_*.py with it, a changed spelling fails the parse), and the inputs those tests share between their CPU half
(the references against each other, and the seed checks: the reference alone puts records on both sides of every edge) and their GPU half."""
import os
import re

import numpy as np

from tests import essential_ref as er
from tests import match_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "panovlm_amd", "csrc")


def _one(path, pattern):
    text = open(os.path.join(CSRC, path)).read()
    found = re.findall(pattern, text)
    if len(found) != 1:
        raise ValueError("%s: %d matches of %r (exactly one is expected)" % (path, len(found), pattern))
    return found[0]


def _int(path, pattern):
    """An integer constant: digits, or `1 << k` / `1ll << k`."""
    v = _one(path, pattern).strip()
    m = re.fullmatch(r"1(?:ll)?\s*<<\s*(\d+)", v)
    return 1 << int(m.group(1)) if m else int(v)


_NUM = r"((?:1(?:ll)?\s*<<\s*)?\d+)"
THREADS = _int("pvlm_compact.h", r"constexpr int kThreads = %s;" % _NUM)
ROUNDS = _int("pvlm_compact.h", r"constexpr int kRounds = %s;" % _NUM)
SCAN = _int("pvlm_compact.h", r"constexpr int kScanThreads = %s;" % _NUM)               # tile counts per trip of k_tile_scan
PIECE_POINTS = _int("pvlm_compact.h", r"constexpr long long kPiecePoints = %s;" % _NUM)
TILE = THREADS * ROUNDS                                                                 # points per tile: one workgroup, ROUNDS rounds of THREADS
SCREEN_Q = _int("pvlm_match.hip", r"constexpr int kScreenQ = %s;" % _NUM)
EXACT_GRID = _int("pvlm_match.hip", r"k_match_exact, dim3\(\(unsigned\)std::min<long long>\(\(nq \+ 3\) / 4, (\d+)\)\), dim3\(256\)")
FALLBACK_GRID = _int("pvlm_match.hip", r"k_match_exact, dim3\((\d+)\), dim3\(256\)")
MATCH_BATCH_PAIRS = _int("pvlm_match.hip", r"constexpr int kBatchPairs = %s;" % _NUM)
MATCH_BATCH_QUERIES = _int("pvlm_match.hip", r"constexpr long long kBatchQueries = %s;" % _NUM)
EXACT_ITEMS = 4 * EXACT_GRID                                                            # a wave per item, 4 waves per workgroup: one trip of the capped grid
FALLBACK_ITEMS = 4 * FALLBACK_GRID                                                      # ... and of the fallback launch
ESS_BATCH_CHAINS = _int("pvlm_essential.hip", r"constexpr int kBatchChains = %s;" % _NUM)
ESS_BATCH_MATCHES = _int("pvlm_essential.hip", r"constexpr long long kBatchMatches = %s;" % _NUM)
PIECE_SCANS = _int("pvlm_fuse.hip", r"constexpr int kPieceScans = %s;" % _NUM)
PIECE_PAIRS = _int("pvlm_texture.hip", r"constexpr int kPiecePairs = %s;" % _NUM)

MATCH_N2 = 70
MATCH_EDGE_N1 = (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
ESS_EDGE_N = (TILE, TILE + 1, 2 * TILE + 1)
ESS_RUNS, ESS_ITERS, ESS_TRI, ESS_SEED = 2, 8, 5, 7


def edge_rows(n):
    """The rows around every tile edge inside n points and around the end: e - 2 .. e + 1 for e = TILE, 2 TILE, ... and n - 2, n - 1."""
    rows = {n - 2, n - 1}
    for e in range(TILE, n + 1, TILE):
        rows.update((e - 2, e - 1, e, e + 1))
    return sorted(r for r in rows if 0 <= r < n)


def rounds_at_edges(n):
    """(lo, hi) of the last round of every full tile and of the first round of the tile behind it, as far as they hold points."""
    out = []
    for e in range(TILE, n + 1, TILE):
        out.append((e - THREADS, e))
        if e < n:
            out.append((e, min(e + THREADS, n)))
    return out


# ---- K33 ---------------------------------------------------------------------------------------------------------------------------------------
def match_edge_descriptors(n1, n2=MATCH_N2):
    """int_descriptors with near neighbours planted at the queries e - 1 and e of every tile edge e and at the last query (kept records on both sides of the
    edge whatever the generator's own stride of 7 gives), and the queries e - 2 and e + 1 left random (dropped: a mix right at the edge)."""
    rng = np.random.default_rng(5000 + n1)
    A, B = mr.int_descriptors(rng, n1, n2)
    plant = [n1 - 1] + [q for e in range(TILE, n1 + 1, TILE) for q in (e - 1, e) if q < n1]
    for q in plant:
        A[q] = B[int(rng.integers(2, n2 - 2))]
        A[q, rng.integers(0, mr.DIM, size=2)] = rng.integers(0, 256, size=2)
    for e in range(TILE, n1 + 1, TILE):
        for q in (e - 2, e + 1):
            if q < n1 and q != n1 - 1:
                A[q] = rng.integers(0, 256, size=mr.DIM)
    return A, B


def match_edges_reached(queries, n1):
    """The kept records' queries (of the reference) cover every round next to a tile edge, sit on e - 1 and e and on the last query, and skip e - 2."""
    q = np.asarray(queries)
    ok = all(((q >= lo) & (q < hi)).any() for lo, hi in rounds_at_edges(n1)) and (n1 - 1) in q
    for e in range(TILE, n1 + 1, TILE):
        ok = ok and (e - 1) in q and (e >= n1 or e in q) and (e - 2) not in q
    return bool(ok)


# ---- K34 ---------------------------------------------------------------------------------------------------------------------------------------
def essential_edge_scene(n):
    """n matches of a two-view scene with 5 % outliers; (b1, b2, matches).  The seed is one at which the pair is kept and the matches e - 1 and e of every tile
    edge are inliers (tests/test_compaction_edges_cpu.py asserts it)."""
    b1, b2, m, inl, R, t = er.two_view_scene(np.random.default_rng(100 + n), n, outlier_fraction=0.05)
    return b1, b2, m


def essential_edges_reached(inlier_idx, n):
    """inlier_idx has entries in the rounds on both sides of every tile edge, and on the rows e - 1 and e themselves where they exist."""
    j = np.asarray(inlier_idx)
    ok = all(((j >= lo) & (j < hi)).any() for lo, hi in rounds_at_edges(n))
    for e in range(TILE, n + 1, TILE):
        ok = ok and (e - 1) in j and (e >= n or e in j)
    return bool(ok)
