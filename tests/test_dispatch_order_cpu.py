"""The dispatch order of the fused kernel on a point table (panovlm_amd/csrc/pvlm_dispatch_core.h) through its host compile (tests/cpp/dispatch_order_driver.cpp):
for random pair lists every work-list slot appears at exactly one grid position, every other position is -1, and the slots that read the same table slice (same
neighbour scan, same chunk number) have positions with the same residue modulo 8 (one XCD) that lie close together.  Cases: pairs without blocks, 1 - 9 blocks per
pair, neighbours shared by 1 - 8 pairs, totals that are no multiple of 8."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(ROOT, "build", "libdispatch_order_check.so")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "dispatch_order_driver.cpp")])
        _LIB = C.CDLL(out)
    return _LIB


def _order(nei, blocks):
    nei = np.ascontiguousarray(nei, np.int32); blocks = np.ascontiguousarray(blocks, np.int32)
    pos = np.full(int(blocks.sum()) * 8 + 64, -7, np.int32)
    n = _lib().chk_dispatch_order(C.c_int(len(nei)), nei.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), C.c_int(len(pos)))
    assert n >= 0
    assert np.all(pos[n:] == -7)                      # nothing written behind the positions returned
    return pos[:n]


def _check(nei, blocks):
    pos = _order(nei, blocks)
    slots = int(np.sum(blocks))
    real = pos[pos != -1]
    assert np.all((pos == -1) | ((pos >= 0) & (pos < slots)))              # padding is -1 and nothing else
    assert len(real) == slots and np.array_equal(np.sort(real), np.arange(slots))   # every slot exactly once
    where = np.empty(slots, np.int64); where[real] = np.nonzero(pos != -1)[0]
    groups, s = {}, 0
    for n, b in zip(nei, blocks):
        for c in range(int(b)):
            groups.setdefault((int(n), c), []).append(int(where[s])); s += 1
    largest = max((len(g) for g in groups.values()), default=0)
    for g in groups.values():
        assert len(set(x % 8 for x in g)) == 1                              # one residue modulo 8: one XCD
        assert max(g) - min(g) == 8 * (len(g) - 1)                          # eight apart, nothing between them: within a few dozen positions
    assert len(pos) - slots < 8 * max(largest, 1) + 8                      # padding stays small
    return pos


def _random_case(rng, n_nei, max_shared, max_blocks, min_blocks=0):
    nei, blocks = [], []
    for n in range(n_nei):
        for _ in range(int(rng.integers(1, max_shared + 1))):
            nei.append(3 + 5 * n); blocks.append(int(rng.integers(min_blocks, max_blocks + 1)))
    perm = rng.permutation(len(nei))
    return np.array(nei)[perm], np.array(blocks)[perm]


@pytest.mark.parametrize("seed", range(40))
def test_random_pair_lists(seed):
    rng = np.random.default_rng(seed)
    nei, blocks = _random_case(rng, int(rng.integers(1, 40)), 8, 9)        # 0 - 9 blocks, neighbours shared by 1 - 8 pairs
    _check(nei, blocks)


def test_pairs_without_blocks_and_the_empty_list():
    assert len(_order(np.zeros(0, np.int32), np.zeros(0, np.int32))) == 0
    assert len(_order([1, 2, 3], [0, 0, 0])) == 0
    _check([4, 4, 9, 4], [0, 3, 0, 2])


@pytest.mark.parametrize("total", [1, 7, 9, 15, 63, 65])
def test_totals_that_are_no_multiple_of_eight(total):
    _check([0], [total])                                                   # one pair: every group has one member
    _check(np.arange(total), np.ones(total, np.int32))                    # `total` groups of one


def test_benchmark_like_list_has_no_padding():
    """Every neighbour shared by 8 pairs of 4 chunks each: groups of 8, tiles of 64 positions, no padding, a group on one residue."""
    F = 64
    nei = np.repeat(np.arange(F), 8); blocks = np.full(F * 8, 4)
    pos = _check(nei, blocks)
    assert len(pos) == F * 8 * 4 and np.all(pos >= 0)


def test_identity_when_nothing_is_shared_in_size_order():
    """Groups of one member: the order is a permutation without padding except in the last tile."""
    pos = _check(np.arange(20), np.ones(20, np.int32))
    assert np.array_equal(pos[:16], np.arange(16))
