"""The host build of csrc/pair_sum.h (the unit partition of the per-pair sums and the run cutter of
cpz_verify_batch_pairs_many's per-proof leaves) against the plain model of tests/pair_sum_model.py.
No GPU."""
import random

import numpy as np
import pytest

import pair_sum_model as M

PAIRS_MAX = 64


def _lib_runs(idx, lo, hi, npairs, max_pairs=PAIRS_MAX):
    idx = np.ascontiguousarray(idx, np.uint32)
    m = max(hi - lo, 1)
    ends = np.zeros(m, np.int64)
    counts = np.zeros(m, np.int32)
    firsts = np.zeros(m, np.uint32)
    r = M.hostlib().pairsum_runs(idx.ctypes.data, lo, hi, npairs, max_pairs, ends.ctypes.data, counts.ctypes.data,
                                 firsts.ctypes.data)
    return [(int(ends[k]), int(counts[k]), int(firsts[k])) for k in range(r)]


def test_unit_counts():
    U = M.unit()
    assert U >= 64 and U % 64 == 0          # whole waves of list entries
    lib = M.hostlib()
    for c in [0, 1, U - 1, U, U + 1, 3 * U, 3 * U + 1, (1 << 20) - 1, 1 << 20]:
        assert lib.pairsum_units(c) == M.units(c, U), c
    assert M.units(0, U) == 0 and M.units(1, U) == 1 and M.units(3 * U + 1, U) == 4
    # the bound the unit scratch is sized by holds for every split of n entries over the pairs
    rng = random.Random(5)
    for _ in range(200):
        npairs = rng.randrange(1, 300)
        n = rng.randrange(1, 5000)
        cuts = sorted(rng.randrange(0, n + 1) for _ in range(npairs - 1))
        counts = [b - a for a, b in zip([0] + cuts, cuts + [n])]
        assert sum(M.units(c, U) for c in counts) <= lib.pairsum_max_units(n, npairs)
    assert lib.pairsum_max_units(3 * U + 1, 1) == 4      # tight: one pair, one partial unit


@pytest.mark.parametrize("name", ["one_pair", "own_pair", "ends_empty", "skewed", "random"])
def test_unit_owner(name):
    U = M.unit()
    rng = random.Random(11)
    if name == "one_pair":
        npairs, idx = 65, [7] * (3 * U + 1)
    elif name == "own_pair":
        npairs, idx = 300, list(range(300))
    elif name == "ends_empty":
        npairs, idx = 70, [1 + i % 68 for i in range(1000)]
    elif name == "skewed":
        npairs, idx = 65, [0] * (3 * U + 1) + list(range(1, 65))
    else:
        npairs, idx = 200, [rng.randrange(200) if rng.random() < 0.6 else 3 for _ in range(5000)]
    start, ustart, lists = M.bucket(idx, npairs, U)
    table = M.unit_table(start, ustart, U)
    assert len(table) == ustart[-1] <= M.hostlib().pairsum_max_units(len(idx), npairs)
    us = np.ascontiguousarray(ustart, np.uint32)
    for u, (p, j0, j1) in enumerate(table):
        assert M.hostlib().pairsum_find(us.ctypes.data, npairs, u) == p == M.find(ustart, u), (name, u)
        assert 0 < j1 - j0 <= U and start[p] <= j0 and j1 <= start[p + 1]
    # the units partition every list
    covered = sorted(j for _, j0, j1 in table for j in range(j0, j1))
    assert covered == list(range(len(idx)))
    if name == "one_pair":
        assert [j1 - j0 for _, j0, j1 in table] == [U, U, U, 1]
    if name == "ends_empty":
        assert ustart[0] == ustart[1] == 0 and ustart[-1] == ustart[-2]


def test_runs_of_exactly_64_and_65_pairs():
    idx = list(range(64)) * 3
    assert _lib_runs(idx, 0, len(idx), 64) == M.runs(idx, 0, len(idx), 64) == [(192, 64, 0)]
    idx = list(range(65)) * 3
    want = M.runs(idx, 0, len(idx), 64)
    assert _lib_runs(idx, 0, len(idx), 65) == want
    # 0..63 | 64, 0..62 | 63, 64, 0..61 | 62, 63, 64
    assert want == [(64, 64, 0), (128, 64, 64), (192, 64, 63), (195, 3, 62)]


def test_run_boundary_on_the_first_and_last_entry():
    # the 65th pair is the last entry: the last run is that entry alone
    idx = list(range(64)) * 2 + [64]
    assert _lib_runs(idx, 0, len(idx), 65) == M.runs(idx, 0, len(idx), 64) == [(128, 64, 0), (129, 1, 64)]
    # max_pairs = 1 and a change after the first entry: the first run is that entry alone
    idx = [5, 9, 9, 9]
    assert _lib_runs(idx, 0, 4, 10, 1) == M.runs(idx, 0, 4, 1) == [(1, 1, 5), (4, 1, 9)]
    # a sub-range: the stamps of a run do not leak into the next range
    idx = list(range(130))
    assert _lib_runs(idx, 1, 130, 130) == M.runs(idx, 1, 130, 64) == [(65, 64, 1), (129, 64, 65), (130, 1, 129)]
    assert _lib_runs(idx, 129, 130, 130) == [(130, 1, 129)]
    assert _lib_runs(idx, 7, 7, 130) == []


def test_one_pair_throughout():
    idx = [3] * 5000
    assert _lib_runs(idx, 0, 5000, 4096) == M.runs(idx, 0, 5000, 64) == [(5000, 1, 3)]


def test_random_runs():
    rng = random.Random(2)
    for _ in range(40):
        npairs = rng.randrange(1, 400)
        n = rng.randrange(1, 3000)
        idx = [rng.randrange(npairs) for _ in range(n)]
        lo = rng.randrange(0, n)
        hi = rng.randrange(lo, n + 1)
        got = _lib_runs(idx, lo, hi, npairs)
        assert got == M.runs(idx, lo, hi, PAIRS_MAX)
        a = lo
        for e, k, _ in got:
            assert len(set(idx[a:e])) == k <= PAIRS_MAX
            assert e == hi or (k == PAIRS_MAX and idx[e] not in set(idx[a:e]))   # the longest such run
            a = e
        assert a == hi or (lo == hi and not got)
