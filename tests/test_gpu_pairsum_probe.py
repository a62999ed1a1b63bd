"""The per-pair sum kernels of a mixed-pair batch over more than CPZ_PAIRS_MAX pairs (csrc/rlc.hip:
k_pair_hist, k_pair_scan, k_pair_scatter, k_pair_unit_sums, k_pair_finish) alone, on chosen pair
indices and products, through tests/native/pairsumprobe.hip.

What comes back -- the bucketed lists, both scans, the digits of every pair's two sums over the
range and the extras' points -- is compared with Python integers mod l (tests/pair_sum_model.py).
The lists are compared as sets per pair: the scatter's order inside a list is not fixed.
CPZ_PAIRSUMPROBE=<path> selects another build of the probe (a mutant)."""
import ctypes
import functools
import os
import random
import zlib

import numpy as np
import pytest

import pair_sum_model as M
import pyoracle as O

pytestmark = pytest.mark.gpu
L = O.L


@functools.lru_cache(maxsize=None)
def _probe():
    path = os.environ.get("CPZ_PAIRSUMPROBE")
    if not path:
        import build_native
        path = build_native.build_pairsumprobe()
    lib = ctypes.CDLL(path)
    ll, vp, ci = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int
    lib.pairsumprobe_const.restype = ll
    lib.pairsumprobe_const.argtypes = [ci]
    lib.pairsumprobe_run.argtypes = [ll, ci, vp, vp, vp, ll, ll, vp, vp, vp, vp, vp]
    return lib


def _U():
    return int(_probe().pairsumprobe_const(0))


def _case(name):
    """(npairs, pair_idx, prod integers [(a, b)], [ranges])."""
    U = _U()
    rng = random.Random(zlib.crc32(name.encode()))
    rnd = lambda n: [(rng.randrange(L), rng.randrange(L)) for _ in range(n)]
    if name == "one_pair_3U_plus_1":
        n = 3 * U + 1
        return 65, [7] * n, rnd(n), [(0, n), (256, 512)]
    if name == "every_entry_its_own_pair":
        n = 4096
        idx = list(range(n))
        rng.shuffle(idx)
        return n, idx, rnd(n), [(0, n), (256, 512)]
    if name == "first_and_last_pair_empty":
        n = 1000
        return 70, [1 + i % 68 for i in range(n)], rnd(n), [(0, n)]
    if name == "npairs_65_two_blocks":
        n = int(_probe().pairsumprobe_const(4)) + 905      # crosses a bucketing workgroup's chunk
        return 65, [rng.randrange(65) for _ in range(n)], rnd(n), [(0, n), (256, 512), (4000, n)]
    if name == "npairs_4096":
        n = 9001
        return 4096, [rng.randrange(4096) for _ in range(n)], rnd(n), [(0, n), (256, 512)]
    if name == "skewed_all_l_minus_1":
        n = 3 * U + 65
        return 65, [0] * (3 * U + 1) + list(range(1, 65)), [(L - 1, L - 1)] * n, [(0, n), (256, 512)]
    if name == "all_zero":
        n = 2 * U + 3
        return 65, [rng.randrange(65) for _ in range(n)], [(0, 0)] * n, [(0, n)]
    if name == "half_the_pairs_outside_the_range":
        n = 1200
        idx = [rng.randrange(50) if i < 600 else 50 + rng.randrange(50) for i in range(n)]
        return 100, idx, rnd(n), [(600, 1100), (0, 600)]
    if name == "n_1":
        return 65, [64], rnd(1), [(0, 1), (0, 0)]
    raise KeyError(name)


CASES = ["one_pair_3U_plus_1", "every_entry_its_own_pair", "first_and_last_pair_empty", "npairs_65_two_blocks",
         "npairs_4096", "skewed_all_l_minus_1", "all_zero", "half_the_pairs_outside_the_range", "n_1"]


def _words(x):
    return [(x >> (32 * k)) & 0xffffffff for k in range(8)]


@pytest.mark.parametrize("name", CASES)
def test_sums_and_lists(name):
    lib = _probe()
    U = _U()
    assert U == M.unit() and lib.pairsumprobe_const(1) == 4096 and lib.pairsumprobe_const(3) == 16
    nbytes = int(lib.pairsumprobe_const(2))
    npairs, idx, prod, ranges = _case(name)
    n = len(idx)
    d_idx = np.asarray(idx, np.uint32)
    d_prod = np.asarray([_words(v) for ab in prod for v in ab], np.uint32).reshape(n, 2, 8)
    gh = np.random.RandomState(7).randint(0, 256, size=(2 * npairs, nbytes)).astype(np.uint8)
    start, ustart, lists = M.bucket(idx, npairs, U)
    for lo, hi in ranges:
        lst = np.zeros(n, np.uint32)
        st = np.zeros(npairs + 1, np.uint32)
        us = np.zeros(npairs + 1, np.uint32)
        dig = np.zeros((16, 2 * npairs), np.int16)
        pts = np.zeros((2 * npairs, nbytes), np.uint8)
        rc = lib.pairsumprobe_run(n, npairs, d_idx.ctypes.data, d_prod.ctypes.data, gh.ctypes.data, lo, hi,
                                  lst.ctypes.data, st.ctypes.data, us.ctypes.data, dig.ctypes.data, pts.ctypes.data)
        assert rc == 0, (name, lo, hi, rc)
        assert st.tolist() == start.tolist() and us.tolist() == ustart.tolist()
        for p in range(npairs):
            assert sorted(lst[start[p]:start[p + 1]].tolist()) == lists[p].tolist(), (name, p)
        want = M.sums(idx, prod, npairs, lo, hi)
        exp = np.zeros((16, 2 * npairs), np.int64)
        for p, (sa, sb) in enumerate(want):
            exp[:, 2 * p] = M.digits(sa)
            exp[:, 2 * p + 1] = M.digits(sb)
        bad = np.nonzero((dig.astype(np.int64) != exp).any(axis=0))[0]
        assert bad.size == 0, (name, lo, hi, bad[:8])
        assert pts.tobytes() == gh.tobytes()
        # a pair with no entry in the range: zero digits
        inside = set(idx[lo:hi])
        for p in range(npairs):
            if p not in inside:
                assert not dig[:, 2 * p:2 * p + 2].any(), (name, p)


def test_the_cases_reach_their_edges():
    U = _U()
    npairs, idx, _, _ = _case("one_pair_3U_plus_1")
    assert len(idx) == 3 * U + 1 and set(idx) == {7}
    npairs, idx, _, _ = _case("every_entry_its_own_pair")
    assert sorted(idx) == list(range(npairs))
    npairs, idx, _, _ = _case("first_and_last_pair_empty")
    assert 0 not in idx and npairs - 1 not in idx and len(set(idx)) == npairs - 2
    npairs, idx, prod, _ = _case("skewed_all_l_minus_1")
    assert idx.count(0) == 3 * U + 1 and (3 * U + 1) * (L - 1) % L != 0 and set(prod) == {(L - 1, L - 1)}
    npairs, idx, _, ranges = _case("half_the_pairs_outside_the_range")
    lo, hi = ranges[0]
    assert len(set(idx[lo:hi])) <= npairs // 2 and min(idx[lo:hi]) >= 50
    assert {(256, 512)} <= set(_case("npairs_4096")[3]) and _case("npairs_4096")[0] == 4096
    assert _case("npairs_65_two_blocks")[0] == 65
