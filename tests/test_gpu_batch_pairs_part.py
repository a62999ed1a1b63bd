"""Mixed-pair RLC batch check: the partitioned search for the invalid entries of a failing batch
(cpz_verify_batch_pairs_ex with CPZ_CALL_PARTITIONED, and the bisection's dense branch from
CPZ_BATCH_PAIRS_PART_MIN entries up).

Proofs, expected statuses (the C oracle under each entry's own pair) and expected partials are made
as in tests/test_gpu_batch_pairs.py, whose helpers are used here."""
import numpy as np
import pytest

import chaum_pedersen as cp
import pyoracle as O
import test_gpu_batch_pairs as BP
from chaum_pedersen import _native

pytestmark = pytest.mark.gpu

Q, SEED = BP.Q, BP.SEED
BLOCK = 128               # kPartProofs


def _forced(gpu, pairs, groups, rows, ctxs, **kw):
    out = gpu.verify_batch_pairs(pairs, groups, *BP._cols(rows), SEED, contexts=ctxs, locate="partitioned", **kw)
    return out, gpu.fallback_stats()


@pytest.fixture(scope="module")
def mix5(gpu):
    """1,283 valid proofs, entry i under pair i % 5 (the default pair and four custom ones)."""
    pairs = [cp.Parameters()] + BP._pairs(4, b"part5")
    n = 1283
    groups = np.arange(n) % 5
    ctxs = [BP._ctx(i) for i in range(n)]
    return pairs, groups, ctxs, BP._prove(gpu, pairs, groups, ctxs, b"p5")


@pytest.fixture(scope="module")
def mix64(gpu):
    """1,283 valid proofs, entry i under pair i % 64 (64 custom pairs)."""
    pairs = BP._pairs(64, b"part64")
    n = 1283
    groups = np.arange(n) % 64
    ctxs = [BP._ctx(i) for i in range(n)]
    return pairs, groups, ctxs, BP._prove(gpu, pairs, groups, ctxs, b"p64")


@pytest.mark.parametrize("equations_only", [False, True])
def test_forced_five_pairs(gpu, mix5, equations_only):
    """n = 1283 over 5 pairs: one forgery in block 0 (63), two in block 1 (128, 255), a mislabelled
    pair in block 2 (256), one in the 3-proof last block (1282); one entry of each decode-level kind
    elsewhere -- the bad point inside failing block 1, the others in otherwise clean blocks."""
    pairs, groups, ctxs, rows = mix5
    n = len(groups)
    groups = groups.copy()
    rows = {q: rows[q].copy() for q in Q}
    forged = [63, 128, 255, 256, 1282]
    for i in (63, 128, 255, 1282):
        BP._s_plus(rows, i, 1)
    groups[256] = (groups[256] + 1) % 5
    rows["r1"][130] = BP.BAD_POINT                          # undecodable point, in failing block 1
    BP._s_plus(rows, 700, O.L)                              # s + l: block 5, otherwise clean
    rows["r1"][900] = 0                                     # identity commitment: block 7
    rows["s"][1100] = 0                                     # zero s: block 8
    exp = BP._statuses(pairs, groups, rows, ctxs)
    assert [int(exp[i]) for i in forged + [130, 700, 900, 1100]] == [1] * 5 + [2, 3, 4, 5]
    assert (exp == 0).sum() == n - 9
    eq_sel = ()
    if equations_only:
        exp[[900, 1100]] = 1
        eq_sel = (900, 1100)
    want = BP._partial(pairs, groups, rows, ctxs, forged, eq_only_sel=eq_sel)
    (partial, ok, st), fb = _forced(gpu, pairs, groups, rows, ctxs, equations_only=equations_only)
    print("fallback stats:", fb)
    assert not ok and partial == want
    assert np.array_equal(st, exp), (np.nonzero(st != exp)[0][:8], st[st != exp][:8], exp[st != exp][:8])
    assert st.tobytes() == gpu.verify_each_pairs_bulk(pairs, groups, *BP._cols(rows), contexts=ctxs,
                                                      equations_only=equations_only).tobytes()
    assert fb["path"] == "partitioned"
    if not equations_only:
        assert fb["blocks_checked"] == 11 and fb["blocks_failing"] == 4
        assert fb["blocks_indexed"] == 4 and fb["blocks_located"] == 3
        assert fb["per_proof"] == 3 + BLOCK and fb["bisection_msms"] == 0


def test_forced_smallest(gpu):
    """n = 7 over 3 pairs on a fresh context: a passing batch reports "none" and builds no table;
    with two forgeries the statuses are exact and the path is "partitioned"."""
    pairs = [cp.Parameters()] + BP._pairs(2, b"part-small")
    idx = np.array([0, 1, 2, 1, 0, 2, 1], np.uint32)
    ctxs = [BP._ctx(i) for i in range(7)]
    rows = BP._prove(gpu, pairs, idx, ctxs, b"ps")
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        (partial, ok, st), fb = _forced(fresh, pairs, idx, rows, ctxs)
        times = fresh.stage_times()
        assert ok and partial == bytes(32) and st.tolist() == [0] * 7
        assert BP._no_table_was_built(times), times
        assert fb["path"] == "none"
        BP._s_plus(rows, 4, 1)
        bad = idx.copy()
        bad[5] = 1                                          # proven under pair 2, labelled pair 1
        exp = BP._statuses(pairs, bad, rows, ctxs)
        assert exp.tolist() == [0, 0, 0, 0, 1, 1, 0]
        want = BP._partial(pairs, bad, rows, ctxs, [4, 5])
        (partial, ok, st), fb = _forced(fresh, pairs, bad, rows, ctxs)
        assert not ok and partial == want and st.tolist() == exp.tolist()
        assert fb["path"] == "partitioned" and fb["blocks_checked"] == 1 and fb["blocks_failing"] == 1


def test_forced_dense_branch(gpu, mix64):
    """n = 261 over 64 pairs, one forgery in each of the three blocks: 3 > 3 / 2 failing blocks is
    the dense branch, every entry per proof."""
    pairs, groups, ctxs, rows = mix64
    n = 261
    groups = groups[:n].copy()
    ctxs = ctxs[:n]
    rows = {q: rows[q][:n].copy() for q in Q}
    forged = [5, 200, 260]
    for i in forged:
        BP._s_plus(rows, i, 1)
    exp = np.zeros(n, np.uint8)
    exp[forged] = 1
    (partial, ok, st), fb = _forced(gpu, pairs, groups, rows, ctxs)
    print("fallback stats:", fb)
    assert not ok and partial == BP._partial(pairs, groups, rows, ctxs, forged)
    assert st.tolist() == exp.tolist()
    assert st.tobytes() == gpu.verify_each_pairs_bulk(pairs, groups, *BP._cols(rows), contexts=ctxs).tobytes()
    assert fb["path"] == "partitioned" and fb["blocks_checked"] == 3 and fb["blocks_failing"] == 3
    assert fb["per_proof"] == n and fb["blocks_indexed"] == 0


def test_forced_64_pairs_all_located(gpu, mix64):
    """n = 1283 over 64 pairs, one forgery in each of blocks 0, 5 and 10: all three located."""
    pairs, groups, ctxs, rows = mix64
    n = len(groups)
    rows = {q: rows[q].copy() for q in Q}
    forged = [7, 5 * BLOCK + 64, 1282]
    assert [i // BLOCK for i in forged] == [0, 5, 10]
    for i in forged:
        BP._s_plus(rows, i, 1)
    exp = BP._statuses(pairs, groups, rows, ctxs)
    assert np.nonzero(exp)[0].tolist() == forged and exp[forged].tolist() == [1, 1, 1]
    (partial, ok, st), fb = _forced(gpu, pairs, groups, rows, ctxs)
    print("fallback stats:", fb)
    assert not ok and partial == BP._partial(pairs, groups, rows, ctxs, forged)
    assert st.tolist() == exp.tolist()
    assert fb["path"] == "partitioned" and fb["blocks_checked"] == 11 and fb["blocks_failing"] == 3
    assert fb["blocks_indexed"] == 3 and fb["blocks_located"] == 3 and fb["per_proof"] == 3


def test_automatic(gpu):
    """n = CPZ_BATCH_PAIRS_PART_MIN rounded up to 256, plus 259, over 5 pairs, one forgery in each
    of five of the eight top-level parts: the bisection's dense branch takes the partitioned
    search over the whole batch."""
    pairs = [cp.Parameters()] + BP._pairs(4, b"part-auto")
    n = (_native.BATCH_PAIRS_PART_MIN + 255) // 256 * 256 + 259
    groups = np.arange(n) % 5
    ctxs = [BP._ctx(i) for i in range(n)]
    rows = BP._prove(gpu, pairs, groups, ctxs, b"pa")
    cuts = BP._cuts(0, n)
    forged = [cuts[k] + 3 + 37 * k for k in (0, 2, 3, 5, 7)]
    assert all(cuts[k] <= f < cuts[k + 1] for k, f in zip((0, 2, 3, 5, 7), forged))
    assert len({f // BLOCK for f in forged}) == 5
    for i in forged:
        BP._s_plus(rows, i, 1)
    exp = np.zeros(n, np.uint8)
    exp[forged] = 1
    sample = sorted(set(forged + [f + d for f in forged for d in (-1, 1) if 0 <= f + d < n] + list(range(0, n, 211))))
    assert BP._statuses(pairs, groups[sample], {q: rows[q][sample] for q in Q},
                        [ctxs[i] for i in sample]).tolist() == exp[sample].tolist()
    partial, ok, st = gpu.verify_batch_pairs(pairs, groups, *BP._cols(rows), SEED, contexts=ctxs)
    fb = gpu.fallback_stats()
    print("fallback stats:", fb)
    assert not ok and partial == BP._partial(pairs, groups, rows, ctxs, forged)
    assert np.array_equal(st, exp), (np.nonzero(st != exp)[0][:8], st[st != exp][:8])
    assert fb["path"] == "partitioned" and fb["bisection_msms"] == BP.FANOUT and fb["per_proof"] == 5
    assert fb["blocks_checked"] == (n + BLOCK - 1) // BLOCK and fb["blocks_failing"] == 5 == fb["blocks_located"]


def test_one_pair_ignores_the_flag(gpu, mix5):
    """npairs == 1 delegates to the single-pair check, flag or not: its results."""
    pairs, groups, ctxs, rows = mix5
    rows = {q: rows[q].copy() for q in Q}
    for i in (6, 401):
        BP._s_plus(rows, i, 1)
    one = np.nonzero(groups == 1)[0]
    cols = BP._cols(rows, one)
    c1 = [ctxs[i] for i in one]
    got = gpu.verify_batch_pairs([pairs[1]], np.zeros(len(one), np.uint32), *cols, SEED, first_index=9, contexts=c1,
                                 locate="partitioned")
    fb = gpu.fallback_stats()
    ref = gpu.verify_batch(*cols, SEED, first_index=9, contexts=c1, params=pairs[1])
    assert got[0] == ref[0] and got[1] == ref[1] and got[2].tobytes() == ref[2].tobytes() and not got[1]
    assert fb == gpu.fallback_stats() and fb["path"] == "bisection"
