"""RLC batch check over up to 4096 (g, h) pairs in one MSM (cpz_verify_batch_pairs_many): above
CPZ_PAIRS_MAX pairs the descriptors are built on the device, the per-pair sums come from the
bucketed lists, a passing batch builds no table, and a failing one is bisected down to single
weight blocks whose entries are verified in runs of at most 64 distinct pairs.

Many generator pairs come from one gpu.prove under the default pair (y1 = [a] B, y2 = [a] H: a
valid, distinct (g, h) row per entry); proofs from gpu.prove_pairs, 64 pairs a call.  Expected
statuses and partials are the C oracle's, per pair, as in tests/test_gpu_batch_pairs.py, whose
helpers are used here (the partial from the forged entries alone: a valid entry adds the
identity)."""
import ctypes
import hashlib

import numpy as np
import pytest

import chaum_pedersen as cp
import pair_sum_model as M
import pyoracle as O
import test_gpu_batch_pairs as B
from chaum_pedersen import _native

pytestmark = pytest.mark.gpu

Q = B.Q
SEED = B.SEED
PREP_BLOCK, PREP_WIDE_MAX, FANOUT = B.PREP_BLOCK, B.PREP_WIDE_MAX, B.FANOUT
PAIRS_MAX, PAIRS_MAX_PROOFS = 64, 2048
BAD_POINT = B.BAD_POINT


def _scalars(tag, n):
    a = np.frombuffer(b"".join(hashlib.sha256(tag + b"-%d" % i).digest() for i in range(n)), np.uint8).reshape(n, 32)
    a = a.copy()
    a[:, 31] &= 0x0f          # below 2^252 < l
    return a


def _many_pairs(gpu, k, tag):
    """k valid, distinct pairs from one prove under the default pair: (y1_i, y2_i) = ([a_i] B, [a_i] H)."""
    out = gpu.prove(_scalars(tag + b"-a", k), _scalars(tag + b"-k", k))
    return [cp.Parameters(out["y1"][i].tobytes(), out["y2"][i].tobytes()) for i in range(k)]


def _prove_many(gpu, pairs, proven, ctxs, tag):
    """Valid proofs, entry i under pairs[proven[i]], 64 pairs per prove_pairs call."""
    proven = np.asarray(proven, np.int64)
    n = len(proven)
    xs, ks = _scalars(tag + b"-x", n), _scalars(tag + b"-k", n)
    rows = {q: np.zeros((n, 32), np.uint8) for q in Q}
    for c in range(0, len(pairs), PAIRS_MAX):
        sel = np.nonzero((proven >= c) & (proven < c + PAIRS_MAX))[0]
        if not len(sel):
            continue
        out = gpu.prove_pairs(pairs[c:c + PAIRS_MAX], proven[sel] - c, np.ascontiguousarray(xs[sel]),
                              np.ascontiguousarray(ks[sel]), contexts=[ctxs[i] for i in sel])
        for q in Q:
            rows[q][sel] = out[q]
    return rows


def _cuts(lo, hi):
    """pairs_many_fallback's cuts: a part per weight block up to FANOUT blocks, else FANOUT aligned parts."""
    if hi - lo <= FANOUT * PREP_BLOCK:
        return [min(lo + k * PREP_BLOCK, hi) for k in range(FANOUT + 1)]
    return B._cuts(lo, hi)


def _route(idx, lo, hi, weighted_bad, depth=0):
    """(leaves, MSMs) of the bisection over [lo, hi): weighted_bad are the invalid entries that
    carry weight (a decode-level failure carries none and fails no part)."""
    leaf = hi - lo <= PAIRS_MAX_PROOFS or depth > 12
    if leaf and depth <= 12 and hi - lo > PREP_BLOCK and len(set(idx[lo:hi].tolist())) > PAIRS_MAX:
        leaf = False
    if leaf:
        return [(lo, hi)], 0
    c = _cuts(lo, hi)
    parts = [(c[k], c[k + 1]) for k in range(FANOUT) if c[k + 1] > c[k]]
    failing = [p for p in parts if any(p[0] <= f < p[1] for f in weighted_bad)]
    if 2 * len(failing) > FANOUT:
        return [(lo, hi)], len(parts)
    leaves, msms = [], len(parts)
    for a, b in failing:
        lv, m = _route(idx, a, b, weighted_bad, depth + 1)
        leaves += lv
        msms += m
    return leaves, msms


def _run_pairs(idx, leaves):
    """Distinct pairs per run, summed over the runs of the leaves."""
    return sum(k for lo, hi in leaves for _, k, _ in M.runs(idx, lo, hi, PAIRS_MAX))


def _sets_built(times):
    return times.get("generators_varbase", (0.0, 0))[1]


def _raw(gpu, flags, pairs, idx, rows, ctxs, first_index=0):
    """The C entry point itself (the wrapper passes no CPZ_CALL_PARTITIONED)."""
    n = len(idx)
    idx = np.ascontiguousarray(idx, np.uint32)
    gh = np.frombuffer(b"".join(p.g + p.h for p in pairs), np.uint8)
    cols = B._cols(rows)
    blob, off, present = cp._ctx_arrays(ctxs, n)
    partial = ctypes.create_string_buffer(32)
    ok = ctypes.c_int(0)
    out = np.empty(n, np.uint8)
    _native.check(gpu._lib.cpz_verify_batch_pairs_many(
        gpu._h, flags, len(pairs), cp._ptr(gh), n, cp._ptr(idx), *[cp._ptr(a) for a in cols], cp._ptr(blob),
        cp._ptr(off), cp._ptr(present), SEED, first_index, partial, ctypes.byref(ok), cp._ptr(out)))
    return partial.raw, bool(ok.value), out


@pytest.fixture(scope="module")
def pool(gpu):
    """1000 distinct pairs."""
    return _many_pairs(gpu, 1000, b"pool")


@pytest.fixture(scope="module")
def mix65(gpu, pool):
    """130 valid proofs over 65 pairs, entry i under pair i % 65."""
    pairs = pool[:65]
    idx = (np.arange(130) % 65).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(130)]
    return pairs, idx, ctxs, _prove_many(gpu, pairs, idx, ctxs, b"m65")


def test_smallest_passing_batch(gpu, mix65):
    """n = 130 over 65 pairs on a fresh context: batch_ok, the identity partial, no table built."""
    pairs, idx, ctxs, rows = mix65
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        partial, ok, st = fresh.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs)
        times = fresh.stage_times()
        assert ok and partial == bytes(32) and st.tolist() == [0] * 130
        assert B._no_table_was_built(times), times
        assert fresh.fallback_stats()["path"] == "none"
        partial, ok, st = fresh.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs, statuses=False)
        assert ok and partial == bytes(32) and st is None


def test_one_pair_per_entry(gpu, pool):
    """n = npairs = 300, every entry its own pair, contexts cycling the four shapes; s + 1, a
    mislabelled pair and undecodable points.  The forgeries that carry weight lie in the first
    weight block, so the second (44 entries, one of them undecodable) is cleared by its MSM and
    the tables built are those of the first block's runs."""
    n = 300
    pairs = pool[:n]
    idx = np.arange(n, dtype=np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    proven = idx.copy()
    proven[100] = 101                                   # proven under pair 101, labelled pair 100
    rows = _prove_many(gpu, pairs, proven, ctxs, b"own")
    B._s_plus(rows, 3, 1)
    rows["r1"][200] = BAD_POINT
    rows["y2"][280] = BAD_POINT
    exp = B._statuses(pairs, idx, rows, ctxs)
    assert np.nonzero(exp)[0].tolist() == [3, 100, 200, 280] and exp[[3, 100, 200, 280]].tolist() == [1, 1, 2, 2]
    want = B._partial(pairs, idx, rows, ctxs, [3, 100])
    leaves, msms = _route(idx, 0, n, [3, 100])
    assert leaves == [(0, 256)] and msms == 2
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        partial, ok, st = fresh.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs)
        times = fresh.stage_times()
        fb = fresh.fallback_stats()
    assert not ok and partial == want
    assert np.array_equal(st, exp), (np.nonzero(st != exp)[0][:8], st[st != exp][:8])
    assert fb["path"] == "bisection" and fb["per_proof"] == 256 and fb["bisection_msms"] == 2, fb
    assert _sets_built(times) == _run_pairs(idx, leaves) == 256 != n, times
    assert times.get("generators", (0.0, 0))[1] == 0, times


def test_sparse_pair_list(gpu, pool):
    """200 rows of which 70 carry entries, a repeated row (150 repeats 20, both used) and the
    default pair at row 130."""
    pairs = list(pool[:200])
    pairs[130] = cp.Parameters()
    pairs[150] = pairs[20]
    used = sorted(set(range(2, 200, 3)) | {0, 1, 130, 150})
    assert 20 in used
    assert len(used) == 70 and len(pairs) == 200
    n = 280
    idx = np.asarray([used[i % 70] for i in range(n)], np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    rows = _prove_many(gpu, pairs, idx, ctxs, b"sparse")
    got = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs)
    assert got[0] == bytes(32) and got[1] and not got[2].any()
    # entries proven under row 20 verify under row 150 and the reverse
    swapped = np.where(idx == 20, 150, np.where(idx == 150, 20, idx)).astype(np.uint32)
    got = gpu.verify_batch_pairs_many(pairs, swapped, *B._cols(rows), SEED, contexts=ctxs)
    assert got[0] == bytes(32) and got[1]
    forged = [int(np.nonzero(idx == 130)[0][1]), int(np.nonzero(idx == 150)[0][0]), 279]
    for i in forged:
        B._s_plus(rows, i, 1)
    exp = B._statuses(pairs, idx, rows, ctxs)
    assert np.nonzero(exp)[0].tolist() == sorted(forged)
    partial, ok, st = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs)
    assert not ok and partial == B._partial(pairs, idx, rows, ctxs, forged)
    assert np.array_equal(st, exp)
    assert gpu.fallback_stats()["path"] == "bisection"


def test_skewed_batch(gpu, pool):
    """npairs = 65, n = 3 U + 65: pair 0 holds all entries but 64 (four work units, the last with
    one entry), pairs 1 .. 64 one each; one forgery in pair 0 and one in pair 64."""
    U = M.unit()
    n = 3 * U + 65
    pairs = pool[100:165]
    idx = np.zeros(n, np.uint32)
    at = np.linspace(5, n - 1, 64).astype(np.int64)      # the other pairs' entries, spread over the batch
    assert len(set(at.tolist())) == 64 and at[-1] == n - 1
    idx[at] = np.arange(1, 65)
    assert (idx == 0).sum() == 3 * U + 1
    ctxs = [B._ctx(i) for i in range(n)]
    rows = _prove_many(gpu, pairs, idx, ctxs, b"skew")
    got = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs)
    assert got[0] == bytes(32) and got[1] and not got[2].any()
    forged = [300, n - 1]
    assert idx[300] == 0 and idx[n - 1] == 64
    for i in forged:
        B._s_plus(rows, i, 1)
    exp = np.zeros(n, np.uint8)
    exp[forged] = 1
    sample = sorted(set(forged + at.tolist() + list(range(0, n, 37))))
    assert B._statuses(pairs, idx[sample], {q: rows[q][sample] for q in Q},
                       [ctxs[i] for i in sample]).tolist() == exp[sample].tolist()
    partial, ok, st = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs)
    assert not ok and partial == B._partial(pairs, idx, rows, ctxs, forged)
    assert np.array_equal(st, exp), np.nonzero(st != exp)[0][:8]


@pytest.fixture(scope="module")
def big1000(gpu, pool):
    """33,027 valid proofs over 1000 pairs, entry i under pair i % 1000."""
    n = PREP_WIDE_MAX + 259
    idx = (np.arange(n) % 1000).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    return pool, idx, ctxs, _prove_many(gpu, pool, idx, ctxs, b"b1000")


def test_above_the_wide_prepare(gpu, big1000):
    """n = 2^15 + 259 over 1000 pairs: the one-lane prepare, the bucketed sums per sub-range, and
    leaves that hold more than 64 distinct pairs, verified in runs."""
    pairs, idx, ctxs, rows = big1000
    n = len(idx)
    assert n == 33027 and n > PREP_WIDE_MAX
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        partial, ok, st = fresh.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs)
        times = fresh.stage_times()
        assert ok and partial == bytes(32) and not st.any()
        assert B._no_table_was_built(times), times
    rows = {q: rows[q].copy() for q in Q}
    idx = idx.copy()
    forged = [0, 20000, n - 1]
    B._s_plus(rows, 0, 1)
    B._s_plus(rows, n - 1, 1)
    idx[20000] = (idx[20000] + 1) % 1000                 # labelled with the next pair
    leaves, msms = _route(idx, 0, n, forged)
    assert len(leaves) == 3 and all(hi - lo <= PREP_BLOCK for lo, hi in leaves)
    assert max(len(set(idx[lo:hi].tolist())) for lo, hi in leaves) > PAIRS_MAX      # the run cutting is exercised
    assert max(len(M.runs(idx, lo, hi, PAIRS_MAX)) for lo, hi in leaves) >= 4
    exp = np.zeros(n, np.uint8)
    exp[forged] = 1
    sample = sorted(set(forged + list(range(0, n, 997)) + [1, 19999, 20001, n - 2]))
    assert B._statuses(pairs, idx[sample], {q: rows[q][sample] for q in Q},
                       [ctxs[i] for i in sample]).tolist() == exp[sample].tolist()
    want = B._partial(pairs, idx, rows, ctxs, forged)
    partial, ok, st = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs)
    assert not ok and partial == want
    assert np.array_equal(st, exp), (np.nonzero(st != exp)[0][:8], st[st != exp][:8])
    fb = gpu.fallback_stats()
    assert fb["path"] == "bisection" and fb["bisection_msms"] == msms, (fb, msms)
    assert fb["per_proof"] == sum(hi - lo for lo, hi in leaves), (fb, leaves)


@pytest.mark.parametrize("npairs", [64, 5])
def test_up_to_64_pairs_is_the_sibling_call(gpu, pool, npairs):
    """Byte-identical partial, statuses and fallback stats to verify_batch_pairs."""
    pairs = pool[200:200 + npairs]
    n = 3 * npairs + 7
    idx = (np.arange(n) % npairs).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    rows = _prove_many(gpu, pairs, idx, ctxs, b"sib%d" % npairs)
    for forged in ((), (1, n - 2)):
        for i in forged:
            B._s_plus(rows, i, 1)
        got = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, first_index=5, contexts=ctxs)
        fb = gpu.fallback_stats()
        ref = gpu.verify_batch_pairs(pairs, idx, *B._cols(rows), SEED, first_index=5, contexts=ctxs)
        assert got[0] == ref[0] and got[1] == ref[1] and got[2].tobytes() == ref[2].tobytes()
        assert fb == gpu.fallback_stats()
        assert got[1] == (not forged)


def test_per_call_flags(gpu, mix65):
    pairs, idx, ctxs, rows = mix65
    rows = {q: rows[q].copy() for q in Q}
    rows["r1"][5] = 0                                    # identity commitment
    # checks on: status 4, zero weight, the partial stays the identity
    partial, ok, st = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs)
    assert not ok and partial == bytes(32) and np.nonzero(st)[0].tolist() == [5] and st[5] == 4
    # equations only: the entry keeps its weight and fails its equations
    want = B._partial(pairs, idx, rows, ctxs, [], eq_only_sel=(5,))
    assert want != bytes(32)
    partial, ok, st = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs, equations_only=True)
    assert not ok and partial == want and np.nonzero(st)[0].tolist() == [5] and st[5] == 1
    low = np.nonzero(idx < 64)[0]                        # what verify_each_pairs reports, 64 pairs at a time
    each = gpu.verify_each_pairs(pairs[:64], idx[low], *[np.ascontiguousarray(c[low]) for c in B._cols(rows)],
                                 contexts=[ctxs[i] for i in low], equations_only=True)
    assert st[low].tobytes() == each.tobytes()
    # CPZ_CALL_PARTITIONED with 65 pairs: ignored, the same statuses by bisection
    rows = {q: mix65[3][q].copy() for q in Q}
    B._s_plus(rows, 77, 1)
    plain = _raw(gpu, 0, pairs, idx, rows, ctxs)
    fb_plain = gpu.fallback_stats()
    flagged = _raw(gpu, _native.CALL_PARTITIONED, pairs, idx, rows, ctxs)
    fb = gpu.fallback_stats()
    assert flagged[0] == plain[0] and flagged[1] == plain[1] and flagged[2].tobytes() == plain[2].tobytes()
    assert np.nonzero(flagged[2])[0].tolist() == [77] and not flagged[1]
    assert fb == fb_plain and fb["path"] == "bisection" and fb["blocks_checked"] == 0, fb


def test_shards_combine(gpu, mix65):
    pairs, idx, ctxs, rows = mix65
    rows = {q: rows[q].copy() for q in Q}
    n = len(idx)
    for i in (9, 70, 129):
        B._s_plus(rows, i, 1)
    whole = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, first_index=1000, contexts=ctxs)
    assert whole[0] == B._partial(pairs, idx, rows, ctxs, [9, 70, 129], first_index=1000) and not whole[1]
    cut = 67                                             # 65 pairs listed in each shard, not all with entries
    halves = [gpu.verify_batch_pairs_many(pairs, idx[lo:hi], *B._cols(rows, slice(lo, hi)), SEED,
                                          first_index=1000 + lo, contexts=ctxs[lo:hi], statuses=False)[0]
              for lo, hi in ((0, cut), (cut, n))]
    assert gpu.combine_partials(halves) == (whole[0], False)


def test_errors_write_nothing(gpu, pool, mix65):
    _, _, ctxs, rows = mix65
    lib, h = gpu._lib, gpu._h
    n = 16
    cols = B._cols(rows, slice(0, n))
    rows100 = b"".join(p.g + p.h for p in pool[:100])
    gh = np.frombuffer(rows100, np.uint8).copy()
    idx = np.arange(n, dtype=np.uint32)
    out = np.full(n, 0xAA, np.uint8)
    partial = np.full(32, 0xAA, np.uint8)
    ok = np.full(1, 0x2AAAAAAA, np.int32)

    def call(npairs, gh_, n_, idx_, seed=SEED):
        return lib.cpz_verify_batch_pairs_many(h, 0, npairs, gh_.ctypes.data, n_, idx_.ctypes.data,
                                               *[c.ctypes.data for c in cols], None, None, None, seed, 0,
                                               partial.ctypes.data, ok.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                               out.ctypes.data)

    big = np.frombuffer(rows100 * 41, np.uint8)[:64 * 4097].copy()
    assert call(4097, big, n, idx) == _native.CPZ_EINVAL
    assert b"CPZ_BATCH_PAIRS_MANY_MAX" in lib.cpz_last_error()
    assert call(100, gh, 0, idx) == _native.CPZ_EEMPTY
    assert call(100, gh, _native.BATCH_PAIRS_MAX_PROOFS + 1, idx) == _native.CPZ_EINVAL
    assert b"CPZ_BATCH_PAIRS_MAX_PROOFS" in lib.cpz_last_error()
    assert call(100, gh, n, idx, seed=None) == _native.CPZ_EINVAL
    bad = idx.copy()
    bad[11] = 100
    bad[13] = 4000
    assert call(100, gh, n, bad) == _native.CPZ_EINVAL
    assert b"pair_idx[11] = 100" in lib.cpz_last_error()
    g70, h70 = pool[70].g, pool[70].h
    for what, g2, h2 in (("identity", bytes(32), h70), ("equal", g70, g70),
                         ("undecodable", bytes.fromhex("01" + "00" * 31), h70)):
        ghb = gh.copy()
        ghb[64 * 70:64 * 71] = np.frombuffer(g2 + h2, np.uint8)
        ghb[64 * 90:64 * 91] = np.frombuffer(g2 + h2, np.uint8)      # pair 90 is bad too: pair 70 is named
        assert call(100, ghb, n, idx) == _native.CPZ_EGENERATOR, what
        assert b"pair 70:" in lib.cpz_last_error(), (what, lib.cpz_last_error())
    assert (out == 0xAA).all() and (partial == 0xAA).all() and ok[0] == 0x2AAAAAAA
    # the context still serves a valid call
    pairs, idx65, ctxs, rows = mix65
    got = gpu.verify_batch_pairs_many(pairs, idx65, *B._cols(rows), SEED, contexts=ctxs)
    assert got[0] == bytes(32) and got[1] and not got[2].any()
