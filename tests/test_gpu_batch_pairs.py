"""Mixed-pair RLC batch check (cpz_verify_batch_pairs): one MSM over entries that carry their own
(g, h), with g_p and h_p of every pair as 2 npairs more MSM points and no table or comb built
while the batch passes.

Proofs are made as in tests/test_gpu_pairs.py (gpu.prove per pair, contexts cycling through the
four shapes).  The expected partial is the point sum over the pairs of the C oracle's
rlc_partial over that pair's entries, weights keyed by first_index + the entry's position in the
call.  A valid entry contributes the identity to that sum, so only the forged entries are passed
to the oracle.  Expected statuses are the C oracle's verify_many_ctx under each entry's own pair."""
import ctypes
import hashlib

import numpy as np
import pytest

import chaum_pedersen as cp
import pyoracle as O
from chaum_pedersen import _native

pytestmark = pytest.mark.gpu

Q = ("y1", "y2", "r1", "r2", "s")
SEED = hashlib.sha256(b"batch-pairs-weights").digest()
PREP_BLOCK = 256          # kRlcPrepBlock: the bisection's alignment
PREP_WIDE_MAX = 1 << 15   # kRlcPrepWideMax: four lanes per proof up to here, one above
FANOUT = 8
BAD_POINT = np.frombuffer(bytes.fromhex("01" + "00" * 31), np.uint8)


def _pairs(k, tag):
    """k distinct custom generator pairs (g_i = [a_i] B, h_i = [b_i] B)."""
    out = []
    for i in range(k):
        a = O.scalar_wide(hashlib.sha512(tag + b"-g-%d" % i).digest())
        b = O.scalar_wide(hashlib.sha512(tag + b"-h-%d" % i).digest())
        out.append(cp.Parameters(O.ristretto_encode(O.pt_mul(O.BASEPOINT, a)),
                                 O.ristretto_encode(O.pt_mul(O.BASEPOINT, b))))
    return out


def _ctx(i):
    """None, 32 bytes, 5 bytes, b"": the two fixed schedules and the byte-wise sponge."""
    return (None, hashlib.sha256(b"ctx-%d" % i).digest(), b"ctx%02d" % (i % 100), b"")[i % 4]


def _prove(gpu, pairs, groups, ctxs, seed):
    """Valid proofs: entry i under pairs[groups[i]] with context ctxs[i]."""
    groups = np.asarray(groups)
    rows = {q: np.zeros((len(groups), 32), np.uint8) for q in Q}
    for p in sorted(set(groups.tolist())):
        idx = np.nonzero(groups == p)[0]
        out = gpu.prove([O.bench_scalar(seed + b"x", int(i)) for i in idx],
                        [O.bench_scalar(seed + b"k", int(i)) for i in idx],
                        contexts=[ctxs[i] for i in idx], params=pairs[p])
        for q in Q:
            rows[q][idx] = out[q]
    return rows


def _statuses(pairs, groups, rows, ctxs):
    """The C oracle's per-entry statuses, every entry under its own pair."""
    import coracle
    groups = np.asarray(groups)
    out = np.full(len(groups), 255, np.uint8)
    for p in sorted(set(groups.tolist())):
        idx = np.nonzero(groups == p)[0]
        out[idx] = coracle.verify_many_ctx({q: np.ascontiguousarray(rows[q][idx]) for q in Q}, [ctxs[i] for i in idx],
                                           g=pairs[p].g, h=pairs[p].h, threads=8)
    return out


def _partial(pairs, groups, rows, ctxs, sel, first_index=0, eq_only_sel=()):
    """The expected partial from the entries `sel` alone (every other entry is valid and
    contributes the identity): per pair, the C oracle's rlc_partial with the entries' global
    indices; summed over the pairs.  eq_only_sel: entries that carry weight only with the
    commitment checks off (identity commitment, zero s), which the C oracle skips -- their terms
    come from pyoracle.rlc_partial(commitment_checks=False), one entry at a time."""
    import coracle
    groups = np.asarray(groups)
    acc = O.IDENTITY
    sel = np.asarray(sorted(sel), np.int64)
    for p in sorted(set(groups[sel].tolist())):
        idx = sel[groups[sel] == p]
        enc, _ = coracle.rlc_partial({q: np.ascontiguousarray(rows[q][idx]) for q in Q}, idx + first_index, SEED,
                                     [ctxs[i] for i in idx], g=pairs[p].g, h=pairs[p].h)
        acc = O.pt_add(acc, O.ristretto_decode(enc))
    for i in eq_only_sel:
        p = pairs[int(groups[i])]
        rec = O.ProofRecord(*(rows[q][i].tobytes() for q in Q), ctxs[i])
        acc = O.pt_add(acc, O.rlc_partial([rec], SEED, first_index + int(i), p.g, p.h, commitment_checks=False))
    return O.ristretto_encode(acc)


def _cols(rows, sel=slice(None)):
    return [np.ascontiguousarray(rows[q][sel]) for q in Q]


def _s_plus(rows, i, d):
    v = int.from_bytes(rows["s"][i].tobytes(), "little") + d
    rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)


def _no_table_was_built(st):
    """stage_times() of a call: 0 launches in stages 7 (combs) and 13 (light sets)."""
    return st.get("generators", (0.0, 0))[1] == 0 and st.get("generators_varbase", (0.0, 0))[1] == 0


@pytest.fixture(scope="module")
def mix5(gpu):
    """515 valid proofs, entry i under pair i % 5 (the default pair and four custom ones)."""
    pairs = [cp.Parameters()] + _pairs(4, b"mix5")
    n = 515
    groups = np.arange(n) % 5
    ctxs = [_ctx(i) for i in range(n)]
    return pairs, groups, ctxs, _prove(gpu, pairs, groups, ctxs, b"m5")


@pytest.fixture(scope="module")
def big64(gpu):
    """33,027 valid proofs over 64 custom pairs, entry i under pair i % 64."""
    pairs = _pairs(64, b"big64")
    n = PREP_WIDE_MAX + 259
    groups = np.arange(n) % 64
    ctxs = [_ctx(i) for i in range(n)]
    return pairs, groups, ctxs, _prove(gpu, pairs, groups, ctxs, b"b64")


def test_smallest_mix(gpu):
    """n = 7 over the default pair and two custom ones on a fresh context: all valid passes with no
    table built; then entry 4 has s + 1 and entry 5 is proven under pair 1 but labelled pair 2."""
    pairs = [cp.Parameters()] + _pairs(2, b"wide")
    idx = np.array([0, 1, 2, 1, 0, 2, 1], np.uint32)
    ctxs = [_ctx(i) for i in range(7)]
    proven = idx.copy()
    proven[5] = 1
    rows = _prove(gpu, pairs, proven, ctxs, b"wd")
    good = idx.copy()
    good[5] = 1
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        partial, ok, st = fresh.verify_batch_pairs(pairs, good, *_cols(rows), SEED, contexts=ctxs)
        times = fresh.stage_times()
        assert ok and partial == bytes(32) and st.tolist() == [0] * 7
        assert _no_table_was_built(times), times
        assert fresh.fallback_stats()["path"] == "none"
        _s_plus(rows, 4, 1)
        exp = _statuses(pairs, idx, rows, ctxs)
        assert exp.tolist() == [0, 0, 0, 0, 1, 1, 0]
        want = _partial(pairs, idx, rows, ctxs, [4, 5])
        assert want != bytes(32)
        partial, ok, st = fresh.verify_batch_pairs(pairs, idx, *_cols(rows), SEED, contexts=ctxs)
        assert not ok and partial == want and st.tolist() == exp.tolist()
        assert fresh.fallback_stats()["path"] == "bisection"
        partial2, ok2, st2 = fresh.verify_batch_pairs(pairs, idx, *_cols(rows), SEED, contexts=ctxs, statuses=False)
        assert not ok2 and partial2 == want and st2 is None


@pytest.mark.parametrize("equations_only", [False, True])
def test_block_edges_of_the_per_pair_sums(gpu, mix5, equations_only):
    """n = 515 with pair = i % 5 crosses the 64-proof quarter, the 128-proof sum block and the
    256-proof prepare block; forgeries sit on both sides of each edge, under different pairs, and
    one entry of each decode-level kind carries zero weight and its own status."""
    pairs, groups, ctxs, rows = mix5
    n = len(groups)
    groups = groups.copy()
    rows = {q: rows[q].copy() for q in Q}
    forged = [63, 64, 127, 128, 255, 256, 514]
    assert len({int(groups[i]) for i in forged}) == 5
    for i in (63, 127, 128, 256, 514):
        _s_plus(rows, i, 1)
    groups[64] = (groups[64] + 1) % 5                       # proven under pair 4, labelled pair 0 (no context)
    groups[255] = (groups[255] + 2) % 5                     # proven under pair 0, labelled pair 2 (empty context)
    rows["r1"][130] = BAD_POINT                             # undecodable point
    _s_plus(rows, 201, O.L)                                 # s + l: not canonical
    rows["r1"][407] = 0                                     # identity commitment
    rows["s"][262] = 0                                      # zero s
    exp = _statuses(pairs, groups, rows, ctxs)
    assert [int(exp[i]) for i in forged + [130, 201, 407, 262]] == [1] * 7 + [2, 3, 4, 5]
    assert (exp == 0).sum() == n - 11
    eq_sel = ()
    if equations_only:
        # commitment checks off: the identity commitment and the zero s keep their weight and are
        # judged by the equations, which neither satisfies
        exp[[407, 262]] = 1
        eq_sel = (407, 262)
    want = _partial(pairs, groups, rows, ctxs, forged, eq_only_sel=eq_sel)
    partial, ok, st = gpu.verify_batch_pairs(pairs, groups, *_cols(rows), SEED, contexts=ctxs,
                                             equations_only=equations_only)
    assert not ok and partial == want
    assert np.array_equal(st, exp), (np.nonzero(st != exp)[0][:8], st[st != exp][:8], exp[st != exp][:8])
    assert st.tobytes() == gpu.verify_each_pairs(pairs, groups, *_cols(rows), contexts=ctxs,
                                                 equations_only=equations_only).tobytes()
    # the decode-level entries alone: P is the identity, yet the batch is not ok
    clean = {q: mix5[3][q].copy() for q in Q}
    clean["r1"][130] = BAD_POINT
    partial, ok, st = gpu.verify_batch_pairs(pairs, mix5[1], *_cols(clean), SEED, contexts=ctxs)
    assert not ok and partial == bytes(32) and np.nonzero(st)[0].tolist() == [130] and st[130] == 2


def _cuts(lo, hi):
    """rlc_fallback's cut arithmetic: FANOUT parts aligned to the prepare block."""
    c = [(lo + ((hi - lo) * k) // FANOUT) // PREP_BLOCK * PREP_BLOCK for k in range(FANOUT + 1)]
    c[0], c[FANOUT] = lo, hi
    return c


def test_one_lane_prepare_and_bisection(gpu, big64):
    """n = 33,027 > kRlcPrepWideMax over 64 pairs: the one-lane prepare, and a failing batch located
    by bisection with pair-mode extras per sub-range."""
    pairs, groups, ctxs, rows = big64
    n = len(groups)
    assert n == 33027 and n > PREP_WIDE_MAX
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        partial, ok, st = fresh.verify_batch_pairs(pairs, groups, *_cols(rows), SEED, contexts=ctxs)
        times = fresh.stage_times()
        assert ok and partial == bytes(32) and not st.any()
        assert _no_table_was_built(times), times
    groups = groups.copy()
    rows = {q: rows[q].copy() for q in Q}
    forged = [0, 255, 256, 300, n - 1]
    for i in (0, 255, 256, n - 1):
        _s_plus(rows, i, 1)
    groups[300] = (groups[300] + 1) % 64                    # proven under pair 44, labelled pair 45
    # the forgeries fall in 2 of the 8 top-level parts, so the dense shortcut (more than half of
    # the parts failing) does not fire and the failing parts are bisected further
    top = _cuts(0, n)
    hit = {max(k for k in range(FANOUT) if top[k] <= i) for i in forged}
    assert len(hit) == 2 and 2 * len(hit) <= FANOUT
    exp = np.zeros(n, np.uint8)
    exp[forged] = 1
    sample = sorted(set(forged + list(range(0, n, 997)) + [1, 254, 257, 299, 301, n - 2]))
    assert _statuses(pairs, groups[sample], {q: rows[q][sample] for q in Q},
                     [ctxs[i] for i in sample]).tolist() == exp[sample].tolist()
    want = _partial(pairs, groups, rows, ctxs, forged)
    partial, ok, st = gpu.verify_batch_pairs(pairs, groups, *_cols(rows), SEED, contexts=ctxs)
    assert not ok and partial == want
    assert np.array_equal(st, exp), (np.nonzero(st != exp)[0][:8], st[st != exp][:8])
    fb = gpu.fallback_stats()
    assert fb["path"] == "bisection" and fb["bisection_msms"] >= FANOUT and 0 < fb["per_proof"] < n, fb


def test_equivalences(gpu, mix5):
    pairs, groups, ctxs, rows = mix5
    n = len(groups)
    rows = {q: rows[q].copy() for q in Q}
    forged = [6, 100, 257, 401]                             # pairs 1, 0, 2, 1
    for i in forged:
        _s_plus(rows, i, 1)
    # one pair: cpz_verify_batch's bytes
    one = np.nonzero(groups == 1)[0]
    cols = _cols(rows, one)
    c1 = [ctxs[i] for i in one]
    got = gpu.verify_batch_pairs([pairs[1]], np.zeros(len(one), np.uint32), *cols, SEED, first_index=9, contexts=c1)
    ref = gpu.verify_batch(*cols, SEED, first_index=9, contexts=c1, params=pairs[1])
    assert got[0] == ref[0] and got[1] == ref[1] and got[2].tobytes() == ref[2].tobytes() and not got[1]
    # a repeated row in `pairs`: the same partial
    whole = gpu.verify_batch_pairs(pairs, groups, *_cols(rows), SEED, contexts=ctxs)
    assert whole[0] == _partial(pairs, groups, rows, ctxs, forged) and not whole[1]
    dup = gpu.verify_batch_pairs(pairs + [pairs[1]], np.where(groups == 1, 5, groups), *_cols(rows), SEED,
                                 contexts=ctxs)
    assert dup[0] == whole[0] and dup[2].tobytes() == whole[2].tobytes()
    # two shards with global first_index values combine to the whole; the cut is not on a block edge
    cut = n // 2
    assert cut % PREP_BLOCK != 0
    halves = [gpu.verify_batch_pairs(pairs, groups[lo:hi], *_cols(rows, slice(lo, hi)), SEED, first_index=lo,
                                     contexts=ctxs[lo:hi], statuses=False)[0] for lo, hi in ((0, cut), (cut, n))]
    assert gpu.combine_partials(halves) == (whole[0], False)


def test_errors_write_nothing(gpu, mix5):
    pairs64 = _pairs(64, b"errs")
    _, _, _, rows = mix5
    lib, h = gpu._lib, gpu._h
    n = 16
    cols = _cols(rows, slice(0, n))
    gh = np.frombuffer(b"".join(p.g + p.h for p in pairs64) + bytes(64), np.uint8).copy()   # 65 rows
    idx = np.arange(n, dtype=np.uint32)
    out = np.full(n, 0xAA, np.uint8)
    partial = np.full(32, 0xAA, np.uint8)
    ok = np.full(1, 0x2AAAAAAA, np.int32)

    def call(npairs, gh_, n_, idx_, cols_=cols, seed=SEED, gh_ptr=True):
        return lib.cpz_verify_batch_pairs(h, npairs, gh_.ctypes.data if gh_ptr else None, n_, idx_.ctypes.data,
                                          *[c.ctypes.data for c in cols_], None, None, None, seed, 0,
                                          partial.ctypes.data, ok.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                          out.ctypes.data)

    assert call(64, gh, 0, idx) == _native.CPZ_EEMPTY
    assert call(0, gh, n, idx) == _native.CPZ_EINVAL
    assert call(65, gh, n, idx) == _native.CPZ_EINVAL
    assert b"CPZ_PAIRS_MAX" in lib.cpz_last_error()
    # n above the bound: refused on the count alone, before any row is read
    assert call(64, gh, _native.BATCH_PAIRS_MAX_PROOFS + 1, idx) == _native.CPZ_EINVAL
    assert b"CPZ_BATCH_PAIRS_MAX_PROOFS" in lib.cpz_last_error()
    assert call(64, gh, n, idx, gh_ptr=False) == _native.CPZ_EINVAL
    assert call(64, gh, n, idx, seed=None) == _native.CPZ_EINVAL
    bad = idx.copy()
    bad[11] = 64
    assert call(64, gh, n, bad) == _native.CPZ_EINVAL
    assert b"pair_idx[11]" in lib.cpz_last_error()
    for what, g2, h2 in (("identity", bytes(32), pairs64[2].h), ("equal", pairs64[2].g, pairs64[2].g),
                         ("undecodable", bytes.fromhex("01" + "00" * 31), pairs64[2].h)):
        ghb = gh.copy()
        ghb[128:192] = np.frombuffer(g2 + h2, np.uint8)
        assert call(64, ghb, n, idx) == _native.CPZ_EGENERATOR, what
        assert b"pair 2" in lib.cpz_last_error(), what
    # nothing was written by the refused calls
    assert (out == 0xAA).all() and (partial == 0xAA).all() and ok[0] == 0x2AAAAAAA
    # the context still serves a valid call
    pairs, groups, ctxs, _ = mix5
    got = gpu.verify_batch_pairs(pairs, groups[:n], *cols, SEED, contexts=ctxs[:n])
    assert got[0] == bytes(32) and got[1] and not got[2].any()
