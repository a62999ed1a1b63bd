"""cpz_verify_batch_pairs_many with CPZ_CALL_PARTITIONED_MANY (Gpu.verify_batch_pairs_many(...,
locate="partitioned")): above CPZ_PAIRS_MAX pairs a failing batch goes at once to the partitioned
search over block-local pair lists (part.hip's many mode), and everything verified per proof is
verified from the call's small per-pair tables -- no 128-entry set, no runs, the light-set cache
untouched.

Pairs, proofs, expected statuses and expected partials are made as in
tests/test_gpu_batch_pairs_many.py, whose helpers are used here: the statuses are the C oracle's
under each entry's own pair, the partial comes from the forged entries alone."""
import numpy as np
import pytest

import chaum_pedersen as cp
import part_many_model as MM
import test_gpu_batch_pairs as B
import test_gpu_batch_pairs_many as M
from chaum_pedersen import _native

pytestmark = pytest.mark.gpu

Q, SEED = B.Q, B.SEED
BLOCK = 128               # kPartProofs
BAD_POINT = B.BAD_POINT


def _flagged(gpu, pairs, idx, rows, ctxs, **kw):
    out = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs, locate="partitioned", **kw)
    return out, gpu.fallback_stats()


def _resident(gpu, pairs):
    """cpz_ctx_pairs_resident over any number of pairs, CPZ_PAIRS_MAX a call."""
    return np.concatenate([gpu.pairs_resident(pairs[c:c + 64]) for c in range(0, len(pairs), 64)])


def _count(times, stage):
    return times.get(stage, (0.0, 0))[1]


@pytest.fixture(scope="module")
def pool(gpu):
    """1000 distinct pairs."""
    return M._many_pairs(gpu, 1000, b"part-pool")


@pytest.fixture(scope="module")
def mix65(gpu, pool):
    """130 valid proofs over 65 pairs, entry i under pair i % 65: block 0 holds all 65 pairs."""
    pairs = pool[:65]
    idx = (np.arange(130) % 65).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(130)]
    return pairs, idx, ctxs, M._prove_many(gpu, pairs, idx, ctxs, b"pm65")


@pytest.fixture(scope="module")
def own600(gpu, pool):
    """600 valid proofs, every entry its own pair, except that entry 200 is proven under pair 201."""
    n = 600
    pairs = pool[:n]
    idx = np.arange(n, dtype=np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    proven = idx.copy()
    proven[200] = 201
    return pairs, idx, ctxs, M._prove_many(gpu, pairs, proven, ctxs, b"pm-own")


@pytest.fixture(scope="module")
def mix1000(gpu, pool):
    """1,283 valid proofs over 1000 pairs, entry i under pair i % 1000."""
    n = 1283
    idx = (np.arange(n) % 1000).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    return pool, idx, ctxs, M._prove_many(gpu, pool, idx, ctxs, b"pm1000")


def test_smallest_case(gpu, mix65):
    """n = 130 over 65 pairs on a fresh context.  Passing and flagged: "none", no table.  One
    forgery: "partitioned", two blocks checked, the entry located and verified alone from the small
    tables -- one stage-13 span that counts the 65 pairs, stage 7 at zero, no pair resident before
    or after."""
    pairs, idx, ctxs, rows = mix65
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        assert not _resident(fresh, pairs).any()
        (partial, ok, st), fb = _flagged(fresh, pairs, idx, rows, ctxs)
        times = fresh.stage_times()
        assert ok and partial == bytes(32) and st.tolist() == [0] * 130
        assert B._no_table_was_built(times), times
        assert fb["path"] == "none"
        (partial, ok, st), fb = _flagged(fresh, pairs, idx, rows, ctxs, statuses=False)
        assert ok and partial == bytes(32) and st is None and fb["path"] == "none"
        rows = {q: rows[q].copy() for q in Q}
        B._s_plus(rows, 77, 1)
        exp = B._statuses(pairs, idx, rows, ctxs)
        assert np.nonzero(exp)[0].tolist() == [77] and exp[77] == 1
        want = B._partial(pairs, idx, rows, ctxs, [77])
        # without status_out nothing is searched
        (partial, ok, st), fb = _flagged(fresh, pairs, idx, rows, ctxs, statuses=False)
        assert not ok and partial == want and fb["path"] == "none"
        fresh.stage_times()
        (partial, ok, st), fb = _flagged(fresh, pairs, idx, rows, ctxs)
        times = fresh.stage_times()
        print("fallback stats:", fb, "stage times:", times)
        assert not ok and partial == want
        assert st.tolist() == exp.tolist()
        assert fb["path"] == "partitioned" and fb["blocks_checked"] == 2 and fb["blocks_failing"] == 1
        assert fb["blocks_indexed"] == 1 and fb["blocks_located"] == 1 and fb["per_proof"] == 1
        assert fb["probe_invalid"] == 0 and fb["bisection_msms"] == 0
        assert _count(times, "generators_varbase") == 65, times          # one span, counted per pair
        assert _count(times, "generators") == 0, times                   # stage 7
        assert _count(times, "part_acc") == 1 and _count(times, "part_acc_locate") == 1, times
        assert not _resident(fresh, pairs).any()


def _own_case(own600, n):
    pairs, idx, ctxs, rows = own600
    pairs, idx, ctxs = pairs[:n], idx[:n].copy(), ctxs[:n]
    rows = {q: rows[q][:n].copy() for q in Q}
    B._s_plus(rows, 3, 1)                                  # block 0: one forgery
    B._s_plus(rows, 130, 1)                                # block 1: a forgery and the mislabelled entry 200
    rows["y2"][280] = BAD_POINT                            # block 2: undecodable, zero weight
    exp = B._statuses(pairs, idx, rows, ctxs)
    assert np.nonzero(exp)[0].tolist() == [3, 130, 200, 280] and exp[[3, 130, 200, 280]].tolist() == [1, 1, 1, 2]
    return pairs, idx, ctxs, rows, exp, B._partial(pairs, idx, rows, ctxs, [3, 130, 200])


def test_one_pair_per_entry(gpu, own600):
    """Every entry its own pair, so the full blocks hold 128 distinct pairs (128 slots, 256 extras).
    Block 0 has one forgery, which is located; block 1 has two (s + 1 and a mislabelled pair), is not
    located and is verified whole; block 2 holds an undecodable point, which keeps status 2,
    carries no weight and leaves the block clean.
    n = npairs = 600, not 300: with 300 entries there are three blocks, two of them failing, and
    more than half of the blocks failing is the dense branch (test_one_pair_per_entry_300)."""
    n = 600
    pairs, idx, ctxs, rows, exp, want = _own_case(own600, n)
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        (partial, ok, st), fb = _flagged(fresh, pairs, idx, rows, ctxs)
        times = fresh.stage_times()
        resident = _resident(fresh, pairs)
    print("fallback stats:", fb)
    assert not ok and partial == want
    assert np.array_equal(st, exp), (np.nonzero(st != exp)[0][:8], st[st != exp][:8])
    assert fb["path"] == "partitioned" and fb["blocks_checked"] == 5 and fb["blocks_failing"] == 2
    assert fb["blocks_indexed"] == 2 and fb["blocks_located"] == 1
    # the lists hold entry 3 alone, then block 1 whole
    assert fb["per_proof"] == MM.per_proof_count(n, BLOCK, [3], [1]) == 1 + BLOCK
    assert _count(times, "generators_varbase") == n and _count(times, "generators") == 0, times
    assert not resident.any()


def test_one_pair_per_entry_300(gpu, own600):
    """The same entries with n = npairs = 300: two of three blocks fail, which is the dense branch --
    every entry per proof from the small tables, the same exact statuses."""
    n = 300
    pairs, idx, ctxs, rows, exp, want = _own_case(own600, n)
    (partial, ok, st), fb = _flagged(gpu, pairs, idx, rows, ctxs)
    assert not ok and partial == want
    assert np.array_equal(st, exp), (np.nonzero(st != exp)[0][:8], st[st != exp][:8])
    assert fb["path"] == "partitioned" and fb["blocks_checked"] == 3 and fb["blocks_failing"] == 2
    assert fb["per_proof"] == n and fb["blocks_indexed"] == 0


def test_dense(gpu, pool):
    """n = 261 over 130 pairs, one forgery in each of the three blocks: the whole batch per proof
    from the small tables."""
    n = 261
    pairs = pool[300:430]
    idx = (np.arange(n) % 130).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    rows = M._prove_many(gpu, pairs, idx, ctxs, b"pm-dense")
    forged = [5, 200, 260]
    for i in forged:
        B._s_plus(rows, i, 1)
    exp = B._statuses(pairs, idx, rows, ctxs)
    assert np.nonzero(exp)[0].tolist() == forged and exp[forged].tolist() == [1, 1, 1]
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        (partial, ok, st), fb = _flagged(fresh, pairs, idx, rows, ctxs)
        times = fresh.stage_times()
        assert not _resident(fresh, pairs).any()
    print("fallback stats:", fb)
    assert not ok and partial == B._partial(pairs, idx, rows, ctxs, forged)
    assert st.tolist() == exp.tolist()
    assert fb["path"] == "partitioned" and fb["blocks_checked"] == 3 and fb["blocks_failing"] == 3
    assert fb["per_proof"] == n and fb["blocks_indexed"] == 0 and fb["blocks_located"] == 0
    assert _count(times, "generators_varbase") == 130 and _count(times, "generators") == 0, times


def test_all_located(gpu, mix1000):
    """1,283 entries over 1000 pairs, one forgery in each of blocks 0, 5 and 10: all three located."""
    pairs, idx, ctxs, rows = mix1000
    n = len(idx)
    rows = {q: rows[q].copy() for q in Q}
    forged = [7, 5 * BLOCK + 64, 1282]
    assert [i // BLOCK for i in forged] == [0, 5, 10]
    for i in forged:
        B._s_plus(rows, i, 1)
    exp = B._statuses(pairs, idx, rows, ctxs)
    assert np.nonzero(exp)[0].tolist() == forged and exp[forged].tolist() == [1, 1, 1]
    want = B._partial(pairs, idx, rows, ctxs, forged)
    (partial, ok, st), fb = _flagged(gpu, pairs, idx, rows, ctxs)
    print("fallback stats:", fb)
    assert not ok and partial == want
    assert st.tolist() == exp.tolist()
    assert fb["path"] == "partitioned" and fb["blocks_checked"] == 11 and fb["blocks_failing"] == 3
    assert fb["blocks_indexed"] == 3 and fb["blocks_located"] == 3 and fb["per_proof"] == 3
    # the unflagged call on the same inputs: the same statuses and partial, by bisection
    plain = gpu.verify_batch_pairs_many(pairs, idx, *B._cols(rows), SEED, contexts=ctxs)
    fb_plain = gpu.fallback_stats()
    assert plain[0] == partial and plain[1] == ok and plain[2].tobytes() == st.tobytes()
    assert fb_plain["path"] == "bisection" and fb_plain["blocks_checked"] == 0
    # verify_each_pairs_many on the same rows: the same statuses, with its own stage counts
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        each = fresh.verify_each_pairs_many(pairs, idx, *B._cols(rows), contexts=ctxs)
        times = fresh.stage_times()
    assert each.tobytes() == st.tobytes()
    assert _count(times, "generators_varbase") == 1000 and _count(times, "verify_each") >= 1, times
    assert _count(times, "part_acc") == 0 and _count(times, "generators") == 0, times


def test_flags(gpu, mix65):
    """An identity commitment: zero weight with the checks on (the batch's partial is the identity
    and nothing is searched); with CPZ_CALL_EQUATIONS_ONLY, or the context's checks off, the entry
    keeps its weight, fails its equations and is found by the flagged route."""
    pairs, idx, ctxs, rows = mix65
    rows = {q: rows[q].copy() for q in Q}
    rows["r1"][5] = 0
    (partial, ok, st), fb = _flagged(gpu, pairs, idx, rows, ctxs)
    assert not ok and partial == bytes(32) and np.nonzero(st)[0].tolist() == [5] and st[5] == 4
    assert fb["path"] == "none"
    want = B._partial(pairs, idx, rows, ctxs, [], eq_only_sel=(5,))
    assert want != bytes(32)
    (partial, ok, st), fb = _flagged(gpu, pairs, idx, rows, ctxs, equations_only=True)
    assert not ok and partial == want and np.nonzero(st)[0].tolist() == [5] and st[5] == 1
    assert fb["path"] == "partitioned" and fb["blocks_located"] == 1 and fb["per_proof"] == 1
    with cp.Gpu(0) as fresh:
        fresh.set_commitment_checks(False)
        (partial, ok, st), fb = _flagged(fresh, pairs, idx, rows, ctxs)
        assert not ok and partial == want and np.nonzero(st)[0].tolist() == [5] and st[5] == 1
        assert fb["path"] == "partitioned" and fb["per_proof"] == 1
    # CPZ_CALL_PARTITIONED (2) stays ignored above 64 pairs, alone and beside nothing else
    raw = M._raw(gpu, _native.CALL_PARTITIONED | _native.CALL_EQUATIONS_ONLY, pairs, idx, rows, ctxs)
    assert raw[0] == want and raw[2].tobytes() == st.tobytes() and gpu.fallback_stats()["path"] == "bisection"
    raw = M._raw(gpu, _native.CALL_PARTITIONED_MANY | _native.CALL_EQUATIONS_ONLY, pairs, idx, rows, ctxs)
    assert raw[0] == want and raw[2].tobytes() == st.tobytes() and gpu.fallback_stats()["path"] == "partitioned"


def test_shards_combine(gpu, mix1000):
    """first_index keys the locate pass's weights too: a batch that starts at 1000 locates its
    forgeries, and so do its two shards (cut inside a block, so their blocks differ from the whole
    batch's), whose partials combine to the whole batch's."""
    pairs, idx, ctxs, rows = mix1000
    rows = {q: rows[q].copy() for q in Q}
    n = len(idx)
    forged = [7, 5 * BLOCK + 64, 1282]
    for i in forged:
        B._s_plus(rows, i, 1)
    exp = np.zeros(n, np.uint8)
    exp[forged] = 1
    sample = sorted(set(forged + [f + d for f in forged for d in (-1, 1) if 0 <= f + d < n] + list(range(0, n, 97))))
    assert B._statuses(pairs, idx[sample], {q: rows[q][sample] for q in Q},
                       [ctxs[i] for i in sample]).tolist() == exp[sample].tolist()
    (partial, ok, st), fb = _flagged(gpu, pairs, idx, rows, ctxs, first_index=1000)
    assert partial == B._partial(pairs, idx, rows, ctxs, forged, first_index=1000) and not ok
    assert st.tolist() == exp.tolist()
    assert fb["path"] == "partitioned" and fb["blocks_located"] == 3 and fb["per_proof"] == 3, fb
    cut = 600
    halves = []
    for lo, hi, located in ((0, cut, 1), (cut, n, 2)):
        (p, ok_h, st_h), fb = _flagged(gpu, pairs, idx[lo:hi], {q: rows[q][lo:hi] for q in Q}, ctxs[lo:hi],
                                       first_index=1000 + lo)
        assert not ok_h and st_h.tolist() == exp[lo:hi].tolist()
        assert fb["path"] == "partitioned" and fb["blocks_located"] == located == fb["per_proof"], fb
        halves.append(p)
    assert gpu.combine_partials(halves) == (partial, False)


@pytest.mark.parametrize("npairs", [64, 5])
def test_up_to_64_pairs_the_flag_is_the_siblings(gpu, pool, npairs):
    """Forwarded with CPZ_CALL_PARTITIONED in the flag's place: byte-identical partial, statuses and
    stats to verify_batch_pairs(..., locate="partitioned")."""
    pairs = pool[200:200 + npairs]
    n = 3 * npairs + 7
    idx = (np.arange(n) % npairs).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    rows = M._prove_many(gpu, pairs, idx, ctxs, b"pm-sib%d" % npairs)
    for forged in ((), (1, n - 2)):
        for i in forged:
            B._s_plus(rows, i, 1)
        (got, fb) = _flagged(gpu, pairs, idx, rows, ctxs, first_index=5)
        ref = gpu.verify_batch_pairs(pairs, idx, *B._cols(rows), SEED, first_index=5, contexts=ctxs,
                                     locate="partitioned")
        assert got[0] == ref[0] and got[1] == ref[1] and got[2].tobytes() == ref[2].tobytes()
        assert fb == gpu.fallback_stats()
        assert fb["path"] == ("partitioned" if forged else "none")
        assert got[1] == (not forged)
