"""cpz_ctx_load_pairs / cpz_ctx_pairs_resident and the one-pass build behind every mixed-pair call:
the light sets of all of a call's missing pairs come from two launches (k_pair_sets_bases,
k_pair_sets_entries) instead of one build per pair.

What is checked, always on fresh contexts:
  - every Niels entry (tab) and every 16-bit-limb row (tab16) of sets built at pair positions >= 1
    of one pass, through the mixed-pair prover and the wide verify kernel, against Gpu.prove
    (the combs: code this feature does not touch) and the C oracle;
  - the cache: the cap of 64, the least-recently-used order, a call's own resident pairs never
    its victims, repeated rows, a cached full set;
  - CPZ_PAIRS_BUILD_BATCH=0 (one build per pair) gives the same bytes;
  - the errors, with nothing launched and no set lost.
Every comparison is exact."""
import ctypes
import random

import numpy as np
import pytest

import chaum_pedersen as cp
import coracle
import digit_vectors as DV
import pyoracle as O
from chaum_pedersen import _native
from test_gpu_varbase import _pairs

pytestmark = pytest.mark.gpu

L = O.L
Q = ("y1", "y2", "r1", "r2", "s")
VARBASE = "generators_varbase"
BAD_POINT = bytes.fromhex("01" + "00" * 31)   # s = 1 is no ristretto255 encoding (as in smoke())


def _rows32(values):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32)


@pytest.fixture(scope="module")
def pool():
    """160 distinct custom pairs, computed once."""
    return _pairs(160, tag=b"load-pairs")


@pytest.fixture(scope="module")
def audit():
    """x = table_audit_scalars() (289 values: every signed byte digit at every position), k the
    same values rotated by 97 (coprime to 289: k_i is never x_i)."""
    xs = list(DV.table_audit_scalars())
    ks = [xs[(i + 97) % len(xs)] for i in range(len(xs))]
    assert all(a != b for a, b in zip(xs, ks))
    return xs, ks, _rows32(xs), _rows32(ks)


def _oracle(pairs, idx, rows):
    """The C oracle's status of every entry under its own pair (no contexts)."""
    idx = np.asarray(idx)
    out = np.zeros(len(idx), np.uint8)
    for p in sorted(set(idx.tolist())):
        sel = np.nonzero(idx == p)[0]
        sub = {q: np.ascontiguousarray(rows[q][sel]) for q in Q}
        out[sel] = coracle.verify_many(sub, g=pairs[p].g, h=pairs[p].h)
    return out


def _four(pool):
    """The default pair, two custom pairs and a repeated row: positions 1, 2, 3 are custom."""
    return [cp.Parameters(), pool[0], pool[1], pool[0]]


# ---- every table entry, pair position >= 1 --------------------------------------------------------
def test_every_table_entry_at_pair_positions(pool, audit):
    """One pass builds 3 sets (the repeated row once).  The mixed-pair prover then reads every
    entry of every level of each set: 289 witnesses and nonces under each of the four rows.  The
    rows equal one Gpu.prove per pair byte for byte and the C oracle accepts all of them."""
    xs, ks, xrows, krows = audit
    m = len(xs)
    pairs = _four(pool)
    idx = np.repeat(np.arange(4, dtype=np.uint32), m)
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        assert fresh.load_pairs(pairs) == 3
        st = fresh.stage_times()
        assert st[VARBASE][1] == 3, st            # one span, counted per set
        assert fresh.pairs_resident(pairs).all()
        got = fresh.prove_pairs(pairs, idx, np.tile(xrows, (4, 1)), np.tile(krows, (4, 1)))
        assert VARBASE not in fresh.stage_times()  # nothing left to build
        for p in range(4):
            exp = fresh.prove(xrows, krows, params=pairs[p])   # the pair's comb
            for q in Q:
                bad = np.nonzero((got[q][p * m:(p + 1) * m] != exp[q]).any(axis=1))[0]
                assert bad.size == 0, (p, q, bad[:8].tolist(), [DV.recode8(xs[i]) for i in bad[:2]])
    want = _oracle(pairs, idx, got)
    assert (want == cp.STATUS_OK).all(), np.nonzero(want)[0][:8].tolist()


# ---- tab16 under pair positions >= 1 ---------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_entries(pool, audit):
    """Entries for the wide kernel (n <= 512) under positions 1, 2, 3 of _four: build_entry over
    table_audit_scalars() as part b of test_gpu_table_audit.py builds them (one challenge per class
    of the split, round-robin), each under its own position's pair; valid transcript proofs from
    the Python oracle; one s + 1 entry; one entry proven under pair 1 and labelled pair 2."""
    pairs = _four(pool)
    pts = [(O.ristretto_decode(p.g), O.ristretto_decode(p.h)) for p in pairs]
    rnd = random.Random(53)
    cs = DV.challenge_list()
    witnesses = [rnd.randrange(1, L) for _ in range(3)]
    ys = {(pos, x): (O.ristretto_encode(O.pt_mul(pts[pos][0], x)), O.ristretto_encode(O.pt_mul(pts[pos][1], x)))
          for pos in (1, 2, 3) for x in witnesses}
    recs, idx = [], []
    for j, sigma in enumerate(DV.table_audit_scalars()):
        pos = 1 + j % 3
        x = witnesses[(j // 3) % 3]
        rec, _, _, _ = DV.build_entry(sigma, cs[j % len(cs)], pts[pos][0], pts[pos][1], x, ys[(pos, x)])
        recs.append(rec)
        idx.append(pos)
    xs, ks = audit[0], audit[1]
    for j in range(96):                                  # valid under the transcript's challenge
        pos = 1 + j % 3
        recs.append(O.prove(xs[3 * j], ks[3 * j + 1], None, pts[pos][0], pts[pos][1]))
        idx.append(pos)
    good = recs[-3]                                      # position 1
    assert idx[-3] == 1
    s1 = (int.from_bytes(good.s, "little") + 1) % L
    recs.append(O.ProofRecord(good.y1, good.y2, good.r1, good.r2, O.scalar_bytes(s1)))
    idx.append(1)
    recs.append(good)                                    # proven under pair 1, labelled pair 2
    idx.append(2)
    assert len(recs) <= 512
    rows = {q: np.frombuffer(b"".join(getattr(r, q) for r in recs), np.uint8).reshape(-1, 32) for q in Q}
    idx = np.array(idx, np.uint32)
    want = _oracle(pairs, idx, rows)
    n = len(recs)
    assert (want[n - 98:n - 2] == cp.STATUS_OK).all() and want[n - 2] == cp.STATUS_EQ_FAIL
    assert want[n - 1] == cp.STATUS_EQ_FAIL
    return pairs, idx, rows, want


def test_tab16_at_pair_positions(wide_entries):
    pairs, idx, rows, want = wide_entries
    with cp.Gpu(0) as fresh:
        assert fresh.load_pairs(pairs) == 3
        st = fresh.verify_each_pairs(pairs, idx, *[rows[q] for q in Q])
    wrong = np.nonzero(st != want)[0]
    assert wrong.size == 0, [(int(i), int(idx[i]), int(st[i]), int(want[i])) for i in wrong[:8]]


# ---- the cap and the least-recently-used order ---------------------------------------------------
def test_cap_and_lru(pool):
    a, b, c = pool[:64], pool[64:128], pool[128:160]
    n = 64
    xs = _rows32([O.bench_scalar(b"lp-x", i) for i in range(n)])
    ks = _rows32([O.bench_scalar(b"lp-k", i) for i in range(n)])
    idx = np.arange(n, dtype=np.uint32)
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        assert fresh.load_pairs(a) == 64
        assert fresh.pairs_resident(a).all()
        assert fresh.stage_times()[VARBASE][1] == 64
        assert fresh.load_pairs(a) == 0
        assert VARBASE not in fresh.stage_times()
        rows = fresh.prove_pairs(a, idx, xs, ks)
        rows["s"][5] = np.frombuffer(O.scalar_bytes((int.from_bytes(rows["s"][5].tobytes(), "little") + 1) % L),
                                     np.uint8)
        rows["y2"][40] = rows["y2"][41]
        rows["r1"][63] = np.frombuffer(BAD_POINT, np.uint8)
        want = _oracle(a, idx, rows)
        assert want[5] == want[40] == cp.STATUS_EQ_FAIL and want[63] == cp.STATUS_BAD_POINT
        assert np.count_nonzero(want) == 3
        fresh.stage_times()
        st = fresh.verify_each_pairs(a, idx, *[rows[q] for q in Q])
        assert np.array_equal(st, want), np.nonzero(st != want)[0][:8].tolist()
        assert VARBASE not in fresh.stage_times()
        # 64 others: every one of the first 64 goes
        assert fresh.load_pairs(b) == 64
        assert not fresh.pairs_resident(a).any() and fresh.pairs_resident(b).all()
        # 32 resident + 32 new: the call's own resident pairs are not its victims, although they
        # are the least recently used half (b was stamped in row order)
        assert fresh.load_pairs(b[:32] + c) == 32
        assert fresh.pairs_resident(b[:32]).all() and fresh.pairs_resident(c).all()
        assert not fresh.pairs_resident(b[32:]).any()
        # a residency query is no use: c[0] stays the oldest of c and is the next victim
        fresh.load_pairs(b[:32])                      # b[:32] newer than all of c
        assert fresh.pairs_resident(c[:1]).all()
        assert fresh.load_pairs(a[:1]) == 1
        assert not fresh.pairs_resident(c[:1]).any()
        assert fresh.pairs_resident(c[1:]).all() and fresh.pairs_resident(b[:32]).all()


# ---- edges -----------------------------------------------------------------------------------------
def test_one_pair_duplicates_and_a_cached_full_set(pool):
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        assert fresh.load_pairs(pool[:1]) == 1
        assert fresh.pairs_resident(pool[:2]).tolist() == [True, False]
        assert fresh.stage_times()[VARBASE][1] == 1
        assert fresh.load_pairs([pool[1], pool[1], pool[2], pool[1], pool[0]]) == 2
        assert fresh.pairs_resident(pool[:4]).tolist() == [True, True, True, False]
        # a full set (the combs, built by a single-pair prove) counts as resident
        fresh.prove(_rows32([7]), _rows32([11]), params=pool[3])
        st = fresh.stage_times()
        assert st["generators"][1] == 1 and st[VARBASE][1] == 2, st
        assert fresh.pairs_resident(pool[3:4]).all()
        assert fresh.load_pairs([pool[3], pool[0]]) == 0
        st = fresh.stage_times()
        assert VARBASE not in st and "generators" not in st, st


def test_default_pair_without_a_comb_takes_a_light_set():
    with cp.Gpu(0) as fresh:
        assert not fresh.pairs_resident([cp.Parameters()]).any()
        assert fresh.load_pairs([cp.Parameters()]) == 1
        assert fresh.pairs_resident([cp.Parameters()]).all()


# ---- equality under the knob ----------------------------------------------------------------------
def test_batched_build_equals_one_by_one(pool, monkeypatch):
    """The same cold prove_pairs and verify_each_pairs calls with CPZ_PAIRS_BUILD_BATCH=0 (one
    build per pair, the single-pair kernels) and with the default: byte-equal rows and statuses."""
    pairs = [pool[10], cp.Parameters()] + pool[11:17] + [pool[10]]
    n = 300
    idx = (np.arange(n) % len(pairs)).astype(np.uint32)
    xs = _rows32([O.bench_scalar(b"knob-x", i) for i in range(n)])
    ks = _rows32([O.bench_scalar(b"knob-k", i) for i in range(n)])
    ctxs = [(None, b"ctx-%d" % i, bytes([i % 251]) * 32, b"")[i % 4] for i in range(n)]
    seen = {}
    for knob in ("0", None):
        if knob is None:
            monkeypatch.delenv("CPZ_PAIRS_BUILD_BATCH", raising=False)
        else:
            monkeypatch.setenv("CPZ_PAIRS_BUILD_BATCH", knob)
        with cp.Gpu(0) as fresh:
            fresh.set_timing(True)
            rows = fresh.prove_pairs(pairs, idx, xs, ks, contexts=ctxs)   # cold
            built = fresh.stage_times()[VARBASE][1]
        forged = {q: rows[q].copy() for q in Q}
        forged["s"][7] = rows["s"][8]
        forged["y1"][150] = rows["y1"][151]
        forged["r2"][299] = np.frombuffer(BAD_POINT, np.uint8)
        with cp.Gpu(0) as fresh:
            st = fresh.verify_each_pairs(pairs, idx, *[forged[q] for q in Q], contexts=ctxs)   # cold
        seen[knob] = (rows, st, built)
    (r0, s0, b0), (r1, s1, b1) = seen["0"], seen[None]
    assert b0 == b1 == 8
    for q in Q:
        assert np.array_equal(r0[q], r1[q]), q
    assert np.array_equal(s0, s1)
    assert np.nonzero(s1)[0].tolist() == [7, 150, 299] and s1[299] == cp.STATUS_BAD_POINT


# ---- errors ----------------------------------------------------------------------------------------
def test_an_undecodable_pair_among_64_builds_nothing(pool):
    pairs = list(pool[64:128])
    pairs[37] = cp.Parameters(BAD_POINT, pool[0].h)
    rows = [np.zeros((1, 32), np.uint8)] * 5
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        for call in (lambda: fresh.load_pairs(pairs),
                     lambda: fresh.verify_each_pairs(pairs, [0], *rows),
                     lambda: fresh.prove_pairs(pairs, [0], rows[0], rows[1])):
            with pytest.raises(cp.CpzError) as e:
                call()
            assert e.value.code == _native.CPZ_EGENERATOR and "pair 37: " in str(e.value), str(e.value)
            assert "does not decode" in str(e.value)
            assert not fresh.pairs_resident(pairs).any()
            assert VARBASE not in fresh.stage_times()
        # and no resident set is lost to a failing list
        assert fresh.load_pairs(pool[:3]) == 3
        with pytest.raises(cp.CpzError):
            fresh.load_pairs(pairs)
        assert fresh.pairs_resident(pool[:3]).all()


def test_argument_errors(pool):
    ident_g = cp.Parameters(bytes(32), pool[0].h)
    ident_h = cp.Parameters(pool[0].g, bytes(32))
    same = cp.Parameters(pool[0].g, pool[0].g)
    with cp.Gpu(0) as fresh:
        for bad, text in ((ident_g, "generator cannot be identity"), (ident_h, "generator cannot be identity"),
                          (same, "generators g and h must be different")):
            with pytest.raises(cp.CpzError) as e:
                fresh.load_pairs([pool[0], pool[1], bad, pool[2]])
            assert e.value.code == _native.CPZ_EGENERATOR and "pair 2: " + text in str(e.value), str(e.value)
            assert not fresh.pairs_resident(pool[:3]).any()
        # the lowest offending pair is named
        with pytest.raises(cp.CpzError) as e:
            fresh.load_pairs([pool[0], same, ident_g])
        assert "pair 1: " in str(e.value)
        lib, h = fresh._lib, fresh._h
        gh = np.frombuffer(b"".join(p.g + p.h for p in pool[:65]), np.uint8)
        built = ctypes.c_size_t(99)
        out = np.zeros(65, np.uint8)
        assert lib.cpz_ctx_load_pairs(h, 0, gh.ctypes.data, ctypes.byref(built)) == _native.CPZ_EINVAL
        assert built.value == 0
        assert lib.cpz_ctx_load_pairs(h, 65, gh.ctypes.data, None) == _native.CPZ_EINVAL
        assert b"CPZ_PAIRS_MAX" in lib.cpz_last_error()
        assert lib.cpz_ctx_load_pairs(h, 2, None, None) == _native.CPZ_EINVAL
        assert lib.cpz_ctx_load_pairs(None, 2, gh.ctypes.data, None) == _native.CPZ_EINVAL
        assert lib.cpz_ctx_pairs_resident(h, 0, gh.ctypes.data, out.ctypes.data) == _native.CPZ_EINVAL
        assert lib.cpz_ctx_pairs_resident(h, 65, gh.ctypes.data, out.ctypes.data) == _native.CPZ_EINVAL
        assert lib.cpz_ctx_pairs_resident(h, 2, None, out.ctypes.data) == _native.CPZ_EINVAL
        assert lib.cpz_ctx_pairs_resident(h, 2, gh.ctypes.data, None) == _native.CPZ_EINVAL
        assert lib.cpz_ctx_pairs_resident(None, 2, gh.ctypes.data, out.ctypes.data) == _native.CPZ_EINVAL
        assert not fresh.pairs_resident(pool[:64]).any()
        assert lib.cpz_ctx_load_pairs(h, 64, gh.ctypes.data, None) == _native.CPZ_OK   # built_out is optional
        assert fresh.pairs_resident(pool[:64]).all()
