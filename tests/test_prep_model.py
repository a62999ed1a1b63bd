"""CPU checks of tests/prep_model.py and tests/scalar_vectors.py: the model's weights are the
oracle's, every named case of tests/test_gpu_prep_probe.py reaches the edge it names, the status
table agrees with the oracle's per-entry decode status, and the model's digits and points add up
to pyoracle.rlc_partial.  No GPU, and nothing here runs the code under test."""
import numpy as np
import pytest

import prep_model as M
import pyoracle as O
import scalar_vectors as SV

L, P = O.L, O.P


def test_weights_are_the_oracles():
    for first in (0, 1000, (1 << 32) - 3, (1 << 63) + 5, M.MIN_HALF_INDEX):
        for i in range(6):
            ha, hb = M.weight_halves(M.SEED, first + i)
            assert (SV.weight_value(ha), SV.weight_value(hb)) == O.rlc_weights(M.SEED, first + i)
    for nm in ("size_65", "counter_wrap32", "counter_2p63"):
        b, m = M.case(nm), M.model(nm)
        for i in range(b.n):
            assert m.weights[i] == O.rlc_weights(b.seed, b.first_index + i)


def test_scalar_vector_families():
    red = SV.reduce_wide_cases()
    red = set(red)
    assert len(red) > 40000 and all(0 <= x < 1 << 512 for x in red)
    assert all((1 << b) + d in red for b in range(1, 512) for d in (-1, 0, 1))
    for k in (0, 1, SV.KMAX, SV.KMAX - 1, 1 << 259, (1 << 259) - 1):
        assert k * L in red and k * L + 1 in red
    assert max(red) == (1 << 512) - 1 and 0 in red
    g = SV.grid_values()
    assert set(SV.GRID_EDGES) <= set(g) and all(0 <= v < L for v in g) and len(SV.grid_pairs()) == len(g) ** 2
    assert any(a + b >= L for a, b in SV.grid_pairs()) and any(a + b == L for a, b in SV.grid_pairs())
    assert {L - 1, L, L + 1, 2**253, 2**255, 2**256 - 1} <= set(SV.CANONICAL_CASES)
    w = SV.weight_cases()
    for k in range(8):
        for v in SV.HALF_EDGES:
            assert any(h[k] == v and all(x == 0 for j, x in enumerate(h) if j != k) for h in w)
    assert (0x8000,) * 8 in w and (0xffff,) * 8 in w
    assert SV.weight_value((0x8000,) * 8) == (-sum(1 << (16 * k + 15) for k in range(8))) % L
    assert SV.weight_value((0xffff,) + (0,) * 7) == L - 1
    assert SV.weight_value((0,) * 7 + (0x8000,)) == L - (1 << 127)


def test_recode16_cases_reach_their_edges():
    for s in SV.recode16_cases():
        d = SV.recode16_model(s)
        assert all(-(1 << 15) <= x < 1 << 15 for x in d), hex(s)
        assert M.digit_value(d) == s, hex(s)
    assert SV.recode16_model(SV.from_windows([0x7fff] * 16)) == [0x7fff] * 16
    assert SV.recode16_model(SV.ALL_7FFF_BELOW_L) == [0x7fff] * 15 + [0x0fff]
    assert SV.recode16_model(SV.RIPPLE) == [-0x8000] + [0] * 14 + [0x1000]   # the carry reaches the top window
    assert SV.RIPPLE < L and SV.ALL_7FFF_BELOW_L < L
    t = SV.recode16_targets()
    assert {SV.RIPPLE, SV.ALL_7FFF_BELOW_L, L - 1, 0, 1, 2**252} <= set(t) and all(x < L for x in t)


def test_min_half_index_is_the_scan():
    assert M.scan_min_half(M.SEED, 0, 1 << 16) == M.MIN_HALF_INDEX
    b, m = M.case("counter_min_half"), M.model("counter_min_half")
    i = M.MIN_HALF_INDEX - b.first_index
    assert 0 <= i < b.n and m.live[i]
    assert -(1 << 15) in m.digits[i][0] + m.digits[i][2]


def test_counter_cases_cross_their_edges():
    b = M.case("counter_wrap32")
    assert b.n >= 8 and b.first_index < 1 << 32 <= b.first_index + b.n - 1
    m = M.model("counter_wrap32")
    # the weights past the carry are those of the 64-bit index, not of its low word
    i = (1 << 32) - b.first_index
    assert m.weights[i] == O.rlc_weights(b.seed, 1 << 32) != O.rlc_weights(b.seed, 0)
    assert M.case("counter_2p63").first_index == (1 << 63) + 5


def test_size_cases():
    assert M.SIZES == (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
    for n in M.SIZES:
        b, m = M.case("size_%d" % n), M.model("size_%d" % n)
        assert b.n == n
        rej = [i for i in range(n) if not m.live[i]]
        assert rej == [i for i in (63, 127, 255) if i < n]
        assert len(m.block_sums) == 2 * ((n + 255) // 256) and len(m.quarter_sums) == (n + 63) // 64
        for k, (sa, sb) in enumerate(m.block_sums):
            rows = range(128 * k, min(n, 128 * k + 128))
            assert sa == sum(m.prod[i][0] for i in rows) % L and sb == sum(m.prod[i][1] for i in rows) % L
            if not len(rows):
                assert (sa, sb) == (0, 0)


def test_product_digits_are_the_targets():
    b, m = M.case("product_digits"), M.model("product_digits")
    targets = b.facts["targets"]
    assert b.n == 2 * len(targets)
    for k, t in enumerate(targets):
        for half in range(2):
            i = 2 * k + half
            w = m.weights[i][half]
            assert w != 0 and m.live[i] and w * b.c[i] % L == t
            assert m.digits[i][1 + 2 * half] == SV.recode16_model(t)
    k = targets.index(SV.RIPPLE)
    assert m.digits[2 * k][1] == [-0x8000] + [0] * 14 + [0x1000] == m.digits[2 * k + 1][3]
    k = targets.index(SV.ALL_7FFF_BELOW_L)
    assert m.digits[2 * k][1] == [0x7fff] * 15 + [0x0fff]


def test_mixed300_wraps_every_addition():
    b, m = M.case("mixed300"), M.model("mixed300")
    assert all(m.live[i] for i in range(256))
    for blk in range(2):
        terms = [m.prod[i][blk] for i in range(128 * blk, 128 * blk + 128)]
        assert terms == [L - 1] * 128
        # a tree over 128 (or 64, then 2) such terms: every partial sum is l - k, so each addition wraps
        assert m.block_sums[blk][blk] == L - 128
        assert m.quarter_sums[2 * blk][blk] == L - 64
    tail = [m.status[i] for i in range(256, 300)]
    assert {M.ST_OK, M.ST_ZERO_S, M.ST_BAD_SCALAR, M.ST_BAD_POINT, M.ST_IDENTITY} == set(tail)
    assert any(b.s[i] == L - 1 and m.live[i] for i in range(256, 300))
    assert len(m.block_sums) == 4 and m.block_sums[3] == (0, 0) and m.block_sums[2] != (0, 0)


@pytest.mark.parametrize("eq_only", [0, 1])
def test_status_table(eq_only):
    """The table is the full cross product, every kind of undecodable encoding is in it, the model
    follows the precedence, a rejected entry has zero digits and products, and wherever the input
    status is what the response check derives from s itself the oracle's decode status agrees."""
    b, m = M.case("status_table_eq%d" % eq_only), M.model("status_table_eq%d" % eq_only)
    table = b.facts["table"]
    bad = M.bad_encodings()
    assert {M.bad_kind(e) for e in bad} == {"non-canonical", "negative", "non-square", "negative-t", "zero-y"}
    assert all(M.decode(e) is None for e in bad)
    want = {(pos, e, st, idm) for pos in M.POSITIONS for e in bad for st in (0, 3, 5) for idm in range(4)}
    want |= {(None, None, st, idm) for st in (0, 3, 5) for idm in range(4)}
    assert set(table) == want and len(table) == len(want) and b.n == len(table) + 3
    compared = 0
    for i, (pos, e, st_in, idm) in enumerate(table):
        ident = bool(idm & 1 and pos != "r1") or bool(idm & 2 and pos != "r2")
        if pos is not None:
            exp = M.ST_BAD_POINT
        elif st_in == M.ST_BAD_SCALAR:
            exp = M.ST_BAD_SCALAR
        elif ident and not eq_only:
            exp = M.ST_IDENTITY
        elif st_in == M.ST_ZERO_S:
            exp = M.ST_ZERO_S
        else:
            exp = M.ST_OK
        assert m.status[i] == exp, i
        if exp != M.ST_OK:
            assert m.digits[i] == [[0] * 16] * 4 and m.prod[i] == (0, 0)
        elif ident:
            assert eq_only
            q = 0 if idm & 1 else 2
            assert m.niels[4 * i + q] == (1, 1, 0) and any(m.digits[i][q]) and m.prod[i] != (0, 0)
        # the response check's own status of s: bad scalar iff s >= l, zero s iff s == 0 and not eq_only
        derived = M.ST_BAD_SCALAR if b.s[i] >= L else (M.ST_ZERO_S if b.s[i] == 0 and not eq_only else M.ST_OK)
        if derived == st_in:
            rec = O.ProofRecord(b.enc["y1"][i], b.enc["y2"][i], b.enc["r1"][i], b.enc["r2"][i],
                                (b.s[i] % (1 << 256)).to_bytes(32, "little"))
            assert O.decode_status(rec, commitment_checks=not eq_only)[0] == exp, i
            compared += 1
    assert compared >= len(table) * 2 // 3
    for i in range(len(table), b.n):   # identity statements stay OK, with the Niels entry (1, 1, 0)
        assert m.status[i] == M.ST_OK
        assert (1, 1, 0) in (m.niels[4 * i + 1], m.niels[4 * i + 3])
    assert any(not v for v in m.live.values()) and any(m.live.values())


def test_all_ok_cases_have_no_rejection():
    for nm in M.ALL_OK_CASES:
        assert all(M.model(nm).live.values()), nm


def test_closure_with_the_oracle():
    """sum digit-value x point over the model's 4 n entries plus g, h with the summed products is
    pyoracle.rlc_partial of the same records: the model is tied to the oracle, not to itself."""
    b, m = M.case("closure24"), M.model("closure24")
    assert [i for i in range(b.n) if not m.live[i]] == sorted((M.CLOSURE_BAD_POINT, M.CLOSURE_ZERO_S))
    assert m.status[M.CLOSURE_BAD_POINT] == M.ST_BAD_POINT and m.status[M.CLOSURE_ZERO_S] == M.ST_ZERO_S
    recs = b.facts["recs"]
    assert [O.verify_one(r) for r in recs].count(O.ST_EQ_FAIL) == len(M.CLOSURE_FORGED)
    cols, pts = [], []
    for i in range(b.n):
        if not m.live[i]:
            continue   # zero digits: the (possibly undecodable) points never enter
        for q in range(4):
            cols.append(m.digits[i][q])
            pts.append(M.point_of_niels(*m.niels[4 * i + q]))
    sums = M.extra_model(m.block_sums, 0, len(m.block_sums))
    cols += sums
    pts += [O.BASEPOINT, O.generator_h()]
    got = M.weighted_sum(cols, pts)
    want = O.rlc_partial(recs, b.seed, b.first_index)
    assert O.ristretto_encode(got) == O.ristretto_encode(want)
    assert not O.pt_is_identity(want)   # three forged entries
    # and without the forged entries the partial is the identity
    ok = [i for i in range(b.n) if m.live[i] and i not in M.CLOSURE_FORGED]
    cols2 = [m.digits[i][q] for i in ok for q in range(4)]
    pts2 = [M.point_of_niels(*m.niels[4 * i + q]) for i in ok for q in range(4)]
    sg = [SV.recode16_model(sum(m.prod[i][k] for i in ok) % L) for k in range(2)]
    assert O.pt_is_identity(M.weighted_sum(cols2 + sg, pts2 + [O.BASEPOINT, O.generator_h()]))


def test_niels_round_trip():
    """fe_limbs / niels_bytes / niels_ints / point_of_niels are inverse to each other, also on
    signed and loose limbs."""
    for enc in M.pool()[:5]:
        pt = M.decode(enc)
        for neg in (False, True):
            raw = np.frombuffer(M.niels_bytes(pt, neg), np.int32).reshape(1, 32)
            f = [v[0] for v in M.niels_ints(raw)]
            q = M.point_of_niels(*f)
            assert O.pt_eq(q, O.pt_neg(pt) if neg else pt) and q[0] == ((-pt[0]) % P if neg else pt[0])
        assert tuple(f) == M.neg_niels_triple(pt)
    loose = np.zeros((1, 32), np.int32)
    loose[0, 0], loose[0, 1], loose[0, 9] = -5, 3, -1
    assert M.niels_ints(loose)[0][0] == (-5 + (3 << 26) - (1 << 230)) % P


def test_extra_cases():
    sums = M.extra_sums()
    assert len(sums) == M.EXTRA_NSUM >= 513
    assert {(0, 1), (0, 2), (1, 2), (3, 260), (0, 513)} <= set(M.EXTRA_RANGES)
    assert sums[0] == (L - 1, L - 1) and sums[3][0] == L - 1   # wrapping terms in every range
    for b0, b1 in M.EXTRA_RANGES:
        for k, col in enumerate(M.extra_model(sums, b0, b1)):
            assert M.digit_value(col) == sum(s[k] for s in sums[b0:b1]) % L
    assert M.extra_model(sums, 5, 5) == [[0] * 16] * 2


def test_pair_cases():
    for npairs in M.PAIR_COUNTS:
        pc = M.pair_case(npairs)
        assert len(pc.idx) == M.PAIR_N == 300 and set(pc.idx) <= set(range(npairs)) and len(pc.gh) == 256 * npairs
        assert (0, 0) in pc.prod and (L - 1, L - 1) in pc.prod
        for lo, hi in M.PAIR_RANGES:
            assert lo % 256 == 0
            cols = M.pair_model(pc, lo, hi)
            total = [sum(M.digit_value(c[k]) for c in cols) % L for k in range(2)]
            assert total == [sum(pc.prod[i][k] for i in range(lo, hi)) % L for k in range(2)]
    pc = M.pair_case(64)
    assert not set(M.PAIR_EMPTY) & set(pc.idx) and len(set(pc.idx)) == 62
    assert M.pair_model(pc, 0, 300)[5] == [[0] * 16] * 2
    assert sum(1 for c in M.pair_model(pc, 0, 1) if c != [[0] * 16] * 2) <= 1
    assert {(0, 300), (256, 300), (0, 1)} == set(M.PAIR_RANGES)
