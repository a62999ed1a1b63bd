"""The partitioned check's integer model (tests/part_model.py) against itself: its identities,
and that every case the GPU probe tests list really has the edge it is listed for.  No GPU."""
import random

import numpy as np

import digit_vectors as DV
import part_model as M
import pyoracle as O

K, L = M.K, O.L


def test_constants_come_from_the_probe():
    assert K.kPartProofs in (128, 256) and K.kPartWindows == 2 * K.kRlcWindows == 32
    assert K.kPartListCap == K.kPartWindows * (4 * K.kPartProofs + 2)
    assert K.kPartOffs == K.kPartWindows * (K.kPartBuckets + 1)
    assert K.kPartUnits == 64 and K.kPartTopBuckets == 16 and K.kPartNoLoc == 0xffff
    assert K.kPartProofs % K.kPartLocLanes == 0
    assert 1 < K.kPartTreeMaxBlocks < 257 < K.kPartLaneMinBlocks   # the dispatch the probe tests rely on


def test_split8_every_digit():
    seen_lo, seen_hi = set(), set()
    for d in range(-32768, 32768):
        lo, hi = M.split8(d)
        assert lo + 256 * hi == d and -128 <= lo < 128 and -128 <= hi <= 128
        seen_lo.add(lo)
        seen_hi.add(hi)
    assert seen_lo == set(range(-128, 128)) and seen_hi == set(range(-128, 129))
    assert M.split8(32640) == (-128, 128) and M.split8(-32768) == (0, -128)
    assert M.split8(32639) == (127, 127) and M.split8(32767) == (-1, 128)


def test_recode16_is_digit_vectors():
    rng = random.Random(1)
    vals = [0, 1, L - 1, 1 << 252, (1 << 253) - 1] + [rng.randrange(1 << 253) for _ in range(500)]
    vals += list(DV.comb_edge_scalars())
    for s in vals:
        assert M.recode16(s) == DV.recode16(s)
        assert M.row_value(M.recode16(s)) == s


def test_low_window_digits_reach_every_listed_edge():
    ds = M.low_window_digits()
    assert len(ds) == len(set(ds)) and all(-32768 <= d < 32768 for d in ds)
    halves = [M.split8(d) for d in ds]
    los = {lo for lo, _ in halves}
    his = {hi for _, hi in halves}
    for e in M.SHARE_EDGES:
        assert -e in los and -e in his, e
        assert (e in los or e == 128) and e in his, e      # lo = +128 does not exist
    # first and last bucket of each of the four 32-bucket shares, in lo and in hi
    for half in (los, his):
        edges = {M.bucket_of(x)[:2] for x in half if x and M.bucket_of(x)[2]}
        assert edges == {(k, k // 32) for k in (0, 31, 32, 63, 64, 95, 96, 127)}
    for e in M.SPLIT_EDGES:
        assert e in ds and -e in ds
    assert (-128, 128) in halves and (0, -128) in halves and (127, 127) in halves and (-1, 128) in halves


def test_top_window_digits():
    ds = M.top_window_digits()
    halves = [M.split8(d) for d in ds]
    assert all(abs(hi) <= K.kPartTopBuckets for _, hi in halves)
    assert {hi for _, hi in halves} >= {s * h for h in M.TOP_HI for s in (1, -1)}
    # TOP_HI: first and last bucket of each four-bucket share
    assert {((h - 1) // M.part_width(31), (h - 1) % 4) for h in M.TOP_HI} == {(s, e) for s in range(4) for e in (0, 3)}
    assert M.split8(4223) == (127, 16) and M.split8(-4224) == (-128, -16)
    for d in M.TOP_OVER_DIGITS:
        assert abs(M.split8(d)[1]) > K.kPartTopBuckets
    assert {abs(M.split8(d)[1]) for d in M.TOP_OVER_DIGITS} >= {17, 128}   # one past the bound, and the largest
    for d in M.TOP_KEPT_DIGITS:
        assert abs(M.split8(d)[1]) == K.kPartTopBuckets
    assert M.split8(M.recode16(M.TOP_OVER_SUM)[15])[1] > K.kPartTopBuckets
    assert M.split8(M.recode16(L - 1)[15]) == (0, 16) and M.split8(M.recode16(1 << 252)[15]) == (0, 16)


def test_one_digit_cases_and_slots():
    cases = M.one_digit_cases()
    assert {w for w, _ in cases} == set(range(16))
    slots = {M.slot_of(i) for i in range(len(cases))}
    assert slots == {4 * t + q for t in (0, 1, 63, 64, K.kPartProofs - 1) for q in range(4)}
    for w, d in cases:
        row = [0] * 16
        row[w] = d
        assert M.row_value(row) == d << (16 * w)


def test_sum_cases():
    cases = M.sum_cases()
    assert all(0 <= a < L and 0 <= b < L for a, b in cases)
    assert {(a, b) for a in M.SUM_SCALARS for b in M.SUM_SCALARS} <= set(cases)
    ds = M.low_window_digits()
    for i, d in enumerate(ds):
        s = M.digit_scalar(i % 15, d)
        assert M.recode16(s)[i % 15] == d and ((s, 0) in cases or (0, s) in cases)


def _one_point_block(slot, w, d):
    rows = np.zeros((4 * K.kPartProofs, 16), np.int64)
    rows[slot, w] = d
    return rows


def test_sort_model_one_digit():
    for i, (w, d) in enumerate(M.one_digit_cases()):
        slot = M.slot_of(i)
        s = M.sort_model(_one_point_block(slot, w, d), 0, 0)
        lo, hi = M.split8(d)
        want = {}
        if lo:
            want[(2 * w, abs(lo) - 1)] = [slot | (0x8000 if lo < 0 else 0)]
        if hi:
            want[(2 * w + 1, abs(hi) - 1)] = [slot | (0x8000 if hi < 0 else 0)]
        keys = sorted(want)
        assert [tuple(x) for x in np.argwhere(s.count).tolist()] == keys and s.count.sum() == len(keys)
        assert s.flat.tolist() == [want[k][0] for k in keys] and s.total == len(want) and not s.top_over
        assert s.offs[-1] == s.total and list(s.offs) == sorted(s.offs)
        M.check_assign(s.assign, s.usz)


def test_sort_model_full_and_random():
    rng = random.Random(7)
    rows, sums = M.full_rows(rng)
    s = M.sort_model(rows.T, *sums)
    assert s.total == K.kPartListCap == s.offs[-1] and not s.top_over
    M.check_assign(s.assign, s.usz)
    r = M.random_rows(rng, 1)
    assert r.shape == (16, 4 * K.kPartProofs) and r[15].min() >= -4224 and r[15].max() <= 4223
    s = M.sort_model(r.T, L - 1, 1)
    assert not s.top_over and s.total < K.kPartListCap
    M.check_assign(s.assign, s.usz)
    for win in s.ids():   # a point enters a window at most once
        ids = [i & 0x7fff for b in win for i in b]
        assert len(ids) == len(set(ids)) and max(ids) <= 4 * K.kPartProofs + 1
    # the flag: exactly when a top-window high half exceeds the bound
    for d in M.TOP_OVER_DIGITS + M.TOP_KEPT_DIGITS:
        s = M.sort_model(_one_point_block(5, 15, d), 0, 0)
        assert s.top_over == (d in M.TOP_OVER_DIGITS)
    assert M.sort_model(_one_point_block(5, 0, 0), M.TOP_OVER_SUM, 0).top_over
    assert M.sort_model(_one_point_block(5, 0, 0), 0, M.TOP_OVER_SUM).top_over


def test_index_weight_digits_and_multipliers():
    js = [M.loc_j(t) for t in range(K.kPartProofs)]
    assert js[0] == K.kPartLocJ0 and len(set(js)) == K.kPartProofs and all(j & 1 for j in js)
    assert (1 << 15) < js[-1] and js[0] < (1 << 16) - 258
    for u, j in M.weight_digit_cases():
        d = M.index_weight_digits(u, j)
        assert len(d) == 16 and d[9:] == [0] * 7
        assert M.row_value(d) == j * M.weight_int(u)                 # exact, as an integer
        assert all(-32768 <= x < 32768 for x in d[:9])               # nine valid int16 digits
    words = {tuple(M.weight_words(u)) for u, _ in M.weight_digit_cases()}
    assert (-32768,) * 8 in words and (32767,) * 8 in words and (-32768, 32767) * 4 in words
    assert {j for _, j in M.weight_digit_cases()} >= {js[0], js[-1]}


def test_index_digit8_strict_bound():
    """|digit 8| of j * weight stays below 2^15 - 128 for every listed weight and every multiplier
    j_t -- the regression test of kPartLocJ0.  With kPartLocJ0 = 2^16 - 257 the weight whose eight
    words are all -32768 gave digit 8 = -32640 = -(2^15 - 128) at j_0 = 65279: the bound was attained,
    not kept (the digit was still a valid int16, so no result was wrong).  2^16 - 259 keeps it: the
    same weight gives -32639 at j_0 = 65277, and all words 32767 give 32638."""
    assert K.kPartLocJ0 < (1 << 16) - 258
    extreme = [[0x80008000] * 4, [0x7fff7fff] * 4]
    cases = M.weight_digit_cases() + [(u, M.loc_j(t)) for u in extreme for t in range(K.kPartProofs)]
    worst = max(cases, key=lambda c: abs(M.index_weight_digits(*c)[8]))
    d8 = M.index_weight_digits(*worst)[8]
    assert abs(d8) < (1 << 15) - 128, "digit 8 = %d for words %r, j = %d" % (d8, M.weight_words(worst[0]), worst[1])
    assert M.index_weight_digits([0x80008000] * 4, (1 << 16) - 257)[8] == -((1 << 15) - 128)   # what the old J0 gave
