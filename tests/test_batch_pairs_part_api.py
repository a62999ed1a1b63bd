"""The mixed-pair batch check's partitioned search, the parts that need no GPU: the per-call flag
and the size threshold in include/cpz.h and their mirrors in chaum_pedersen._native, the Python
keyword, the model of the per-block per-pair sums (tests/part_pairs_model.py) against a brute-force
sum, and the pair-mode capacity and id-width arithmetic of csrc/rlc.h for both block sizes."""
import random

import pytest

import chaum_pedersen as cp
import part_pairs_model as PM
from chaum_pedersen import _native

L = PM.L


def test_header_and_mirror():
    assert PM.header_define("CPZ_CALL_PARTITIONED") == 2 == _native.CALL_PARTITIONED
    assert PM.header_define("CPZ_CALL_EQUATIONS_ONLY") == 1 == _native.CALL_EQUATIONS_ONLY
    assert _native.CALL_PARTITIONED & _native.CALL_EQUATIONS_ONLY == 0
    part_min = PM.header_define("CPZ_BATCH_PAIRS_PART_MIN")
    assert part_min is not None and part_min == _native.BATCH_PAIRS_PART_MIN
    # tests/test_gpu_pairs_bulk.py pins 4104 entries to bisection with every entry per proof
    assert part_min > 4104
    assert part_min <= PM.header_define("CPZ_BATCH_PAIRS_MAX_PROOFS")
    assert PM.header_define("CPZ_ABI_VERSION") == 5 == _native.ABI_VERSION
    assert PM.header_define("CPZ_FALLBACK_PARTITIONED") == 2 and _native.FALLBACK_PATHS[2] == "partitioned"


def test_locate_keyword_is_checked_before_the_library():
    """Any value but "auto" and "partitioned" raises InvalidParams with nothing loaded or called:
    `self` is an object without a library handle."""
    for bad in ("nonsense", "", "Partitioned", None, 2):
        with pytest.raises(cp.InvalidParams):
            cp.Gpu.verify_batch_pairs(object(), [], [], [], [], [], [], [], bytes(32), locate=bad)


@pytest.mark.parametrize("seed", range(6))
def test_pair_sum_model_against_brute_force(seed):
    """Random small batches: 1..9 pairs (some unused), a partial last block, zero products."""
    rng = random.Random(7000 + seed)
    proofs = rng.choice((4, 8, 128))
    n = rng.randrange(1, 3 * proofs + 1)
    npairs = rng.randrange(1, 10)
    used = rng.sample(range(npairs), rng.randrange(1, npairs + 1))
    idx = [rng.choice(used) for _ in range(n)]
    prod = [(rng.choice((0, 1, L - 1, rng.randrange(L))), rng.randrange(L)) for _ in range(n)]
    # poison past n, as an over-allocated buffer would hold: never read
    idx_p = idx + [used[0]] * proofs
    prod_p = prod + [(L - 2, L - 3)] * proofs
    nblk = (n + proofs - 1) // proofs
    total = [0] * (2 * npairs)
    for b in range(nblk):
        got = PM.pair_sums(prod_p, idx_p, n, npairs, proofs, b)
        assert got == PM.pair_sums_brute(prod, idx, n, npairs, proofs, b)
        assert all(0 <= v < L for v in got)
        total = [(x + y) % L for x, y in zip(total, got)]
    assert total == [sum(prod[i][k] for i in range(n) if idx[i] == p) % L for p in range(npairs) for k in range(2)]
    # a pair whose products cancel has a zero sum
    idx2, prod2 = [0, 1, 0], [(5, 7), (9, 9), (L - 5, L - 7)]
    assert PM.pair_sums(prod2, idx2, 3, 2, 4, 0) == [0, 0, 9, 9]
    # the index multipliers of the locate pass
    mult = [65277 - 2 * t for t in range(4)]
    assert PM.pair_sums(prod2, idx2, 3, 2, 4, 0, mult) == [(5 * mult[0] + (L - 5) * mult[2]) % L,
                                                          (7 * mult[0] + (L - 7) * mult[2]) % L,
                                                          9 * mult[1] % L, 9 * mult[1] % L]


def test_capacity_and_id_width():
    """A pair-mode block lists at most kPartWindows * (4 kPartProofs + 2 CPZ_PAIRS_MAX) entries --
    20,480 at 128 proofs, 36,864 at 256 -- which fits the 16-bit offsets, and every id fits 15 bits
    (bit 15 is the sign); csrc/rlc.h states the same."""
    pairs_max = PM.header_define("CPZ_PAIRS_MAX")
    assert pairs_max == 64 == _native.PAIRS_MAX == PM.rlc_constant("kPartMaxPairs")
    assert PM.list_cap_pairs(128, pairs_max) == 20480
    assert PM.list_cap_pairs(256, pairs_max) == 36864
    for proofs in (128, 256):
        assert PM.list_cap_pairs(proofs, pairs_max) <= 0xffff
        assert PM.max_id(proofs, pairs_max) < 0x8000
        assert 2 * pairs_max <= proofs          # one sort thread per extra
        # the extras' ids follow the points' and do not collide with them
        assert 4 * proofs + 2 * (pairs_max - 1) + 1 == PM.max_id(proofs, pairs_max)
    src = PM._read("chaum-pedersen-zkp_amd", "csrc", "rlc.h")
    assert "kPartListCapPairs = kPartWindows * (4 * kPartProofs + 2 * kPartMaxPairs)" in src
    assert "static_assert(kPartListCapPairs <= 0xffff" in src
    assert "static_assert(4 * kPartProofs + 2 * kPartMaxPairs <= 0x8000" in src
    assert PM.rlc_constant("kPartBuckets") == PM.BUCKETS and PM.rlc_constant("kPartTopBuckets") == PM.TOP_BUCKETS


def test_extra_scalar_stays_in_the_top_window():
    """An extra's scalar is below l, so its top radix-2^16 digit is at most 4097 and the high half
    at most 16 = kPartTopBuckets: fail bit 1 cannot come from an extra."""
    for s in (L - 1, 1 << 252, (1 << 252) + (1 << 124)):
        top = PM.recode16(s)[15]
        assert 0 <= top <= 4097 and 0 <= PM.split8(top)[1] <= PM.TOP_BUCKETS
        assert PM.row_value(PM.recode16(s)) == s
