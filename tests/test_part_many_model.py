"""Host-side checks of the partitioned check's many mode (CPZ_CALL_PARTITIONED_MANY): the capacity
and id bounds that csrc/rlc.h states, the first-occurrence slot order of the model the GPU probe is
compared with, and the flag through every mirror -- the header, the Python constants and wrapper,
the Rust sys crate -- with the pinned phrases of the header comment still in place."""
import random
import re

import numpy as np
import pytest

import chaum_pedersen as cp
import part_many_model as MM
import part_pairs_model as PM
from chaum_pedersen import _native


def _header():
    return PM._read("include", "cpz.h")


# ---- capacity and ids ------------------------------------------------------------------------------

@pytest.mark.parametrize("proofs", [128, 256])
def test_capacity_and_id_bounds(proofs):
    """The list offsets are 16-bit and the ids take 15 bits (bit 15: negate) for both block sizes."""
    assert PM.rlc_constant("kPartWindows") is None          # an expression in the header: 2 kRlcWindows
    assert PM.rlc_constant("kRlcWindows") == 16 and MM.WINDOWS == 2 * 16
    cap = MM.list_cap_many(proofs)
    assert cap == 32 * 6 * proofs
    assert cap <= 0xffff
    assert MM.max_id(proofs) < 0x8000
    # every half-digit of every point and of every extra has its list entry, and no more exist
    assert cap == MM.WINDOWS * (4 * proofs) + MM.WINDOWS * (2 * proofs)


def test_header_constants_of_the_many_mode():
    src = MM.rlc_source()
    assert MM.list_cap_many_expr() == "kPartWindows*(4*kPartProofs+2*kPartProofs)"
    assert PM.rlc_constant("kPartMaxPairs") == 64           # the pair mode keeps its bound ...
    assert "constexpr int kPartListCapPairs = kPartWindows * (4 * kPartProofs + 2 * kPartMaxPairs);" in src
    assert "static_assert(2 * kPartMaxPairs <= kPartProofs" in src
    assert PM.rlc_constant("kPairBucketMaxPairs") == 4096   # ... and the slot tables hold 16-bit pair indices
    assert re.search(r"constexpr\s+uint16_t\s+kPartNoPair\s*=\s*0xffff\s*;", src)
    assert re.search(r"static_assert\(kPairBucketMaxPairs <= kPartNoPair", src)
    assert "part_many_fits(128) && part_many_fits(256)" in src
    assert 4096 <= MM.NO_PAIR
    proofs = 128
    assert MM.list_cap_many(proofs) == 24576 and MM.max_id(proofs) == 767
    assert MM.list_cap_many(proofs) > PM.list_cap_pairs(proofs, 64)


# ---- the slots -------------------------------------------------------------------------------------

def test_slot_order_is_first_occurrence():
    idx = [7, 3, 7, 4095, 3, 0, 0, 9]
    assert MM.slot_table(idx, 8, 8, 0) == [7, 3, 4095, 0, 9, MM.NO_PAIR, MM.NO_PAIR, MM.NO_PAIR]
    # two blocks that share pairs in different orders; the last block is partial
    idx = [5, 6, 5, 7, 7, 6, 5]
    assert MM.slot_table(idx, 7, 4, 0) == [5, 6, 7, MM.NO_PAIR]
    assert MM.slot_table(idx, 7, 4, 1) == [7, 6, 5, MM.NO_PAIR]
    # rows past n hold no pair
    assert MM.slot_table(idx, 5, 4, 1) == [7] + [MM.NO_PAIR] * 3
    # every entry its own pair: the identity map
    assert MM.slot_table(list(range(300)), 300, 128, 1) == list(range(128, 256))


def test_slot_sums_agree_with_the_per_pair_sums():
    """The sums by slot are the pair-mode model's sums by pair, permuted by the block's table."""
    rng = random.Random(3)
    proofs, npairs, n = 128, 200, 2 * 128 + 3
    idx = [rng.randrange(npairs) for _ in range(n)]
    prod = [(rng.randrange(MM.L), rng.randrange(MM.L)) for _ in range(n)]
    mult = [65277 - 2 * t for t in range(proofs)]
    for block in range(3):
        table = MM.slot_table(idx, n, proofs, block)
        used = [p for p in table if p != MM.NO_PAIR]
        assert len(set(used)) == len(used) == len({idx[i] for i in range(block * proofs, min(n, (block + 1) * proofs))})
        for m in (None, mult):
            by_pair = PM.pair_sums(prod, idx, n, npairs, proofs, block, m)
            by_slot = MM.slot_sums(prod, idx, n, proofs, block, mult=m)
            for s, p in enumerate(table):
                want = [0, 0] if p == MM.NO_PAIR else by_pair[2 * p:2 * p + 2]
                assert by_slot[2 * s:2 * s + 2] == want
            assert sum(by_slot) % MM.L == sum(by_pair) % MM.L


def test_block_scalar_and_per_proof_count():
    table = [9, 2, MM.NO_PAIR, MM.NO_PAIR]
    gh = {9: (3, 5), 2: (7, 11)}
    sums = [1, 2, 3, 4, 0, 0, 0, 0]
    assert MM.block_scalar([10, 20], [2, 3], sums, table, gh.__getitem__) == 10 * 2 + 20 * 3 + 1 * 3 + 2 * 5 + 3 * 7 + 4 * 11
    assert MM.per_proof_count(300, 128, [5], [1]) == 1 + 128
    assert MM.per_proof_count(300, 128, [], [2]) == 44


# ---- the flag through the mirrors ------------------------------------------------------------------

def test_header_declares_the_flag():
    src = _header()
    m = re.search(r"^#define\s+CPZ_CALL_PARTITIONED_MANY\s+(\d+)u\s*$", src, re.M)
    assert m and int(m.group(1)) == 4
    assert PM.header_define("CPZ_CALL_PARTITIONED") == 2 and PM.header_define("CPZ_CALL_EQUATIONS_ONLY") == 1
    assert PM.header_define("CPZ_ABI_VERSION") == 5 == _native.ABI_VERSION
    assert PM.header_define("CPZ_PAIRS_MAX") == 64


def test_python_and_rust_constants_agree():
    assert _native.CALL_PARTITIONED_MANY == 4
    assert _native.CALL_PARTITIONED_MANY & (_native.CALL_PARTITIONED | _native.CALL_EQUATIONS_ONLY) == 0
    rust = PM._read("rust", "chaum-pedersen-gpu-sys", "src", "lib.rs")
    m = re.search(r"pub const CPZ_CALL_PARTITIONED_MANY: u32 = (\d+);", rust)
    assert m and int(m.group(1)) == 4
    assert re.search(r"pub const CPZ_CALL_PARTITIONED: u32 = 2;", rust)
    assert re.search(r"pub const CPZ_ABI_VERSION: c_int = 5;", rust)


def test_many_comment_keeps_its_phrases_and_gains_the_route():
    src = _header()
    end = src.index("#define CPZ_BATCH_PAIRS_MANY_MAX")
    comment = src[src.rindex("/*", 0, end):end]
    flat = " ".join(comment.replace("*", " ").split())
    for phrase in ("CPZ_BATCH_PAIRS_MANY_MAX", "npairs <= CPZ_PAIRS_MAX is cpz_verify_batch_pairs_ex itself",
                   "CPZ_CALL_PARTITIONED is ignored", "builds no table", "cpz_combine_partials", "Host buffers only",
                   "CPZ_FALLBACK_NONE or _BISECTION", "no output buffer is written"):
        assert phrase in flat, phrase
    for phrase in ("CPZ_CALL_PARTITIONED_MANY", "not automatic", "first occurrence", "stage-13",
                   "CPZ_FALLBACK_PARTITIONED", "out[1] = 0", "out[5] = 0", "light-set cache",
                   "profiles/batch_pairs_many_part_ab.json"):
        assert phrase in flat, phrase
    # the flag's own comment
    at = src.index("#define CPZ_CALL_PARTITIONED_MANY")
    own = " ".join(src[src.rindex("/*", 0, at):at].replace("*", " ").split())
    assert "cpz_verify_batch_pairs_many alone" in own and "not automatic" in own and "CPZ_CALL_PARTITIONED in its place" in own


class _Recorder:
    """Stands for the library: records the flags of the one call it accepts."""

    def __init__(self):
        self.flags = []

    def cpz_verify_batch_pairs_many(self, h, flags, *rest):
        self.flags.append(flags)
        return 0


def _gpu(lib):
    g = cp.Gpu.__new__(cp.Gpu)
    g._lib = lib
    g._h = None
    return g


def test_wrapper_sets_the_flag_and_checks_locate():
    rows = [np.zeros((2, 32), np.uint8)] * 5
    pairs = [cp.Parameters()] * 2
    rec = _Recorder()
    g = _gpu(rec)
    g.verify_batch_pairs_many(pairs, [0, 1], *rows, bytes(32))
    g.verify_batch_pairs_many(pairs, [0, 1], *rows, bytes(32), locate="auto", equations_only=True)
    g.verify_batch_pairs_many(pairs, [0, 1], *rows, bytes(32), locate="partitioned")
    g.verify_batch_pairs_many(pairs, [0, 1], *rows, bytes(32), locate="partitioned", equations_only=True)
    assert rec.flags == [0, 1, 4, 5]
    with pytest.raises(cp.InvalidParams) as many:
        g.verify_batch_pairs_many(pairs, [0, 1], *rows, bytes(32), locate="dense")
    with pytest.raises(cp.InvalidParams) as sibling:
        g.verify_batch_pairs(pairs, [0, 1], *rows, bytes(32), locate="dense")
    assert str(many.value) == str(sibling.value) and "locate must be" in str(many.value)
    assert len(rec.flags) == 4                              # nothing reached the library
    g._lib = None
