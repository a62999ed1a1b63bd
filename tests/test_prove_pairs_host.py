"""The mixed-pair prover's table walk (csrc/scalarmul.h pair_table_mul) on the host build of the
device headers -- the code k_prove_points_pairs runs, with the limb-bound assertions on -- against
the Python oracle's pt_mul.  The tables are built by tests/native/hostlib_prove.cpp with the
library's own small_mul / p3_to_niels and the level doublings.  No GPU."""
import ctypes

import numpy as np
import pytest

import pyoracle as O
from prove_pairs_cases import EDGES, custom_pairs_scalars

ENTRIES = 128


@pytest.fixture(scope="module")
def lib():
    import build_native
    lib = ctypes.CDLL(build_native.build_hosttest())
    lib.cpzt_pair_tables_bytes.restype = ctypes.c_int
    lib.cpzt_niels_bytes.restype = ctypes.c_int
    lib.cpzt_pair_tables.restype = ctypes.c_int
    lib.cpzt_pair_tables.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
    lib.cpzt_pair_table_mul.restype = None
    lib.cpzt_pair_table_mul.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_char_p]
    return lib


@pytest.fixture(scope="module")
def pair(lib):
    """A custom pair (g, h) = ([a] B, [b] B) as points, and its tables as rows of one entry each:
    [8 levels][g, h][128 entries]."""
    (a, b), = custom_pairs_scalars(1, b"prove-pairs-host")
    g, h = O.pt_mul(O.BASEPOINT, a), O.pt_mul(O.BASEPOINT, b)
    nb = lib.cpzt_niels_bytes()
    assert lib.cpzt_pair_tables_bytes() == 16 * ENTRIES * nb
    tab = np.zeros((16 * ENTRIES, nb), np.uint8)
    assert lib.cpzt_pair_tables(tab.ctypes.data, O.ristretto_encode(g), O.ristretto_encode(h)) == 1
    return g, h, tab


def _walk(lib, tab, raw):
    og, oh = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    dig = (ctypes.c_int8 * 32)()
    tab = np.ascontiguousarray(tab)
    lib.cpzt_pair_table_mul(og, oh, dig, tab.ctypes.data, raw)
    return og.raw, oh.raw, list(dig)


def _expect(g, h, raw):
    v = int.from_bytes(raw, "little") % O.L
    return O.ristretto_encode(O.pt_mul(g, v)), O.ristretto_encode(O.pt_mul(h, v))


def test_edges_and_random_scalars_match_the_oracle(lib, pair):
    g, h, tab = pair
    rng = np.random.default_rng(20261)
    cases = list(EDGES) + [("random %d" % i, O.scalar_bytes(int.from_bytes(rng.bytes(64), "little") % O.L))
                           for i in range(200)]
    seen = set()
    for name, raw in cases:
        og, oh, dig = _walk(lib, tab, raw)
        assert sum(d << (8 * j) for j, d in enumerate(dig)) == int.from_bytes(raw, "little") % O.L, name
        assert all(-128 <= d <= 127 for d in dig), name
        assert (og, oh) == _expect(g, h, raw), name
        seen.update(dig)
    assert {0, -128, 127, -1, 1} <= seen               # the digit edges were walked
    assert _walk(lib, tab, EDGES[0][1])[:2] == (bytes(32), bytes(32))   # [0] g, [0] h: the identity


def _row(level, e, mag):
    return (2 * level + e) * ENTRIES + mag - 1


LEVEL_OF_PART = [0, 4, 2, 5, 1, 6, 3, 7]     # kNielsLevelOfPart


def test_digit_minus_128_reads_entry_127_and_no_other(lib, pair):
    """128 = -128 + 1 * 256: digit 0 is -128, digit 1 is +1, both on part 0.  With every other entry
    of the tables replaced by a wrong (valid) point the products are unchanged, so nothing else is
    read; with entry 127 of part 0 replaced they change, so index |d| - 1 = 127 is the one read."""
    g, h, tab = pair
    raw = (128).to_bytes(32, "little")
    want = _expect(g, h, raw)
    og, oh, dig = _walk(lib, tab, raw)
    assert dig[:3] == [-128, 1, 0] and not any(dig[2:]) and (og, oh) == want
    used = [_row(0, e, m) for e in (0, 1) for m in (128, 1)]
    wrong = tab[_row(3, 0, 77)].copy()             # a valid Niels point that is none of the four
    only = np.repeat(wrong[None, :], len(tab), 0)
    only[used] = tab[used]
    assert _walk(lib, only, raw)[:2] == want
    for e in (0, 1):
        bad = tab.copy()
        bad[_row(0, e, 128)] = wrong
        got = _walk(lib, bad, raw)[:2]
        assert got[e] != want[e] and got[1 - e] == want[1 - e]
        # the neighbouring entry (index 126, the multiple 127) is not the one read
        bad = tab.copy()
        bad[_row(0, e, 127)] = wrong
        assert _walk(lib, bad, raw)[:2] == want


def test_a_zero_digit_adds_nothing(lib, pair):
    """2^32 has the single non-zero digit 1, on part 1 (digit 4): the other 31 digits read no
    entry -- every other row replaced by a wrong point leaves the products unchanged -- and the
    scalar 0 reads none at all."""
    g, h, tab = pair
    raw = (1 << 32).to_bytes(32, "little")
    want = _expect(g, h, raw)
    wrong = tab[_row(3, 0, 77)].copy()
    only = np.repeat(wrong[None, :], len(tab), 0)
    used = [_row(LEVEL_OF_PART[1], e, 1) for e in (0, 1)]
    only[used] = tab[used]
    og, oh, dig = _walk(lib, only, raw)
    assert [j for j, d in enumerate(dig) if d] == [4] and dig[4] == 1
    assert (og, oh) == want
    none = np.repeat(wrong[None, :], len(tab), 0)
    assert _walk(lib, none, bytes(32))[:2] == (bytes(32), bytes(32))


def test_every_part_reads_its_own_level(lib, pair):
    """2^(32 q) + 2^(32 q + 8): digits 4 q and 4 q + 1 are 1, on part q alone, whose level is
    kNielsLevelOfPart[q]."""
    g, h, tab = pair
    wrong = tab[_row(3, 0, 77)].copy()
    for q in range(8):
        raw = ((1 << (32 * q)) + (1 << (32 * q + 8))).to_bytes(32, "little")
        only = np.repeat(wrong[None, :], len(tab), 0)
        used = [_row(LEVEL_OF_PART[q], e, 1) for e in (0, 1)]
        only[used] = tab[used]
        assert _walk(lib, only, raw)[:2] == _expect(g, h, raw), q
