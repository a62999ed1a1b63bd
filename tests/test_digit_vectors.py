"""The coverage that tests/test_gpu_table_audit.py relies on, checked without a GPU: the audit
scalars enumerate every signed digit of every window and byte position, the challenge search
finds every class of the split, and the plain-Python recoding models (tests/digit_vectors.py)
give exactly the packed digits of sc_recode_radix65536, sc_recode_radix256,
sc_recode_radix16_half and sc_recode_radix4_half in the host build of the device source."""
import ctypes
import random

import pytest

import digit_vectors as DV
import pyoracle as O
import split_cases

L = O.L


@pytest.fixture(scope="module")
def lib():
    import build_native
    return ctypes.CDLL(build_native.build_hosttest())


def test_comb_audit_meets_every_digit_of_every_window():
    xs = DV.comb_audit_scalars()
    assert len(xs) == DV.COMB_AUDIT_BODY + 5 and len(set(xs)) == len(xs)
    seen = [set() for _ in range(16)]
    for i in range(0, DV.COMB_AUDIT_BODY):
        d = DV.comb_audit_digits(i)
        for w in range(16):
            seen[w].add(d[w])
    for w in range(15):
        assert seen[w] == set(range(-32768, 32768)), w      # 65,536 digits, once each
    assert seen[15] == set(range(1, 4096))
    # the formula's digits are what the recoding finds (a stride here; all of them in the GPU test's
    # own assertion would cost a second), and the tail adds the top digits 0 and 4096
    for i in list(range(0, DV.COMB_AUDIT_BODY, 251)) + [DV.COMB_AUDIT_BODY - 1]:
        assert DV.recode16(xs[i]) == DV.comb_audit_digits(i), i
    tops = {DV.recode16(x)[15] for x in xs[DV.COMB_AUDIT_BODY:]}
    assert tops == {0, 4096}
    # no canonical scalar has a larger top digit: l - 1 is the largest
    assert DV.recode16(L - 1)[15] == 4096 and (4097 << 240) - (1 << 239) > L


def test_table_audit_meets_every_digit_of_every_byte():
    xs = DV.table_audit_scalars()
    assert len(xs) == DV.TABLE_AUDIT_BODY + 2 + 31 and len(set(xs)) == len(xs)
    seen = [set() for _ in range(32)]
    for m in range(DV.TABLE_AUDIT_BODY):
        d = DV.recode8(xs[m])
        assert d == DV.table_audit_digits(m), m
        for p in range(32):
            seen[p].add(d[p])
    for p in range(31):
        assert seen[p] == set(range(-128, 128)), p
    assert seen[31] == set(range(1, 16))
    tail = xs[DV.TABLE_AUDIT_BODY:]
    assert DV.recode8(tail[0])[31] == 16                     # l - 1: the largest top digit
    assert DV.recode8(tail[1])[0] == -128 and set(DV.recode8(tail[1])[1:31]) == {-127}
    for p in range(31):
        d = DV.recode8(tail[2 + p])
        assert d[p] == -128 and d[p + 1] == 1 and sum(map(abs, d)) == 129, p


def test_comb_edges_hold_the_extremes():
    xs = DV.comb_edge_scalars()
    digs = [DV.recode16(x) for x in xs]
    for w in range(15):
        assert any(d[w] == -32768 for d in digs) and any(d[w] == 32767 for d in digs), w
    assert any(d[:15] == [-32768] + [-32767] * 14 for d in digs)
    assert max(d[15] for d in digs) == 4096
    b = [DV.recode8(x) for x in xs]
    # the carry out of byte 15 into the 2^128 B half, from -128 at byte 0 and from 0xff.. below
    assert DV.recode8((1 << 128) - 128)[:17] == [-128] + [0] * 15 + [1]
    assert DV.recode8((1 << 128) - 1)[:17] == [-1] + [0] * 15 + [1]
    assert any(d[15] == -128 and d[16] == 1 for d in b)      # 0x8000 << 112
    assert max(d[31] for d in b) == 16


def test_challenge_classes_are_all_twelve():
    found, small = DV.challenge_classes()
    assert len(found) == DV.N_CLASSES == 12
    assert set(found) == {(ut, vt, neg) for ut in (0, 1, 2) for vt in (0, 1) for neg in (False, True)}
    for cls, c in found.items():
        assert 0 < c < L and DV.challenge_class(c) == cls
    # a longer scan without the early stop meets no thirteenth class (radix4_half itself asserts
    # the top digits' range), so a change of the split bound shows here
    rng = random.Random(5)
    more = {DV.challenge_class(rng.randrange(L)) for _ in range(4000)}
    more |= {DV.challenge_class(c) for c in split_cases.edge_cases() + split_cases.near_rational_cases()}
    assert more <= set(found)
    assert set(DV.radix4_half(small["all -2"])[:63]) == {-2}
    assert set(DV.radix16_half(small["all -8"])[:31]) == {-8}
    assert all(c < DV.HALF_BOUND for c in small.values())


def _words(x, n):
    return (ctypes.c_uint32 * n)(*[(x >> (32 * k)) & 0xffffffff for k in range(n)])


def _native(lib, name, x, n):
    out = (ctypes.c_uint32 * n)()
    getattr(lib, name)(out, _words(x, n))
    return list(out)


def test_models_equal_the_device_recodings(lib):
    rng = random.Random(20261019)
    audit = DV.comb_audit_scalars()
    full = list(DV.comb_edge_scalars()) + list(DV.table_audit_scalars())
    full += list(audit[::DV.COMB_AUDIT_BODY // 4096]) + list(audit[DV.COMB_AUDIT_BODY:])
    full += [rng.randrange(L) for _ in range(2000)] + [0, 1, L - 1]
    for s in full:
        assert DV.unpack16(_native(lib, "cpzt_recode_radix65536", s, 8)) == DV.recode16(s), hex(s)
        assert DV.unpack8(_native(lib, "cpzt_recode_radix256", s, 8)) == DV.recode8(s), hex(s)
    halves = []
    for c in DV.challenge_list() + split_cases.edge_cases() + [rng.randrange(L) for _ in range(2000)]:
        u, v = split_cases.euclid_half(c)
        halves += [u, abs(v)]
    halves += [0, 1, DV.HALF_BOUND - 1, DV.ALL_MINUS_2, DV.ALL_MINUS_8]
    halves += [rng.randrange(DV.HALF_BOUND) for _ in range(2000)]
    for x in halves:
        assert DV.unpack_radix16_half(_native(lib, "cpzt_recode_radix16_half", x, 4)) == DV.radix16_half(x), hex(x)
        assert DV.unpack_radix4_half(_native(lib, "cpzt_recode_radix4", x, 4)) == DV.radix4_half(x), hex(x)


def test_entry_builder_hits_its_target():
    """An entry built for a target sigma verifies under the oracle and its s' is sigma."""
    g, h = O.BASEPOINT, O.generator_h()
    cs = DV.challenge_list()
    for j, sigma in enumerate(DV.comb_edge_scalars()[:3] + DV.table_audit_scalars()[-2:]):
        c = cs[(5 * j) % len(cs)]
        rec, cb, x, k = DV.build_entry(sigma, c, g, h, 1000 + j)
        _, v = split_cases.euclid_half(c)
        assert v * int.from_bytes(rec.s, "little") % L == sigma
        assert O.verify_response(rec, cb) == O.ST_OK
