"""Plain-Python models of the scalar recodings (csrc/scalar25519.h) and the scalar lists that
walk every fixed-base table entry and every digit edge of the per-proof verify kernels.

Shared by tests/test_part_bounds.py, tests/test_digit_vectors.py (which ties the models to the
host build of the device source) and tests/test_gpu_table_audit.py.  Every model asserts that
its digits sum back to the value.  Test infrastructure only; no GPU."""
import functools
import random

import pyoracle as O
import split_cases

L = O.L
HALF_BOUND = 3 << 125   # sc_half_split: u, |v| < 3 * 2^125


# ---- the recodings ------------------------------------------------------------------------------

def _recode(s, bits, ndigits):
    half, mask = 1 << (bits - 1), (1 << bits) - 1
    d, carry = [], 0
    for w in range(ndigits):
        chunk = ((s >> (bits * w)) & mask) + carry
        carry = (chunk + half) >> bits
        d.append(chunk - (carry << bits))
    assert carry == 0 and s >> (bits * ndigits) == 0, hex(s)
    assert all(-half <= x < half for x in d)
    assert sum(x << (bits * w) for w, x in enumerate(d)) == s
    return d


def recode16(s):
    """sc_recode_radix65536 (and rlc_dev.h recode16): 16 signed radix-2^16 digits in
    [-2^15, 2^15 - 1] of s < 2^253."""
    assert 0 <= s < 1 << 253
    return _recode(s, 16, 16)


def recode8(s):
    """sc_recode_radix256: 32 signed digits in [-128, 127] of s < 2^253."""
    assert 0 <= s < 1 << 253
    return _recode(s, 8, 32)


def radix16_half(x):
    """sc_recode_radix16_half: 32 signed digits in [-8, 7] of a value below 6 * 2^124."""
    assert 0 <= x < 6 << 124
    return _recode(x, 4, 32)


def radix4_half(x):
    """sc_recode_radix4_half: 64 digits of a value below 3 * 2^125; digits 0..62 in [-2, 1], the
    top digit unsigned, in 0..2."""
    assert 0 <= x < HALF_BOUND
    d, carry = [], 0
    for i in range(64):
        n = ((x >> (2 * i)) & 3) + carry
        if i == 63:
            assert 0 <= n <= 2
            carry = 0
            d.append(n)
        else:
            carry = (n + 2) >> 2
            d.append(n - (carry << 2))
    assert all(-2 <= v <= 1 for v in d[:63])
    assert sum(v << (2 * i) for i, v in enumerate(d)) == x
    return d


# ---- the packed forms the device code stores ---------------------------------------------------

def _signed_fields(words, bits):
    per, mask, half = 32 // bits, (1 << bits) - 1, 1 << (bits - 1)
    out = []
    for w in words:
        for m in range(per):
            v = (int(w) >> (bits * m)) & mask
            out.append(v - (mask + 1) if v >= half else v)
    return out


def unpack16(words):
    """The 16 digits of sc_recode_radix65536's 8 words (int16 halves)."""
    return _signed_fields(words, 16)


def unpack8(words):
    """The 32 digits of sc_recode_radix256's 8 words (signed bytes)."""
    return _signed_fields(words, 8)


def unpack_radix16_half(words):
    """The 32 digits of sc_recode_radix16_half's 4 words (two's-complement nibbles)."""
    return _signed_fields(words, 4)


def unpack_radix4_half(words):
    """The 64 digits of sc_recode_radix4_half's 4 words: 2-bit two's complement, the top one
    unsigned."""
    d = _signed_fields(words, 2)
    d[63] = (int(words[3]) >> 30) & 3
    return d


# ---- scalars that enumerate the tables ---------------------------------------------------------

COMB_AUDIT_BODY = 1 << 16


def comb_audit_digits(i):
    """The radix-2^16 digits of comb_audit_scalars()[i], i < 65536."""
    return [((i * (2 * k + 1) + 7919 * k) & 0xFFFF) - 32768 for k in range(15)] + [1 + i % 4095]


@functools.lru_cache(maxsize=None)
def comb_audit_scalars():
    """65,536 values whose windows 0..14 each meet every signed digit exactly once (the odd
    multiplier 2 k + 1 makes i -> digit a bijection of each window) and whose top window meets
    1..4095; a tail with top digits 0 and 4096 (the largest a canonical scalar has): every comb
    entry a scalar below l can select, both signs."""
    body = [sum(d << (16 * k) for k, d in enumerate(comb_audit_digits(i))) for i in range(COMB_AUDIT_BODY)]
    out = tuple(body + [1, 2, L - 1, L - 2, 1 << 252])
    assert all(0 < x < L for x in out)
    return out


TABLE_AUDIT_BODY = 256


def table_audit_digits(m):
    """The radix-256 digits of table_audit_scalars()[m], m < 256."""
    return [((m + 37 * p) & 255) - 128 for p in range(31)] + [1 + m % 15]


@functools.lru_cache(maxsize=None)
def table_audit_scalars():
    """256 values whose byte positions 0..30 each meet every signed digit -128..127 and whose
    top byte meets 1..15; then l - 1 (top digit 16), -128 at every position at once, and -128
    at one position p = 0..30 (the carry leaves byte p for byte p + 1; p = 15 carries from the
    B half into the 2^128 B half)."""
    body = [sum(d << (8 * p) for p, d in enumerate(table_audit_digits(m))) for m in range(TABLE_AUDIT_BODY)]
    out = tuple(body + [L - 1, int("80" * 31, 16)] + [0x80 << (8 * p) for p in range(31)])
    assert all(0 < x < L for x in out)
    return out


@functools.lru_cache(maxsize=None)
def comb_edge_scalars():
    """The short list for the verify kernels: per window the digits 1, 2^15 - 1 and -2^15 (comb
    slot 32768, with the carry into the next window), -2^15 in windows 0..14 at once, the
    largest top digits, and the carry out of byte 15 / window 7."""
    out = []
    for k in range(16):
        out += [v << (16 * k) for v in (1, 0x7fff, 0x8000) if v << (16 * k) < L]
    out.append(sum(0x8000 << (16 * w) for w in range(15)))
    out += [L - 1, L - 2, 1 << 252, 1 << 128, (1 << 128) - 1, (1 << 128) - 128]
    out = list(dict.fromkeys(out))   # 2^128 is also window 8's digit 1
    assert all(0 < x < L for x in out)
    return tuple(out)


# ---- challenges by the class of their split ------------------------------------------------------

CLASS_SEARCH_SEED = 20261019
CLASS_SEARCH_MAX = 200_000
# u < 3 * 2^125 has a top radix-4 digit in 0..2; |v| < l / (3 * 2^125) < 2^126 / 1.5 has one in
# 0..1 (2 would need |v| >= 2^126); v has two signs.
N_CLASSES = 3 * 2 * 2


def challenge_class(c):
    u, v = split_cases.euclid_half(c)
    return radix4_half(u)[63], radix4_half(abs(v))[63], v < 0


def digits_value(digits, bits):
    return sum(d << (bits * i) for i, d in enumerate(digits))


ALL_MINUS_2 = digits_value([-2] * 63 + [1], 2)    # 0x2aaa...aab: radix-4 digits 0..62 all -2
ALL_MINUS_8 = digits_value([-8] * 31 + [1], 4)    # 0x0777...778: radix-16 digits 0..30 all -8


@functools.lru_cache(maxsize=None)
def challenge_classes():
    """{class: challenge}: one challenge per (top radix-4 digit of u, top radix-4 digit of |v|,
    sign of v), from a seeded search that stops once all N_CLASSES are found (or after
    CLASS_SEARCH_MAX draws); and the small challenges, for which v = 1 and u = c: 1, 2, the
    largest such c, the literal 0xaaaa / 0x8888 patterns and the values whose radix-4 digits are
    all -2 and whose radix-16 digits are all -8."""
    rng = random.Random(CLASS_SEARCH_SEED)
    found = {}
    for _ in range(CLASS_SEARCH_MAX):
        c = rng.randrange(L)
        found.setdefault(challenge_class(c), c)
        if len(found) == N_CLASSES:
            break
    small = {"one": 1, "two": 2, "largest u": HALF_BOUND - 1,
             "0xaaaa": int("aa" * 16, 16) >> 2, "0x8888": int("88" * 16, 16) >> 4,
             "all -2": ALL_MINUS_2, "all -8": ALL_MINUS_8}
    for name, c in small.items():
        assert split_cases.euclid_half(c) == (c, 1), name
    assert set(radix4_half(ALL_MINUS_2)[:63]) == {-2} and set(radix16_half(ALL_MINUS_8)[:31]) == {-8}
    return found, small


def challenge_list():
    found, small = challenge_classes()
    return [found[k] for k in sorted(found)] + list(small.values())


# ---- entries whose s' = v s mod l is a chosen value ---------------------------------------------

def response_for(sigma, c):
    """s with v s = sigma (mod l) for the split (u, v) of c: the scalar whose digits the verify
    kernels then recode is sigma itself."""
    _, v = split_cases.euclid_half(c)
    s = sigma * pow(v % L, L - 2, L) % L
    assert (v * s - sigma) % L == 0
    return s


def build_entry(sigma, c, g, h, x, y=None):
    """A valid verify_response entry under generators (g, h) (points) with challenge c whose
    s' = v s mod l equals sigma: s = sigma / v, k = s - c x, y = [x] (g, h), r = [k] (g, h).
    Returns (ProofRecord, c bytes, x, k).  y: the encodings of [x] g, [x] h when known."""
    assert 0 < sigma < L and 0 <= c < L
    s = response_for(sigma, c)
    k = (s - c * x) % L
    while k == 0:
        x = (x + 1) % L
        y = None
        k = (s - c * x) % L
    if y is None:
        y = (O.ristretto_encode(O.pt_mul(g, x)), O.ristretto_encode(O.pt_mul(h, x)))
    rec = O.ProofRecord(y[0], y[1], O.ristretto_encode(O.pt_mul(g, k)), O.ristretto_encode(O.pt_mul(h, k)),
                        O.scalar_bytes(s))
    _, v = split_cases.euclid_half(c)
    sp = v * s % L
    assert sp == sigma and digits_value(recode16(sp), 16) == sigma and digits_value(recode8(sp), 8) == sigma
    return rec, c.to_bytes(32, "little"), x, k
