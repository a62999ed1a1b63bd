"""The per-proof path's joint table (csrc/scalar25519.h sc_recode_radix4_half, csrc/scalarmul.h
build_joint_table / straus_half_joint, csrc/verify.h verify_proof) on the host build of the
device headers -- the same code the kernels run, with the limb-bound assertions -- against the
Python oracle.  No GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 3 << 125  # sc_half_split: u, |v| < 3 * 2^125
U32x4 = ctypes.c_uint32 * 4


@pytest.fixture(scope="module")
def lib():
    import build_native
    return ctypes.CDLL(build_native.build_hosttest())


def _words(x):
    return U32x4(*[(x >> (32 * k)) & 0xffffffff for k in range(4)])


def _recode(lib, x):
    out = U32x4()
    lib.cpzt_recode_radix4(out, _words(x))
    return out


def _digits(w):
    """The 64 digits of a recoding: 2-bit two's complement, the top one unsigned."""
    d = []
    for i in range(64):
        v = (w[i // 16] >> (2 * (i % 16))) & 3
        d.append(v if i == 63 or v < 2 else v - 4)
    return d


def _scalars():
    rng = np.random.default_rng(20251)
    rnd = [int.from_bytes(rng.bytes(16), "little") % BOUND for _ in range(10_000)]
    # short ones too: the high digits all zero
    rnd += [int.from_bytes(rng.bytes(16), "little") >> int(rng.integers(1, 127)) for _ in range(200)]
    twos = sum(2 << (2 * i) for i in range(62))        # every digit 2 before the carry (bits 0..123)
    edges = [0, 1, 2, 3, BOUND - 1, 1 << 126, (1 << 126) - 1, (1 << 125) - 1,
             twos, twos | (1 << 124), twos | (1 << 126), twos | (2 << 124),
             # top digit forced to 2: bits 126..127 = 1 and a carry out of digit 62
             (1 << 126) | (1 << 124) | twos, (1 << 126) | (1 << 124) | (2 << 122), (1 << 126) + (1 << 125) - 1,
             sum(3 << (2 * i) for i in range(62)), sum(1 << (2 * i) for i in range(63))]
    assert all(0 <= e < BOUND for e in edges)
    return rnd + edges


def test_recoding_digits_sum_and_slots(lib):
    xs = _scalars()
    top_two = 0
    recs = []
    for x in xs:
        d = _digits(_recode(lib, x))
        assert all(-2 <= v <= 1 for v in d[:63]) and 0 <= d[63] <= 2, hex(x)
        assert sum(v << (2 * i) for i, v in enumerate(d)) == x, hex(x)
        top_two += d[63] == 2
        recs.append(d)
    assert top_two >= 3  # the forced cases reached the top digit 2
    # slot and sign reproduce the digit pair of every window (pairs of consecutive random
    # scalars, and every edge with every edge)
    slot, neg = ctypes.c_int(), ctypes.c_int()
    edge = range(len(xs) - 17, len(xs))
    pairs = [(i, i + 1) for i in range(0, 2000, 2)] + [(i, j) for i in edge for j in edge]
    seen = set()
    for iu, iv in pairs:
        wu, wv = _recode(lib, xs[iu]), _recode(lib, xs[iv])
        for i in range(64):
            lib.cpzt_joint_window(wu, wv, i, ctypes.byref(slot), ctypes.byref(neg))
            a, b = recs[iu][i], recs[iv][i]
            assert 0 <= slot.value <= 12
            sa, sb = divmod(slot.value + 2, 5)  # slot = 5 a + b, b in -2..2
            sb -= 2
            sign = -1 if neg.value else 1
            assert (sign * sa, sign * sb) == (a, b), (hex(xs[iu]), hex(xs[iv]), i)
            assert not (i == 63 and neg.value)
            seen.add(slot.value)
    assert seen >= set(range(13)) - {8}  # (2, -2) is the one combination no window selects


def _enc(k):
    return O.ristretto_encode(O.pt_mul(O.BASEPOINT, k % O.L))


TABLE_CASES = [(3, 5), (O.L - 7, 0x1234567890abcdef1234567890abcdef), (2**200 + 9, 2**251 + 17),
               (11, 11), (11, O.L - 11), (1, 2), (2, 1), (6, O.L - 3)]


@pytest.mark.parametrize("alpha,beta", TABLE_CASES)
def test_joint_table_entries(lib, alpha, beta):
    """All 13 entries are [a alpha + b beta] B, also where entries coincide, double or cancel
    (R' = Y', R' = -Y', R' = 2 Y', Y' = 2 R', 2 R' = -Y'): the formulas are complete."""
    out = ctypes.create_string_buffer(13 * 32)
    ok = (ctypes.c_int * 13)()
    assert lib.cpzt_joint_table(out, ok, _enc(alpha), _enc(beta)) == 13
    for a in range(3):
        for b in range(-2, 3):
            e = 5 * a + b
            if e < 0:
                continue
            assert out.raw[32 * e:32 * e + 32] == _enc(a * alpha + b * beta), (a, b)
            assert ok[e] == 1, (a, b)


def test_straus_joint_against_oracle(lib):
    rng = np.random.default_rng(77)
    Y, R = O.pt_mul(O.BASEPOINT, 0xabcdef123457), O.generator_h()
    g = O.G_BYTES

    def r128():
        return int.from_bytes(rng.bytes(16), "little") % BOUND

    twos = sum(2 << (2 * i) for i in range(62))
    cases = [(r128(), r128(), int.from_bytes(rng.bytes(32), "little") % O.L) for _ in range(12)]
    x = r128()
    cases += [(0, r128(), 5), (r128(), 0, O.L - 1), (0, 0, 0), (0, 0, 12345), (x, x, 1), (1, 1, 0), (2, 1, 0),
              (BOUND - 1, BOUND - 1, O.L - 1), (1 << 126, (1 << 126) | (1 << 124) | twos, 2**252),
              ((1 << 126) | (1 << 124) | twos, twos, 7), (twos, 0, 0), (1, BOUND - 1, 3)]
    out = ctypes.create_string_buffer(32)
    for pts in ((Y, R), (Y, Y), (Y, O.pt_neg(Y))):
        ye, re_ = O.ristretto_encode(pts[0]), O.ristretto_encode(pts[1])
        for u, v, sp in cases if pts[1] is R else cases[:6] + cases[-8:]:
            assert lib.cpzt_straus_joint(out, g, ye, re_, u.to_bytes(16, "little"), v.to_bytes(16, "little"),
                                         sp.to_bytes(32, "little")) == 0
            want = O.pt_add(O.pt_mul(O.BASEPOINT, sp), O.pt_add(O.pt_mul(pts[0], u), O.pt_mul(pts[1], v)))
            assert out.raw == O.ristretto_encode(want), (hex(u), hex(v), hex(sp))


def test_verify_proof_golden_statuses(lib, golden):
    """verify_proof (host build) on every golden proof, valid and each forgery kind: the
    oracle's status."""
    g, h = bytes.fromhex(golden["g"]), bytes.fromhex(golden["h"])
    kinds = set()
    for p in golden["proofs"]:
        f = {k: bytes.fromhex(p[k]) for k in ("y1", "y2", "r1", "r2", "s")}
        ctx = bytes.fromhex(p["ctx"]) if p.get("ctx") is not None else None
        rec = O.ProofRecord(f["y1"], f["y2"], f["r1"], f["r2"], f["s"], ctx)
        want = O.verify_one(rec, g, h)
        assert want == p["status"]
        got = lib.cpzt_verify(g, h, f["y1"], f["y2"], f["r1"], f["r2"], f["s"], ctx or b"", len(ctx or b""),
                              0 if ctx is None else 1)
        assert got == want, p["kind"]
        kinds.add(p["kind"])
    assert len(kinds) > 3


def test_opcount_within_prediction(lib, golden):
    """Field products per proof against the count predicted from the schedule.

    Counted: 2,224 M and 2,068 S = 336,140 MADs (parent: 2,304 M, 2,036 S, 342,380 MADs).
    Per equation: table 108 M + 8 S -> 70 M + 16 S; two more doublings, 3 M + 4 S each; the top
    window's addition (8 M) replaced by a product-free conversion.  The squarings are the
    predicted 2,036 + 2 (8 + 8).  The multiplications are 2,304 - 2 (38 + 8) + 2 * 6: the 6 M
    of the two extra doublings (p1p1 -> p2) are part of their 1,040 MADs, and the start costs 0 M
    where 1 M was allowed, so the bound in M is 2,304 - 2 (38 + 7) + 2 * 6 = 2,226, and in MADs
    the predicted saving of 2,320 + 700 per equation: 342,380 - 6,040 = 336,340."""
    g, h = bytes.fromhex(golden["g"]), bytes.fromhex(golden["h"])
    p = next(q for q in golden["proofs"] if "c" in q)
    f = {k: bytes.fromhex(p[k]) for k in ("y1", "y2", "r1", "r2", "s", "c")}
    m, s = ctypes.c_ulonglong(), ctypes.c_ulonglong()
    lib.cpzt_verify_opcount(ctypes.byref(m), ctypes.byref(s), g, h, f["y1"], f["y2"], f["r1"], f["r2"], f["s"], f["c"])
    print("verify_proof: %d M, %d S, %d MADs" % (m.value, s.value, 100 * m.value + 55 * s.value))
    assert s.value <= 2036 + 2 * (8 + 8)
    assert m.value <= 2304 - 2 * (38 + 7) + 2 * 6
    assert 100 * m.value + 55 * s.value <= 342380 - 2 * (2320 + 700)
    oc = json.load(open(os.path.join(ROOT, "bench", "opcount.json")))["verify_each"]
    assert (m.value, s.value) == (oc["fe_mul"], oc["fe_sq"])
