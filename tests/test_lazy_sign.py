"""The per-proof path's lazy window sign and lean joint table (csrc/scalarmul.h straus_half_joint,
comb_add, build_joint_table<false>) on the host build of the device headers -- the same code the
kernels run, with the limb-bound assertions -- against the Python oracle.  No GPU.

The Straus loop keeps its sum as sigma * cur and negates X of the completed point when the sign of
a window's table slot differs from the previous one's, so what has to be met is every sequence
of window signs, not only random ones: the scalars here are put together from chosen digits."""
import ctypes
import os

import numpy as np
import pytest

import pyoracle as O

BOUND = 3 << 125  # sc_half_split: u, |v| < 3 * 2^125
U32x4 = ctypes.c_uint32 * 4
NEG = [(a, b) for a in (-2, -1) for b in (-2, -1, 0, 1)] + [(0, -2), (0, -1)]  # 5 a + b < 0
POS = [(1, b) for b in (-2, -1, 0, 1)] + [(0, 1)]                              # 5 a + b > 0


@pytest.fixture(scope="module")
def lib():
    import build_native
    return ctypes.CDLL(build_native.build_hosttest())


def _words(x):
    return U32x4(*[(x >> (32 * k)) & 0xffffffff for k in range(4)])


def _window_signs(lib, u, v):
    """Sign (-1, 0, +1) of the table slot of windows 0..63 as the loop reads them."""
    wu, wv = U32x4(), U32x4()
    lib.cpzt_recode_radix4(wu, _words(u))
    lib.cpzt_recode_radix4(wv, _words(v))
    slot, neg = ctypes.c_int(), ctypes.c_int()
    out = []
    for i in range(64):
        lib.cpzt_joint_window(wu, wv, i, ctypes.byref(slot), ctypes.byref(neg))
        out.append(0 if slot.value == 0 else (-1 if neg.value else 1))
    return out


def _scalars(signs, rng, top=(1, 1), only=None):
    """(u, v) whose windows 0..62 have the given signs (-1, 0, +1; signs[i] is window i), the
    digit pairs drawn from all that give the sign.  Digits in [-2, 1] are the recoding's own
    (the representation is unique), so the loop sees exactly these.  top: the unsigned top digits
    (1 keeps the value inside [0, 3 * 2^125) whatever the lower digits are).  only = "u" / "v":
    the other scalar is 0, the sign carried by one digit alone."""
    a, b = [], []
    for s in signs:
        if only == "u":
            a.append(0 if s == 0 else (int(rng.choice((-2, -1))) if s < 0 else 1))
            b.append(0)
        elif only == "v":
            a.append(0)
            b.append(0 if s == 0 else (int(rng.choice((-2, -1))) if s < 0 else 1))
        else:
            p = (0, 0) if s == 0 else (NEG if s < 0 else POS)[int(rng.integers(len(NEG if s < 0 else POS)))]
            a.append(p[0])
            b.append(p[1])
    tu, tv = (top[0] if only != "v" else 0), (top[1] if only != "u" else 0)
    u = sum(d << (2 * i) for i, d in enumerate(a)) + (tu << 126)
    v = sum(d << (2 * i) for i, d in enumerate(b)) + (tv << 126)
    assert 0 <= u < BOUND and 0 <= v < BOUND
    return u, v


def _comb_scalar(digits15, top=1):
    """s' < 2^253 whose radix-2^16 recoding is digits15 (15 digits in [-2^15, 2^15)) and `top`."""
    assert len(digits15) == 15 and all(-32768 <= d < 32768 for d in digits15) and 0 < top < (1 << 13)
    sp = sum(d << (16 * j) for j, d in enumerate(digits15)) + (top << 240)
    assert 0 < sp < (1 << 253)
    return sp


def _cases(lib):
    rng = np.random.default_rng(9496)
    alt = [(-1) ** i for i in range(63)]
    pat = {
        "all_negative": [-1] * 63,
        "alternating": alt,
        "alternating_from_plus": [-s for s in alt],
        "first_below_top_negative": [1] * 62 + [-1],
        "last_negative": [-1] + [1] * 62,
        "only_last_negative": [-1] + [0] * 62,
        # slot 0 (the identity, sign +) between windows of opposite and of equal signs
        "zeros_between": [(-1, 0, 1, 0, 0, -1, 0, -1, 1, 0)[i % 10] for i in range(63)],
        "random": [int(rng.integers(-1, 2)) for _ in range(63)],
    }
    combs = {
        "all_negative": _comb_scalar([-int(rng.integers(1, 32769)) for _ in range(15)]),
        "alternating": _comb_scalar([(-1) ** j * int(rng.integers(1, 32768)) for j in range(15)]),
        "alternating_from_minus": _comb_scalar([-(-1) ** j * int(rng.integers(1, 32768)) for j in range(15)]),
        "all_min": _comb_scalar([-32768] * 15),
        "zeros_between": _comb_scalar([(-5, 0, 7, 0, -32768, 0, 0, 32767, -1, 1, 0, -9, 0, 3, -2)[j] for j in range(15)]),
        "zero": 0,
        "random": int.from_bytes(rng.bytes(32), "little") % O.L,
    }
    ck = list(combs)
    cases = []
    for k, (name, signs) in enumerate(pat.items()):
        for only in (None, "u", "v") if name in ("all_negative", "alternating", "zeros_between") else (None,):
            u, v = _scalars(signs, rng, only=only)
            got = _window_signs(lib, u, v)
            assert got[:63] == signs and got[63] >= 0, name  # the premise: the loop reads these signs
            cn = ck[(k + len(cases)) % len(ck)]
            cases.append((name + ("" if only is None else "_only_" + only) + "/" + cn, u, v, combs[cn]))
    # every comb pattern after a sum that arrives negated (last window negative) and one that does not
    for cn, sp in combs.items():
        for name in ("last_negative", "first_below_top_negative"):
            u, v = _scalars(pat[name], rng)
            cases.append((name + "/" + cn, u, v, sp))
    # the top window's other slots before a negative window: (2, 0) = slot 10 (a top digit 2 needs
    # digit 62 = -2 to stay below 3 * 2^125) and (0, 0) = the identity
    def val(d, top):
        return sum(x << (2 * i) for i, x in enumerate(d)) + (top << 126)

    u, v = val([-1] * 62 + [-2], 2), val([1, -2] * 31 + [1], 0)
    assert _window_signs(lib, u, v) == [-1] * 63 + [1]
    cases.append(("top_slot_10", u, v, combs["all_negative"]))
    u, v = val([-1, 1] * 31 + [1], 0), val([0] * 62 + [1], 0)
    assert _window_signs(lib, u, v) == [-1, 1] * 31 + [1, 0]
    cases.append(("top_slot_0", u, v, combs["alternating"]))
    assert all(0 <= u < BOUND and 0 <= v < BOUND for _, u, v, _ in cases)
    return cases


def test_comb_recoding_premise():
    """The comb scalars above recode to the digits they were made from (the recoding is the
    signed radix-2^16 one of sc_recode_radix65536: n + carry in [-2^15, 2^15))."""
    sp = _comb_scalar([-32768] * 15)
    carry, digits = 0, []
    for j in range(16):
        n = ((sp >> (16 * j)) & 0xffff) + carry
        carry = (n + 32768) >> 16
        digits.append(n - (carry << 16))
    assert digits == [-32768] * 15 + [1] and carry == 0


def test_straus_joint_sign_patterns(lib):
    """[s'] B + [u] Y + [v] R through straus_half_joint for chosen window and comb sign sequences,
    with R = Y and R = -Y too, so sums that double or cancel are met under a flipped sum."""
    _check_sign_patterns(lib)


def _check_sign_patterns(lib):
    Y, R = O.pt_mul(O.BASEPOINT, 0xabcdef123457), O.generator_h()
    g = O.G_BYTES
    out = ctypes.create_string_buffer(32)
    cases = _cases(lib)
    assert len(cases) >= 25
    for pts in ((Y, R), (Y, Y), (Y, O.pt_neg(Y))):
        ye, re_ = O.ristretto_encode(pts[0]), O.ristretto_encode(pts[1])
        for name, u, v, sp in cases if pts[1] is R else cases[::2]:
            assert lib.cpzt_straus_joint(out, g, ye, re_, u.to_bytes(16, "little"), v.to_bytes(16, "little"),
                                         sp.to_bytes(32, "little")) == 0
            want = O.pt_add(O.pt_mul(O.BASEPOINT, sp), O.pt_add(O.pt_mul(pts[0], u), O.pt_mul(pts[1], v)))
            assert out.raw == O.ristretto_encode(want), (name, hex(u), hex(v), hex(sp))


def test_comb_sum_ending_negated(lib):
    """A scalar below 2^253 has a top comb digit >= 0, so its sum always leaves the comb with the
    sign +.  The loop must return the true point for any digits: the 16 digits of 2^256 - k are
    those of -k (the carry out of the top one is dropped), the last of them negative."""
    _check_comb_ending_negated(lib)


def _check_comb_ending_negated(lib):
    Y, R = O.pt_mul(O.BASEPOINT, 0xabcdef123457), O.generator_h()
    ye, re_ = O.ristretto_encode(Y), O.ristretto_encode(R)
    out = ctypes.create_string_buffer(32)
    for k in (12345, (1 << 241) + 77, (1 << 252) + 5):
        for u, v in ((0, 0), (5, (1 << 126) - 3)):
            sp = (1 << 256) - k
            assert lib.cpzt_straus_joint(out, O.G_BYTES, ye, re_, u.to_bytes(16, "little"), v.to_bytes(16, "little"),
                                         sp.to_bytes(32, "little")) == 0
            want = O.pt_add(O.pt_mul(O.BASEPOINT, O.L - k % O.L), O.pt_add(O.pt_mul(Y, u), O.pt_mul(R, v)))
            assert out.raw == O.ristretto_encode(want), (k, u, v)


def _enc(k):
    return O.ristretto_encode(O.pt_mul(O.BASEPOINT, k % O.L))


# tests/test_joint_table.py's TABLE_CASES: generic, coinciding (R' = Y'), cancelling (R' = -Y'),
# doubling (R' = 2 Y', Y' = 2 R') and 2 R' = -Y'
TABLE_CASES = [(3, 5), (O.L - 7, 0x1234567890abcdef1234567890abcdef), (2**200 + 9, 2**251 + 17),
               (11, 11), (11, O.L - 11), (1, 2), (2, 1), (6, O.L - 3)]


@pytest.mark.parametrize("alpha,beta", TABLE_CASES)
@pytest.mark.parametrize("fill", [0xa5, 0x00])
def test_lean_table_entries(lib, alpha, beta, fill):
    """build_joint_table<false>: slot 8 = (2, -2) is left as it was found, the other 12 entries
    are [a alpha + b beta] B (compared as points, through the completed form the loop starts from)."""
    out = ctypes.create_string_buffer(13 * 32)
    untouched, ok = (ctypes.c_int * 13)(), (ctypes.c_int * 13)()
    assert lib.cpzt_joint_table_lean(out, untouched, ok, _enc(alpha), _enc(beta), fill) == 13
    assert [e for e in range(13) if untouched[e]] == [8]
    for a in range(3):
        for b in range(-2, 3):
            e = 5 * a + b
            if e < 0 or e == 8:
                continue
            assert out.raw[32 * e:32 * e + 32] == _enc(a * alpha + b * beta), (a, b)
            assert ok[e] == 1, (a, b)


def test_no_window_selects_slot_8(lib):
    """Every digit pair in [-2, 1]^2 at a signed window and every pair in [0, 2]^2 at the top
    window, through the loop's own slot function on crafted digit words: never slot 8."""
    slot, neg = ctypes.c_int(), ctypes.c_int()
    seen = set()
    for m in (0, 7, 15):
        for word in (0, 3):
            if word == 3 and m == 15:
                continue  # that is the top window, below
            for a in range(-2, 2):
                for b in range(-2, 2):
                    wu, wv = U32x4(), U32x4()
                    wu[word], wv[word] = (a & 3) << (2 * m), (b & 3) << (2 * m)
                    lib.cpzt_joint_window(wu, wv, 16 * word + m, ctypes.byref(slot), ctypes.byref(neg))
                    s = -slot.value if neg.value else slot.value
                    assert s == 5 * a + b and slot.value != 8 and 0 <= slot.value <= 12
                    seen.add(slot.value)
    for a in range(3):
        for b in range(3):
            wu, wv = U32x4(), U32x4()
            wu[3], wv[3] = a << 30, b << 30
            lib.cpzt_joint_window(wu, wv, 63, ctypes.byref(slot), ctypes.byref(neg))
            assert slot.value == 5 * a + b and not neg.value and slot.value != 8
            seen.add(slot.value)
    assert seen == set(range(13)) - {8}


@pytest.mark.parametrize("off", ["CPZ_LAZY_SIGN=0", "CPZ_TABLE_LEAN=0"])
def test_switch_off_keeps_working(off, golden):
    """The code each switch replaces still compiles and gives the same points and statuses: the host
    library built with the switch at 0 (beside the default one), on the sign patterns above and on
    every golden proof."""
    import build_native
    name = "libcpz_hosttest_%s_off.so" % off.split("=")[0].lower()
    lib = ctypes.CDLL(build_native.build_hosttest(out=os.path.join(os.path.dirname(build_native.HOSTTEST), name),
                                                  defines=(off,)))
    _check_sign_patterns(lib)
    _check_comb_ending_negated(lib)
    g, h = bytes.fromhex(golden["g"]), bytes.fromhex(golden["h"])
    for p in golden["proofs"]:
        f = {k: bytes.fromhex(p[k]) for k in ("y1", "y2", "r1", "r2", "s")}
        ctx = bytes.fromhex(p["ctx"]) if p.get("ctx") is not None else None
        got = lib.cpzt_verify(g, h, f["y1"], f["y2"], f["r1"], f["r2"], f["s"], ctx or b"", len(ctx or b""),
                              0 if ctx is None else 1)
        assert got == p["status"], p["kind"]
