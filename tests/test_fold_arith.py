"""The factor 2 of fe_sq2 folded into the square's operand multiples (csrc/fe25519.h fe_sq2_fold)
against the form it replaces, and the joint-table
build over word columns (csrc/scalarmul.h build_joint_table_cols) against build_joint_table<false>:
the host build of the device headers with the limb-bound assertions (a bound that is passed aborts
the process, so a test that returns has met none).  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import pyoracle as O

P = O.P
OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]   # bit offset of limb i (radix 2^25.5)
WID = [26, 25] * 5
I32x10 = ctypes.c_int32 * 10


@pytest.fixture(scope="module")
def lib():
    import build_native
    return ctypes.CDLL(build_native.build_hosttest())


def limbs_of(x):
    """The limbs fe_fromwords gives a value below 2^255."""
    return [(x >> OFF[i]) & ((1 << WID[i]) - 1) for i in range(10)]


def value_of(limbs):
    return sum(v << OFF[i] for i, v in enumerate(limbs)) % P


def operands(loose):
    """(name, limbs) of the operand set: 0, 1, p - 1; all limbs at +-(2^25 + 127); loose limbs
    at +-(kLooseBound - 1) on every limb and on the odd limbs only (the even ones 0, and tight
    random); 1,000 seeded random elements, half in canonical limbs, half in signed tight limbs."""
    rng = np.random.default_rng(25519)
    t = (1 << 25) + 127
    ops = [("zero", [0] * 10), ("one", [1] + [0] * 9), ("p-1", limbs_of(P - 1))]
    for sg in (1, -1):
        ops.append(("tight%+d" % sg, [sg * t] * 10))
        ops.append(("loose%+d" % sg, [sg * (loose - 1)] * 10))
        ops.append(("loose_odd%+d" % sg, [sg * (loose - 1) if i & 1 else 0 for i in range(10)]))
        ops.append(("loose_odd_tight_even%+d" % sg,
                    [sg * (loose - 1) if i & 1 else int(rng.integers(-t, t + 1)) for i in range(10)]))
    # alternating signs: the largest cancellation inside a column
    ops.append(("loose_alt", [(loose - 1) * (-1) ** i for i in range(10)]))
    for k in range(500):
        ops.append(("rand%d" % k, limbs_of(int.from_bytes(rng.bytes(32), "little") % P)))
    for k in range(500):
        ops.append(("srand%d" % k, [int(rng.integers(-t, t + 1)) for _ in range(10)]))
    return ops


def test_sq2_fold_equals_shift(lib):
    """fe_sq2 folded == fe_sq2 unfolded: the same limbs out of the carry, the same canonical bytes,
    and 2 f^2 mod p by Python's integers."""
    ops = operands(lib.cpzt_loose_bound())
    assert len(ops) >= 1000 + 12
    la, lb = I32x10(), I32x10()
    ba, bb = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    for name, f in ops:
        same = lib.cpzt_fe_sq2_forms(la, lb, ba, bb, I32x10(*f))
        assert same == 1 and list(la) == list(lb), name
        assert ba.raw == bb.raw, name
        v = value_of(f)
        assert int.from_bytes(ba.raw, "little") == 2 * v * v % P, name


def test_sq2_callers_take_the_fold(lib):
    """The library's fe_sq2 (what p2_dbl calls) gives the folded form's bytes."""
    rng = np.random.default_rng(7)
    out = ctypes.create_string_buffer(32)
    for _ in range(50):
        a = int.from_bytes(rng.bytes(32), "little") % P
        lib.cpzt_fe_sq2(out, a.to_bytes(32, "little"))
        assert int.from_bytes(out.raw, "little") == 2 * a * a % P


def _enc(k):
    return O.ristretto_encode(O.pt_mul(O.BASEPOINT, k % O.L))


# tests/test_joint_table.py's TABLE_CASES: generic, coinciding, cancelling, doubling, 2 R' = -Y'
TABLE_CASES = [(3, 5), (O.L - 7, 0x1234567890abcdef1234567890abcdef), (2**200 + 9, 2**251 + 17),
               (11, 11), (11, O.L - 11), (1, 2), (2, 1), (6, O.L - 3)]


@pytest.mark.parametrize("alpha,beta", TABLE_CASES)
def test_column_build_writes_the_same_table(lib, alpha, beta):
    """build_joint_table_cols after put_point(Y'), put_point(R') == build_joint_table<false>, byte
    for byte over all 13 slots (slot 8 untouched in both), for the points as decoded and negated,
    at the stride of a host array and at the kernels' (one word per thread of a block)."""
    y, r = _enc(alpha), _enc(beta)
    for negate in (0, 1):
        for stride in (1, 256):
            for fill in (0x00, 0xa5):
                assert lib.cpzt_joint_table_cols_diff(y, r, negate, stride, fill) == 0, (negate, stride, fill)


@pytest.mark.parametrize("off", ["CPZ_SQ2_FOLD=0"])
def test_switch_off_keeps_working(off, golden):
    """The form each switch replaces still compiles and gives the same statuses on every golden
    proof: the host library built with the switch at 0, beside the default one."""
    import build_native
    name = "libcpz_hosttest_%s_off.so" % off.split("=")[0].lower()
    lib = ctypes.CDLL(build_native.build_hosttest(out=os.path.join(os.path.dirname(build_native.HOSTTEST), name),
                                                  defines=(off,)))
    g, h = bytes.fromhex(golden["g"]), bytes.fromhex(golden["h"])
    for p in golden["proofs"]:
        f = {k: bytes.fromhex(p[k]) for k in ("y1", "y2", "r1", "r2", "s")}
        ctx = bytes.fromhex(p["ctx"]) if p.get("ctx") is not None else None
        got = lib.cpzt_verify(g, h, f["y1"], f["y2"], f["r1"], f["r2"], f["s"], ctx or b"", len(ctx or b""),
                              0 if ctx is None else 1)
        assert got == p["status"], p["kind"]
