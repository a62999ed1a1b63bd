"""CPU tests of tests/row_model.py, the plain-Python transcription of csrc/fe16.h, over the
vectors the GPU probes run (tests/row_vectors.py): values against big integers and the Python
oracle; the header's bound claims are assertions inside the model, so they are checked on the
way.  tests/test_gpu_row_arith.py ties the model to the device limb for limb."""
import random

import pyoracle as O
import row_model as M
import row_vectors as V

P = O.P


def _check_products(fn, vec):
    out = fn([x for x, _ in vec], [y for _, y in vec])
    assert M.is_tight(out)
    for (x, y), r in zip(vec, out):
        assert M.value(r) % P == M.value(x) * M.value(y) % P
    return out


def test_mul_values_and_bounds():
    out = _check_products(M.mul, V.mul_vectors(False))
    # the 2p + j representation does occur: this is what to_words must reduce twice
    assert any(M.value(r) >= 2**256 - 19 for r in out)


def test_mul_pair_values_and_bounds():
    out = _check_products(M.mul_pair, V.mul_vectors(True))
    assert any(2**256 - 19 <= M.value(r) < 2**256 for r in out)


def test_operand_bounds_are_the_limit():
    """The bounds are not slack by an order of magnitude: ten times the documented operand
    breaks a claim (the model raises), so the assertions do bite."""
    big = [10 * M.MUL_OPERAND] * 16
    try:
        M.mul(big, big, check_operands=False)
    except AssertionError:
        pass
    else:
        raise AssertionError("mul accepted operands ten times its bound")
    big = [10 * M.PAIR_OPERAND] * 16
    try:
        M.mul_pair(big, big, check_operands=False)
    except AssertionError:
        pass
    else:
        raise AssertionError("mul_pair accepted operands ten times its bound")


def test_to_words():
    before = set()
    for v, limbs in V.words_vectors():
        assert M.to_words(limbs) == v % P, v
        if M.to_words(limbs, fixed=False) != v % P:
            before.add(v)
    # the header before the fix: exactly the folded values 2^256 - 19 .. 2^256 - 1 came back wrong
    assert before == {2**256 - j for j in range(1, 20)}


def test_invsqrt_m1():
    vals = V.invsqrt_values()
    sq, r = M.invsqrt_m1([M.canonical_limbs(v) for v in vals])
    for v, was_square, limbs in zip(vals, sq, r):
        assert (was_square, M.value(limbs) % P) == O.sqrt_ratio_m1(1, v), v


def test_small_x_literals():
    """The four encodings the to_words fault was shown on: valid, and x = 2 s den_x is 28, 29,
    32, 34 before |x|; the search finds the same four."""
    found = V.small_encodings()
    for j, enc in V.SMALL_X_LITERALS.items():
        b = bytes.fromhex(enc)
        assert O.ristretto_decode(b) is not None
        assert V.decode_pre_abs(b)[0] == j
        assert found["x"][j] == b
    assert sorted(j for j in found["x"] if 19 <= j <= 37) == [28, 29, 32, 34]
    assert any(19 <= j <= 37 for j in found["y"]) and any(19 <= j <= 37 for j in found["t"])


def test_decode(golden):
    vec = V.decode_vectors(golden)
    ok, X, Y, Z, T = M.decode(vec)
    for i, enc in enumerate(vec):
        want = O.ristretto_decode(enc)
        assert ok[i] == (want is not None), enc.hex()
        if want is not None:
            assert (M.value(X[i]) % P, M.value(Y[i]) % P, M.value(T[i]) % P) == (want[0], want[1], want[3])
            assert list(Z[i]) == [1] + [0] * 15
    # before the fix three of the four small-x encodings (and two of the small-y / small-t
    # ones) were rejected: the model reproduces the fault it was written to find
    ok_before = M.decode(vec, fixed=False)[0]
    wrong = {vec[i].hex() for i in range(len(vec)) if ok_before[i] != ok[i]}
    lit = V.SMALL_X_LITERALS
    assert {lit[28], lit[32], lit[34]} <= wrong and lit[29] not in wrong


def test_decode_basepoint_multiples():
    rnd = random.Random(9)
    pts = [O.pt_mul(O.BASEPOINT, k) for k in list(range(1, 17)) + [rnd.randrange(O.L) for _ in range(16)]]
    encs = [O.ristretto_encode(p) for p in pts]
    ok, X, Y, Z, T = M.decode(encs)
    for i, enc in enumerate(encs):
        want = O.ristretto_decode(enc)
        assert ok[i] and (M.value(X[i]) % P, M.value(Y[i]) % P, M.value(T[i]) % P) == (want[0], want[1], want[3])
        assert O.pt_eq(want, pts[i])
