"""Plain-Python transcription of the 16-lane row arithmetic of csrc/fe16.h.

fe16.h is device-only (DPP, permlane): no CPU build can run it.  This module follows it
instruction by instruction -- 16 signed limbs per row element, value = sum_k limb_k 2^(16 k),
held in int64 (a batch of rows at a time) -- with the header's bound claims written as
assertions, so a bound that does not hold raises here instead of wrapping silently in a 32- or
64-bit register.
tests/test_row_model.py checks its values against big integers and the Python oracle;
tests/test_gpu_row_arith.py requires the GPU's raw limbs of mul / mul_pair to equal the
model's, which makes the model a checked CPU stand-in for the header.

Test infrastructure only.
"""
import numpy as np

P = 2**255 - 19

# A product's output ("tight") has |limb| < 90.8K (fe16.h).  Largest operand limb:
MUL_OPERAND = 363000   # mul: sums of four tight elements
PAIR_OPERAND = 181600  # mul_pair: two (38 x 181,600 < 2^23 keeps its second v_mul_i32_i24 exact)
# the documented tight ranges: limb 0 in (-2^14.7, 2^16 + 2^14.7), the others (-2^9.4, 2^16 + 2^9.4)
TIGHT0 = 26616         # ceil(2^14.7)
TIGHTK = 676           # ceil(2^9.4)

D_LIMBS = [0x78a3, 0x1359, 0x4dca, 0x75eb, 0xd8ab, 0x4141, 0x0a4d, 0x0070,
           0xe898, 0x7779, 0x4079, 0x8cc7, 0xfe73, 0x2b6f, 0x6cee, 0x5203]
SQRT_M1_LIMBS = [0xa0b0, 0x4a0e, 0x1b27, 0xc4ee, 0xe478, 0xad2f, 0x1806, 0x2f43,
                 0xd7a7, 0x3dfb, 0x0099, 0x2b4d, 0xdf0b, 0x4fc1, 0x2480, 0x2b83]
NEG_SQRT_M1_WORDS = [0xb5f15f3d, 0x3b11e4d8, 0x52d01b87, 0xd0bce7f9, 0xc2042858, 0xd4b2ff66, 0xb03e20f4, 0x547cdb7f]


def value(limbs):
    return sum(int(v) << (16 * k) for k, v in enumerate(limbs))


def canonical_limbs(v):
    """16-bit limbs of v in [0, 2^256)."""
    assert 0 <= v < 1 << 256
    return [(v >> (16 * k)) & 0xffff for k in range(16)]


def rows(x):
    """Elements as an int64 array (n, 16): the arithmetic below runs on a batch of rows at once
    (every check is on all of them), which is what keeps the decode's ~265 products affordable."""
    a = np.asarray(x, dtype=np.int64)
    a = a.reshape(1, 16) if a.ndim == 1 else a
    assert a.ndim == 2 and a.shape[1] == 16
    return a


def is_tight(x):
    x = rows(x)
    return bool(np.all((x[:, 0] > -TIGHT0) & (x[:, 0] < 65536 + TIGHT0)) and
                np.all((x[:, 1:] > -TIGHTK) & (x[:, 1:] < 65536 + TIGHTK)))


def _i32(v):
    assert np.all((v >= -(1 << 31)) & (v < 1 << 31)), "32-bit register overflow"
    return v


_K = np.arange(16)


def _shifted(y, i):
    """shifted<I>: lane k reads y through row_ror:i (lane k - i mod 16) times its wrap factor,
    one v_mul_i32_i24 -- exact only for 24-bit signed operands."""
    if i == 0:
        return y
    assert np.all((y >= -(1 << 23)) & (y < 1 << 23)), "v_mul_i32_i24 operand beyond 24 bits"
    return _i32(y[:, (_K - i) % 16] * np.where(_K < i, 38, 1))


def _columns(x, y, steps):
    """col_step<0..steps-1>: lane k accumulates bcast_i(x) * shifted<i>(y) (v_mad_i64_i32)."""
    _i32(x)
    acc = np.zeros_like(x)
    for i in range(steps):
        term = x[:, i:i + 1] * _i32(_shifted(y, i))
        assert np.all(np.abs(term) < 1 << 47)
        acc = acc + term
        assert np.all(np.abs(acc) < 1 << 62)
    return acc


def _floor16(v):
    assert np.all(np.abs(v) < 1 << 47), "column beyond alignbit's 32-bit window"
    return v >> 16


def _ror1w(c):
    """row_ror:1 times the lane's w: limb 0 receives 38 x limb 15's carry."""
    return c[:, (_K - 1) % 16] * np.where(_K == 0, 38, 1)


def carry3(acc):
    """The three rounds of the parallel carry (the tail of mul / mul_pair)."""
    c1 = _floor16(acc)
    t = _ror1w(c1) + (acc & 0xffff)
    c2 = _floor16(t)
    u = _i32((t & 0xffff) + _i32(_ror1w(c2)))
    c3 = u >> 16
    out = _i32((u & 0xffff) + _i32(_ror1w(c3)))
    assert is_tight(out), "product outside the tight range"
    return out


def mul(x, y, check_operands=True):
    """r16::mul: row by row."""
    x, y = rows(x), rows(y)
    if check_operands:
        assert np.all(np.abs(x) <= MUL_OPERAND) and np.all(np.abs(y) <= MUL_OPERAND), "mul operand"
    return carry3(_columns(x, y, 16))


def mul_pair(x, y, check_operands=True):
    """r16::mul_pair on a row pair holding the same x and y: the even row sums i = 0..7, the odd
    row i = 8..15 from x rotated by 8 and y shifted by 8, one v_permlane16_swap adds the halves."""
    x, y = rows(x), rows(y)
    if check_operands:
        assert np.all(np.abs(x) <= PAIR_OPERAND) and np.all(np.abs(y) <= PAIR_OPERAND), "mul_pair operand"
    xr = x[:, (_K - 8) % 16]
    yr = _shifted(y, 8)
    return carry3(_columns(x, y, 8) + _columns(xr, yr, 8))


def to_words(x, fixed=True):
    """r16::to_words: the canonical value of the row's element as an integer in [0, p).

    fixed=False is the header before the carry-out of the conditional subtraction was kept:
    for a folded x in [2^256 - 19, 2^256) it returned x + 19 - 2^256 instead of x - 2p."""
    x = [int(v) for v in x]
    c = -76
    h = [0] * 16
    for i in range(16):
        c += x[i]
        h[i] = c & 0xffff
        c >>= 16
    c += 2
    assert 0 <= c < 4, "to_words carry %d" % c
    for _ in range(2):
        d = c * 38
        for i in range(16):
            d += h[i]
            h[i] = d & 0xffff
            d >>= 16
        c = d
    assert c == 0, "the second fold carried out"
    x8 = [h[2 * i] | (h[2 * i + 1] << 16) for i in range(8)]
    for _ in range(2):
        cc = 19
        y = [0] * 8
        for i in range(8):
            cc += x8[i]
            y[i] = cc & 0xffffffff
            cc >>= 32
        ge = (y[7] >> 31) != 0 or cc != 0
        if fixed and cc != 0:
            y[7] |= 0x80000000   # x + 19 = 2^256 + y: x - p = y + 2^255
        else:
            y[7] &= 0x7fffffff
        if ge:
            x8 = y
    out = sum(w << (32 * i) for i, w in enumerate(x8))
    assert not fixed or out < P
    return out


def words(x, fixed=True):
    """to_words of every row: a list of integers."""
    return [to_words(r, fixed) for r in rows(x)]


def _sq(x):
    return mul_pair(x, x)


def _sqn(x, n):
    for _ in range(n):
        x = mul_pair(x, x)
    return x


def pow22523(z):
    t0 = _sq(z)
    t1 = _sqn(t0, 2)
    t1 = mul_pair(z, t1)
    t0 = mul_pair(t0, t1)
    t0 = _sq(t0)
    t0 = mul_pair(t1, t0)
    t1 = _sqn(t0, 5)
    t0 = mul_pair(t1, t0)
    t1 = _sqn(t0, 10)
    t1 = mul_pair(t1, t0)
    t2 = _sqn(t1, 20)
    t1 = mul_pair(t2, t1)
    t1 = _sqn(t1, 10)
    t0 = mul_pair(t1, t0)
    t1 = _sqn(t0, 50)
    t1 = mul_pair(t1, t0)
    t2 = _sqn(t1, 100)
    t1 = mul_pair(t2, t1)
    t1 = _sqn(t1, 50)
    t0 = mul_pair(t1, t0)
    t0 = _sqn(t0, 2)
    return mul_pair(t0, z)


def _col(flags):
    return np.asarray(flags, dtype=bool).reshape(-1, 1)


def _abs(x, fixed):
    """is_negative(x) ? -x : x, row by row."""
    return np.where(_col([w & 1 for w in words(x, fixed)]), -x, x)


NEG_SQRT_M1 = sum(w << (32 * i) for i, w in enumerate(NEG_SQRT_M1_WORDS))


def invsqrt_m1(v, fixed=True):
    """r16::invsqrt_m1 of every row: (was_square flags, limbs)."""
    v = rows(v)
    v3 = mul_pair(_sq(v), v)
    v7 = mul_pair(_sq(v3), v)
    r = mul_pair(v3, pow22523(v7))
    check = words(mul_pair(v, _sq(r)), fixed)
    correct = [c == 1 for c in check]
    flipped = [c == P - 1 for c in check]
    flipped_i = [c == NEG_SQRT_M1 for c in check]
    ri = mul_pair(r, rows(SQRT_M1_LIMBS))
    r = np.where(_col([a or b for a, b in zip(flipped, flipped_i)]), ri, r)
    return [a or b for a, b in zip(correct, flipped)], _abs(r, fixed)


def decode(encs, fixed=True):
    """r16::decode of 32-byte strings: (ok flags, X, Y, Z, T) as raw limbs, one row per string."""
    if isinstance(encs, (bytes, bytearray)):
        encs = [encs]
    sv = [int.from_bytes(e, "little") for e in encs]
    canonical = [v < P and v & 1 == 0 for v in sv]
    s = rows([canonical_limbs(v) for v in sv])
    s[:, 15] &= 0x7fff
    one = rows([1] + [0] * 15)
    ss = _sq(s)
    u1 = one - ss
    u2 = one + ss
    u2_sqr = _sq(u2)
    v = -mul_pair(rows(D_LIMBS), _sq(u1)) - u2_sqr
    was_square, inv = invsqrt_m1(mul_pair(v, u2_sqr), fixed)
    den_x = mul_pair(inv, u2)
    den_y = mul_pair(mul_pair(inv, den_x), v)
    x = _abs(mul_pair(s + s, den_x), fixed)
    y = mul_pair(u1, den_y)
    t = mul_pair(x, y)
    tw, yw = words(t, fixed), words(y, fixed)
    ok = [c and sq and not (a & 1) and b != 0 for c, sq, a, b in zip(canonical, was_square, tw, yw)]
    return ok, x, y, np.broadcast_to(one, x.shape).copy(), t
