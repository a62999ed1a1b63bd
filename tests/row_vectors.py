"""Test vectors of the 16-lane row arithmetic (csrc/fe16.h), shared by the CPU test of the
Python model (tests/test_row_model.py) and the GPU probes (tests/test_gpu_row_arith.py).
Everything is deterministic.  Test infrastructure only."""
import random

import pyoracle as O
import row_model as M

P = O.P
EDGE = [0, 1, 2, 19, P - 1, P - 2, 2**255 - 20, 2**254, 2**26, 2**25 - 1, (2**255 - 19) // 2]

# Valid ristretto255 encodings whose decode computes x = 2 s den_x = 28, 29, 32, 34 before it
# takes |x|: field values 19..37, which a product may hold as 2p + j (found by small_encodings)
SMALL_X_LITERALS = {
    28: "f4629fac3b5109e039b671c408bee62fd8f7d8da737db7fea8c5a4ce53c6b70e",
    29: "921ee0c196e53035266228671be5964d9e23f7c879257eb452265b4932110411",
    32: "047342f812e89c33c11fbffe91ada93f89023f49b4b6941e1fa0014bf6d2554a",
    34: "90c5f72c8bf9bef90384ce7971fdb4f03a0a6f51985df38be303a4d0d8b87744",
}


def _patterns(bound):
    pats = [[bound] * 16, [-bound] * 16, [bound if k % 2 == 0 else -bound for k in range(16)],
            [-bound if k % 2 == 0 else bound for k in range(16)]]
    for k in range(16):
        for sgn in (1, -1):
            v = [0] * 16
            v[k] = sgn * bound
            pats.append(v)
    return pats


def _random_limbs(rnd, bound):
    def one():
        t = rnd.randrange(8)
        return bound if t == 0 else (-bound if t == 1 else (0 if t == 2 else rnd.randint(-bound, bound)))
    return [one() for _ in range(16)]


def mul_vectors(pair):
    """(x, y) raw-limb operand pairs for r16::mul (pair=False: limbs up to four tight elements)
    or r16::mul_pair (pair=True: up to two tight elements): 12,000 + 8,000 pairs."""
    bound = M.PAIR_OPERAND if pair else M.MUL_OPERAND
    total = 8000 if pair else 12000
    rnd = random.Random(1601 if pair else 1600)
    pats = _patterns(bound)
    vec = []
    # the sign patterns against every pattern, both ways round
    for a in pats[:4]:
        for b in pats:
            vec.append((a, b))
            vec.append((b, a))
    # single limbs against single limbs: every wrap position
    for a in pats[4::2]:
        for b in pats[4:]:
            vec.append((a, b))
    # canonical limbs of the field edge values
    for a in EDGE:
        for b in EDGE:
            vec.append((M.canonical_limbs(a), M.canonical_limbs(b)))
    # products equal to j and p - j, j = 0..40, from canonical operands: y = j / x
    for j in list(range(41)) + [P - j for j in range(1, 41)]:
        for _ in range(24):
            x = rnd.randrange(1, P)
            y = j * pow(x, P - 2, P) % P
            vec.append((M.canonical_limbs(x), M.canonical_limbs(y)))
    while len(vec) < total:
        vec.append((_random_limbs(rnd, bound), _random_limbs(rnd, bound)))
    return vec


def relimb(rnd, limbs):
    """The same value with d 2^16 moved between adjacent limbs, d in -5..5."""
    out = list(limbs)
    for k in range(15):
        d = rnd.randint(-5, 5)
        out[k] += d << 16
        out[k + 1] -= d
    return out


def wide_limbs(v):
    """Limbs 0..14 in [0, 2^16), limb 15 the (signed) rest: any integer."""
    out = [(v >> (16 * k)) & 0xffff for k in range(15)]
    out.append(v >> 240)
    return out


def words_vectors():
    """(V, limbs) for r16::to_words / is_zero / is_negative: each V in canonical limbs and in a
    signed re-limbing."""
    rnd = random.Random(1602)
    vals = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1]
    vals += [2**256 - j for j in range(1, 130)]
    vals += [-j for j in range(1, 130)]
    vals += [-P, -2 * P, 1 - 2**256, 2**256 + 600 * 2**240]
    vals += [rnd.randrange(-2**256 + 1, 2**256 + 2**250) for _ in range(2000)]
    vec = []
    for v in vals:
        limbs = wide_limbs(v)
        assert M.value(limbs) == v
        vec.append((v, limbs))
        re = relimb(rnd, limbs)
        assert M.value(re) == v
        vec.append((v, re))
    return vec


def invsqrt_values():
    rnd = random.Random(3)
    return [0, 1, P - 1, 2, 5] + [rnd.randrange(1, P) for _ in range(60)]


def _sqrt(a):
    """A square root of a mod p, or None."""
    ok, r = O.sqrt_ratio_m1(a, 1)
    return r if ok and r * r % P == a % P else None


def decode_pre_abs(enc):
    """What RFC 9496 DECODE computes for a canonical encoding: (x before |x|, y, t), oracle values."""
    s = int.from_bytes(enc, "little")
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    u2_sqr = u2 * u2 % P
    v = (-(O.D * u1 % P * u1) - u2_sqr) % P
    _, inv = O.sqrt_ratio_m1(1, v * u2_sqr)
    den_x = inv * u2 % P
    den_y = inv * den_x % P * v % P
    x = 2 * s * den_x % P
    y = u1 * den_y % P
    return x, y, O.fe_abs(x) * y % P


def small_encodings(limit=41):
    """Valid encodings whose decode meets a small field value: x = 2 s den_x (before |x|), y or
    t equal to j < limit.  Found by solving the curve equation -x^2 + y^2 = 1 + d x^2 y^2 for the
    coordinate, keeping the points whose encoding decodes (oracle) back to that value.
    Returns {"x": {j: enc}, "y": {j: enc}, "t": {j: enc}}."""
    found = {"x": {}, "y": {}, "t": {}}

    def consider(x, y):
        if x is None or y is None:
            return
        for xx in (x, P - x):
            for yy in (y, P - y):
                enc = O.ristretto_encode((xx, yy, 1, xx * yy % P))
                if O.ristretto_decode(enc) is None:
                    continue
                px, py, pt = decode_pre_abs(enc)
                for name, val in (("x", px), ("y", py), ("t", pt)):
                    if val < limit:
                        found[name].setdefault(val, enc)

    inv = lambda a: pow(a, P - 2, P)
    for j in range(limit):
        # x = +-j: y^2 = (1 + x^2) / (1 - d x^2)
        consider(j, _sqrt((1 + j * j) * inv(1 - O.D * j * j) % P))
        # y = +-j: x^2 = (y^2 - 1) / (1 + d y^2)
        consider(_sqrt((j * j - 1) * inv(1 + O.D * j * j) % P), j)
        # x y = +-j: x^4 + (1 + d j^2) x^2 - j^2 = 0
        b = (1 + O.D * j * j) % P
        disc = _sqrt((b * b + 4 * j * j) % P)
        if disc is not None and j:
            for r in (disc, P - disc):
                x = _sqrt((r - b) * inv(2) % P)
                if x:
                    consider(x, j * inv(x) % P)
    return found


def decode_vectors(golden):
    """32-byte strings for r16::decode."""
    rnd = random.Random(3)
    vec = [bytes.fromhex(e) for e in golden["rfc9496_multiples"]]
    vec += [bytes.fromhex(e) for e in golden["rfc9496_bad"]]
    vec += [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(400)]
    for s in (0, P - 1, P, P + 1, 2**255 - 1):
        vec.append(s.to_bytes(32, "little"))
        vec.append((s | 1 << 255).to_bytes(32, "little"))  # bit 255 set: non-canonical
    vec += [bytes.fromhex(e) for e in SMALL_X_LITERALS.values()]
    for group in small_encodings().values():
        vec += list(group.values())
    return vec
