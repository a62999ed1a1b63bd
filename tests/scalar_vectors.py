"""The scalar-arithmetic vectors and their exact references, shared by the host test
(tests/test_device_arith.py::test_scalars, the host build of csrc/scalar25519.h) and the device
tests (tests/test_gpu_prep_probe.py, the gfx950 build through tests/native/prepprobe.hip): one list
per family, Python integers throughout.  rlc_weight and recode16 (csrc/rlc_dev.h) are device-only
code; their vectors run on the GPU alone.  Test infrastructure only."""
import functools
import random

import pyoracle as O

L = O.L
M512 = (1 << 512) - 1
KMAX = M512 // L            # the largest k with k l < 2^512
N_RANDOM_K = 3000
N_WORD_PATTERNS = 20000
DELTAS = (-2, -1, 0, 1, 2, L - 2, L - 1)


# ---- sc_reduce_wide ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reduce_wide_cases():
    """512-bit inputs: k l + d around every multiple of l that a carry or a quotient estimate
    could get wrong, powers of two and their neighbours, the all-ones value, and word patterns."""
    rnd = random.Random(5)
    ks = [0, 1, 2, 3, 2**32 - 1, 2**32, 2**64, 2**128, 2**224, 2**255, 2**256, 2**259, KMAX, KMAX - 1]
    ks += [rnd.randrange(KMAX + 1) for _ in range(N_RANDOM_K)]
    ks += [(1 << b) + d for b in range(260) for d in (-1, 0, 1) if 0 <= (1 << b) + d <= KMAX]
    out = [k * L + d for k in ks for d in DELTAS if 0 <= k * L + d <= M512]
    out += [(1 << b) + d for b in range(512) for d in (-1, 0, 1) if 0 <= (1 << b) + d <= M512]
    out.append(M512)
    words = (0, 0xffffffff, 1, 0x80000000, 0x7fffffff)
    for _ in range(N_WORD_PATTERNS):
        ws = [rnd.choice(words + (rnd.getrandbits(32),)) for _ in range(16)]
        out.append(sum(w << (32 * i) for i, w in enumerate(ws)))
    return tuple(out)


# ---- sc_mul / sc_add / sc_neg -----------------------------------------------------------------------------

GRID_EDGES = (0, 1, 2, L - 1, L - 2, (L - 1) // 2, (L + 1) // 2, 2**252, 2**252 - 1, 2**128, 2**128 - 1, 2**127,
              2**64, 2**32 - 1)
N_GRID_RANDOM = 50


@functools.lru_cache(maxsize=None)
def grid_values():
    rnd = random.Random(6)
    return GRID_EDGES + tuple(rnd.randrange(L) for _ in range(N_GRID_RANDOM))


@functools.lru_cache(maxsize=None)
def grid_pairs():
    """Every ordered pair of grid_values(): canonical operands of sc_mul and sc_add."""
    v = grid_values()
    return tuple((a, b) for a in v for b in v)


# ---- sc_is_canonical --------------------------------------------------------------------------------------

CANONICAL_CASES = (0, 1, L - 2, L - 1, L, L + 1, 2**252, 2**253, 2**255, 2**256 - 1,
                   L + (1 << 128), L - (1 << 128), (L & ~0xffffffff), (L | 0xffffffff))


# ---- rlc_weight -------------------------------------------------------------------------------------------

HALF_EDGES = (0, 1, 0x7fff, 0x8000, 0xffff)


def weight_value(halves):
    """sum_k int16(halves[k]) 2^(16 k) mod l: pyoracle.rlc_weights' definition."""
    return sum(((h ^ 0x8000) - 0x8000) << (16 * k) for k, h in enumerate(halves)) % L


@functools.lru_cache(maxsize=None)
def weight_cases():
    """8-tuples of unsigned half-words (the ChaCha20 block's words as the kernel splits them):
    every edge half at every position over backgrounds of 0, 0xffff, 0x8000, 0x7fff and random
    halves; all halves 0x8000 (the most negative weight); all 0xffff (-1 in every window, a
    borrow through every word); only the top sign set; only the bottom sign set; random."""
    rnd = random.Random(8)
    out = []
    for bg in (0, 0xffff, 0x8000, 0x7fff, None):
        for k in range(8):
            for v in HALF_EDGES:
                h = [bg if bg is not None else rnd.getrandbits(16) for _ in range(8)]
                h[k] = v
                out.append(tuple(h))
    out.append((0x8000,) * 8)
    out.append((0xffff,) * 8)
    out.append((0,) * 7 + (0x8000,))
    out.append((0x8000,) + (0,) * 7)
    out.append((0xffff,) + (0,) * 7)      # -1: the reduced value is l - 1
    out.append((0,) + (0x8000,) * 7)
    out.append((1,) + (0x8000,) * 7)
    out += [tuple(rnd.getrandbits(16) for _ in range(8)) for _ in range(200)]
    return tuple(out)


# ---- recode16 ---------------------------------------------------------------------------------------------

def from_windows(ws):
    return sum(w << (16 * k) for k, w in enumerate(ws))


RIPPLE = from_windows([0x8000] + [0xffff] * 14 + [0x0fff])       # a carry through every window
ALL_7FFF_BELOW_L = from_windows([0x7fff] * 15 + [0x0fff])       # no carry anywhere, every digit the largest


def recode16_model(s):
    """Signed radix-2^16 digits, each in [-2^15, 2^15), carry rule (chunk + 2^15) >> 16."""
    d, carry = [], 0
    for w in range(16):
        chunk = ((s >> (16 * w)) & 0xffff) + carry
        carry = (chunk + 0x8000) >> 16
        d.append(chunk - (carry << 16))
    return d


@functools.lru_cache(maxsize=None)
def recode16_cases():
    """Inputs of recode16 (values below 2^255 whose top window takes no carry out)."""
    rnd = random.Random(9)
    out = [from_windows([0x7fff] * 16), ALL_7FFF_BELOW_L, RIPPLE, L - 1, 0, 1, 2**252,
           from_windows([0x8000] + [0] * 15),                       # digit -2^15, one carry
           from_windows([0x8000] * 15 + [0x0fff]),                  # every digit -2^15 + carry
           from_windows([0x7fff, 0x8000] * 7 + [0x7fff, 0x0fff]),   # alternating carry / no carry
           from_windows([0xffff] * 15 + [0x0fff]),
           from_windows([0] * 7 + [0x8000] + [0xffff] * 7 + [0x0fff]),  # a ripple from the word boundary up
           L - 2, (L - 1) // 2, 2**252 - 1]
    out += [rnd.randrange(L) for _ in range(200)]
    return tuple(out)


def recode16_targets():
    """The cases that are reduced scalars: what a product a c mod l can be made to equal."""
    return tuple(t for t in recode16_cases()[:15] if t < L)
