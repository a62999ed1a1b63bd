"""The challenge-split case list and its exact reference, shared by the host test
(tests/test_device_arith.py::test_half_split) and the device tests
(tests/test_gpu_row_arith.py).  Test infrastructure only."""
import random

import pyoracle as O

L = O.L

N_EDGE = 15       # the hand-picked challenges at the head of the list
N_RANDOM = 20000  # then the uniform ones; the near-rational ones follow


def euclid_half(c):
    """Exact partial extended Euclid on (l, c): first remainder below 3 * 2^125."""
    T = 3 << 125
    r0, r1, t0, t1 = L, c, 0, 1
    while r1 >= T:
        q = r0 // r1
        r0, r1 = r1, r0 - q * r1
        t0, t1 = t1, t0 - q * t1
    return r1, t1


def half_split_cases():
    rng = random.Random(7)
    cases = [0, 1, 2, (3 << 125) - 1, 3 << 125, L - 1, L - 2, L // 2, L // 3, (L >> 70), (L >> 140) + 5,
             (L >> 126), (L >> 127) + 1, 2**252, (2**128 + 1) % L]
    assert len(cases) == N_EDGE
    cases += [rng.randrange(L) for _ in range(N_RANDOM)]
    # Values near rationals p/q of l: a few tiny-then-huge partial quotients, which stress
    # the Lehmer batch's exactness conditions and the huge-quotient single steps.
    for q in (2, 3, 5, 7, 1000, 65537, 2**31 - 1, 2**40 + 3, 2**64 + 13, 2**100 + 7):
        for p in (1, q // 2 + 1, q - 1):
            base = L * p // q
            cases += [(base + d) % L for d in (-2, -1, 0, 1, 2, 1 << 20, rng.randrange(1 << 60))]
    return cases


def edge_cases():
    return half_split_cases()[:N_EDGE]


def near_rational_cases():
    return half_split_cases()[N_EDGE + N_RANDOM:]
