"""Inputs shared by tests/test_hash_to_group_host.py and tests/test_gpu_hash_to_group.py: the edge
rows of RistrettoPoint::from_uniform_bytes, SHA-derived random rows, the message lengths at
SHA-512's padding edges, and the expected encodings from the Python oracle (computed once)."""
import functools
import hashlib

import pyoracle as O

P = O.P
TOP = 1 << 255
RFC_A3_MSG = b"Ristretto is traditionally a short shot of espresso coffee"
RFC_A3_POINT = bytes.fromhex("3066f82a1a747d45120d1740f14358531a8f04bbffe6a819f86dfe50f44a0a46")
DEFAULT_H = bytes.fromhex("c8db6f46e1b91e7e93ace69eab46976efebe07deaf5b9a2a7442fd0236401623")
# a fixed half for the rows whose other half is the edge
_T = int.from_bytes(hashlib.sha512(b"cpz-h2g-edge-half").digest()[:32], "little") & (TOP - 1)


def half(v: int) -> bytes:
    assert 0 <= v < 1 << 256
    return v.to_bytes(32, "little")


def random_rows(n: int, tag: bytes = b"cpz-h2g-row"):
    return [hashlib.sha512(tag + b"%d" % i).digest() for i in range(n)]


# (name, 64-byte row).  Pairs named "x" / "x reduced" must give one point.
EDGE_ROWS = [
    ("zero", bytes(64)),                                              # MAP(0) + MAP(0): the identity
    ("bits 255 only", half(TOP) + half(TOP)),                          # the bits are ignored: the identity again
    ("p", half(P) + half(_T)),
    ("p reduced", half(0) + half(_T)),
    ("p-1", half(P - 1) + half(_T)),
    ("p+1", half(P + 1) + half(_T)),
    ("p+1 reduced", half(1) + half(_T)),
    ("2^255-1", half(TOP - 1) + half(_T)),
    ("2^255-1 reduced", half(18) + half(_T)),
    ("p+1 alone", half(P + 1) + half(0)),
    ("1 alone", half(1) + half(0)),
    ("second half p", half(_T) + half(P)),
    ("second half 2^255-1, bit 255 set", half(_T) + half(2 * TOP - 1)),
    ("all ff", b"\xff" * 64),
    ("both halves equal", half(_T) + half(_T)),                        # a point added to itself
    ("t, t", half(5) + half(_T)),
    ("p-t, t", half(P - 5) + half(_T)),                                # t and p - t give one point
    ("first half zero", half(0) + half(_T)),                          # the identity plus a point
    ("second half zero", half(_T) + half(0)),
]
SAME_POINT = [("p", "p reduced"), ("p+1", "p+1 reduced"), ("2^255-1", "2^255-1 reduced"), ("p+1 alone", "1 alone"),
              ("t, t", "p-t, t"), ("first half zero", "second half zero"), ("zero", "bits 255 only"),
              ("second half p", "second half zero")]

# SHA-512's padding edges: 111 / 112 and 239 / 240 (at 112 and 240 the length field spills into another block)
HASH_LENGTHS = [0, 1, 55, 56, 111, 112, 113, 127, 128, 129, 239, 240, 255, 256, 257, 4096]


def message(length: int, tag: int = 0) -> bytes:
    out = b""
    k = 0
    while len(out) < length:
        out += hashlib.sha512(b"cpz-h2g-msg-%d-%d-%d" % (length, tag, k)).digest()
        k += 1
    return out[:length]


def was_square(t: int) -> bool:
    """Which arm MAP(t) takes: SQRT_RATIO_M1's first result for its u / v."""
    r = O.SQRT_M1 * t % P * t % P
    u = (r + 1) * O.ONE_MINUS_D_SQ % P
    v = (-1 - r * O.D) * (r + O.D) % P
    return O.sqrt_ratio_m1(u, v)[0]


@functools.lru_cache(maxsize=None)
def expected_point(row: bytes) -> bytes:
    return O.ristretto_encode(O.ristretto_from_uniform_bytes(row))


def expected_hash(msg: bytes) -> bytes:
    return expected_point(hashlib.sha512(msg).digest())


PAIR_DST_G = b"chaum-pedersen-zkp-v1.0.0-generator-g/"
PAIR_DST_H = b"chaum-pedersen-zkp-v1.0.0-generator-h/"


def expected_pair(label: bytes) -> bytes:
    return expected_hash(PAIR_DST_G + label) + expected_hash(PAIR_DST_H + label)
