"""Scalars at which the many-pair prover's radix-16 walk (kernels.hip k_prove_points_micro) can go
wrong, shared by the host test and the GPU tests: digit -8 and its carry, a carry through every
digit, the carry from digit 31 (the last on B) into digit 32 (the first on 2^128 B), the top digit.

Each case is (name, the 32 little-endian bytes handed to the call).  Values of l and above are
handed in reduced, except the last, which the call itself takes mod l."""
import hashlib

L = 2**252 + 27742317777372353535851937790883648493


def _le(v: int) -> bytes:
    return v.to_bytes(32, "little")


EDGES = [
    ("0", _le(0)),
    ("1", _le(1)),
    ("7", _le(7)),
    ("8", _le(8)),                          # digit -8 and a carry
    ("9", _le(9)),
    ("0x77..77 mod l", _le(int.from_bytes(b"\x77" * 32, "little") % L)),
    ("0x88..88 mod l", _le(int.from_bytes(b"\x88" * 32, "little") % L)),   # 0x88..88: a carry through every digit
    ("2^128-1", _le((1 << 128) - 1)),       # a carry from digit 31 into digit 32
    ("2^128", _le(1 << 128)),
    ("2^128+8", _le((1 << 128) + 8)),
    ("2^124", _le(1 << 124)),
    ("2^252", _le(1 << 252)),
    ("l-1", _le(L - 1)),
    ("2^256-1 unreduced", b"\xff" * 32),
]


def recode_radix16(v: int):
    """scalar25519.h sc_recode_radix16 of v < 2^255: 64 digits in [-8, 7], lowest first, and the
    carry out of the last one."""
    out, carry = [], 0
    for i in range(64):
        n = ((v >> (4 * i)) & 15) + carry
        carry = (n + 8) >> 4
        out.append(n - (carry << 4))
    return out, carry


def random_scalar(tag: bytes, i: int) -> int:
    return int.from_bytes(hashlib.sha512(b"prove-many-" + tag + b"-%d" % i).digest(), "little") % L
