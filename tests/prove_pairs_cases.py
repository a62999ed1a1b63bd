"""Scalars at which the mixed-pair prover's table walk (scalarmul.h pair_table_mul) can go wrong,
shared by the host test, the golden fixture's generator and the GPU tests: digits 0 and +-128,
the carry chain of the signed radix-256 recoding, and a carry across a 32-bit part.

Each case is (name, the 32 little-endian bytes handed to the call).  Values of l and above are
handed in reduced, except the last, which the call itself takes mod l."""
import hashlib

L = 2**252 + 27742317777372353535851937790883648493


def _le(v: int) -> bytes:
    return v.to_bytes(32, "little")


EDGES = [
    ("0", _le(0)),
    ("1", _le(1)),
    ("127", _le(127)),
    ("128", _le(128)),                      # digit -128 and a carry
    ("129", _le(129)),
    ("l-1", _le(L - 1)),
    ("2^252", _le(1 << 252)),
    ("2^32-1", _le((1 << 32) - 1)),         # -1 and a carry into the next 32-bit part
    ("2^32", _le(1 << 32)),
    ("2^128-1", _le((1 << 128) - 1)),
    ("2^128", _le(1 << 128)),
    ("2^224", _le(1 << 224)),
    ("0x7f..7f mod l", _le(int.from_bytes(b"\x7f" * 32, "little") % L)),
    ("0x80..80 mod l", _le(int.from_bytes(b"\x80" * 32, "little") % L)),
    ("2^256-1 unreduced", b"\xff" * 32),
]

CONTEXTS = [None, hashlib.sha256(b"prove-pairs-ctx").digest(), b"ctx05", b""]


def custom_pairs_scalars(k: int, tag: bytes):
    """(a_i, b_i) of k custom pairs g_i = [a_i] B, h_i = [b_i] B, as tests/test_gpu_pairs_bulk.py
    derives them (reduced mod l)."""
    out = []
    for i in range(k):
        a = int.from_bytes(hashlib.sha512(tag + b"-g-%d" % i).digest(), "little") % L
        b = int.from_bytes(hashlib.sha512(tag + b"-h-%d" % i).digest(), "little") % L
        out.append((a, b))
    return out


def random_scalar(tag: bytes, i: int) -> int:
    return int.from_bytes(hashlib.sha512(b"prove-pairs-" + tag + b"-%d" % i).digest(), "little") % L
