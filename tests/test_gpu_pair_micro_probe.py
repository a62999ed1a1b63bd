"""GPU tests of the small per-pair generator tables of cpz_verify_each_pairs_many on chosen inputs
(csrc/kernels.hip: k_pair_micro through the product's launch_pair_micro, and pair_micro_window, the
generator additions of one window of k_verify_quad's small-table arm).

In a real proof the digits of s' = +-v s mod l are fixed by the transcript, so the whole-call tests
cannot steer a carry out of digit 31 into the digits of 2^128 B, a scalar whose every digit sits at
the edge of the table, or the top digit.  tests/native/microprobe.hip includes kernels.hip
unchanged and returns the tables themselves and [k] g, [k] h for chosen k.  All comparisons are
exact, against the Python oracle's points.

CPZ_MICROPROBE=<path> loads another build of the probe (over a mutated copy of csrc)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import chaum_pedersen as cp
import pyoracle as O
import test_gpu_batch_pairs_many as BM

pytestmark = pytest.mark.gpu

P, L = O.P, O.L
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_INTS, ENTRIES, TABLES = 40, 9, 4
_failed = []


@pytest.fixture(scope="module")
def probe():
    lib = ctypes.CDLL(os.environ.get("CPZ_MICROPROBE") or os.path.join(ROOT, "tests", "native", "libcpz_microprobe.so"))
    lib.microprobe_consts.restype = None
    lib.microprobe_consts.argtypes = [ctypes.POINTER(ctypes.c_int)]
    lib.microprobe_tables.restype = ctypes.c_int
    lib.microprobe_tables.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.microprobe_mul.restype = ctypes.c_int
    lib.microprobe_mul.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p]
    return lib


@pytest.fixture(autouse=True)
def _stop_after_hip_error():
    """Once an entry point has returned a HIP error nothing more is launched from this process."""
    if _failed:
        pytest.exit("stopping after " + _failed[0], returncode=3)


def _check(rc, what):
    if rc != 0:
        _failed.append("%s returned hipError %d" % (what, rc))
    assert rc == 0, _failed[-1]


@pytest.fixture(scope="module")
def pairs(gpu):
    """The default pair, two derived ones, and the first of them again (a repeated row)."""
    two = BM._many_pairs(gpu, 2, b"micro-probe")
    return [cp.Parameters(), two[0], two[1], two[0]]


def _gh(pairs):
    return np.frombuffer(b"".join(p.g + p.h for p in pairs), np.uint8).copy()


def _fe(limbs):
    """Ten signed limbs, radix 2^25.5 (limb i at bit ceil(25.5 i)), as an integer mod p."""
    return sum(int(v) << ((51 * i + 1) // 2) for i, v in enumerate(limbs)) % P


def _affine(pt):
    x, y, z, _ = pt
    zi = pow(z, P - 2, P)
    return x * zi % P, y * zi % P


def test_constants(probe):
    k = (ctypes.c_int * 4)()
    probe.microprobe_consts(k)
    assert (k[0], k[1], k[2]) == (TABLES * ENTRIES * ENTRY_INTS, ENTRIES * ENTRY_INTS, TABLES)
    assert k[0] * 4 == 5760 and k[3] % 16 == 0


def test_table_contents(probe, pairs):
    """Every entry k = 0..8 of [g | 2^128 g | h | 2^128 h] of every pair: the cached form
    (Y+X, Y-X, 2dT, Z), reassembled from its four fields and normalised by Z, is k B."""
    out = np.empty(len(pairs) * TABLES * ENTRIES * ENTRY_INTS, np.int32)
    gh = _gh(pairs)
    _check(probe.microprobe_tables(len(pairs), gh.ctypes.data, out.ctypes.data), "microprobe_tables")
    tabs = out.reshape(len(pairs), TABLES, ENTRIES, 4, 10)
    inv2 = pow(2, P - 2, P)
    for p, pr in enumerate(pairs):
        for t in range(TABLES):
            base = O.ristretto_decode(pr.g if t < 2 else pr.h)
            if t & 1:
                base = O.pt_mul(base, 1 << 128)
            for k in range(ENTRIES):
                ypx, ymx, t2d, z = (_fe(tabs[p, t, k, f]) for f in range(4))
                assert z != 0, (p, t, k)
                zi = pow(z, P - 2, P)
                x, y = (ypx - ymx) * inv2 * zi % P, (ypx + ymx) * inv2 * zi % P
                want = _affine(O.pt_mul(base, k)) if k else (0, 1)
                assert (x, y) == want, "pair %d table %d entry %d" % (p, t, k)
                assert t2d * zi % P == 2 * O.D * x * y % P, "pair %d table %d entry %d: 2dT" % (p, t, k)
    assert np.array_equal(tabs[1], tabs[3])      # the repeated row: the same tables, bit for bit


def _cases():
    ks = [0, 1, 8, 9,                    # the first carry: 8 -> (-8, 1), 9 -> (-7, 1)
          (1 << 128) - 1,                # the carry crosses from B's digits into those of 2^128 B
          1 << 128, (1 << 128) + 1, (1 << 128) - 8,
          L - 1, 1 << 252,               # the top digit
          int("8" * 63, 16), int("7" * 63, 16),     # 252 bits of 0x8 / 0x7 nibbles: digits at both table edges
          int("8" * 32, 16), int("f" * 63, 16) % L, 8 << 124]
    ks += [int.from_bytes(hashlib.sha256(b"micro-k-%d" % i).digest(), "little") % L for i in range(6)]
    return ks


def test_case_digits_reach_the_edges_they_name():
    """sc_recode_radix16's digits of the chosen k, by the same rule in Python: every value of
    -8..7 occurs, a carry leaves digit 31, and the top digit is non-zero for the 252-bit cases."""
    def digits(k):
        d, carry = [], 0
        for i in range(64):
            n = ((k >> (4 * i)) & 15) + carry
            carry = (n + 8) >> 4
            d.append(n - 16 * carry)
        assert carry == 0 and sum(v << (4 * i) for i, v in enumerate(d)) == k
        return d

    seen = set()
    for k in _cases():
        seen |= set(digits(k))
    assert seen == set(range(-8, 8))
    d = digits((1 << 128) - 1)
    assert d[:32] == [-1] + [0] * 31 and d[32] == 1
    assert digits(1 << 252)[63] == 1 and digits(L - 1)[63] == 1
    assert set(digits(int("7" * 63, 16))) == {7} | {0} and -8 in digits(int("8" * 63, 16))


def test_generator_term_on_chosen_digits(probe, pairs):
    """[k] g and [k] h by the 32-window loop with pair_micro_window alone, every case under every pair."""
    ks = _cases()
    pair_of = np.repeat(np.arange(len(pairs), dtype=np.uint32), len(ks))
    kk = ks * len(pairs)
    words = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in kk), np.uint32).copy()
    out = np.empty((len(kk), 2, 32), np.uint8)
    gh = _gh(pairs)
    _check(probe.microprobe_mul(len(pairs), gh.ctypes.data, len(kk), pair_of.ctypes.data, words.ctypes.data,
                                out.ctypes.data), "microprobe_mul")
    bases = [(O.ristretto_decode(p.g), O.ristretto_decode(p.h)) for p in pairs]
    for v, k in enumerate(kk):
        for e in range(2):
            want = O.ristretto_encode(O.pt_mul(bases[int(pair_of[v])][e], k))
            assert out[v, e].tobytes() == want, "k = %#x under pair %d, generator %d" % (k, int(pair_of[v]), e)
