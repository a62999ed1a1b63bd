"""Plain-integer model of the partitioned check's indexing (csrc/part.hip) and the case lists
that tests/test_gpu_part_probe.py drives through its kernels.

The model: split8, the integer a digit row stands for, the counting sort's offsets / per-bucket
ids / top-window flag / lane assignment, index_weight_digits and the locate multipliers.  The
constants come from the probe library's getter (tests/native/partprobe.hip), which needs no GPU.
tests/test_part_model.py asserts the model's own identities and that every listed case has the
edge it claims.  Test infrastructure only."""
import ctypes
import functools
import importlib.util
import os
import random

import numpy as np

import digit_vectors as DV
import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = O.L
_CONST = ["kPartProofs", "kPartTopBuckets", "kPartLocJ0", "kPartLocLanes", "kPartListCap", "kPartOffs",
          "kPartUnits", "kPartNoLoc", "kPartTreeMaxBlocks", "kPartLaneMinBlocks", "kRlcSumBlock",
          "kPartWindows", "kPartBuckets", "kRlcWindows", "kPartSumRun"]


def probe_path():
    """The probe library: CPZ_PARTPROBE (a mutant build), or the in-tree one, built if stale."""
    path = os.environ.get("CPZ_PARTPROBE")
    if not path:
        spec = importlib.util.spec_from_file_location(
            "build_native", os.path.join(ROOT, "chaum-pedersen-zkp_amd", "build_native.py"))
        bn = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bn)
        path = bn.build_partprobe()
    return path


@functools.lru_cache(maxsize=None)
def load_probe():
    lib = ctypes.CDLL(probe_path())
    lib.partprobe_const.restype = ctypes.c_longlong
    lib.partprobe_const.argtypes = [ctypes.c_int]
    return lib


class _Consts:
    """The probe's constants, read on first use: never while pytest collects (it asks every
    module-level object for attributes of its own), so that no HIP library is loaded before the
    tests that need one run."""

    def __getattr__(self, name):
        if name not in _CONST:
            raise AttributeError(name)
        lib = load_probe()
        for i, n in enumerate(_CONST):
            self.__dict__[n] = int(lib.partprobe_const(i))
        assert lib.partprobe_const(len(_CONST)) == -1
        return self.__dict__[name]


K = _Consts()   # K.kPartProofs, ...


# ---- digits --------------------------------------------------------------------------------------

def split8(d):
    """part.hip split8: d = lo + 256 hi, lo in [-128, 128), hi in [-128, 128] for an int16 d."""
    lo = ((d + 128) & 255) - 128
    return lo, (d - lo) >> 8


def row_value(row):
    """The integer a row of radix-2^16 digits stands for."""
    return sum(int(d) << (16 * w) for w, d in enumerate(row))


def recode16(s):
    """rlc_dev.h recode16 of a scalar below 2^253 (no assertion on the value: a digit loop)."""
    d, carry = [], 0
    for w in range(16):
        chunk = ((s >> (16 * w)) & 0xffff) + carry
        carry = (chunk + 0x8000) >> 16
        d.append(chunk - (carry << 16))
    return d


def part_width(v):
    return K.kPartTopBuckets // 4 if v == K.kPartWindows - 1 else 32


def bucket_of(x):
    """(bucket index, lane share, first / last of the share) of a non-zero 8-bit digit in a
    32-wide window."""
    k = abs(x) - 1
    return k, k // 32, k % 32 in (0, 31)


# ---- the sort ------------------------------------------------------------------------------------

class Sorted:
    """What k_part_sort must leave for one block: count[v][k], offs (kPartOffs values), total,
    flat (the list with every bucket's ids in ascending order; bit 15 = negative digit),
    top_over, usz (walk unit sizes) and assign (kPartUnits values)."""

    def ids(self):
        """ids[v][k]: the sorted ids of window v's bucket k."""
        cut = np.cumsum(self.count.reshape(-1))[:-1]
        flat = [x.tolist() for x in np.split(self.flat, cut)]
        nb = self.count.shape[1]
        return [flat[v * nb:(v + 1) * nb] for v in range(self.count.shape[0])]


def canonical_list(lst, count):
    """A block's list with the ids inside every bucket put in ascending order (their order
    there comes from LDS atomics)."""
    total = int(count.sum())
    key = np.repeat(np.arange(count.size), count.reshape(-1))
    seg = np.asarray(lst[:total], dtype=np.int64)
    return seg[np.lexsort((seg, key))]


def sort_model(rows, sum_a, sum_b):
    """rows: int array [4 kPartProofs][16], zero for the proofs past the batch's end; sum_a /
    sum_b: the block's two sums (integers below 2^256, recoded as the kernel recodes them)."""
    nw, nb = K.kPartWindows, K.kPartBuckets
    D = np.concatenate([np.asarray(rows, dtype=np.int64).reshape(4 * K.kPartProofs, 16),
                        np.array([recode16(sum_a), recode16(sum_b)], dtype=np.int64)])
    lo = ((D + 128) & 255) - 128
    hi = (D - lo) >> 8
    assert np.all(lo + 256 * hi == D) and lo.min() >= -128 and lo.max() < 128 and np.abs(hi).max() <= 128
    H = np.empty((D.shape[0], nw), np.int64)
    H[:, 0::2], H[:, 1::2] = lo, hi
    s = Sorted()
    pid, v = np.nonzero(H)
    x = H[pid, v]
    k = np.abs(x) - 1
    ident = pid | np.where(x < 0, 0x8000, 0)
    s.flat = ident[np.lexsort((ident, k, v))]
    cnt = np.zeros((nw, nb), np.int64)
    np.add.at(cnt, (v, k), 1)
    s.count = cnt
    start = np.concatenate([[0], np.cumsum(cnt.reshape(-1))])
    offs = np.empty((nw, nb + 1), np.int64)
    offs[:, :nb] = start[:-1].reshape(nw, nb)
    offs[:, nb] = start[nb::nb]
    s.offs = offs.reshape(-1)
    assert s.offs.size == K.kPartOffs and start[-1] <= K.kPartListCap
    s.total = int(start[-1])
    s.top_over = bool(cnt[nw - 1, K.kPartTopBuckets:].any())
    # walk units (window v, share h): size = entries + buckets; low units (windows 0..15) ranked
    # by size descending, high units ascending, ties by unit number
    wt = part_width(nw - 1)
    usz = np.concatenate([cnt[:nw - 1].reshape(nw - 1, 4, 32).sum(axis=2).reshape(-1) + 32,
                          cnt[nw - 1, :4 * wt].reshape(4, wt).sum(axis=1) + wt]).tolist()
    s.usz = usz
    low = sorted(range(K.kPartUnits), key=lambda u: (-usz[u], u))
    high = sorted(range(K.kPartUnits, 2 * K.kPartUnits), key=lambda u: (usz[u], u))
    s.assign = [low[r] | (high[r] << 8) for r in range(K.kPartUnits)]
    return s


def check_assign(assign, usz):
    """The properties k_part_acc needs of a block's assignment: every low and every high unit
    exactly once, low sizes descending, high sizes ascending."""
    lowu = [a & 0xff for a in assign]
    highu = [a >> 8 for a in assign]
    assert sorted(lowu) == list(range(K.kPartUnits)), "low units are not a permutation"
    assert sorted(highu) == list(range(K.kPartUnits, 2 * K.kPartUnits)), "high units are not a permutation"
    ls, hs = [usz[u] for u in lowu], [usz[u] for u in highu]
    assert ls == sorted(ls, reverse=True), "low unit sizes do not descend"
    assert hs == sorted(hs), "high unit sizes do not ascend"


# ---- the locate pass -------------------------------------------------------------------------------

def loc_j(t):
    return K.kPartLocJ0 - 2 * t


def weight_words(u):
    """The eight int16 words of a weight's four 32-bit words."""
    return DV.unpack16(u)


def weight_int(u):
    """The weight as a (signed) integer: sum_k w_k 2^(16 k)."""
    return row_value(weight_words(u))


def index_weight_digits(u, j):
    """part.hip index_weight_digits: the 16 signed radix-2^16 digits of the integer j * weight."""
    d, carry = [], 0
    for w in weight_words(u):
        chunk = j * w + carry
        lo = ((chunk + 0x8000) & 0xffff) - 0x8000
        d.append(lo)
        carry = (chunk - lo) >> 16
    return d + [carry] + [0] * 7


# ---- case lists ------------------------------------------------------------------------------------

SHARE_EDGES = (1, 32, 33, 64, 65, 96, 97, 127, 128)     # |lo| or |hi|: first / last bucket of each share
SPLIT_EDGES = (127, 128, 129, 255, 256, 257)
TOP_HI = (1, 4, 5, 8, 9, 12, 13, 16)                     # first / last bucket of the top window's shares


def low_window_digits():
    """16-bit digits for windows 0..14: lo or hi on +-1 and the share edges, the split edges in
    both signs, and the four largest-magnitude patterns."""
    out = []
    for e in SHARE_EDGES:
        for sgn in (1, -1):
            if -128 <= sgn * e < 128:
                out.append(sgn * e)             # lo = +-e, hi = 0
            if e < 128:
                out.append(sgn * e * 256)       # lo = 0, hi = +-e
    out += [sgn * e for e in SPLIT_EDGES for sgn in (1, -1)]
    out += [32639, 32640, 32767, -32768]
    return list(dict.fromkeys(out))


def top_window_digits():
    """Digits for window 15 that stay inside the top window's 16 buckets."""
    out = [sgn * h * 256 for h in TOP_HI for sgn in (1, -1)]
    out += [4223, -4224, -4223, 1, -1, 127, -128, 128]
    return list(dict.fromkeys(out))


TOP_OVER_DIGITS = (4224, -4225, 17 * 256, 32767, -32768)
TOP_OVER_SUM = (1 << 253) - 1
TOP_KEPT_DIGITS = (4223, -4224)
SUM_SCALARS = (0, 1, L - 1, 1 << 252)


def slot_of(i):
    """The i-th case's point slot 4 t + q: q over 0..3, t over {0, 1, 63, 64, kPartProofs - 1}."""
    ts = (0, 1, 63, 64, K.kPartProofs - 1)
    return 4 * ts[(i // 4) % 5] + i % 4


def one_digit_cases():
    """[(window, digit)]: windows 0..14 with every low-window digit, window 15 with its own."""
    return [(w, d) for w in range(15) for d in low_window_digits()] + [(15, d) for d in top_window_digits()]


def digit_scalar(w, d):
    """A scalar below l whose recode16 has digit d in window w (and, for d < 0, 1 in window w + 1)."""
    assert w < 15
    return (d if d > 0 else d + (1 << 16)) << (16 * w)


def sum_cases():
    """[(sum_a, sum_b)]: the scalars 0, 1, l - 1, 2^252 in each sum, and the low-window digits
    through either sum, the window rotating."""
    out = [(a, b) for a in SUM_SCALARS for b in SUM_SCALARS]
    for i, d in enumerate(low_window_digits()):
        s = digit_scalar(i % 15, d)
        out.append((s, 0) if i & 1 else (0, s))
    return out


def random_rows(rng, nblk):
    """int16 digit rows [16][4 kPartProofs nblk]: every window random, window 15 in [-4224, 4223]."""
    n4 = 4 * K.kPartProofs * nblk
    d = np.array([[rng.randrange(-32768, 32768) for _ in range(n4)] for _ in range(15)] +
                 [[rng.randrange(-4224, 4224) for _ in range(n4)]], dtype=np.int16)
    return d


def full_rows(rng):
    """One block's rows [16][4 kPartProofs] and two sums with every half-digit non-zero."""
    def digit(top):
        lo = rng.choice([x for x in range(-128, 128) if x])
        hi = rng.randrange(1, 16) if top else rng.choice([x for x in range(-127, 128) if x])
        return lo + 256 * hi
    n4 = 4 * K.kPartProofs
    rows = np.array([[digit(w == 15) for _ in range(n4)] for w in range(16)], dtype=np.int16)
    sums = []
    while len(sums) < 2:
        s = row_value([digit(w == 15) for w in range(16)])
        if 0 < s < L and all(all(split8(x)) for x in recode16(s)):
            sums.append(s)
    return rows, sums


def weight_digit_cases():
    """[(u words, j)]: every weight word -32768, every word 32767, alternating, and random words,
    each with j at both ends of its range and in the middle."""
    rng = random.Random(20261019)
    words = [[0x80008000] * 4, [0x7fff7fff] * 4, [0x7fff8000] * 4, [0x80007fff] * 4, [0] * 4, [1, 0, 0, 0],
             [0xffffffff] * 4, [0x00008000, 0, 0, 0x7fff0000]]
    words += [[rng.getrandbits(32) for _ in range(4)] for _ in range(24)]
    js = (loc_j(0), loc_j(K.kPartProofs - 1), loc_j(K.kPartProofs // 2))
    return [(u, j) for u in words for j in js]
