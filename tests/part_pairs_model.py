"""Plain-integer model of the partitioned check's pair mode (csrc/part.hip, k_part_sort_pairs and
k_part_index_digits_pairs) for tests/test_gpu_part_pairs_probe.py and
tests/test_batch_pairs_part_api.py.

The model: a block's per-pair sums of the prepare's products, the counting sort with 2 npairs
extras (offsets, per-bucket ids, top-window flag, lane assignment: part_model.sort_model with the
pairs' points in place of g and h), and the pair-mode capacity arithmetic read from csrc/rlc.h and
include/cpz.h.  Nothing here needs a GPU or loads a library, except load_probe().  Test
infrastructure only."""
import ctypes
import functools
import importlib.util
import os
import re

import numpy as np

import pyoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = O.L
WINDOWS = 32            # kPartWindows: signed radix-2^8 windows
BUCKETS = 128           # kPartBuckets
TOP_BUCKETS = 16        # kPartTopBuckets


def probe_path():
    """The pair probe library: CPZ_PARTPAIRSPROBE (a mutant build), or the in-tree one, built if stale."""
    path = os.environ.get("CPZ_PARTPAIRSPROBE")
    if not path:
        spec = importlib.util.spec_from_file_location(
            "build_native", os.path.join(ROOT, "chaum-pedersen-zkp_amd", "build_native.py"))
        bn = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bn)
        path = bn.build_partpairsprobe()
    return path


@functools.lru_cache(maxsize=None)
def load_probe():
    lib = ctypes.CDLL(probe_path())
    lib.partpairsprobe_const.restype = ctypes.c_longlong
    lib.partpairsprobe_const.argtypes = [ctypes.c_int]
    return lib


# ---- constants as the sources state them -----------------------------------------------------------

def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def header_define(name):
    """The integer value of `#define name value` in include/cpz.h, or None."""
    m = re.search(r"^#define\s+%s\s+\(?\s*(0x[0-9a-fA-F]+|\d+)u?\b" % re.escape(name), _read("include", "cpz.h"), re.M)
    return int(m.group(1), 0) if m else None


def rlc_constant(name):
    """The integer value of `constexpr int name = <integer>;` in csrc/rlc.h, or None."""
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % re.escape(name),
                  _read("chaum-pedersen-zkp_amd", "csrc", "rlc.h"))
    return int(m.group(1)) if m else None


def list_cap_pairs(proofs, max_pairs):
    """kPartListCapPairs for blocks of `proofs` proofs: every half-digit of every point and extra."""
    return WINDOWS * (4 * proofs + 2 * max_pairs)


def max_id(proofs, max_pairs):
    """The largest point id of a pair-mode block."""
    return 4 * proofs + 2 * max_pairs - 1


# ---- the per-pair sums -----------------------------------------------------------------------------

def pair_sums(prod, pair_idx, n, npairs, proofs, block, mult=None):
    """Block `block`'s extras' scalars [2 npairs]: entry 2 p + k is the sum mod l of prod[i][k]
    (times mult[t], t the proof's index in the block, when given) over the block's proofs i < n
    with pair_idx[i] == p.  Rows at or beyond n are not read."""
    out = [0] * (2 * npairs)
    for t in range(proofs):
        i = block * proofs + t
        if i >= n:
            break
        m = 1 if mult is None else mult[t]
        p = int(pair_idx[i])
        out[2 * p] = (out[2 * p] + m * prod[i][0]) % L
        out[2 * p + 1] = (out[2 * p + 1] + m * prod[i][1]) % L
    return out


def pair_sums_brute(prod, pair_idx, n, npairs, proofs, block):
    """The same by the definition: one pass over the whole batch per (pair, component)."""
    return [sum(prod[i][k] for i in range(n) if i // proofs == block and pair_idx[i] == p) % L
            for p in range(npairs) for k in range(2)]


# ---- the sort --------------------------------------------------------------------------------------

def split8(d):
    lo = ((d + 128) & 255) - 128
    return lo, (d - lo) >> 8


def recode16(s):
    d, carry = [], 0
    for w in range(16):
        chunk = ((s >> (16 * w)) & 0xffff) + carry
        carry = (chunk + 0x8000) >> 16
        d.append(chunk - (carry << 16))
    return d


def row_value(row):
    return sum(int(d) << (16 * w) for w, d in enumerate(row))


class Sorted:
    pass


def canonical_list(lst, count):
    """A block's list with the ids inside every bucket in ascending order (LDS atomics order them)."""
    total = int(count.sum())
    key = np.repeat(np.arange(count.size), count.reshape(-1))
    seg = np.asarray(lst[:total], dtype=np.int64)
    return seg[np.lexsort((seg, key))]


def sort_model(rows, extras, proofs, cap):
    """rows: int array [4 proofs][16], zero for the proofs past the batch's end; extras: the
    2 npairs scalars of the block (integers below l, recoded as the kernel recodes them).  What
    k_part_sort_pairs must leave: count, offs, total, flat (ids ascending per bucket, bit 15 = a
    negative digit), top_over, usz and assign."""
    nw, nb = WINDOWS, BUCKETS
    D = np.concatenate([np.asarray(rows, dtype=np.int64).reshape(4 * proofs, 16),
                        np.array([recode16(e) for e in extras], dtype=np.int64).reshape(len(extras), 16)])
    lo = ((D + 128) & 255) - 128
    hi = (D - lo) >> 8
    assert np.all(lo + 256 * hi == D) and np.abs(hi).max() <= 128
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
    assert start[-1] <= cap
    s.total = int(start[-1])
    s.top_over = bool(cnt[nw - 1, TOP_BUCKETS:].any())
    wt = TOP_BUCKETS // 4
    usz = np.concatenate([cnt[:nw - 1].reshape(nw - 1, 4, 32).sum(axis=2).reshape(-1) + 32,
                          cnt[nw - 1, :4 * wt].reshape(4, wt).sum(axis=1) + wt]).tolist()
    s.usz = usz
    units = nw * 4 // 2
    low = sorted(range(units), key=lambda u: (-usz[u], u))
    high = sorted(range(units, 2 * units), key=lambda u: (usz[u], u))
    s.assign = [low[r] | (high[r] << 8) for r in range(units)]
    return s
