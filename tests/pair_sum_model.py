"""Plain-integer model of the per-pair sums of a mixed-pair batch over more than CPZ_PAIRS_MAX pairs
(csrc/pair_sum.h, csrc/rlc.hip's k_pair_* kernels) and of the run cutting of its per-proof leaves.

The model: the bucketing of the entry ids by pair (counts, exclusive scans, lists), the partition
of the lists into work units of at most U entries and the pair that owns a unit, the sums mod l of
a range's products per pair with their signed radix-2^16 digits, and the cut of a range of entries
into consecutive runs of at most `max_pairs` distinct pairs.  U comes from the host build of
pair_sum.h (tests/native/hostlib_pairsum.cpp) or from the probe (tests/native/pairsumprobe.hip).
tests/test_pair_sum_model.py checks the host build against it, tests/test_gpu_pairsum_probe.py
the kernels.  Test infrastructure only."""
import ctypes
import functools

import numpy as np

import digit_vectors as DV
import pyoracle as O

L = O.L


@functools.lru_cache(maxsize=None)
def hostlib():
    import build_native
    lib = ctypes.CDLL(build_native.build_hosttest())
    ll, vp, ci, u32 = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    lib.pairsum_unit.restype = ci
    lib.pairsum_units.restype = u32
    lib.pairsum_units.argtypes = [u32]
    lib.pairsum_max_units.restype = ll
    lib.pairsum_max_units.argtypes = [ll, ll]
    lib.pairsum_find.restype = ci
    lib.pairsum_find.argtypes = [vp, ci, u32]
    lib.pairsum_runs.restype = ll
    lib.pairsum_runs.argtypes = [vp, ll, ll, ci, ci, vp, vp, vp]
    return lib


def unit():
    return int(hostlib().pairsum_unit())


def units(count, U):
    """Work units of a pair with `count` entries: none for an empty pair."""
    return -(-count // U)


def bucket(pair_idx, npairs, U):
    """(start, ustart, lists): exclusive scans of the pairs' entry and unit counts (npairs + 1
    values each) and every pair's entry ids, ascending."""
    pair_idx = np.asarray(pair_idx, np.int64)
    counts = np.bincount(pair_idx, minlength=npairs)
    start = np.concatenate([[0], np.cumsum(counts)])
    ustart = np.concatenate([[0], np.cumsum([units(int(c), U) for c in counts])])
    order = np.argsort(pair_idx, kind="stable")
    lists = [order[start[p]:start[p + 1]] for p in range(npairs)]
    return start, ustart, lists


def unit_table(start, ustart, U):
    """[(pair, j0, j1)] per unit: the slice [j0, j1) of the bucketed list it adds."""
    out = []
    for p in range(len(start) - 1):
        for k in range(int(ustart[p + 1] - ustart[p])):
            j0 = int(start[p]) + k * U
            out.append((p, j0, min(j0 + U, int(start[p + 1]))))
    return out


def find(ustart, u):
    """The pair that owns unit u: the largest p with ustart[p] <= u."""
    return int(np.searchsorted(np.asarray(ustart[:-1]), u, side="right")) - 1


def runs(pair_idx, lo, hi, max_pairs):
    """[(end, distinct, first pair)] of the consecutive runs of [lo, hi), each the longest with
    at most max_pairs distinct pairs."""
    out, a = [], lo
    while a < hi:
        seen, e = [], a
        while e < hi:
            p = int(pair_idx[e])
            if p not in seen:
                if len(seen) == max_pairs:
                    break
                seen.append(p)
            e += 1
        out.append((e, len(seen), seen[0]))
        a = e
    return out


def sums(pair_idx, prod, npairs, lo, hi):
    """[(sum a, sum b)] mod l per pair over the entries of [lo, hi); prod: [(a_i, b_i)] integers."""
    acc = [[0, 0] for _ in range(npairs)]
    for i in range(lo, hi):
        p = int(pair_idx[i])
        acc[p][0] = (acc[p][0] + prod[i][0]) % L
        acc[p][1] = (acc[p][1] + prod[i][1]) % L
    return [tuple(v) for v in acc]


def digits(x):
    """recode16 of a sum: 16 signed radix-2^16 digits."""
    return DV.recode16(x)
