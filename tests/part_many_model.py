"""Plain-integer model of the partitioned check's many mode (csrc/part.hip, k_part_sort_many and
k_part_index_digits_many) for tests/test_part_many_model.py and tests/test_gpu_part_many_probe.py.

Above CPZ_PAIRS_MAX pairs a block's extras are keyed by block-local slot: a pair's slot is its rank
by first occurrence among the block's proofs, so a block of kPartProofs proofs has at most
kPartProofs slots whatever the batch's pair count.  Extra id 4 kPartProofs + 2 slot + k is the point
gh[2 pair(slot) + k] with the sum mod l of prod[i][k] over the block's proofs in that slot.  The
sort itself is part_pairs_model.sort_model with these 2 kPartProofs extras.  Nothing here needs a
GPU or loads a library, except load_probe().  Test infrastructure only."""
import ctypes
import functools
import importlib.util
import os
import re

import part_pairs_model as PM
import pyoracle as O

ROOT = PM.ROOT
L = O.L
WINDOWS = PM.WINDOWS
NO_PAIR = 0xffff        # kPartNoPair: an unused slot of a block's table


def probe_path():
    """The many-mode probe library: CPZ_PARTMANYPROBE (a mutant build), or the in-tree one, built if stale."""
    path = os.environ.get("CPZ_PARTMANYPROBE")
    if not path:
        spec = importlib.util.spec_from_file_location(
            "build_native", os.path.join(ROOT, "chaum-pedersen-zkp_amd", "build_native.py"))
        bn = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bn)
        path = bn.build_partmanyprobe()
    return path


@functools.lru_cache(maxsize=None)
def load_probe():
    lib = ctypes.CDLL(probe_path())
    lib.partmanyprobe_const.restype = ctypes.c_longlong
    lib.partmanyprobe_const.argtypes = [ctypes.c_int]
    return lib


# ---- constants as the sources state them -----------------------------------------------------------

def rlc_source():
    return PM._read("chaum-pedersen-zkp_amd", "csrc", "rlc.h")


def list_cap_many_expr():
    """The right-hand side of kPartListCapMany in csrc/rlc.h, spaces removed, or None."""
    m = re.search(r"constexpr\s+int\s+kPartListCapMany\s*=\s*([^;]+);", rlc_source())
    return re.sub(r"\s+", "", m.group(1)) if m else None


def list_cap_many(proofs):
    """kPartListCapMany for blocks of `proofs` proofs: every half-digit of every point and extra."""
    return WINDOWS * (4 * proofs + 2 * proofs)


def max_id(proofs):
    """The largest point id of a many-mode block."""
    return 4 * proofs + 2 * proofs - 1


# ---- the slots -------------------------------------------------------------------------------------

def slot_table(pair_idx, n, proofs, block):
    """Block `block`'s slot -> pair table [proofs]: the block's pairs in order of first occurrence
    among its proofs i < n, then NO_PAIR.  Rows at or beyond n hold no pair and are not read."""
    seen = []
    for t in range(proofs):
        i = block * proofs + t
        if i >= n:
            break
        p = int(pair_idx[i])
        if p not in seen:
            seen.append(p)
    return seen + [NO_PAIR] * (proofs - len(seen))


def slot_sums(prod, pair_idx, n, proofs, block, table=None, mult=None):
    """Block `block`'s extras' scalars [2 proofs] by slot: entry 2 s + k is the sum mod l of
    prod[i][k] (times mult[t], t the proof's index in the block, when given) over the block's
    proofs i < n whose pair is table[s]; zero for an unused slot.  `table` defaults to the block's
    own (the locate pass passes the prepared block's)."""
    table = slot_table(pair_idx, n, proofs, block) if table is None else table
    where = {p: s for s, p in enumerate(table) if p != NO_PAIR}
    out = [0] * (2 * proofs)
    for t in range(proofs):
        i = block * proofs + t
        if i >= n:
            break
        m = 1 if mult is None else mult[t]
        s = where[int(pair_idx[i])]
        out[2 * s] = (out[2 * s] + m * prod[i][0]) % L
        out[2 * s + 1] = (out[2 * s + 1] + m * prod[i][1]) % L
    return out


def block_scalar(row_values, point_mult, sums, table, gh_mult):
    """The scalar K with P_b = [K] B of a many-mode block whose points are known multiples of the
    basepoint: row_values[j] the integer scalar of point j (4 proofs of them), point_mult[j] its
    multiple, sums / table the block's slot sums and slot -> pair table, gh_mult(p) = (m_g, m_h)."""
    tot = sum(v * m for v, m in zip(row_values, point_mult))
    for s, p in enumerate(table):
        if p != NO_PAIR:
            m_g, m_h = gh_mult(p)
            tot += sums[2 * s] * m_g + sums[2 * s + 1] * m_h
    return tot % L


def per_proof_count(n, proofs, located, whole_blocks):
    """Entries the partitioned search verifies per proof: the located ones alone, and every entry of
    the blocks not located (the last may be partial)."""
    return len(located) + sum(min(proofs, n - b * proofs) for b in whole_blocks)
