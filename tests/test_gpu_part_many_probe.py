"""GPU tests of the partitioned check's many-mode kernels (csrc/part.hip: block-local pair slots,
more than 64 pairs in the batch) on chosen digits, products and pair indices.

tests/native/partmanyprobe.hip includes part.hip unchanged and drives k_part_sort_many,
k_part_acc_many, the combine, k_part_sum1/2, k_part_index_digits_many and k_part_locate.  Every
point -- the blocks' and the pairs' g_p, h_p -- is a known multiple of the basepoint, so a block's
expected partial is [(sum_j K_j m_j + sum_slots (S_a m_g + S_b m_h of the slot's pair)) mod l] B:
Python integers (tests/part_many_model.py) and one pt_mul of the Python oracle.  Partials are
compared as 32-byte encodings, fail flags, offsets, assignments and slot tables exactly, lists per
bucket as multisets.  The helpers of tests/test_gpu_part_pairs_probe.py are used here.

CPZ_PARTMANYPROBE=<path> loads another build of the probe (over a mutated copy of csrc)."""
import ctypes
import functools
import random
import struct

import numpy as np
import pytest

import part_many_model as MM
import part_model as M
import part_pairs_model as PM
import pyoracle as O
import test_gpu_part_pairs_probe as T

pytestmark = pytest.mark.gpu

K, L = M.K, O.L
NPAIRS = 4096
_ptr, _ll, _enc_mul, _words, _scalar_words = T._ptr, T._ll, T._enc_mul, T._words, T._scalar_words


@pytest.fixture(scope="module")
def probe():
    lib = MM.load_probe()
    assert lib.partmanyprobe_const(2) == K.kPartProofs and lib.partmanyprobe_const(3) == K.kPartWindows
    assert lib.partmanyprobe_const(1) == NPAIRS and lib.partmanyprobe_const(4) == MM.NO_PAIR
    assert lib.partmanyprobe_const(5) == -1
    return lib


@functools.lru_cache(maxsize=None)
def _cap():
    cap = int(MM.load_probe().partmanyprobe_const(0))
    assert cap == MM.list_cap_many(K.kPartProofs)
    return cap


def _gh_mult(p):
    """(m_g, m_h) of pair p: [m] B are its points, from the pool of small multiples."""
    return 1 + (2 * p) % 509, 1 + (7 * p + 3) % 503


@functools.lru_cache(maxsize=None)
def _gh_words():
    return _words([_enc_mul(m) for p in range(NPAIRS) for m in _gh_mult(p)])


class Batch:
    """nblk blocks over nprep prepared blocks: mult[point] (the point is [mult] B), digits
    int16[16][dstride], n proofs, and either per-proof products with pair indices (rows may exceed
    n) or, with presummed set, the per-block sums by slot and the prepared blocks' tables."""

    def __init__(self, nblk, n=None, nprep=None, pmap=None, rows=None):
        self.nblk, self.nprep, self.pmap = nblk, nprep or nblk, pmap
        self.n = K.kPartProofs * nblk if n is None else n
        self.pb = 4 * K.kPartProofs
        self.mult = [0] * (self.pb * self.nprep)
        self.dstride = self.pb * nblk + 4
        self.digits = np.zeros((16, self.dstride), np.int16)
        r = self.n if rows is None else rows
        self.prod = [(0, 0)] * r
        self.idx = [0] * r
        self.presummed = None          # [nblk][2 kPartProofs] when the sums are given directly ...
        self.tables = None             # ... with the prepared blocks' tables [nprep][kPartProofs]

    def rows(self, b):
        r = self.digits[:, self.pb * b:self.pb * (b + 1)].T.astype(np.int64)
        live = max(0, min(K.kPartProofs, self.n - K.kPartProofs * b))
        r[4 * live:] = 0
        return r

    def table(self, b):
        if self.presummed is not None:
            return self.tables[self.pmap[b]]
        return MM.slot_table(self.idx, self.n, K.kPartProofs, b)

    def extras(self, b):
        if self.presummed is not None:
            return list(self.presummed[b])
        return MM.slot_sums(self.prod, self.idx, self.n, K.kPartProofs, b)


def _block_scalar(bt, b):
    r = bt.rows(b)
    pts = bt.pb * (bt.pmap[b] if bt.pmap else b)
    live = np.nonzero(r.any(axis=1))[0].tolist()
    return MM.block_scalar([M.row_value(r[j].tolist()) for j in live], [bt.mult[pts + j] for j in live],
                           bt.extras(b), bt.table(b), _gh_mult)


def run_blocks(probe, bt, per_launch=4):
    cap = _cap()
    o = T.Out()
    o.part = np.full((bt.nblk, 8), 0xffffffff, np.uint32)
    o.fail = np.full(bt.nblk, 0xff, np.uint8)
    o.lists = np.full((bt.nblk, cap), 0xffff, np.uint16)
    o.offs = np.full((bt.nblk, K.kPartOffs), 0xffff, np.uint16)
    o.assign = np.full((bt.nblk, K.kPartUnits), 0xffff, np.uint16)
    o.partial = np.full(8, 0xffffffff, np.uint32)
    o.identity = np.full(1, -1, np.int32)
    o.slots = np.full((bt.nblk, K.kPartProofs), 0x5555, np.uint16)
    pmap = np.array(bt.pmap, np.uint32) if bt.pmap else None
    if bt.presummed is not None:
        prod = _scalar_words([v for blk in bt.presummed for v in blk])
        idx, prod_rows = None, bt.nblk * K.kPartProofs
        slots_in, slots_out = np.array(bt.tables, np.uint16).reshape(bt.nprep, K.kPartProofs), None
    else:
        prod = _scalar_words([v for pr in bt.prod for v in pr])
        idx, prod_rows = np.array(bt.idx, np.uint32), len(bt.prod)
        slots_in, slots_out = None, o.slots
    rc = probe.partmanyprobe_blocks(
        _ll(bt.nblk), _ll(bt.n), _ll(bt.nprep), _ptr(_words([_enc_mul(m) for m in bt.mult])), _ptr(bt.digits),
        _ll(bt.dstride), _ptr(prod), _ptr(idx), _ll(prod_rows), _ptr(_gh_words()), ctypes.c_int(NPAIRS), _ptr(pmap),
        _ptr(slots_in), _ll(per_launch), _ptr(o.part), _ptr(o.fail), _ptr(o.lists), _ptr(o.offs), _ptr(o.assign),
        _ptr(o.partial), _ptr(o.identity), _ptr(slots_out))
    assert rc == 0, "partmanyprobe_blocks: hipError %d" % rc
    o.enc = [o.part[b].tobytes() for b in range(bt.nblk)]
    return o


def check(bt, o):
    """every block's partial, flags, offsets, lists, assignment and slot table, and the summed partial"""
    cap = _cap()
    ks = [_block_scalar(bt, b) for b in range(bt.nblk)]
    for b in range(bt.nblk):
        if bt.presummed is None:
            assert o.slots[b].tolist() == bt.table(b), "slot table of block %d" % b
        assert o.enc[b] == _enc_mul(ks[b]), "partial of block %d" % b
        s = PM.sort_model(bt.rows(b), bt.extras(b), K.kPartProofs, cap)
        assert int(o.fail[b]) == int(ks[b] != 0) | (2 if s.top_over else 0), "fail flag of block %d: %d" % (b, o.fail[b])
        assert np.array_equal(o.offs[b].astype(np.int64), s.offs), "offs of block %d" % b
        assert np.all(o.lists[b, s.total:] == 0xffff), "block %d: list entries written past its end" % b
        assert np.array_equal(PM.canonical_list(o.lists[b], s.count), s.flat), "lists of block %d" % b
        assign = o.assign[b].tolist()
        M.check_assign(assign, s.usz)
        assert assign == s.assign, "assign of block %d" % b
    tot = sum(ks) % L
    assert o.partial.tobytes() == _enc_mul(tot) and int(o.identity[0]) == int(tot == 0)
    return ks


def fill_random(bt, rng):
    bt.digits[:, :bt.pb * bt.nblk] = M.random_rows(rng, bt.nblk)   # non-zero digits past n too
    bt.mult = [1 + rng.randrange(4 * K.kPartProofs + 2) for _ in bt.mult]
    bt.prod = [(rng.randrange(L), rng.randrange(L)) for _ in bt.prod]


# ---- the sort, the walk and the combine ------------------------------------------------------------

def test_128_pairs_at_full_capacity(probe):
    """One block of 128 proofs under 128 distinct pairs spread over [0, 4096), every half-digit of
    every point and of every extra non-zero within the top-window bound: 256 extras, and the list
    holds exactly the many-mode cap."""
    cap, kp = _cap(), K.kPartProofs
    rng = random.Random(5)
    rows, _ = M.full_rows(rng)

    def full_scalar():
        while True:
            s = rng.randrange(1, L)
            if all(all(M.split8(x)) for x in M.recode16(s)):
                return s
    bt = Batch(1)
    bt.digits[:, :bt.pb] = rows
    bt.mult = [1 + rng.randrange(4 * kp + 2) for _ in bt.mult]
    bt.idx = [(37 * t + 5) % NPAIRS for t in range(kp)]
    assert len(set(bt.idx)) == kp
    bt.prod = [(full_scalar(), full_scalar()) for _ in range(kp)]
    assert bt.table(0) == bt.idx and bt.extras(0) == [v for pr in bt.prod for v in pr]
    o = run_blocks(probe, bt)
    assert int(o.offs[0, -1]) == cap and np.all(o.lists[0] != 0xffff)
    check(bt, o)
    assert T.extra_ids(o, 0, cap) == {u: K.kPartWindows for u in range(2 * kp)}


def test_65_pairs_with_the_extreme_indices(probe):
    """One block with 65 distinct pairs, one more than the pair mode's bound, among them global
    indices 0 and 4095."""
    rng = random.Random(7)
    bt = Batch(1)
    fill_random(bt, rng)
    pairs65 = [4095, 0] + rng.sample(range(1, 4095), 63)
    bt.idx = [pairs65[t % 65] for t in range(K.kPartProofs)]
    table = bt.table(0)
    assert table[:65] == pairs65 and table[65] == MM.NO_PAIR
    o = run_blocks(probe, bt)
    check(bt, o)
    assert set(T.extra_ids(o, 0, int(o.offs[0, -1]))) == set(range(130))


def test_repeats_and_two_orders(probe):
    """Pairs repeated non-contiguously within a block, and two blocks that share their pairs in
    different first-occurrence orders: each block's slots are its own."""
    rng = random.Random(11)
    kp = K.kPartProofs
    bt = Batch(2)
    fill_random(bt, rng)
    shared = [3000, 17, 4095, 900, 64]
    b0 = [shared[k] for k in (0, 1, 0, 2, 1, 3, 0, 4)] + [rng.choice(shared + [70, 71]) for _ in range(kp - 8)]
    b1 = [shared[k] for k in (4, 3, 4, 2, 1, 0, 3, 2)] + [rng.choice(shared + [5, 71]) for _ in range(kp - 8)]
    bt.idx = b0 + b1
    t0, t1 = bt.table(0), bt.table(1)
    assert t0[:5] == shared and t1[:5] == shared[::-1] and t0 != t1
    o = run_blocks(probe, bt, per_launch=1)
    check(bt, o)


def test_partial_last_block(probe):
    """n = 128 + 3: the last block has 3 proofs; prod and pair_idx are 256 rows long and the rows
    past n hold non-zero poison under valid indices, which must neither be counted nor take a slot."""
    rng = random.Random(9)
    kp = K.kPartProofs
    n = kp + 3
    bt = Batch(2, n=n, rows=2 * kp)
    fill_random(bt, rng)
    bt.idx = [rng.randrange(NPAIRS) for _ in range(n)] + [(100 + t) % NPAIRS for t in range(2 * kp - n)]
    assert all(a and b for a, b in bt.prod[n:]) and bt.digits[:, 4 * n:bt.pb * 2].any()
    o = run_blocks(probe, bt)
    check(bt, o)
    assert o.slots[1].tolist() == bt.idx[kp:n] + [MM.NO_PAIR] * (kp - 3)
    assert MM.slot_table(bt.idx, 2 * kp, kp, 1) != bt.table(1)


def test_slot_sum_that_cancels(probe):
    """The pair in slot 1 has two entries in the block with products x and l - x in both components:
    its sum is 0 mod l, it contributes no list entry, and the partial is right."""
    rng = random.Random(13)
    bt = Batch(1)
    fill_random(bt, rng)
    bt.idx = [2222] * K.kPartProofs
    bt.idx[5] = bt.idx[100] = 77
    bt.idx[6] = 4000
    x, y = rng.randrange(1, L), rng.randrange(1, L)
    bt.prod[5], bt.prod[100] = (x, y), (L - x, L - y)
    assert bt.table(0)[:4] == [2222, 77, 4000, MM.NO_PAIR] and bt.extras(0)[2:4] == [0, 0]
    o = run_blocks(probe, bt)
    check(bt, o)
    got = T.extra_ids(o, 0, int(o.offs[0, -1]))
    assert 2 not in got and 3 not in got and set(got) == {0, 1, 4, 5}


def test_launchers_refuse_what_they_cannot_serve(probe):
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    assert probe.partmanyprobe_refusals(ctypes.byref(a), ctypes.byref(b)) == 0
    assert a.value == 1 and b.value == 1                     # hipErrorInvalidValue, not a launch


# ---- the locate pass -------------------------------------------------------------------------------

def test_locate_pass(probe):
    """Three prepared blocks of proofs that are valid by construction -- proof i under pair p has
    -r1 = [-(s m_g + c m_y1)] B, so a (s g - r1 - c y1) is the identity, and likewise for h -- with
    the weights of the oracle's ChaCha20 block.  Block 2 holds one forged proof (s + 1 in its
    products), block 0 two.  The first pass, then the locate pass over blocks [2, 0] through pmap,
    out of order: each listed block reads its prepared block's slots, the sums by slot are Python's
    sum j_t prod mod l, block 2 is located at its t, block 0 is not."""
    kp = K.kPartProofs
    rng = random.Random(31)
    n = 3 * kp - 7
    seed = bytes(rng.randrange(256) for _ in range(32))
    first_index = (1 << 33) + 5
    few = [4095, 0, 1234, 65, 3001]
    idx = [rng.choice(few) if i < kp else rng.randrange(NPAIRS) for i in range(n)]   # block 0: five pairs, repeated
    forged = {2 * kp + 41, 9, 77}
    s = [rng.randrange(L) for _ in range(n)]
    c = [rng.randrange(L) for _ in range(n)]
    status = np.zeros(n, np.uint8)
    status[[3, kp + 1, 2 * kp + 2]] = [2, 4, 3]         # zero weight: zero digits and products
    bt = Batch(3, n=n)
    bt.idx = idx
    weights = []
    for i in range(n):
        u = struct.unpack("<16I", O.chacha20_block(seed, first_index + i))
        ua, ub = list(u[0:4]), list(u[4:8])
        a, b = M.weight_int(ua), M.weight_int(ub)
        weights.append((ua, ub, a, b))
        my1, my2 = 1 + rng.randrange(4 * kp), 1 + rng.randrange(4 * kp)
        mg, mh = _gh_mult(idx[i])
        bt.mult[4 * i:4 * i + 4] = [-(s[i] * mg + c[i] * my1) % L, my1, -(s[i] * mh + c[i] * my2) % L, my2]
        if status[i]:
            continue
        si = s[i] + 1 if i in forged else s[i]
        bt.prod[i] = (a * si % L, b * si % L)
        bt.digits[:, 4 * i + 0] = M.weight_words(ua) + [0] * 8
        bt.digits[:, 4 * i + 1] = M.recode16(a * c[i] % L)
        bt.digits[:, 4 * i + 2] = M.weight_words(ub) + [0] * 8
        bt.digits[:, 4 * i + 3] = M.recode16(b * c[i] % L)
    o = run_blocks(probe, bt)
    ks = check(bt, o)
    assert ks[1] == 0 and ks[0] and ks[2] and o.fail.tolist() == [1, 0, 1]
    i2 = 2 * kp + 41
    assert ks[2] == (weights[i2][2] * _gh_mult(idx[i2])[0] + weights[i2][3] * _gh_mult(idx[i2])[1]) % L
    tables = [bt.table(b) for b in range(3)]
    assert tables[0] != tables[2] and o.slots.tolist() == tables

    blocks = [2, 0]
    dstride = 4 * kp * len(blocks) + 8
    digits = np.full((16, dstride), -1, np.int16)
    sums = np.full((len(blocks) * 2 * kp, 8), 0xffffffff, np.uint32)
    rc = probe.partmanyprobe_index_digits(
        _ll(len(blocks)), _ll(n), _ll(3), _ptr(np.array(blocks, np.uint32)), ctypes.c_ulonglong(first_index),
        _ptr(np.frombuffer(seed, "<u4").copy()), _ptr(_scalar_words(c)), _ptr(status),
        _ptr(_scalar_words([v for pr in bt.prod for v in pr])), _ptr(np.array(idx, np.uint32)), ctypes.c_int(NPAIRS),
        _ptr(o.slots), _ll(dstride), _ptr(digits), _ptr(sums))
    assert rc == 0
    mult = [M.loc_j(t) for t in range(kp)]
    want_sums = [MM.slot_sums(bt.prod, idx, n, kp, blk, table=tables[blk], mult=mult) for blk in blocks]
    got_sums = [int.from_bytes(sums[k].tobytes(), "little") for k in range(len(sums))]
    assert got_sums == [v for blk in want_sums for v in blk]
    want = np.zeros((16, 4 * kp * len(blocks)), np.int64)
    for b, blk in enumerate(blocks):
        for t in range(kp):
            i, o4 = blk * kp + t, 4 * (b * kp + t)
            if i >= n or status[i]:
                continue
            ua, ub, a, bw = weights[i]
            j = mult[t]
            want[:, o4] = M.index_weight_digits(ua, j)
            want[:, o4 + 1] = M.recode16(j * a * c[i] % L)
            want[:, o4 + 2] = M.index_weight_digits(ub, j)
            want[:, o4 + 3] = M.recode16(j * bw * c[i] % L)
    assert np.array_equal(digits[:, :4 * kp * len(blocks)].astype(np.int64), want)
    assert np.all(digits[:, 4 * kp * len(blocks):] == -1), "digits written past the listed blocks"

    lt = Batch(len(blocks), nprep=3, pmap=blocks)
    lt.mult = bt.mult
    lt.dstride = dstride
    lt.digits = digits
    lt.presummed = want_sums
    lt.tables = tables
    lo = run_blocks(probe, lt)
    lks = check(lt, lo)
    assert lks[0] == M.loc_j(41) * ks[2] % L
    assert all((M.loc_j(t) * ks[0] - lks[1]) % L for t in range(kp))

    loc = np.full(len(blocks), 0x5555, np.uint16)
    rc = probe.partmanyprobe_locate(_ll(len(blocks)), _ll(3), _ptr(o.part), _ptr(lo.part), _ptr(lo.fail),
                                    _ptr(np.array(blocks, np.uint32)), _ptr(loc))
    assert rc == 0
    assert loc.tolist() == [41, K.kPartNoLoc]
