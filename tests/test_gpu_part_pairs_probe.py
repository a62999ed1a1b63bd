"""GPU tests of the partitioned check's pair-mode kernels (csrc/part.hip) on chosen digits,
products and pair indices.

tests/native/partpairsprobe.hip includes part.hip unchanged and drives k_part_sort_pairs,
k_part_acc_pairs, the combine, k_part_sum1/2, k_part_index_digits_pairs and k_part_locate.  Every
point -- the blocks' and the pairs' g_p, h_p -- is a known multiple of the basepoint, so a block's
expected partial is [(sum_j K_j m_j + sum_p (S_{a,p} m_{g,p} + S_{b,p} m_{h,p})) mod l] B: Python
integers (tests/part_pairs_model.py) and one pt_mul of the Python oracle.  Partials are compared as
32-byte encodings, fail flags, offsets and assignments exactly, lists per bucket as multisets.

CPZ_PARTPAIRSPROBE=<path> loads another build of the probe (over a mutated copy of csrc)."""
import ctypes
import functools
import random
import struct

import numpy as np
import pytest

import part_model as M
import part_pairs_model as PM
import pyoracle as O

pytestmark = pytest.mark.gpu

K, L = M.K, O.L
ZERO32 = bytes(32)


@pytest.fixture(scope="module")
def probe():
    lib = PM.load_probe()
    assert lib.partpairsprobe_const(2) == K.kPartProofs and lib.partpairsprobe_const(3) == K.kPartWindows
    return lib


@functools.lru_cache(maxsize=None)
def _cap():
    lib = PM.load_probe()
    cap, mp = int(lib.partpairsprobe_const(0)), int(lib.partpairsprobe_const(1))
    assert cap == PM.list_cap_pairs(K.kPartProofs, mp) and lib.partpairsprobe_const(4) == -1
    return cap, mp


def _ptr(a):
    if a is None:
        return ctypes.c_void_p(None)
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def _ll(x):
    return ctypes.c_longlong(int(x))


@functools.lru_cache(maxsize=None)
def _pool():
    """encodings of [m] B for m = 0 .. 4 kPartProofs + 2, by repeated addition"""
    out, p = [ZERO32], O.BASEPOINT
    for _ in range(4 * K.kPartProofs + 2):
        out.append(O.ristretto_encode(p))
        p = O.pt_add(p, O.BASEPOINT)
    return out


@functools.lru_cache(maxsize=None)
def _enc_mul(m):
    m %= L
    if m < len(_pool()):
        return _pool()[m]
    if L - m < len(_pool()):
        return O.ristretto_encode(O.pt_neg(O.ristretto_decode(_pool()[L - m])))
    return O.ristretto_encode(O.pt_mul(O.BASEPOINT, m))


def _words(encs):
    return np.frombuffer(b"".join(encs), dtype="<u4").reshape(len(encs), 8).copy()


def _scalar_words(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u4").reshape(len(vals), 8).copy()


def _gh_mult(npairs):
    """(m_g, m_h) of pair p: [m] B are its points"""
    return [(1000003 + 17 * p, 777777777777 + 29 * p) for p in range(npairs)]


class Batch:
    """nblk blocks over nprep prepared blocks: mult[slot] (the point is [mult] B), digits
    int16[16][dstride], n proofs, and either per-proof products with pair indices (rows may exceed
    n) or, with presummed set, the per-block per-pair sums themselves."""

    def __init__(self, nblk, npairs, n=None, nprep=None, pmap=None, rows=None):
        self.nblk, self.nprep, self.pmap, self.npairs = nblk, nprep or nblk, pmap, npairs
        self.n = K.kPartProofs * nblk if n is None else n
        self.pb = 4 * K.kPartProofs
        self.mult = [0] * (self.pb * self.nprep)
        self.dstride = self.pb * nblk + 4
        self.digits = np.zeros((16, self.dstride), np.int16)
        r = self.n if rows is None else rows
        self.prod = [(0, 0)] * r
        self.idx = [0] * r
        self.gh = _gh_mult(npairs)
        self.presummed = None          # [nblk][2 npairs] when the sums are given directly

    def rows(self, b):
        r = self.digits[:, self.pb * b:self.pb * (b + 1)].T.astype(np.int64)
        live = max(0, min(K.kPartProofs, self.n - K.kPartProofs * b))
        r[4 * live:] = 0
        return r

    def extras(self, b):
        if self.presummed is not None:
            return list(self.presummed[b])
        return PM.pair_sums(self.prod, self.idx, self.n, self.npairs, K.kPartProofs, b)

    def scalar(self, b):
        r = self.rows(b)
        pts = self.pb * (self.pmap[b] if self.pmap else b)
        ex = self.extras(b)
        tot = sum(ex[2 * p] * self.gh[p][0] + ex[2 * p + 1] * self.gh[p][1] for p in range(self.npairs))
        for slot in np.nonzero(r.any(axis=1))[0].tolist():
            tot += M.row_value(r[slot].tolist()) * self.mult[pts + slot]
        return tot % L


class Out:
    pass


def run_blocks(probe, bt, per_launch=4):
    cap, _ = _cap()
    o = Out()
    o.part = np.full((bt.nblk, 8), 0xffffffff, np.uint32)
    o.fail = np.full(bt.nblk, 0xff, np.uint8)
    o.lists = np.full((bt.nblk, cap), 0xffff, np.uint16)
    o.offs = np.full((bt.nblk, K.kPartOffs), 0xffff, np.uint16)
    o.assign = np.full((bt.nblk, K.kPartUnits), 0xffff, np.uint16)
    o.partial = np.full(8, 0xffffffff, np.uint32)
    o.identity = np.full(1, -1, np.int32)
    pmap = np.array(bt.pmap, np.uint32) if bt.pmap else None
    if bt.presummed is not None:
        prod = _scalar_words([v for blk in bt.presummed for v in blk])
        idx, prod_rows = None, bt.nblk * bt.npairs
    else:
        prod = _scalar_words([v for pr in bt.prod for v in pr])
        idx, prod_rows = np.array(bt.idx, np.uint32), len(bt.prod)
    gh = _words([_enc_mul(m) for pr in bt.gh for m in pr])
    rc = probe.partpairsprobe_blocks(
        _ll(bt.nblk), _ll(bt.n), _ll(bt.nprep), _ptr(_words([_enc_mul(m) for m in bt.mult])), _ptr(bt.digits),
        _ll(bt.dstride), _ptr(prod), _ptr(idx), _ll(prod_rows), _ptr(gh), ctypes.c_int(bt.npairs), _ptr(pmap),
        _ll(per_launch), _ptr(o.part), _ptr(o.fail), _ptr(o.lists), _ptr(o.offs), _ptr(o.assign), _ptr(o.partial),
        _ptr(o.identity))
    assert rc == 0, "partpairsprobe_blocks: hipError %d" % rc
    o.enc = [o.part[b].tobytes() for b in range(bt.nblk)]
    return o


def check(bt, o):
    """every block's partial, flags, offsets, lists and assignment, and the summed partial"""
    cap, _ = _cap()
    ks = [bt.scalar(b) for b in range(bt.nblk)]
    for b in range(bt.nblk):
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


def extra_ids(o, b, total):
    """{extra u: list entries} of block b"""
    ids = o.lists[b, :total].astype(np.int64) & 0x7fff
    base = 4 * K.kPartProofs
    return {int(u): int((ids == base + u).sum()) for u in np.unique(ids[ids >= base] - base)}


# ---- the sort, the walk and the combine ------------------------------------------------------------

def test_two_pairs(probe):
    """One block, two pairs: every proof under pair 0 except t = 77 under pair 1."""
    rng = random.Random(1)
    bt = Batch(1, 2)
    fill_random(bt, rng)
    bt.idx = [1 if t == 77 else 0 for t in range(K.kPartProofs)]
    o = run_blocks(probe, bt)
    check(bt, o)
    ex = bt.extras(0)
    assert ex[2] == bt.prod[77][0] and ex[3] == bt.prod[77][1]
    assert ex[0] == sum(bt.prod[t][0] for t in range(K.kPartProofs) if t != 77) % L


def test_64_pairs_at_full_capacity(probe):
    """One block, 64 pairs, pair = t % 64, every half-digit of every point and of every extra
    non-zero within the top-window bound: the list holds exactly the pair-mode cap."""
    cap, mp = _cap()
    assert mp == 64
    rng = random.Random(5)
    rows, _ = M.full_rows(rng)

    def full_scalar():
        while True:
            s = rng.randrange(1, L)
            if all(all(M.split8(x)) for x in M.recode16(s)):
                return s
    bt = Batch(1, mp)
    bt.digits[:, :bt.pb] = rows
    bt.mult = [1 + rng.randrange(4 * K.kPartProofs + 2) for _ in bt.mult]
    bt.idx = [t % mp for t in range(K.kPartProofs)]
    # the pair's sums are chosen, its last proof's products make them up
    per = K.kPartProofs // mp
    want = [full_scalar() for _ in range(2 * mp)]
    prod = [[rng.randrange(L), rng.randrange(L)] for _ in range(K.kPartProofs)]
    for p in range(mp):
        last = p + mp * (per - 1)
        for k in range(2):
            prod[last][k] = (want[2 * p + k] - sum(prod[p + mp * r][k] for r in range(per - 1))) % L
    bt.prod = [tuple(x) for x in prod]
    assert bt.extras(0) == want
    o = run_blocks(probe, bt)
    assert int(o.offs[0, -1]) == cap and np.all(o.lists[0] != 0xffff)
    check(bt, o)
    assert extra_ids(o, 0, cap) == {u: K.kPartWindows for u in range(2 * mp)}


def test_partial_last_block(probe):
    """n = 131 over 3 pairs: the last block has 3 proofs; prod and pair_idx are 256 rows long and
    the rows past n hold non-zero poison under valid indices, which must not be counted."""
    rng = random.Random(9)
    n = K.kPartProofs + 3
    bt = Batch(2, 3, n=n, rows=2 * K.kPartProofs)
    fill_random(bt, rng)
    bt.idx = [rng.randrange(3) for _ in range(n)] + [t % 3 for t in range(2 * K.kPartProofs - n)]
    assert all(a and b for a, b in bt.prod[n:]) and bt.digits[:, 4 * n:bt.pb * 2].any()
    o = run_blocks(probe, bt)
    check(bt, o)
    poisoned = PM.pair_sums(bt.prod, bt.idx, 2 * K.kPartProofs, 3, K.kPartProofs, 1)
    assert poisoned != bt.extras(1)


def test_pair_sum_that_cancels(probe):
    """Pair 1 has two entries in the block with products x and l - x in both components: its sum
    is 0 mod l, it contributes no list entry, and the partial is right."""
    rng = random.Random(13)
    bt = Batch(1, 3)
    fill_random(bt, rng)
    bt.idx = [0] * K.kPartProofs
    bt.idx[5] = bt.idx[100] = 1
    bt.idx[6] = 2
    x, y = rng.randrange(1, L), rng.randrange(1, L)
    bt.prod[5], bt.prod[100] = (x, y), (L - x, L - y)
    assert bt.extras(0)[2:4] == [0, 0]
    o = run_blocks(probe, bt)
    check(bt, o)
    got = extra_ids(o, 0, int(o.offs[0, -1]))
    assert 2 not in got and 3 not in got and set(got) == {0, 1, 4, 5}


def test_largest_extra_scalar(probe):
    """An extra with scalar l - 1 (and one with 2^252): fail bit 1 stays clear."""
    bt = Batch(1, 2)
    bt.mult = [3 + t for t in range(bt.pb)]
    bt.digits[2, 8] = 0x0101
    bt.idx = [0] * K.kPartProofs
    bt.idx[3] = 1
    bt.prod[0] = (L - 1, 0)
    bt.prod[3] = (0, 1 << 252)
    assert bt.extras(0) == [L - 1, 0, 0, 1 << 252]
    o = run_blocks(probe, bt)
    check(bt, o)
    assert o.fail[0] == 1


def test_sum_over_blocks(probe):
    """Three blocks over 5 pairs, two blocks per launch: sum_b P_b is the whole partial."""
    rng = random.Random(21)
    bt = Batch(3, 5, n=3 * K.kPartProofs - 50)
    fill_random(bt, rng)
    bt.idx = [rng.randrange(5) for _ in range(bt.n)]
    o = run_blocks(probe, bt, per_launch=2)
    ks = check(bt, o)
    assert all(ks) and o.identity[0] == 0


# ---- the locate pass -------------------------------------------------------------------------------

def test_locate_pass(probe):
    """Three prepared blocks of proofs that are valid by construction -- proof i under pair p has
    -r1 = [-(s m_g + c m_y1)] B, so a (s g - r1 - c y1) is the identity, and likewise for h -- with
    the weights of the oracle's ChaCha20 block.  Block 2 holds one forged proof (s + 1 in its
    products) under a pair other than the block's majority, block 0 two.  The first pass, then the
    locate pass over blocks [2, 0] through pmap: the compact per-pair sums are Python's
    sum j_t prod mod l, block 2 is located at its t, block 0 is not."""
    kp, npairs = K.kPartProofs, 3
    rng = random.Random(31)
    n = 3 * kp - 7
    seed = bytes(rng.randrange(256) for _ in range(32))
    first_index = (1 << 33) + 5
    gh = _gh_mult(npairs)
    idx = [0 if i >= 2 * kp else rng.randrange(npairs) for i in range(n)]   # block 2: pair 0 throughout ...
    forged = {2 * kp + 41: 2, 9: idx[9], 77: idx[77]}
    idx[2 * kp + 41] = 2                                                     # ... but for the forged proof
    s = [rng.randrange(L) for _ in range(n)]
    c = [rng.randrange(L) for _ in range(n)]
    status = np.zeros(n, np.uint8)
    status[[3, kp + 1, 2 * kp + 2]] = [2, 4, 3]         # zero weight: zero digits and products
    bt = Batch(3, npairs, n=n)
    bt.idx = idx
    weights = []
    for i in range(n):
        u = struct.unpack("<16I", O.chacha20_block(seed, first_index + i))
        ua, ub = list(u[0:4]), list(u[4:8])
        a, b = M.weight_int(ua), M.weight_int(ub)
        weights.append((ua, ub, a, b))
        my1, my2 = 1 + rng.randrange(4 * kp), 1 + rng.randrange(4 * kp)
        mg, mh = gh[idx[i]]
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
    assert ks[2] == (weights[i2][2] * gh[2][0] + weights[i2][3] * gh[2][1]) % L

    blocks = [2, 0]
    dstride = 4 * kp * len(blocks) + 8
    digits = np.full((16, dstride), -1, np.int16)
    sums = np.full((len(blocks) * 2 * npairs, 8), 0xffffffff, np.uint32)
    rc = probe.partpairsprobe_index_digits(
        _ll(len(blocks)), _ll(n), _ptr(np.array(blocks, np.uint32)), ctypes.c_ulonglong(first_index),
        _ptr(np.frombuffer(seed, "<u4").copy()), _ptr(_scalar_words(c)), _ptr(status),
        _ptr(_scalar_words([v for pr in bt.prod for v in pr])), _ptr(np.array(idx, np.uint32)), ctypes.c_int(npairs),
        _ll(dstride), _ptr(digits), _ptr(sums))
    assert rc == 0
    mult = [M.loc_j(t) for t in range(kp)]
    want_sums = [PM.pair_sums(bt.prod, idx, n, npairs, kp, blk, mult) for blk in blocks]
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

    lt = Batch(len(blocks), npairs, nprep=3, pmap=blocks)
    lt.mult = bt.mult
    lt.dstride = dstride
    lt.digits = digits
    lt.presummed = want_sums
    lo = run_blocks(probe, lt)
    lks = check(lt, lo)
    assert lks[0] == M.loc_j(41) * ks[2] % L
    assert all((M.loc_j(t) * ks[0] - lks[1]) % L for t in range(kp))

    loc = np.full(len(blocks), 0x5555, np.uint16)
    rc = probe.partpairsprobe_locate(_ll(len(blocks)), _ll(3), _ptr(o.part), _ptr(lo.part), _ptr(lo.fail),
                                     _ptr(np.array(blocks, np.uint32)), _ptr(loc))
    assert rc == 0
    assert loc.tolist() == [41, K.kPartNoLoc]
