"""GPU tests of the partitioned check's kernels (csrc/part.hip) on chosen digits and blocks.

The public ABI reaches part.hip only at 2^19 proofs or more and with seed-derived scalars, so
tests/native/partprobe.hip includes part.hip unchanged and drives k_part_sort, k_part_acc, the
three combine kernels, k_part_sum1/2, k_part_index_digits and k_part_locate on hand-made digit
rows.  Every point is a known multiple m_j of the basepoint, so a block's expected partial is
[(sum_j K_j m_j + s_a m_g + s_b m_h) mod l] B: Python integers (tests/part_model.py) and one
pt_mul of the Python oracle.  Partials are compared as 32-byte encodings, fail flags, offsets,
assignments and digit rows exactly, lists per bucket as multisets.

k_part_combine_lane's own dispatch needs 65,536 blocks (2.6 GB of window sums); it stays with
the 2^24-proof tests of tests/test_gpu_scale.py, and here the kernel is launched by name.

CPZ_PARTPROBE=<path> loads another build of the probe (over a mutated copy of csrc)."""
import ctypes
import functools
import random
import struct

import numpy as np
import pytest

import part_model as M
import pyoracle as O

pytestmark = pytest.mark.gpu

K, L = M.K, O.L
ZERO32 = bytes(32)
AUTO, QUAD, LANE, TREE = 0, 1, 2, 3
M_G, M_H = 1000003, 777777777777


@pytest.fixture(scope="module")
def probe():
    return M.load_probe()


def _ptr(a):
    if a is None:
        return ctypes.c_void_p(None)
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def _ll(x):
    return ctypes.c_longlong(int(x))


# ---- points that are known multiples of the basepoint -------------------------------------------

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


# ---- a batch of blocks ----------------------------------------------------------------------------

class Batch:
    """nblk blocks over nprep prepared blocks of points: mult[slot] (the point is [mult] B),
    digits int16[16][dstride], sums[b] = (s_a, s_b), n proofs."""

    def __init__(self, nblk, n=None, nprep=None, pmap=None):
        self.nblk, self.nprep, self.pmap = nblk, nprep or nblk, pmap
        self.n = K.kPartProofs * nblk if n is None else n
        self.pb = 4 * K.kPartProofs
        self.mult = [0] * (self.pb * self.nprep)
        self.dstride = self.pb * nblk + 4     # a stride that is not the row length
        self.digits = np.zeros((16, self.dstride), np.int16)
        self.sums = [(0, 0)] * nblk

    def put(self, b, slot, m, w, d):
        """slot of listed block b: the point [m] B with digit d in window w"""
        self.mult[self.pb * (self.pmap[b] if self.pmap else b) + slot] = m
        self.digits[w, self.pb * b + slot] = d

    def rows(self, b):
        """block b's digit rows [4 kPartProofs][16] as the kernels must see them: zero past n"""
        r = self.digits[:, self.pb * b:self.pb * (b + 1)].T.astype(np.int64)
        live = max(0, min(K.kPartProofs, self.n - K.kPartProofs * b))
        r[4 * live:] = 0
        return r

    def scalar(self, b):
        """(sum_j K_j m_j + s_a m_g + s_b m_h) mod l of block b"""
        r = self.rows(b)
        pts = self.pb * (self.pmap[b] if self.pmap else b)
        tot = self.sums[b][0] * M_G + self.sums[b][1] * M_H
        for slot in np.nonzero(r.any(axis=1))[0].tolist():
            tot += M.row_value(r[slot].tolist()) * self.mult[pts + slot]
        return tot % L

    def expected(self):
        ks = [self.scalar(b) for b in range(self.nblk)]
        return ks, [_enc_mul(k) for k in ks]


class Out:
    pass


def run_blocks(probe, bt, per_launch, combine=AUTO):
    R = K.kPartProofs // K.kRlcSumBlock
    sums = []
    for sa, sb in bt.sums:
        sums += [sa, sb] + [0, 0] * (R - 1)
    o = Out()
    o.part = np.full((bt.nblk, 8), 0xffffffff, np.uint32)
    o.fail = np.full(bt.nblk, 0xff, np.uint8)
    o.lists = np.full((bt.nblk, K.kPartListCap), 0xffff, np.uint16)
    o.offs = np.full((bt.nblk, K.kPartOffs), 0xffff, np.uint16)
    o.assign = np.full((bt.nblk, K.kPartUnits), 0xffff, np.uint16)
    o.partial = np.full(8, 0xffffffff, np.uint32)
    o.identity = np.full(1, -1, np.int32)
    pmap = np.array(bt.pmap, np.uint32) if bt.pmap else None
    rc = probe.partprobe_blocks(
        _ll(bt.nblk), _ll(bt.n), _ll(bt.nprep), _ptr(_words([_enc_mul(m) for m in bt.mult])), _ptr(bt.digits),
        _ll(bt.dstride), _ptr(_scalar_words(sums)), _ptr(_words([_enc_mul(M_G), _enc_mul(M_H)])), _ptr(pmap),
        _ll(per_launch), ctypes.c_int(combine), _ptr(o.part), _ptr(o.fail), _ptr(o.lists), _ptr(o.offs),
        _ptr(o.assign), _ptr(o.partial), _ptr(o.identity))
    assert rc == 0, "partprobe_blocks: hipError %d" % rc
    o.enc = [o.part[b].tobytes() for b in range(bt.nblk)]
    return o


def check_partials(bt, o, skip=()):
    """every block's partial and fail flag, and the summed partial (when no block is skipped)"""
    ks, encs = bt.expected()
    bad = [b for b in range(bt.nblk) if b not in skip and o.enc[b] != encs[b]]
    assert not bad, "wrong partials at blocks %r" % bad[:10]
    want = [int(k != 0) for k in ks]
    badf = [(b, int(o.fail[b])) for b in range(bt.nblk) if b not in skip and o.fail[b] != want[b]]
    assert not badf, "wrong fail flags (block, flag): %r" % badf[:10]
    if not skip:
        tot = sum(ks) % L
        assert o.partial.tobytes() == _enc_mul(tot) and int(o.identity[0]) == int(tot == 0)


def check_sort(bt, o, blocks=None):
    """offs, lists and assign of the listed blocks against the model; bit 1 of fail"""
    for b in (range(bt.nblk) if blocks is None else blocks):
        s = M.sort_model(bt.rows(b), *bt.sums[b])
        assert np.array_equal(o.offs[b].astype(np.int64), s.offs), "offs of block %d" % b
        assert np.all(o.lists[b, s.total:] == 0xffff), "block %d: list entries written past its end" % b
        assert np.array_equal(M.canonical_list(o.lists[b], s.count), s.flat), "lists of block %d" % b
        assign = o.assign[b].tolist()
        M.check_assign(assign, s.usz)
        assert assign == s.assign, "assign of block %d" % b
        assert bool(o.fail[b] & 2) == s.top_over and o.fail[b] < 4, "fail flags of block %d: %d" % (b, o.fail[b])


def _mult(i):
    return 1 + (i * 37 + 11) % (4 * K.kPartProofs)


def one_digit_batch(cases):
    bt = Batch(len(cases))
    for i, (w, d) in enumerate(cases):
        bt.put(i, M.slot_of(i), _mult(i), w, d)
    return bt


def random_batch(seed, nblk, ragged=True, nprep=None, pmap=None):
    rng = random.Random(seed)
    n = K.kPartProofs * nblk - (K.kPartProofs - 1 if ragged else 0)
    bt = Batch(nblk, n, nprep, pmap)
    bt.digits[:, :bt.pb * nblk] = M.random_rows(rng, nblk)   # non-zero digits past n too
    bt.mult = [1 + rng.randrange(4 * K.kPartProofs + 2) for _ in bt.mult]
    bt.sums = [(rng.randrange(L), rng.randrange(L)) for _ in range(nblk)]
    return bt


# ---- a. one-digit blocks ----------------------------------------------------------------------------

def test_one_digit_blocks(probe):
    """One block per (window, digit) of part_model.one_digit_cases(): one point, one non-zero
    16-bit digit -- lo / hi on +-1, the first and last bucket of every lane share, the split
    edges, (lo, hi) = (-128, 128) and (0, -128), and the top window's 16 buckets -- the slot
    rotating over q = 0..3 and t in {0, 1, 63, 64, kPartProofs - 1}.  256 blocks per sort / walk
    launch (blk0 = 0, 256, ...), the quad combine by launch_part_combine's own dispatch."""
    cases = M.one_digit_cases()
    bt = one_digit_batch(cases)
    assert bt.nblk > K.kPartTreeMaxBlocks
    o = run_blocks(probe, bt, 256)
    check_partials(bt, o)
    assert np.all(o.fail == 1)
    check_sort(bt, o)


def test_block_sum_digits(probe):
    """The same edges through the g and h block sums: 0, 1, l - 1 and 2^252 in each of the two
    sums, and every low-window digit as a digit of one sum.  No point has a digit."""
    cases = M.sum_cases()
    bt = Batch(len(cases))
    bt.mult = [_mult(i) for i in range(len(bt.mult))]
    bt.sums = list(cases)
    o = run_blocks(probe, bt, 64)
    check_partials(bt, o)
    assert [int(f) for f in o.fail] == [int((a, b) != (0, 0)) for a, b in cases]
    check_sort(bt, o)


# ---- b. full and ragged blocks ----------------------------------------------------------------------

@pytest.mark.parametrize("nblk", [1, 5, 17])
def test_random_ragged_blocks(probe, nblk):
    """Random int16 digits in all 16 windows of all four points (window 15 inside [-4224, 4223]),
    random block sums; the last block has one proof, with non-zero digits in memory for the
    proofs past n; 4 blocks per sort / walk launch, so blk0 = 4, 8, ... separates the buffers
    indexed by the launch's block from those indexed by the batch's."""
    bt = random_batch(100 + nblk, nblk)
    assert bt.n == K.kPartProofs * (nblk - 1) + 1 and bt.digits[:, 4 * bt.n:bt.pb * nblk].any()
    o = run_blocks(probe, bt, 4)
    check_partials(bt, o)
    check_sort(bt, o)


def test_full_block(probe):
    """Every half-digit of every point and of both sums non-zero: the list holds exactly
    kPartListCap entries and the last offset is kPartListCap."""
    rng = random.Random(5)
    rows, sums = M.full_rows(rng)
    bt = Batch(1)
    bt.digits[:, :bt.pb] = rows
    bt.mult = [1 + rng.randrange(4 * K.kPartProofs + 2) for _ in bt.mult]
    bt.sums = [tuple(sums)]
    o = run_blocks(probe, bt, 4)
    assert int(o.offs[0, -1]) == K.kPartListCap and np.all(o.lists[0] != 0xffff)
    check_partials(bt, o)
    check_sort(bt, o)


def test_pmap(probe):
    """Three listed blocks over six prepared ones, pmap = [4, 0, 5]: the points come through
    the map, the digits, sums and outputs are compact."""
    bt = random_batch(33, 3, ragged=False, nprep=6, pmap=[4, 0, 5])
    o = run_blocks(probe, bt, 2)
    check_partials(bt, o)
    check_sort(bt, o)


# ---- c. degenerate blocks ---------------------------------------------------------------------------

def test_degenerate_blocks(probe):
    """Block 0: all digits zero.  1: all 4 kPartProofs slots the same point with the same digit
    (one bucket of 512 entries; the run doubles).  2: P, -P, and P twice with opposite digit
    signs in one bucket, and one more point (the run returns to the identity mid-bucket).  3: P
    and -P alone (the terms sum to the identity: fail 0).  4, 5: one-digit blocks with partials
    Q and -Q."""
    bt = Batch(6)
    for slot in range(bt.pb):
        bt.put(1, slot, 77, 3, 0x2142)
    for slot, m, d in ((0, 9, 0x0505), (5, L - 9, 0x0505), (130, 9, 0x0505), (261, 9, -0x0505), (300, 12, 0x0606)):
        bt.put(2, slot, m, 6, d)
    bt.put(3, 2, 41, 2, 0x1111)
    bt.put(3, 4 * K.kPartProofs - 1, L - 41, 2, 0x1111)
    bt.put(4, 7, 5, 1, 300)
    bt.put(5, 7, L - 5, 1, 300)
    o = run_blocks(probe, bt, 4)
    ks, _ = bt.expected()
    assert ks[0] == 0 and ks[3] == 0 and ks[1] == 4 * K.kPartProofs * 77 * (0x2142 << 48) % L
    assert ks[2] == 12 * (0x0606 << 96) % L and (ks[4] + ks[5]) % L == 0 and ks[4]
    check_partials(bt, o)
    assert [int(f) for f in o.fail] == [0, 1, 1, 0, 1, 1] and o.enc[0] == ZERO32 == o.enc[3]
    check_sort(bt, o)


def test_identity_batch(probe):
    """All digits zero: the summed partial is 32 zero bytes and the identity flag is 1; two
    blocks with partials Q and -Q sum to the identity as well."""
    o = run_blocks(probe, Batch(1), 4)
    assert o.enc[0] == ZERO32 and o.fail[0] == 0 and o.partial.tobytes() == ZERO32 and o.identity[0] == 1
    bt = Batch(2)
    bt.put(0, 7, 5, 1, 300)
    bt.put(1, 9, L - 5, 1, 300)
    o = run_blocks(probe, bt, 4)
    check_partials(bt, o)
    assert [int(f) for f in o.fail] == [1, 1] and o.partial.tobytes() == ZERO32 and o.identity[0] == 1


# ---- d. top-window overflow -------------------------------------------------------------------------

def test_top_window_overflow(probe):
    """A window-15 digit whose high half exceeds kPartTopBuckets (4224, -4225, 17 * 256, 32767,
    -32768), or a block sum of 2^253 - 1, sets bit 1 of that block's fail flag (its partial is
    not asserted); 4223 and -4224 leave it clear with the partial exact; the neighbouring blocks
    of the same launch are unaffected."""
    over = [("d", d) for d in M.TOP_OVER_DIGITS] + [("a", M.TOP_OVER_SUM), ("b", M.TOP_OVER_SUM)]
    kept = [("d", d) for d in M.TOP_KEPT_DIGITS]
    plan = []
    for c in over:
        plan += [("d", 0x0101), c]
    plan += kept + [("d", 0x0101)]
    bt = Batch(len(plan))
    for b, (kind, v) in enumerate(plan):
        if kind == "d":
            bt.put(b, M.slot_of(b), _mult(b), 15, v)
        else:
            bt.put(b, M.slot_of(b), _mult(b), 4, 0x0101)
            bt.sums[b] = (v, 0) if kind == "a" else (0, v)
    flagged = {b for b, c in enumerate(plan) if c in over}
    o = run_blocks(probe, bt, 4)
    assert {b for b in range(bt.nblk) if o.fail[b] & 2} == flagged
    check_partials(bt, o, skip=flagged)
    assert all(o.fail[b] == 1 for b in range(bt.nblk) if b not in flagged)
    check_sort(bt, o)


# ---- e. combine variants and block-count edges --------------------------------------------------

@functools.lru_cache(maxsize=None)
def _mixed_batch(nblk):
    """random ragged blocks with a sample of the one-digit cases written over every third"""
    bt = random_batch(200 + nblk, nblk)
    cases = M.one_digit_cases()
    for b in range(0, nblk - 1, 3):
        lo, hi = bt.pb * b, bt.pb * (b + 1)
        bt.digits[:, lo:hi] = 0
        bt.sums[b] = (0, 0)
        w, d = cases[(b * 131 + nblk) % len(cases)]
        bt.put(b, M.slot_of(b), _mult(b), w, d)
    bt.expected_cache = bt.expected()
    bt.expected = lambda: bt.expected_cache
    return bt


@pytest.mark.parametrize("nblk", [1, 17, 33])
def test_combine_variants(probe, nblk):
    """k_part_combine (with dead quads: nblk is no multiple of 16), k_part_combine_lane and
    k_part_combine_tree launched by name over the same blocks; nblk % 4 != 0 leaves k_part_acc a
    partial workgroup.  Each equals the reference and the three agree on the flags."""
    bt = _mixed_batch(nblk)
    fails = []
    for combine in (QUAD, LANE, TREE):
        o = run_blocks(probe, bt, 8, combine)
        check_partials(bt, o)
        fails.append(o.fail.tolist())
    assert fails[0] == fails[1] == fails[2]


@pytest.mark.parametrize("nblk", [1, 257])
def test_combine_dispatch(probe, nblk):
    """launch_part_combine's own choice: the tree at 1 block, the quad kernel at 257 (above
    kPartTreeMaxBlocks, below kPartLaneMinBlocks)."""
    assert nblk <= K.kPartTreeMaxBlocks or K.kPartTreeMaxBlocks < nblk < K.kPartLaneMinBlocks
    cases = M.one_digit_cases()
    bt = one_digit_batch([cases[(i * 53 + 7) % len(cases)] for i in range(nblk)])
    o = run_blocks(probe, bt, 128)
    check_partials(bt, o)


@pytest.mark.parametrize("nblk", [1, 63, 64, 65, 1025])
def test_part_sum(probe, nblk):
    """launch_part_sum over nblk points [m_i] B: one run short, exact and one over a quad's 64
    entries, and more than one wave of runs."""
    ms = [_mult(i) for i in range(nblk)]
    if nblk > 2:
        ms[nblk - 2] = 0                    # an identity among them
        ms[1] = L - ms[0]                   # P, -P next to each other
    partial = np.full(8, 0xffffffff, np.uint32)
    ident = np.full(1, -1, np.int32)
    rc = probe.partprobe_sum(_ll(nblk), _ptr(_words([_enc_mul(m) for m in ms])), _ptr(partial), _ptr(ident))
    assert rc == 0
    tot = sum(ms) % L
    assert tot and partial.tobytes() == _enc_mul(tot) and ident[0] == 0
    ms[-1] = (ms[-1] - tot) % L             # now the sum is the identity
    rc = probe.partprobe_sum(_ll(nblk), _ptr(_words([_enc_mul(m) for m in ms])), _ptr(partial), _ptr(ident))
    assert rc == 0 and partial.tobytes() == ZERO32 and ident[0] == 1


# ---- f. index digits --------------------------------------------------------------------------------

def test_index_digits(probe):
    """k_part_index_digits over listed blocks out of order, the batch's last block partial,
    first_index above 2^32 and some statuses non-zero, against the model with the weights
    unpacked from the oracle's ChaCha20 block."""
    kp = K.kPartProofs
    R = kp // K.kRlcSumBlock
    rng = random.Random(77)
    n = 3 * kp + 5
    blocks = [3, 0, 2]
    first_index = (1 << 32) + 12345
    seed = bytes(rng.randrange(256) for _ in range(32))
    s = [rng.randrange(L) for _ in range(n)]
    c = [rng.randrange(L) for _ in range(n)]
    s[2 * kp + 1], c[2 * kp + 2], s[3 * kp], c[3 * kp + 1] = 0, 0, L - 1, L - 1
    status = np.zeros(n, np.uint8)
    for i in (0, 1, kp - 1, 2 * kp + 7, 3 * kp + 2):
        status[i] = 1 + i % 5
    nblk = len(blocks)
    dstride = 4 * kp * nblk + 8
    digits = np.full((16, dstride), -1, np.int16)
    sums = np.full((nblk * R * 2, 8), 0xffffffff, np.uint32)
    rc = probe.partprobe_index_digits(
        _ll(nblk), _ll(n), _ptr(np.array(blocks, np.uint32)), ctypes.c_ulonglong(first_index),
        _ptr(np.frombuffer(seed, "<u4").copy()), _ptr(_scalar_words(s)), _ptr(_scalar_words(c)), _ptr(status),
        _ll(dstride), _ptr(digits), _ptr(sums))
    assert rc == 0
    want = np.zeros((16, dstride), np.int64)
    want_sums = [[0, 0] for _ in range(nblk * R)]
    dead = []
    for b, blk in enumerate(blocks):
        for t in range(kp):
            i, o4 = blk * kp + t, 4 * (b * kp + t)
            if i >= n or status[i]:
                dead.append(o4)
                continue
            j = M.loc_j(t)
            u = struct.unpack("<16I", O.chacha20_block(seed, first_index + i))
            ua, ub = list(u[0:4]), list(u[4:8])
            a, bw = M.weight_int(ua), M.weight_int(ub)
            assert (a % L, bw % L) == O.rlc_weights(seed, first_index + i)
            rows = [M.index_weight_digits(ua, j), M.recode16(j * a * c[i] % L),
                    M.index_weight_digits(ub, j), M.recode16(j * bw * c[i] % L)]
            assert M.row_value(rows[0]) == j * a and M.row_value(rows[2]) == j * bw
            for q in range(4):
                want[:, o4 + q] = rows[q]
            sb = want_sums[b * R + t // K.kRlcSumBlock]
            sb[0] = (sb[0] + j * a * s[i]) % L
            sb[1] = (sb[1] + j * bw * s[i]) % L
    assert len(dead) >= 5 + (kp - 5)
    got = digits.astype(np.int64)
    for o4 in dead:
        assert not got[:, o4:o4 + 4].any(), "a dead proof's rows are not zero"
    assert not got[9:, 0:4 * kp * nblk:2].any(), "rows 9..15 of the integer scalars j a, j b"
    assert np.array_equal(got[:, :4 * kp * nblk], want[:, :4 * kp * nblk])
    assert np.all(got[:, 4 * kp * nblk:] == -1), "digits written past the listed blocks"
    got_sums = [int.from_bytes(sums[k].tobytes(), "little") for k in range(2 * nblk * R)]
    assert got_sums == [v for pair in want_sums for v in pair]


def test_index_weight_digits(probe):
    """index_weight_digits in one wave: every weight word -32768, every word 32767, alternating
    words and random ones, with j at both ends of its range; the digits are the model's and sum to
    the integer j * weight."""
    cases = M.weight_digit_cases()
    n = len(cases)
    assert n > 64                                     # lanes take more than one case
    u = np.array([c[0] for c in cases], np.uint32)
    j = np.array([c[1] for c in cases], np.int64)
    out = np.full((n, 16), -1, np.int16)
    rc = probe.partprobe_weight_digits(ctypes.c_int(n), _ptr(u), _ptr(j), _ptr(out))
    assert rc == 0
    for i, (uw, jj) in enumerate(cases):
        got = out[i].tolist()
        assert got == M.index_weight_digits(uw, jj), "case %d" % i
        assert M.row_value(got) == jj * M.weight_int(uw)


# ---- g. locate ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _locate_cases():
    """kPartProofs + 6 listed blocks (part multiple m, lpart multiple, lfail, expected loc):
    block t's P' = [j_t] P, and six that must not be located, early in the list."""
    kp, no = K.kPartProofs, K.kPartNoLoc
    special = {
        3: lambda m: (m, (M.loc_j(10) - 1) * m, 0),     # between two candidates
        7: lambda m: (m, (M.loc_j(0) + 2) * m, 0),      # j_{-1}
        11: lambda m: (m, M.loc_j(kp) * m, 0),          # j_{kPartProofs}
        15: lambda m: (m, 0x1234567 * m + 1, 0),        # unrelated
        19: lambda m: (0, M.loc_j(5) * m, 0),           # P the identity
        23: lambda m: (m, M.loc_j(6) * m, 2),           # incomplete P'
    }
    out, t = [], 0
    for b in range(kp + 6):
        m = 3 + 5 * b
        if b in special:
            pm, lm, lf = special[b](m)
            if pm:   # no candidate multiplier maps P to P'
                assert lf or all((M.loc_j(x) * pm - lm) % L for x in range(kp))
            out.append((pm, lm % L, lf, no))
        else:
            out.append((m, M.loc_j(t) * m % L, t & 1, t))   # bit 0 of lfail is not an obstacle
            t += 1
    assert t == kp
    return out


@pytest.mark.parametrize("nblk", [1, 33, "kPartProofs + 6"])
def test_locate(probe, nblk):
    """k_part_locate: loc == t where P' = [j_t] P, kPartNoLoc for a multiplier between two
    candidates, j_{-1}, j_{kPartProofs}, an unrelated point, P the identity and an incomplete
    P'; part is read through a permuted blocks[]; the block counts leave partial workgroups."""
    cases = _locate_cases()
    npart = len(cases)
    nblk = npart if isinstance(nblk, str) else nblk
    assert (nblk * K.kPartLocLanes) % 256 != 0
    blocks = [(b * 37 + 5) % npart for b in range(nblk)]
    assert len(set(blocks)) == nblk
    part = [77] * npart
    for b in range(nblk):
        part[blocks[b]] = cases[b][0]
    loc = np.full(nblk, 0x5555, np.uint16)
    rc = probe.partprobe_locate(
        _ll(nblk), _ll(npart), _ptr(_words([_enc_mul(m) for m in part])),
        _ptr(_words([_enc_mul(c[1]) for c in cases[:nblk]])), _ptr(np.array([c[2] for c in cases[:nblk]], np.uint8)),
        _ptr(np.array(blocks, np.uint32)), _ptr(loc))
    assert rc == 0
    assert loc.tolist() == [c[3] for c in cases[:nblk]]
