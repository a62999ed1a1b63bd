"""Python-integer model of the RLC batch check's prepare stage (csrc/rlc.hip: k_rlc_prepare,
k_rlc_prepare4, their pair-mode forms, k_rlc_bsum4, k_rlc_extra, k_rlc_extra_pairs), the named
cases of tests/test_gpu_prep_probe.py, and the loader of the probe (tests/native/prepprobe.hip).

The prepare turns (seed, first_index, c, s, four encodings, response status) per proof into

  * a decode-level status, by the precedence  bad point > bad scalar > identity r1 / r2 (unless
    eq_only) > zero s > OK;
  * 64 signed radix-2^16 digits: the r-points' are the weight's int16 words themselves (windows
    8..15 empty), the y-points' recode16(a c mod l) and recode16(b c mod l);
  * four negated affine Niels points (y - x, y + x, -2 d x y) mod p;
  * the products a s, b s mod l -- per proof in pair mode (`prod`), summed per 128 proofs
    otherwise (`block_sums`; the four-lane form sums 64 first, `quarter_sums`).

An entry whose status is not OK carries zero weight: all 64 digit slots zero, zero products.
Everything here is plain integers plus pyoracle's decode; nothing is taken from the code under
test.  The model, the cases and load_probe() need no GPU; tests/test_prep_model.py proves on
the CPU that every case reaches the edge it names.  CPZ_PREPPROBE=<path> selects another build of
the probe (a mutant).  Test infrastructure only."""
import ctypes
import functools
import hashlib
import importlib.util
import json
import os
import random
import struct
from types import SimpleNamespace

import numpy as np

import pyoracle as O
import scalar_vectors as SV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = O.P, O.L
M64 = (1 << 64) - 1
ST_OK, ST_BAD_POINT, ST_BAD_SCALAR, ST_IDENTITY, ST_ZERO_S = (O.ST_OK, O.ST_BAD_POINT, O.ST_BAD_SCALAR, O.ST_IDENTITY,
                                                              O.ST_ZERO_S)
PREP_BLOCK, SUM_BLOCK, QUARTER = 256, 128, 64   # checked against the probe's constants on the GPU
WIDE_MAX = 1 << 15
NIELS_BYTES = 128
_CONST = ["kRlcWindows", "kRlcPrepBlock", "kRlcSumBlock", "kRlcPrepWideMax", "kNielsEntriesRlc", "sizeof_ge_niels",
          "kStOk", "kStEqFail", "kStBadPoint", "kStBadScalar", "kStIdentity", "kStZeroS", "kStBadChallenge"]
LIMB_OFF = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230)   # radix 2^25.5


# ---- the probe --------------------------------------------------------------------------------------------

def probe_path():
    """The probe library: CPZ_PREPPROBE (a mutant build), or the in-tree one, built if stale."""
    path = os.environ.get("CPZ_PREPPROBE")
    if not path:
        spec = importlib.util.spec_from_file_location(
            "build_native", os.path.join(ROOT, "chaum-pedersen-zkp_amd", "build_native.py"))
        bn = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bn)
        path = bn.build_prepprobe()
    return path


@functools.lru_cache(maxsize=None)
def load_probe():
    lib = ctypes.CDLL(probe_path())
    ll, ull, vp, ci = ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_int
    lib.prepprobe_const.restype = ll
    lib.prepprobe_const.argtypes = [ci]
    lib.prepprobe_dstride.restype = ll
    lib.prepprobe_dstride.argtypes = [ll]
    lib.prepprobe_prepare.argtypes = [ci, ci, ll, ull] + [vp] * 8 + [ci] + [vp] * 7
    lib.prepprobe_extra.argtypes = [ll, vp, ll, ll, ll, ll, vp, vp, vp, vp]
    lib.prepprobe_extra_pairs.argtypes = [ll, vp, vp, ll, ll, ci, vp, ll, ll, vp, vp]
    lib.prepprobe_scalar.argtypes = [ci, ll, vp, vp, vp]
    return lib


def probe_consts():
    lib = load_probe()
    assert lib.prepprobe_const(len(_CONST)) == -1
    return {n: int(lib.prepprobe_const(i)) for i, n in enumerate(_CONST)}


def dstride_of(n):
    """The runtime's rounding of the digit rows (4 n points + 4 extra slots, whole 16-byte loads)
    plus the probe's eight spare columns."""
    return ((4 * n + 4 + 7) & ~7) + 8


# ---- integers <-> the kernels' words ------------------------------------------------------------------------

def words_of(vals, nbytes=32):
    """ints -> uint32[len][nbytes / 4], little-endian"""
    raw = b"".join(int(v).to_bytes(nbytes, "little") for v in vals)
    return np.frombuffer(raw, np.uint32).reshape(len(vals), nbytes // 4).copy()


def ints_of(words):
    """uint32[..., k] -> list of ints (row-major over the leading axes)"""
    w = np.ascontiguousarray(words, np.uint32)
    k = w.shape[-1]
    raw = w.tobytes()
    return [int.from_bytes(raw[4 * k * i:4 * k * (i + 1)], "little") for i in range(w.size // k)]


def fe_limbs(x):
    """x mod p as ten radix-2^25.5 limbs (26, 25, 26, ... bits), the form the kernels store"""
    x %= P
    out = []
    for k in range(10):
        width = 26 if k % 2 == 0 else 25
        out.append(x & ((1 << width) - 1))
        x >>= width
    return out


def niels_bytes(pt, neg=False, pad=0x5a5a5a5a):
    """An affine point as a ge_niels: (y + x, y - x, 2 d x y), or its negative's; 128 bytes."""
    x, y, z, _ = pt
    zi = pow(z, P - 2, P)
    x, y = x * zi % P, y * zi % P
    if neg:
        x = (-x) % P
    limbs = fe_limbs(y + x) + fe_limbs(y - x) + fe_limbs(O.D2 * x % P * y)
    return struct.pack("<30i2I", *limbs, pad, pad ^ 0xffffffff)


def niels_ints(pts):
    """int32[m][32] (ge_niels as stored) -> three lists of ints mod p: the fields in struct order
    (ypx, ymx, xy2d); the limbs are signed and may be loose.  The pad words are dropped."""
    a = np.ascontiguousarray(pts).view(np.int32).reshape(-1, 32).astype(object)
    out = []
    for f in range(3):
        acc = a[:, 10 * f] * 1
        for k in range(1, 10):
            acc = acc + a[:, 10 * f + k] * (1 << LIMB_OFF[k])
        out.append([int(v) % P for v in acc])
    return out


def point_of_niels(ypx, ymx, xy2d):
    """The affine point whose ge_niels fields these are; asserts xy2d = 2 d x y."""
    inv2 = (P + 1) // 2
    y, x = (ypx + ymx) * inv2 % P, (ypx - ymx) * inv2 % P
    assert xy2d == O.D2 * x % P * y % P, "xy2d is not 2 d x y"
    return (x, y, 1, x * y % P)


@functools.lru_cache(maxsize=None)
def decode(enc):
    return O.ristretto_decode(enc)


def neg_niels_triple(pt):
    """(y - x, y + x, -2 d x y) mod p of an affine point: the ge_niels of its negative"""
    x, y, _, _ = pt
    return ((y - x) % P, (y + x) % P, (-O.D2 * x * y) % P)


# ---- weights and digits -------------------------------------------------------------------------------------

def weight_halves(seed, index):
    """The 16 unsigned half-words the kernels split ChaCha20 block `index` (mod 2^64) into:
    a from the first eight, b from the next eight."""
    h = struct.unpack("<32H", O.chacha20_block(seed, index & M64))
    return h[:8], h[8:16]


def int16(h):
    return (h ^ 0x8000) - 0x8000


# ---- the model -----------------------------------------------------------------------------------------------

def entry_status(decodes, ident, st_in, eq_only):
    if not decodes:
        return ST_BAD_POINT
    if st_in == ST_BAD_SCALAR:
        return ST_BAD_SCALAR
    if ident and not eq_only:
        return ST_IDENTITY
    if st_in == ST_ZERO_S:
        return ST_ZERO_S
    return ST_OK


def prepare_model(b, first_index=None, rows=None):
    """The prepare of batch `b` (a case of this module).  Input statuses are what the batch path
    produces -- 0, bad scalar (3) or zero s (5): the internal kStBadChallenge comes only from
    cpz_verify_response, which never runs the prepare, so it is no input here.

    Per entry i: status[i]; live[i]; digits[w][4 i + q] for q = 0: -r1 (a), 1: -y1 (a c),
    2: -r2 (b), 3: -y2 (b c); niels[4 i + q] = (y - x, y + x, -2 d x y) mod p, or None where
    the encoding does not decode; prod[i] = (a s mod l, b s mod l), zero unless live.  Then
    block_sums[2 ceil(n / 256)] and quarter_sums[ceil(n / 64)], pairs of sums of prod mod l.
    `rows`: model these entries only (the sums are then not formed)."""
    n = b.n
    first = b.first_index if first_index is None else first_index
    which = range(n) if rows is None else rows
    m = SimpleNamespace(n=n, status={}, live={}, digits={}, niels={}, prod={}, weights={})
    for i in which:
        ha, hb = weight_halves(b.seed, first + i)
        wa, wb = SV.weight_value(ha), SV.weight_value(hb)
        m.weights[i] = (wa, wb)
        pts = [decode(b.enc[k][i]) for k in ("r1", "y1", "r2", "y2")]
        ident = b.enc["r1"][i] == bytes(32) or b.enc["r2"][i] == bytes(32)
        st = entry_status(all(p is not None for p in pts), ident, int(b.status_in[i]), b.eq_only)
        m.status[i], m.live[i] = st, st == ST_OK
        for q, p in enumerate(pts):
            m.niels[4 * i + q] = None if p is None else neg_niels_triple(p)
        if st == ST_OK:
            c, s = b.c[i], b.s[i]
            m.digits[i] = [[int16(h) for h in ha] + [0] * 8, SV.recode16_model(wa * c % L),
                           [int16(h) for h in hb] + [0] * 8, SV.recode16_model(wb * c % L)]
            m.prod[i] = (wa * s % L, wb * s % L)
        else:
            m.digits[i] = [[0] * 16] * 4
            m.prod[i] = (0, 0)
    if rows is None:
        def sums(block, count):
            out = []
            for k in range(count):
                part = [m.prod[i] for i in range(block * k, min(n, block * (k + 1)))]
                out.append((sum(p[0] for p in part) % L, sum(p[1] for p in part) % L))
            return out
        m.block_sums = sums(SUM_BLOCK, 2 * ((n + PREP_BLOCK - 1) // PREP_BLOCK))
        m.quarter_sums = sums(QUARTER, (n + QUARTER - 1) // QUARTER)
    return m


def model_digit_array(m):
    """int16[16][4 n] of a whole-batch model"""
    d = np.zeros((16, 4 * m.n), np.int16)
    for i in range(m.n):
        for q in range(4):
            d[:, 4 * i + q] = m.digits[i][q]
    return d


def digit_value(col):
    return sum(int(d) << (16 * w) for w, d in enumerate(col))


def weighted_sum(columns, points):
    """sum_j [sum_w d_jw 2^(16 w)] P_j over digit columns and affine points"""
    acc = O.IDENTITY
    for col, pt in zip(columns, points):
        v = digit_value(col)
        if v:
            acc = O.pt_add(acc, O.pt_mul(pt, v % L))
    return acc


# ---- cases -----------------------------------------------------------------------------------------------------

POOL = 61   # prime: the cycle lines up with no quarter, sum block or workgroup


@functools.lru_cache(maxsize=None)
def pool():
    """POOL encodings of valid, distinct, non-identity points"""
    step = O.pt_mul(O.generator_h(), 0x1234567)
    pt, out = O.pt_mul(O.BASEPOINT, 0xabcdef), []
    for _ in range(POOL):
        out.append(O.ristretto_encode(pt))
        pt = O.pt_add(pt, step)
    assert len(set(out)) == POOL and bytes(32) not in out
    return tuple(out)


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        return json.load(f)


def bad_encodings():
    return [bytes.fromhex(e) for e in golden()["rfc9496_bad"]]


def bad_kind(enc):
    """Why RFC 9496's decode refuses an encoding: the first check that fails."""
    s = int.from_bytes(enc, "little")
    if s >= P:
        return "non-canonical"
    if s & 1:
        return "negative"
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    v = (-(O.D * u1 % P * u1) - u2 * u2) % P
    sq, inv = O.sqrt_ratio_m1(1, v * u2 % P * u2)
    if not sq:
        return "non-square"
    dx = inv * u2 % P
    x = O.fe_abs(2 * s * dx)
    y = u1 * (inv * dx % P * v % P) % P
    if O.fe_is_negative(x * y):
        return "negative-t"
    assert y == 0
    return "zero-y"


SEED = hashlib.sha256(b"cpz-prep-probe").digest()
NONCANONICAL_S = (L + 1, 2**256 - 1, L + 12345, 2**255)   # none a multiple of l: a product kept by mistake shows


class Batch:
    """One prepare's inputs.  enc[k][i]: 32 bytes; s, c: ints; status_in: 0 / 3 / 5."""

    def __init__(self, name, n, first_index=0, eq_only=0, seed=SEED, rnd=None):
        rnd = rnd or random.Random(name)
        pl = pool()
        self.name, self.n, self.first_index, self.eq_only, self.seed = name, n, first_index, eq_only, seed
        self.enc = {k: [pl[rnd.randrange(POOL)] for _ in range(n)] for k in ("y1", "y2", "r1", "r2")}
        self.s = [rnd.randrange(1, L) for _ in range(n)]
        self.c = [rnd.randrange(L) for _ in range(n)]
        self.status_in = np.zeros(n, np.uint8)
        self.facts = {}

    def reject_scalar(self, i, k=0):
        self.status_in[i] = ST_BAD_SCALAR
        self.s[i] = NONCANONICAL_S[k % len(NONCANONICAL_S)]

    def zero_s(self, i):
        self.status_in[i] = ST_ZERO_S
        self.s[i] = 0

    def weights(self, i):
        ha, hb = weight_halves(self.seed, self.first_index + i)
        return SV.weight_value(ha), SV.weight_value(hb)

    def arrays(self, rows=None):
        """the probe's inputs: uint32[n][8] per row, uint8[n]; `rows`: entry i is row rows[i]"""
        idx = range(self.n) if rows is None else rows
        out = {k: np.frombuffer(b"".join(self.enc[k][i] for i in idx), np.uint32).reshape(-1, 8).copy()
               for k in ("y1", "y2", "r1", "r2")}
        out["s"] = words_of([self.s[i] for i in idx])
        out["c"] = words_of([self.c[i] for i in idx])
        out["status_in"] = np.ascontiguousarray(self.status_in[list(idx)])
        return out


SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)
BOUNDARY_REJECTS = (63, 127, 255)   # the last entry of a quarter, a sum block, a workgroup


def scan_min_half(seed, start, count):
    """The first index >= start whose block has the half-word 0x8000 (digit -2^15) among the 16
    that make the weights: a scan over indices, the seed fixed.  None if none within `count`."""
    for idx in range(start, start + count):
        ha, hb = weight_halves(seed, idx)
        if 0x8000 in ha or 0x8000 in hb:
            return idx
    return None


# scan_min_half(SEED, 0, 1 << 16), done once (about 16 / 65536 of the indices qualify);
# tests/test_prep_model.py repeats the scan
MIN_HALF_INDEX = 3740


def _size_case(n):
    b = Batch("size_%d" % n, n)
    for k, i in enumerate(BOUNDARY_REJECTS):
        if i < n:
            b.reject_scalar(i, k)
    b.facts = {"rejected": [i for i in BOUNDARY_REJECTS if i < n]}
    return b


def _product_digits():
    targets = SV.recode16_targets()
    b = Batch("product_digits", 2 * len(targets))
    for k, t in enumerate(targets):
        for half in range(2):
            i = 2 * k + half
            w = b.weights(i)[half]
            assert w % L != 0
            b.c[i] = t * pow(w, L - 2, L) % L
    b.facts = {"targets": targets}
    return b


def _mixed300():
    """Sum block 0: a_i s_i = l - 1 throughout; sum block 1: b_i s_i = l - 1 throughout (every
    sc_add of either tree wraps past l); then s = l - 1, s = 0 with status zero-s, a bad scalar,
    an undecodable r1, an identity r2, over a ragged tail."""
    n = 300
    b = Batch("mixed300", n)
    for i in range(256):
        w = b.weights(i)[i // SUM_BLOCK]
        assert w % L != 0
        b.s[i] = (L - 1) * pow(w, L - 2, L) % L
    bad = bad_encodings()
    for i in range(256, n):
        k = i % 4
        if k == 0:
            b.s[i] = L - 1
        elif k == 1:
            b.zero_s(i)
        elif k == 3 and i >= 280:
            j = (i - 280) // 4
            if j % 3 == 0:
                b.reject_scalar(i, j)
            elif j % 3 == 1:
                b.enc["r1"][i] = bad[j % len(bad)]
            else:
                b.enc["r2"][i] = bytes(32)
    return b


POSITIONS = ("y1", "y2", "r1", "r2")


def _status_table(eq_only):
    """The cross product of (no decode failure, or every undecodable encoding of the golden list
    at each of the four positions) x input status {0, 3, 5} x identity at {neither, r1, r2,
    both}; then identity at y1, y2 and both, which must stay OK.  An undecodable encoding
    replaces an identity at the same position."""
    combos = [(None, None)] + [(pos, e) for pos in POSITIONS for e in bad_encodings()]
    table = [(pos, e, st, idm) for (pos, e) in combos for st in (ST_OK, ST_BAD_SCALAR, ST_ZERO_S) for idm in range(4)]
    n = len(table) + 3
    b = Batch("status_table_eq%d" % eq_only, n, eq_only=eq_only, first_index=7 << 20)
    for i, (pos, e, st, idm) in enumerate(table):
        if idm & 1:
            b.enc["r1"][i] = bytes(32)
        if idm & 2:
            b.enc["r2"][i] = bytes(32)
        if pos is not None:
            b.enc[pos][i] = e
        if st == ST_BAD_SCALAR:
            b.reject_scalar(i, i)
        elif st == ST_ZERO_S:
            b.zero_s(i)
    for k, i in enumerate(range(len(table), n)):
        if k in (0, 2):
            b.enc["y1"][i] = bytes(32)
        if k in (1, 2):
            b.enc["y2"][i] = bytes(32)
    b.facts = {"table": table}
    return b


CLOSURE_FORGED, CLOSURE_BAD_POINT, CLOSURE_ZERO_S = (3, 11, 20), 7, 15


def _closure24():
    """24 real proofs under the default generators, their own Fiat-Shamir challenges as c: three
    forged (s + 1), one undecodable r1, one zero s."""
    n = 24
    b = Batch("closure24", n, first_index=1000)
    recs = [O.prove(O.bench_scalar(b"x", i, b"cpz-prep"), O.bench_scalar(b"k", i, b"cpz-prep")) for i in range(n)]
    for i in CLOSURE_FORGED:
        recs[i].s = O.scalar_bytes(int.from_bytes(recs[i].s, "little") + 1)
    recs[CLOSURE_BAD_POINT].r1 = bad_encodings()[6]
    recs[CLOSURE_ZERO_S].s = bytes(32)
    for i, r in enumerate(recs):
        for k in POSITIONS:
            b.enc[k][i] = getattr(r, k)
        b.s[i] = int.from_bytes(r.s, "little")
        b.c[i] = O.challenge(O.G_BYTES, O.H_BYTES, r.y1, r.y2, r.r1, r.r2, None)
    b.status_in[CLOSURE_ZERO_S] = ST_ZERO_S
    b.facts = {"recs": recs}
    return b


def _counter(name, n, first_index):
    return Batch(name, n, first_index=first_index)


_BUILDERS = {"product_digits": _product_digits, "mixed300": _mixed300,
             "status_table_eq0": lambda: _status_table(0), "status_table_eq1": lambda: _status_table(1),
             "closure24": _closure24,
             "counter_wrap32": lambda: _counter("counter_wrap32", 70, (1 << 32) - 3),
             "counter_2p63": lambda: _counter("counter_2p63", 9, (1 << 63) + 5),
             "counter_min_half": lambda: _counter("counter_min_half", 8, MIN_HALF_INDEX - 3)}
SIZE_CASES = tuple("size_%d" % n for n in SIZES)
CASE_NAMES = SIZE_CASES + ("counter_wrap32", "counter_2p63", "counter_min_half", "product_digits",
                           "mixed300", "status_table_eq0", "status_table_eq1", "closure24")
ALL_OK_CASES = ("size_1", "counter_wrap32", "counter_2p63", "counter_min_half", "product_digits")


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("size_"):
        return _size_case(int(name[5:]))
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def model(name):
    return prepare_model(case(name))


# ---- k_rlc_extra / k_rlc_extra_pairs ------------------------------------------------------------------------------

EXTRA_RANGES = ((0, 1), (0, 2), (1, 2), (3, 260), (0, 513), (5, 5))
EXTRA_NSUM = 520


@functools.lru_cache(maxsize=None)
def extra_sums():
    """EXTRA_NSUM block sums as the prepare can leave them: every third pair l - 1 (what the
    wrapping blocks of mixed300 give; a run of them makes every tree addition wrap), zeros
    (a block of rejected entries), random."""
    rnd = random.Random("extra")
    out = []
    for k in range(EXTRA_NSUM):
        if k % 3 == 0:
            out.append((L - 1, L - 1 - k))
        elif k % 7 == 0:
            out.append((0, rnd.randrange(L)))
        else:
            out.append((rnd.randrange(L), rnd.randrange(L)))
    return tuple(out)


def extra_model(sums, b0, b1):
    """the two digit columns of k_rlc_extra"""
    return [SV.recode16_model(sum(s[k] for s in sums[b0:b1]) % L) for k in range(2)]


PAIR_COUNTS = (1, 2, 64)
PAIR_EMPTY = (5, 63)          # of 64 pairs, these two own no entry
PAIR_RANGES = ((0, 300), (256, 300), (0, 1))
PAIR_N = 300


@functools.lru_cache(maxsize=None)
def pair_case(npairs):
    """prod[i] (zero for a zero-weight entry, l - 1 on every seventh), pair_idx[i], and 2 npairs
    points with distinct pad words"""
    rnd = random.Random("pairs%d" % npairs)
    prod, idx = [], []
    for i in range(PAIR_N):
        if i % 5 == 0:
            prod.append((0, 0))
        elif i % 7 == 0:
            prod.append((L - 1, L - 1))
        else:
            prod.append((rnd.randrange(L), rnd.randrange(L)))
        p = rnd.randrange(npairs)
        while npairs == 64 and p in PAIR_EMPTY:
            p = rnd.randrange(npairs)
        idx.append(p)
    gh = b"".join(niels_bytes(decode(pool()[(3 * j + 1) % POOL]), pad=0x01010101 * (j % 251 + 1))
                  for j in range(2 * npairs))
    return SimpleNamespace(npairs=npairs, prod=tuple(prod), idx=tuple(idx), gh=gh)


def pair_model(pc, lo, hi):
    """per pair: the two digit columns of k_rlc_extra_pairs over entries [lo, hi)"""
    out = []
    for p in range(pc.npairs):
        mine = [pc.prod[i] for i in range(lo, hi) if pc.idx[i] == p]
        out.append([SV.recode16_model(sum(v[k] for v in mine) % L) for k in range(2)])
    return out


# ---- calling the probe ---------------------------------------------------------------------------------------------

def _ptr(a):
    return a.ctypes.data


hip_failure = None   # the first entry point that returned a hipError_t other than hipSuccess


def _check(rc, what):
    global hip_failure
    if rc != 0 and hip_failure is None:
        hip_failure = "%s: hipError %d" % (what, rc)
    assert rc == 0, "%s: hipError %d" % (what, rc)


def probe_prepare(b, form, pairs, rows=None, first_index=None, eq_only=None):
    """prepprobe_prepare on a case (`rows`: entry i is the case's row rows[i], a tiling)"""
    lib = load_probe()
    a = b.arrays(rows)
    n = len(a["status_in"])
    ds = dstride_of(n)
    assert lib.prepprobe_dstride(n) == ds
    blocks, nq = (n + PREP_BLOCK - 1) // PREP_BLOCK, (n + QUARTER - 1) // QUARTER
    o = SimpleNamespace(n=n, dstride=ds, status=np.zeros(n, np.uint8), pts=np.zeros((4 * n, 32), np.int32),
                        digits=np.zeros((16, ds), np.int16), block_sums=np.zeros((2 * blocks, 2, 8), np.uint32),
                        prod=np.zeros((n, 2, 8), np.uint32), quarter_sums=np.zeros((nq, 2, 8), np.uint32),
                        any_bad=np.zeros(1, np.int32))
    seed = np.frombuffer(b.seed, np.uint32).copy()
    first = b.first_index if first_index is None else first_index
    rc = lib.prepprobe_prepare(form, pairs, n, first, _ptr(seed), _ptr(a["y1"]), _ptr(a["y2"]), _ptr(a["r1"]),
                               _ptr(a["r2"]), _ptr(a["s"]), _ptr(a["c"]), _ptr(a["status_in"]),
                               b.eq_only if eq_only is None else eq_only, _ptr(o.status), _ptr(o.pts), _ptr(o.digits),
                               _ptr(o.block_sums), _ptr(o.prod), _ptr(o.quarter_sums), _ptr(o.any_bad))
    _check(rc, "prepprobe_prepare")
    return o


def probe_extra(sums, b0, b1, e0, dstride, g, h):
    lib = load_probe()
    w = words_of([v for s in sums for v in s])
    pts, dig = np.zeros((2, 32), np.int32), np.zeros((16, dstride), np.int16)
    gb, hb = np.frombuffer(g, np.uint8).copy(), np.frombuffer(h, np.uint8).copy()
    rc = lib.prepprobe_extra(len(sums), _ptr(w), b0, b1, e0, dstride, _ptr(gb), _ptr(hb), _ptr(pts), _ptr(dig))
    _check(rc, "prepprobe_extra")
    return pts, dig


def probe_extra_pairs(pc, lo, hi, e0, dstride):
    lib = load_probe()
    w = words_of([v for s in pc.prod for v in s])
    idx = np.array(pc.idx, np.uint32)
    gh = np.frombuffer(pc.gh, np.uint8).copy()
    pts, dig = np.zeros((2 * pc.npairs, 32), np.int32), np.zeros((16, dstride), np.int16)
    rc = lib.prepprobe_extra_pairs(len(pc.idx), _ptr(w), _ptr(idx), lo, hi, pc.npairs, _ptr(gh), e0, dstride,
                                   _ptr(pts), _ptr(dig))
    _check(rc, "prepprobe_extra_pairs")
    return pts, dig


OPS = {"mul": 0, "add": 1, "neg": 2, "reduce_wide": 3, "is_canonical": 4, "weight": 5, "recode16": 6}


def probe_scalar(op, a, b=None):
    """prepprobe_scalar: a, b uint32[m][k]; returns uint32[m][8]"""
    lib = load_probe()
    m = a.shape[0]
    out = np.zeros((m, 8), np.uint32)
    rc = lib.prepprobe_scalar(OPS[op], m, _ptr(a), _ptr(b) if b is not None else None, _ptr(out))
    _check(rc, "prepprobe_scalar")
    return out
