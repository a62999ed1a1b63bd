"""Plain-integer model of the Pippenger MSM's sort and reduction (csrc/rlc.hip) and the case list
that tests/test_gpu_msm_probe.py drives through its kernels.

The model: rlc_sort_geometry, the per-window bucket offsets and sorted ids of a digit matrix, the
coarse-bin region sizes and the arm of k_rlc_fine each takes, the sparse flag, the chunks every
bucket spans, and the integers the window sums and the total stand for.  Every point is a known
multiple m_j of the basepoint (a pool of 257 of them, cycled over the flat positions: 257 is
prime, so the cycle lines up with no tile, chunk or group size), so an expected value is one
pt_mul on an integer.  The constants come from the probe library's getter
(tests/native/msmprobe.hip), which needs no GPU; CPZ_MSMPROBE=<path> selects another build (a
mutant).  tests/test_msm_model.py asserts the model's identities and that every listed case
reaches the edge it names.  Test infrastructure only."""
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
_CONST = ["kRlcWindows", "kRlcBuckets", "kRlcSegLen", "kRlcSortBlock", "kRlcSortGroups", "kRlcSortChunk", "kRlcChunk",
          "kRlcMinChunk", "kRlcMinHeads", "kRlcSparsePts", "kRlcCoarse", "kRlcTile", "kRlcFineCap", "kRlcWinQuads",
          "kRlcSparseMaxGroups"]


def probe_path():
    """The probe library: CPZ_MSMPROBE (a mutant build), or the in-tree one, built if stale."""
    path = os.environ.get("CPZ_MSMPROBE")
    if not path:
        spec = importlib.util.spec_from_file_location(
            "build_native", os.path.join(ROOT, "chaum-pedersen-zkp_amd", "build_native.py"))
        bn = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bn)
        path = bn.build_msmprobe()
    return path


@functools.lru_cache(maxsize=None)
def load_probe():
    lib = ctypes.CDLL(probe_path())
    ll, vp, ci = ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int
    lib.msmprobe_const.restype = ll
    lib.msmprobe_const.argtypes = [ci]
    lib.msmprobe_geometry.argtypes = [ll, vp]
    lib.msmprobe_dstride.restype = ll
    lib.msmprobe_dstride.argtypes = [ll, ll, ll, ll]
    lib.msmprobe_sort.argtypes = [ll, ll, ll, ll, vp, vp, vp]
    lib.msmprobe_reduce.argtypes = [ll, ll, ll, ll, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]
    return lib


class _Consts:
    """The probe's constants, read on first use: never while pytest collects, so that no HIP
    library is loaded before the tests that need one run."""

    def __getattr__(self, name):
        if name not in _CONST:
            raise AttributeError(name)
        lib = load_probe()
        for i, n in enumerate(_CONST):
            self.__dict__[n] = int(lib.msmprobe_const(i))
        assert lib.msmprobe_const(len(_CONST)) == -1
        return self.__dict__[name]


K = _Consts()   # K.kRlcBuckets, ...


# ---- geometry ------------------------------------------------------------------------------------

def geometry(npts):
    """rlc_sort_geometry: (groups, chunk, echunk) for an MSM of npts points."""
    g = min(max(-(-npts // K.kRlcSortChunk), 1), K.kRlcSortGroups)
    chunk = (-(-npts // g) + 63) & ~63
    e = K.kRlcMinChunk
    while e < K.kRlcChunk and e * K.kRlcMinHeads < npts:
        e <<= 1
    return g, chunk, e


def probe_geometry(npts):
    out = (ctypes.c_longlong * 3)()
    assert load_probe().msmprobe_geometry(npts, ctypes.addressof(out)) == 0
    return tuple(int(x) for x in out)


def dstride_of(np_, nextra, p0, e0):
    """The digit rows' stride the probe assumes (msmprobe_dstride)."""
    return (e0 + nextra + 7) & ~7


def sparse_groups(npts):
    """launch_rlc_msm's workgroups per window of the sparse reduction."""
    return min(K.kRlcSparseMaxGroups, max(4, (npts + 127) // 128))


# ---- points: a pool of known multiples of the basepoint --------------------------------------------

POOL = 257
ZERO32 = bytes(32)


@functools.lru_cache(maxsize=None)
def pool():
    """(m, enc): 257 random multipliers and the encodings of [m_j] B as uint32[257][8]."""
    rng = random.Random(20261020)
    m = [rng.randrange(1, L) for _ in range(POOL)]
    enc = b"".join(O.ristretto_encode(O.pt_mul(O.BASEPOINT, x)) for x in m)
    return m, np.frombuffer(enc, dtype="<u4").reshape(POOL, 8).copy()


def enc_mul(k):
    """enc([k mod l] B)"""
    k %= L
    return ZERO32 if k == 0 else O.ristretto_encode(O.pt_mul(O.BASEPOINT, k))


# ---- digits ----------------------------------------------------------------------------------------

def recode16_rows(chunks):
    """rlc_dev.h recode16 of scalars given as their sixteen 16-bit words, uint16[n][16] ->
    int64[n][16] (the scalar recoding of digit_vectors.recode16, a row at a time)."""
    c = np.asarray(chunks, dtype=np.int64)
    out = np.empty_like(c)
    carry = np.zeros(c.shape[0], np.int64)
    for w in range(16):
        v = c[:, w] + carry
        carry = (v + 0x8000) >> 16
        out[:, w] = v - (carry << 16)
    assert not carry.any(), "a scalar of 2^255 or more"
    return out


def chunks_to_ints(chunks):
    raw = np.ascontiguousarray(chunks, dtype="<u2").tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(chunks))]


def row_value(row):
    """The integer a column of radix-2^16 digits stands for."""
    return sum(int(d) << (16 * w) for w, d in enumerate(row))


DECOYS = (12345, -777, 1, -32768)   # digits outside the MSM's ranges: must not be counted


class Case:
    """One MSM: np_ points at p0.., nextra extras at e0.., and the flat digit matrix
    F int16[16][np_ + nextra] over the flat positions t (the points, then the extras).
    `chunks` (uint16[n][16], scalars) makes a case that cpz_msm can run too: F is their recoding,
    p0 = 0 and the two extras carry zero digits.  `claims` names the edge the case is there for
    (facts() keys and the values they must have)."""

    def __init__(self, name, edge, np_, nextra, build=None, chunks=None, p0=0, gap=0, claims=None, both=False):
        self.name, self.edge, self.np, self.nextra, self.p0 = name, edge, np_, nextra, p0
        self.e0 = p0 + np_ + gap
        self.npts = np_ + nextra
        self._build, self._chunks = build, chunks
        self.claims = claims or {}
        self.both = both           # small enough for either reduction: run both
        assert (build is None) != (chunks is None)
        assert chunks is None or (p0 == 0 and nextra == 2)

    def __repr__(self):
        return self.name

    @functools.cached_property
    def chunks(self):
        return None if self._chunks is None else np.asarray(self._chunks(), dtype=np.uint16)

    @functools.cached_property
    def F(self):
        if self._build is not None:
            F = np.asarray(self._build(self), dtype=np.int64)
        else:
            assert self.chunks.shape == (self.np, 16)
            F = np.zeros((16, self.npts), np.int64)
            rows = recode16_rows(self.chunks)
            for i in (0, self.np // 2, self.np - 1):    # the vectorised recoding against the scalar one
                assert rows[i].tolist() == DV.recode16(chunks_to_ints(self.chunks[i:i + 1])[0])
            F[:, :self.np] = rows.T
        assert F.shape == (16, self.npts) and F.min() >= -32768 and F.max() <= 32767
        return F.astype(np.int16)

    @functools.cached_property
    def ids(self):
        """msm_point: the point id of flat position t"""
        t = np.arange(self.npts, dtype=np.int64)
        return np.where(t < self.np, self.p0 + t, self.e0 + (t - self.np))

    @property
    def dstride(self):
        return dstride_of(self.np, self.nextra, self.p0, self.e0)

    @functools.cached_property
    def digits(self):
        """int16[16][dstride] as the kernels see it: decoys everywhere outside the two ranges"""
        D = np.empty((16, self.dstride), np.int16)
        D[:] = np.resize(np.array(DECOYS, np.int16), self.dstride)
        D[:, self.ids] = self.F
        return D

    @functools.cached_property
    def enc(self):
        """uint32[npts][8]: flat position t is the point [m_(t mod 257)] B"""
        return pool()[1][np.arange(self.npts) % POOL].copy()

    # -- the sort --
    @functools.cached_property
    def sorted(self):
        """(offsets int64[16][kRlcBuckets + 1], idx uint32[16][npts]): every bucket's ids in
        ascending order, bit 31 = negative digit; the rows' tails are 0xffffffff."""
        nb = K.kRlcBuckets
        offsets = np.zeros((16, nb + 1), np.int64)
        idx = np.full((16, self.npts), 0xffffffff, np.uint32)
        for w in range(16):
            d = self.F[w].astype(np.int64)
            t = np.nonzero(d)[0]
            b = np.abs(d[t]) - 1
            val = self.ids[t] | np.where(d[t] < 0, 1 << 31, 0)
            order = np.lexsort((val, b))
            idx[w, :t.size] = val[order]
            offsets[w, 1:] = np.cumsum(np.bincount(b, minlength=nb))
        return offsets, idx

    def canonical(self, w, row):
        """a window's returned idx row with the ids inside every bucket put in ascending order"""
        off = self.sorted[0][w]
        total = int(off[-1])
        key = np.repeat(np.arange(K.kRlcBuckets), np.diff(off))
        seg = np.asarray(row[:total], dtype=np.int64)
        return seg[np.lexsort((seg, key))]

    # -- what the case reaches --
    @functools.cached_property
    def facts(self):
        g, chunk, e = geometry(self.npts)
        off = self.sorted[0]
        per = K.kRlcBuckets // K.kRlcCoarse
        region = off[:, per::per] - off[:, :-1:per]                  # [16][kRlcCoarse]
        s, en = off[:, :-1], off[:, 1:]
        span = np.where(en > s, (en - 1) // e - s // e, 0)           # heads k_rlc_bucket_fix adds per bucket
        return {
            "groups": g, "chunk": chunk, "echunk": e,
            "sparse": self.npts <= K.kRlcSparsePts,
            "np_mod8": self.np % 8, "p0_mod8": self.p0 % 8,
            "last_group": self.npts - (g - 1) * chunk,
            "partial_tile": chunk % K.kRlcTile != 0,
            "region": region,
            "unstaged": {(int(w), int(c)) for w, c in np.argwhere(region > K.kRlcFineCap)},
            "max_span": int(span.max()),
            "nonempty": en > s,                                      # [16][kRlcBuckets]
            "extras_nonzero": bool(self.F[:, self.np:].any()),
            "extra_signs": {int(x) for x in np.sign(self.F[:, self.np:]).reshape(-1)} - {0},
        }

    # -- the values --
    @functools.cached_property
    def window_ints(self):
        """[sum_t F[w][t] m_(t mod 257) for w]"""
        m = pool()[0]
        j = np.arange(self.npts) % POOL
        out = []
        for w in range(16):
            s = np.bincount(j, weights=self.F[w].astype(np.float64), minlength=POOL)   # exact: |sum| < 2^53
            out.append(sum(int(x) * mj for x, mj in zip(s.tolist(), m) if x))
        return out

    @functools.cached_property
    def total_int(self):
        return sum(v << (16 * w) for w, v in enumerate(self.window_ints)) % L

    @functools.cached_property
    def scalars(self):
        return None if self.chunks is None else chunks_to_ints(self.chunks)


# ---- the probe's entry points ----------------------------------------------------------------------

def _ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


def probe_sort(c):
    """msmprobe_sort on a case: (offsets uint32[16][kRlcBuckets + 1], idx uint32[16][npts])"""
    off = np.full((16, K.kRlcBuckets + 1), 0xffffffff, np.uint32)
    idx = np.full((16, c.npts), 0xffffffff, np.uint32)
    rc = load_probe().msmprobe_sort(c.np, c.nextra, c.p0, c.e0, _ptr(c.digits), _ptr(off), _ptr(idx))
    assert rc == 0, "msmprobe_sort: hipError %d" % rc
    return off, idx


def probe_reduce(c, sparse, off=None, idx=None, echunk=None):
    """msmprobe_reduce on a case, fed the model's offsets and ids unless others are given:
    (rc, win_enc uint32[16][8], partial, identity, partial16, identity16)"""
    moff, midx = c.sorted
    off = np.ascontiguousarray(moff if off is None else off, dtype=np.uint32)
    idx = np.ascontiguousarray(midx if idx is None else idx, dtype=np.uint32)
    win = np.full((16, 8), 0xffffffff, np.uint32)
    part, part16 = np.full(8, 0xffffffff, np.uint32), np.full(8, 0xffffffff, np.uint32)
    ident, ident16 = np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    rc = load_probe().msmprobe_reduce(c.np, c.nextra, c.p0, c.e0, _ptr(c.enc), _ptr(off), _ptr(idx),
                                      echunk or c.facts["echunk"], int(sparse), _ptr(win), _ptr(part), _ptr(ident),
                                      _ptr(part16), _ptr(ident16))
    return rc, win, part, ident, part16, ident16


# ---- the case list -----------------------------------------------------------------------------------

WEIGHT_WINDOWS = (0, 7, 8, 15)
# segment boundaries (kRlcSegLen = 32: values 32 | 33), the quad boundaries of k_rlc_window
# (256 buckets per quad: 256 | 257, and 256 * 127 + 1, the first value of the last quad), the ends
WEIGHT_DIGITS = [s * v for v in (1, 31, 32, 33, 255, 256, 257, 256 * 127 + 1) for s in (1, -1)] + [32767, -32768]
TOP_WEIGHT_DIGITS = [s * v for v in (1, 31, 32, 33, 255, 256, 257, 256 * 31 + 1, 8192) for s in (1, -1)]  # <= 2^13


def weight_entries(npts):
    """[(t, window, digit)]: one point per (window, digit), spread over the flat positions; the last
    two positions (the extras) carry one digit of each sign."""
    out, i = [], 0
    for w in WEIGHT_WINDOWS:
        for d in (TOP_WEIGHT_DIGITS if w == 15 else WEIGHT_DIGITS):
            out.append(((i * 29) % (npts - 2), w, d))
            i += 1
    assert len({t for t, _, _ in out}) == len(out)
    return out + [(npts - 2, 0, -255), (npts - 1, 8, 257)]


def _weights_build(case):
    F = np.zeros((16, case.npts), np.int64)
    for t, w, d in weight_entries(case.npts):
        F[w, t] = d
    return F


def _weights_chunks(n):
    """the same list as scalars, where a scalar below 2^253 has the digit: every window below the
    top one (a negative digit carries 1 into the next window), the top one's positive digits"""
    def make():
        c = np.zeros((n, 16), np.int64)
        for t, w, d in weight_entries(n + 2):
            if t < n and (w < 15 or 0 < d < 8192):      # 8192 in the top window is 2^253
                c[t, w] = d & 0xffff
        return c
    return make


def _weights_claims(sparse):
    return {"sparse": sparse, "echunk": 4, "groups": 1,
            "has_buckets": {(w, abs(d) - 1) for w in WEIGHT_WINDOWS
                            for d in (TOP_WEIGHT_DIGITS if w == 15 else WEIGHT_DIGITS)},
            "has_segments": {(w, s) for w in (0, 7, 8) for s in (0, 1, 7, 8, 1016, 1023)},
            "has_quads": {(w, q) for w in (0, 7, 8) for q in (0, 1, 127)} | {(15, 0), (15, 1), (15, 31)},
            "extras_nonzero": True, "extra_signs": {1, -1}}


def _distinct_build(case):
    F = np.zeros((16, case.npts), np.int64)
    t = np.arange(case.npts)
    F[5] = (16 * t + 1) * np.where(t & 1, -1, 1)
    return F


def _one_bucket_build(case):
    F = np.zeros((16, case.npts), np.int64)
    t = np.arange(case.npts)
    F[2] = 77 * np.where(t % 3 == 0, -1, 1)
    return F


def _one_bucket_chunks(n):
    def make():
        c = np.zeros((n, 16), np.int64)
        c[:, 2] = 77
        return c
    return make


LADDER_WINDOW, LADDER_DIGIT = 6, 1000


def _ladder_build(case):
    rng = np.random.default_rng(case.npts)
    F = rng.integers(-32768, 32768, size=(16, case.npts))
    heavy = rng.random(case.npts) < 0.9
    F[LADDER_WINDOW] = np.where(heavy, np.where(rng.random(case.npts) < 0.5, -LADDER_DIGIT, LADDER_DIGIT),
                                F[LADDER_WINDOW])
    return F


def _uniform_build(case):
    rng = np.random.default_rng(case.npts + 7 * case.p0)
    F = rng.integers(-32768, 32768, size=(16, case.npts))
    F[:, case.np:] = np.where(F[:, case.np:] == 0, 5, F[:, case.np:])   # the extras: every digit non-zero ...
    F[0, case.np], F[0, case.npts - 1] = -4242, 4242                  # ... and both signs
    return F


def _uniform_chunks(n, heavy=False):
    def make():
        rng = np.random.default_rng(n)
        c = rng.integers(0, 65536, size=(n, 16))
        c[:, 15] &= 0x0fff                                              # below 2^252
        if heavy:
            c[:, LADDER_WINDOW] = np.where(rng.random(n) < 0.9, LADDER_DIGIT, c[:, LADDER_WINDOW])
        return c
    return make


FINE_WINDOW, FINE_NP = 3, 20000


def _fine_chunks(last_bin, count):
    """`count` scalars whose window-3 digit lies in coarse bin 0 (values 1..128) or 255 (values
    32641..32768), both signs; the other FINE_NP - count in the neighbouring bin (129.. or 32640)."""
    def make():
        i = np.arange(FINE_NP)
        base = 32641 if last_bin else 1
        v = base + i % 128
        neg = (i % 3 == 0) | (v == 32768)                                # 32768 exists as -32768 only
        rest = (32640 - i % 2) if last_bin else (129 + i % 5)            # bucket 127 | 128 straddles the bin edge
        v = np.where(i < count, v, rest)
        c = np.zeros((FINE_NP, 16), np.int64)
        c[:, FINE_WINDOW] = np.where(neg, 65536 - v, v)
        return c
    return make


def _extras_build(case):
    F = np.zeros((16, case.npts), np.int64)
    ds = WEIGHT_DIGITS
    for j in range(case.nextra):
        w = j % 16
        F[w, case.np + j] = (TOP_WEIGHT_DIGITS if w == 15 else ds)[(j // 16 + 5 * w) % 18]
    return F


def _identity_build(case):
    """The total is the identity with no empty window sum behind it: P in one bucket against the
    same P (257 positions on) in others."""
    F = np.zeros((16, case.npts), np.int64)
    F[0, 3], F[0, 3 + POOL], F[0, 3 + 2 * POOL] = 6, -2, -4              # window 0 alone sums to nothing
    F[1, 10], F[0, 10 + POOL], F[0, 10 + 2 * POOL] = 1, -32768, -32768   # 2^16 P - 2 * 2^15 P
    F[15, 20], F[14, 20 + POOL], F[14, 20 + 2 * POOL] = 1, -32768, -32768
    F[9, 30], F[9, 30 + POOL] = 4097, -4097                              # one bucket, P and -P
    return F


@functools.lru_cache(maxsize=None)
def cases():
    cap = K.kRlcFineCap
    sp = K.kRlcSparsePts
    out = [
        Case("weights_dense", "k_rlc_segment / k_rlc_window multipliers on chosen digits", sp - 1, 2,
             build=_weights_build, claims=_weights_claims(False)),
        Case("weights_sparse", "the same digits through k_rlc_window_sparse", sp - 2, 2, build=_weights_build,
             claims=_weights_claims(True), both=True),
        Case("weights_dense_scalars", "the weight digits a scalar can carry, dense", sp - 1, 2,
             chunks=_weights_chunks(sp - 1), claims={"sparse": False, "has_quads": {(0, 127), (8, 127), (15, 31)}}),
        Case("weights_sparse_scalars", "the weight digits a scalar can carry, sparse", sp - 2, 2,
             chunks=_weights_chunks(sp - 2), claims={"sparse": True, "has_quads": {(0, 127), (8, 127), (15, 31)}}),
        Case("sparse_distinct", "kRlcSparsePts non-empty buckets in one window", sp - 2, 2, build=_distinct_build,
             claims={"sparse": True, "max_nonempty": sp, "extras_nonzero": True}, both=True),
        Case("sparse_one_bucket", "every point in one bucket: 512 chunks of 4", sp - 2, 2, build=_one_bucket_build,
             claims={"sparse": True, "echunk": 4, "max_span": sp // 4 - 1, "max_nonempty": 1}, both=True),
        Case("one_bucket_scalars", "one bucket of 2046 entries through cpz_msm", sp - 2, 2,
             chunks=_one_bucket_chunks(sp - 2), claims={"sparse": True, "max_span": (sp - 2 - 1) // 4}),
    ]
    for npts, e in ((8192, 4), (8193, 8), (16384, 8), (16385, 16), (32768, 16), (32769, 32), (65536, 32), (65537, 64)):
        out.append(Case("ladder_%d" % npts, "echunk = %d; one bucket over hundreds of chunks" % e, npts - 2, 2,
                        build=_ladder_build,
                        claims={"echunk": e, "min_span": 300, "groups": 2 if npts > 65536 else 1, "sparse": False,
                                "extras_nonzero": True}))
    for npts in (8193, 65537):
        out.append(Case("ladder_scalars_%d" % npts, "random scalars, 90 %% with one digit in window 6", npts - 2, 2,
                        chunks=_uniform_chunks(npts - 2, heavy=True),
                        claims={"echunk": geometry(npts)[2], "min_span": 300}))
    for last_bin in (0, 1):
        c = (K.kRlcCoarse - 1) if last_bin else 0
        for extra in (0, 1):
            out.append(Case("fine_bin%d_cap%s" % (c, "+1" if extra else ""),
                            "a region of kRlcFineCap%s entries: %s arm" % (" + 1" if extra else "",
                                                                         "unstaged" if extra else "staged"),
                            FINE_NP, 2, chunks=_fine_chunks(last_bin, cap + extra),
                            claims={"region_at": ((FINE_WINDOW, c), cap + extra),
                                    "unstaged": {(FINE_WINDOW, c)} if extra else set(),
                                    "has_buckets": {(FINE_WINDOW, 32639), (FINE_WINDOW, 32640), (FINE_WINDOW, 32767)}
                                    if last_bin else {(FINE_WINDOW, 0), (FINE_WINDOW, 127), (FINE_WINDOW, 128)},
                                    "region_signs": (FINE_WINDOW, c)}))
    out += [
        Case("groups2_np65541", "two sort groups, np % 8 = 5, extras in the scalar tail", 65541, 2, build=_uniform_build,
             claims={"groups": 2, "np_mod8": 5, "partial_tile": True, "short_last_group": True, "extras_nonzero": True,
                     "extra_signs": {1, -1}}),
        Case("groups2_np65535", "the last vector load against the point range's end", 65535, 2, build=_uniform_build,
             claims={"groups": 2, "np_mod8": 7, "partial_tile": True, "short_last_group": True}),
        Case("groups3_np131075", "three sort groups, np % 8 = 3", 131075, 2, build=_uniform_build,
             claims={"groups": 3, "np_mod8": 3, "partial_tile": True, "short_last_group": True, "extras_nonzero": True}),
        Case("groups3_np131072", "three sort groups, np % 8 = 0", 131072, 2, build=_uniform_build,
             claims={"groups": 3, "np_mod8": 0, "partial_tile": True, "short_last_group": True}),
        Case("groups2_scalars", "two sort groups through cpz_msm", 65541, 2, chunks=_uniform_chunks(65541),
             claims={"groups": 2, "np_mod8": 5}),
        Case("groups3_scalars", "three sort groups through cpz_msm", 131075, 2, chunks=_uniform_chunks(131075),
             claims={"groups": 3}),
        Case("p0_1024", "a leaf's range: p0 = 1024, extras beyond a gap, decoys around", 4096, 2, build=_uniform_build,
             p0=1024, gap=1024, claims={"p0_mod8": 0, "sparse": False, "decoys": True, "extras_nonzero": True}),
        Case("p0_2048", "p0 = 2048", 4096, 2, build=_uniform_build, p0=2048, gap=1024,
             claims={"p0_mod8": 0, "decoys": True, "extras_nonzero": True}),
        Case("p0_1028", "p0 no multiple of 8: the one-at-a-time digit loads alone", 4096, 2, build=_uniform_build,
             p0=1028, gap=1020, claims={"p0_mod8": 4, "decoys": True}),
        Case("extras128_sparse", "128 extras with chosen digits, the points empty", sp - 128, 128, build=_extras_build,
             gap=64, claims={"sparse": True, "extras_nonzero": True, "extra_signs": {1, -1}, "points_zero": True},
             both=True),
        Case("extras128_dense", "128 extras with chosen digits, dense", 4096, 128, build=_extras_build,
             claims={"sparse": False, "extras_nonzero": True, "extra_signs": {1, -1}, "points_zero": True}),
        Case("identity_total", "P against -P in other buckets: the total is the identity", 600, 2,
             build=_identity_build, claims={"identity": True}, both=True),
    ]
    assert len({c.name for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


CASE_NAMES = [
    "weights_dense", "weights_sparse", "weights_dense_scalars", "weights_sparse_scalars", "sparse_distinct",
    "sparse_one_bucket", "one_bucket_scalars", "ladder_8192", "ladder_8193", "ladder_16384", "ladder_16385",
    "ladder_32768", "ladder_32769", "ladder_65536", "ladder_65537", "ladder_scalars_8193", "ladder_scalars_65537",
    "fine_bin0_cap", "fine_bin0_cap+1", "fine_bin255_cap", "fine_bin255_cap+1", "groups2_np65541", "groups2_np65535",
    "groups3_np131075", "groups3_np131072", "groups2_scalars", "groups3_scalars", "p0_1024", "p0_2048", "p0_1028",
    "extras128_sparse", "extras128_dense", "identity_total"]
SCALAR_CASES = [n for n in CASE_NAMES if "scalars" in n or n.startswith("fine_")]
# reduce runs: every case in the reduction its size selects, the small ones in the other too
BOTH_CASES = ["weights_sparse", "sparse_distinct", "sparse_one_bucket", "extras128_sparse", "identity_total"]
