"""The MSM's integer model (tests/msm_model.py) against itself and against the probe's host-side
entry points: its identities, its geometry, and that every case the GPU probe tests list really
reaches the edge it is listed for, with the constants read from the built probe.  No GPU."""
import random

import numpy as np
import pytest

import digit_vectors as DV
import msm_model as M
import pyoracle as O

K, L = M.K, O.L


def test_constants_come_from_the_probe():
    assert K.kRlcWindows == 16 and K.kRlcBuckets == 1 << 15
    assert K.kRlcBuckets % K.kRlcCoarse == 0 and K.kRlcBuckets % K.kRlcSegLen == 0
    nseg = K.kRlcBuckets // K.kRlcSegLen
    assert nseg % K.kRlcWinQuads == 0
    # what the case list is written against: 32-bucket segments, 256 buckets per window quad, 128 per coarse bin
    assert K.kRlcSegLen == 32 and K.kRlcBuckets // K.kRlcWinQuads == 256 and K.kRlcBuckets // K.kRlcCoarse == 128
    assert K.kRlcMinChunk == 4 and K.kRlcChunk == 64 and K.kRlcSparsePts == 2048
    assert K.kRlcFineCap + 1 + 500 < M.FINE_NP   # the fine-cap cases keep entries outside the capped bin
    assert M.sparse_groups(1) == 4 and M.sparse_groups(K.kRlcSparsePts) == 16 <= K.kRlcSparseMaxGroups


def test_case_names():
    assert [c.name for c in M.cases()] == M.CASE_NAMES
    assert [c.name for c in M.cases() if c.both] == M.BOTH_CASES
    assert [c.name for c in M.cases() if c.chunks is not None] == M.SCALAR_CASES
    assert all(c.npts <= K.kRlcSparsePts for c in M.cases() if c.both)


def test_geometry_equals_the_probes():
    rng = random.Random(3)
    sweep = set(range(1, 4200))
    for k in range(11, 24):
        sweep |= {(1 << k) + d for d in (-2, -1, 0, 1, 2)}
    for g in range(1, K.kRlcSortGroups + 2):
        sweep |= {g * K.kRlcSortChunk + d for d in (-1, 0, 1)}
    sweep |= {rng.randrange(1, 1 << 24) for _ in range(2000)}
    sweep |= {c.npts for c in M.cases()}
    for npts in sorted(sweep):
        got = M.probe_geometry(npts)
        assert got == M.geometry(npts), npts
        g, chunk, e = got
        assert g * chunk >= npts and chunk % 64 == 0 and (g - 1) * chunk < npts
        assert -(-npts // e) <= max(-(-npts // K.kRlcChunk), K.kRlcMinHeads)
    # the ladder's steps
    steps = [n for n in range(1, 70000) if M.geometry(n)[2] != M.geometry(n + 1)[2]]
    assert steps == [8192, 16384, 32768, 65536]
    assert M.geometry(65536)[0] == 1 and M.geometry(65537)[0] == 2 and M.geometry(131073)[0] == 3


def test_dstride_equals_the_probes():
    lib = M.load_probe()
    for c in M.cases():
        assert lib.msmprobe_dstride(c.np, c.nextra, c.p0, c.e0) == c.dstride
        assert c.dstride % 8 == 0 and c.dstride >= c.e0 + c.nextra


def test_recode16_rows_is_digit_vectors():
    rng = random.Random(1)
    vals = [0, 1, L - 1, 1 << 252, (1 << 253) - 1, 0x8000 << 48, 0x7fff << 48] + [rng.randrange(1 << 253) for _ in range(300)]
    chunks = np.array([[(s >> (16 * w)) & 0xffff for w in range(16)] for s in vals], np.uint16)
    rows = M.recode16_rows(chunks)
    assert M.chunks_to_ints(chunks) == vals
    for s, r in zip(vals, rows.tolist()):
        assert r == DV.recode16(s) and M.row_value(r) == s


def test_pool():
    m, enc = M.pool()
    assert len(m) == len(set(m)) == M.POOL == 257 and enc.shape == (257, 8)
    for j in (0, 100, 256):
        assert enc[j].tobytes() == M.enc_mul(m[j])
    assert M.enc_mul(0) == M.enc_mul(L) == O.ristretto_encode(O.IDENTITY) == M.ZERO32


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_model_identities(name):
    c = M.case(name)
    off, idx = c.sorted
    nb = K.kRlcBuckets
    assert off.shape == (16, nb + 1) and np.all(off[:, 0] == 0) and np.all(np.diff(off, axis=1) >= 0)
    assert np.array_equal(off[:, nb], np.count_nonzero(c.F, axis=1))
    D = c.digits
    for w in range(16):
        tot = int(off[w, nb])
        row = idx[w, :tot].astype(np.int64)
        assert np.all(idx[w, tot:] == 0xffffffff)
        pid, neg = row & 0x7fffffff, row >> 31
        # every id names a point of the MSM whose digit (read where the kernels read it) lies in the bucket
        d = D[w, pid].astype(np.int64)
        assert np.array_equal(np.abs(d) - 1, np.repeat(np.arange(nb), np.diff(off[w])))
        assert np.array_equal(d < 0, neg == 1)
        assert np.array_equal(np.sort(pid), c.ids[np.nonzero(c.F[w])[0]])
        assert np.array_equal(c.canonical(w, idx[w]), row)
    # the values: the window sums recombine to the total, and to the scalars' own sum
    m = M.pool()[0]
    assert c.total_int == sum(v << (16 * w) for w, v in enumerate(c.window_ints)) % L
    if c.scalars is not None:
        assert len(c.scalars) == c.np and max(c.scalars) < 1 << 253
        assert c.total_int == sum(s * m[i % 257] for i, s in enumerate(c.scalars)) % L
        assert not c.F[:, c.np:].any()
        for i in (0, c.np // 2, c.np - 1):
            assert c.F[:, i].tolist() == DV.recode16(c.scalars[i])
    # small cases: the window sums term by term
    if c.npts <= 5000:
        for w in range(16):
            assert c.window_ints[w] == sum(int(x) * m[u % 257] for u, x in enumerate(c.F[w].tolist()) if x)


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_case_reaches_its_edge(name):
    c = M.case(name)
    f = c.facts
    assert c.claims, "a case must name what it is there for"
    for key, want in c.claims.items():
        if key in ("groups", "echunk", "sparse", "np_mod8", "p0_mod8", "partial_tile", "extras_nonzero", "unstaged",
                   "extra_signs", "max_span"):
            assert f[key] == want, (key, f[key], want)
        elif key == "min_span":
            assert f["max_span"] >= want, (key, f["max_span"])
        elif key == "max_nonempty":
            assert int(f["nonempty"].sum(axis=1).max()) == want
        elif key == "short_last_group":
            assert 0 < f["last_group"] < f["chunk"] and c.np + c.nextra > (f["groups"] - 1) * f["chunk"]
            # the extras lie in the last group, after the last whole 8-digit load of the points
            assert c.np > (f["groups"] - 1) * f["chunk"]
        elif key == "has_buckets":
            for w, b in want:
                assert f["nonempty"][w, b], (w, b)
        elif key == "has_segments":
            for w, s in want:
                assert f["nonempty"][w, s * K.kRlcSegLen:(s + 1) * K.kRlcSegLen].any(), (w, s)
        elif key == "has_quads":
            bpq = K.kRlcBuckets // K.kRlcWinQuads
            for w, q in want:
                assert f["nonempty"][w, q * bpq:(q + 1) * bpq].any(), (w, q)
        elif key == "region_at":
            (w, b), size = want
            assert int(f["region"][w, b]) == size
            assert (size <= K.kRlcFineCap) == ((w, b) not in f["unstaged"])
        elif key == "region_signs":
            w, b = want
            per = K.kRlcBuckets // K.kRlcCoarse
            d = c.F[w].astype(np.int64)
            inside = d[(np.abs(d) - 1) // per == b]
            assert (inside > 0).any() and (inside < 0).any()
        elif key == "decoys":
            mask = np.ones(c.dstride, bool)
            mask[c.ids] = False
            assert mask[:c.p0].all() and mask[c.p0 + c.np:c.e0].all() and c.e0 > c.p0 + c.np and c.p0 > 0
            assert np.all(c.digits[:, mask] != 0)
        elif key == "points_zero":
            assert not c.F[:, :c.np].any()
        elif key == "identity":
            assert c.total_int == 0 and sum(1 for v in c.window_ints if v % L) >= 4
            assert c.window_ints[0] % L and c.window_ints[9] == 0 and f["nonempty"][9, 4096]
        else:
            raise AssertionError("unknown claim %r" % key)


def test_ladder_straddles_every_step():
    for lo, hi in ((8192, 8193), (16384, 16385), (32768, 32769), (65536, 65537)):
        a, b = M.case("ladder_%d" % lo), M.case("ladder_%d" % hi)
        assert a.npts == lo and b.npts == hi and b.facts["echunk"] == 2 * a.facts["echunk"]
    assert M.case("weights_dense").npts == K.kRlcSparsePts + 1 and M.case("weights_sparse").npts == K.kRlcSparsePts
    # the same digit list on both sides of the sparse switch
    assert [x[1:] for x in M.weight_entries(2048)] == [x[1:] for x in M.weight_entries(2049)]


def test_reduce_refuses_what_it_cannot_check():
    """msmprobe_reduce checks its offsets and ids on the host before it touches the GPU: an id
    outside the supplied points (one past the extras, inside the gap, below p0, with or without
    bit 31), a falling offsets row, a total beyond the points, the sparse reduction above its
    limit, an echunk off the ladder -- hipErrorInvalidValue each, nothing launched."""
    INVALID = 1
    c = M.case("p0_1024")
    moff, midx = c.sorted
    w = int(np.argmax(moff[:, -1]))
    for bad_id in (c.e0 + c.nextra, c.p0 + c.np, c.p0 - 1, 0, 0x7fffffff, (c.e0 + c.nextra) | 0x80000000):
        for slot in (0, int(moff[w, -1]) - 1):
            idx = midx.copy()
            idx[w, slot] = bad_id
            assert M.probe_reduce(c, False, idx=idx)[0] == INVALID, (bad_id, slot)
    b = int(np.nonzero(np.diff(moff[w]))[0][1])
    off = moff.copy()
    off[w, b] = off[w, b + 1] + 1
    assert M.probe_reduce(c, False, off=off)[0] == INVALID
    off = moff.copy()
    off[w, -1] = c.npts + 1
    assert M.probe_reduce(c, False, off=off)[0] == INVALID
    off = moff.copy()
    off[w, 0] = 1
    assert M.probe_reduce(c, False, off=off)[0] == INVALID
    assert M.probe_reduce(c, True)[0] == INVALID                      # 4098 points: no sparse reduction
    small = M.case("weights_sparse")
    for e in (2, 3, 12, 128):
        assert M.probe_reduce(small, True, echunk=e)[0] == INVALID
