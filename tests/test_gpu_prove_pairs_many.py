"""The prover over up to 4096 (g, h) pairs in one call (cpz_prove_pairs_many[_device]): above
CPZ_PAIRS_MAX pairs the descriptors are built on the device, every pair gets small tables (multiples
0..8 of g, 2^128 g, h, 2^128 h) in one launch, and every proof's four points come from its own
pair's small tables on four lanes (k_prove_points_micro); no 128-entry set is built and the
light-set cache is not touched.

Row i of every output must be byte for byte what cpz_prove writes for (x_i, k_i, context i) under
pairs[pair_idx[i]].  The expected rows come from code this feature does not touch: Gpu.prove_pairs in
runs of at most 64 pairs (the route the call replaces), Gpu.prove per pair for the digit edges of
tests/prove_many_cases.py, and the Python oracle's prove for a sample.  Pairs are made as in
tests/test_gpu_batch_pairs_many.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import chaum_pedersen as cp
import pyoracle as O
import test_gpu_batch_pairs as B
import test_gpu_batch_pairs_many as BM
from chaum_pedersen import _native
from prove_many_cases import EDGES, random_scalar

pytestmark = pytest.mark.gpu

Q = B.Q
BAD_POINT = B.BAD_POINT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARBASE = "generators_varbase"
PAIRS_MAX = 64


def _scalars(n, tag):
    xs = np.frombuffer(b"".join(O.scalar_bytes(random_scalar(tag + b"-x", i)) for i in range(n)), np.uint8)
    ks = np.frombuffer(b"".join(O.scalar_bytes(random_scalar(tag + b"-k", i)) for i in range(n)), np.uint8)
    return xs.reshape(n, 32).copy(), ks.reshape(n, 32).copy()


def _runs64(gpu, pairs, idx, xs, ks, ctxs):
    """The same entries through Gpu.prove_pairs, 64 pairs per call on gathered rows."""
    idx = np.asarray(idx, np.int64)
    rows = {q: np.zeros((len(idx), 32), np.uint8) for q in Q}
    for c in range(0, len(pairs), PAIRS_MAX):
        sel = np.nonzero((idx >= c) & (idx < c + PAIRS_MAX))[0]
        if not len(sel):
            continue
        out = gpu.prove_pairs(pairs[c:c + PAIRS_MAX], idx[sel] - c, np.ascontiguousarray(xs[sel]),
                              np.ascontiguousarray(ks[sel]), contexts=None if ctxs is None else [ctxs[i] for i in sel])
        for q in Q:
            rows[q][sel] = out[q]
    return rows


def _same(got, exp, n=None):
    for q in Q:
        g, e = got[q], exp[q] if n is None else exp[q][:n]
        bad = np.nonzero((g != e).any(axis=1))[0]
        assert bad.size == 0, (q, bad[:8].tolist())


def _resident(g, pairs):
    """pairs_resident over any number of rows (the call takes PAIRS_MAX at a time)."""
    return np.concatenate([g.pairs_resident(pairs[c:c + PAIRS_MAX]) for c in range(0, len(pairs), PAIRS_MAX)])


def _gh(pairs):
    return np.frombuffer(b"".join(p.g + p.h for p in pairs), np.uint8).copy()


@pytest.fixture(scope="module")
def pool(gpu):
    """200 distinct pairs."""
    return BM._many_pairs(gpu, 200, b"prove-many-pool")


@pytest.fixture(scope="module")
def mix65(gpu, pool):
    """130 entries over 65 pairs, entry i under pair i % 65, contexts cycling the four shapes; the
    expected rows from two prove_pairs runs (64 pairs, then one), computed once."""
    pairs = pool[:65]
    idx = (np.arange(130) % 65).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(130)]
    xs, ks = _scalars(130, b"m65")
    return pairs, idx, ctxs, xs, ks, _runs64(gpu, pairs, idx, xs, ks, ctxs)


# ---- 1. n = 130 over 65 pairs: the smallest call that does not forward -------------------------------

def test_smallest_call_that_does_not_forward(gpu, mix65):
    pairs, idx, ctxs, xs, ks, exp = mix65
    assert [type(c) for c in ctxs[:4]] == [type(None), bytes, bytes, bytes] and [len(c) for c in ctxs[1:4]] == [32, 5, 0]
    with cp.Gpu(0) as fresh:
        assert not _resident(fresh, pairs).any()
        fb = fresh.fallback_stats()
        fresh.set_timing(True)
        fresh.stage_times()
        got = fresh.prove_pairs_many(pairs, idx, xs, ks, contexts=ctxs)
        times = fresh.stage_times()
        _same(got, exp)
        assert times[VARBASE][1] == 65, times                      # one span that counts the pairs
        assert "generators" not in times, times                    # no comb
        assert times["prove"][1] == 2, times                       # the points; challenges + responses
        assert not _resident(fresh, pairs).any()                   # no set was built or cached
        again = fresh.prove_pairs_many(pairs, idx, xs, ks, contexts=ctxs)
        times = fresh.stage_times()
        _same(again, exp)
        assert times[VARBASE][1] == 65 and "generators" not in times, times     # rebuilt per call
        assert not _resident(fresh, pairs).any()
        assert fresh.fallback_stats() == fb
    # eight entries against the Python oracle: its points and its response
    for i in (0, 1, 2, 3, 64, 65, 100, 129):
        p = pairs[int(idx[i])]
        rec = O.prove(int.from_bytes(xs[i].tobytes(), "little"), int.from_bytes(ks[i].tobytes(), "little"), ctxs[i],
                      g=O.ristretto_decode(p.g), h=O.ristretto_decode(p.h))
        assert [got[q][i].tobytes() for q in Q] == [rec.y1, rec.y2, rec.r1, rec.r2, rec.s], i
    st = gpu.verify_each_pairs_many(pairs, idx, *[got[q] for q in Q], contexts=ctxs)
    assert st.tolist() == [0] * 130


def test_the_light_set_cache_keeps_its_order(mix65, pool):
    """Sets made resident before the call are still resident after it, and the least recently used
    of them is still the first to go."""
    pairs, idx, ctxs, xs, ks, exp = mix65
    with cp.Gpu(0) as fresh:
        old = pool[100:164]
        assert fresh.load_pairs(old) == 64
        fresh.load_pairs(old[1:])                                    # old[0] is now the least recently used
        _same(fresh.prove_pairs_many(pairs, idx, xs, ks, contexts=ctxs), exp)
        assert _resident(fresh, old).all() and not _resident(fresh, pairs).any()
        assert fresh.load_pairs([pool[199]]) == 1
        assert _resident(fresh, old).tolist() == [0] + [1] * 63


# ---- 2. digit edges ----------------------------------------------------------------------------------------

def test_digit_edges(gpu, pool):
    """Every case of prove_many_cases as x (with a random k) and as k (with a random x), over 65
    pairs, against Gpu.prove under the entry's own pair (cpz_prove: the comb path)."""
    pairs = pool[:65]
    m = len(EDGES)
    n = 2 * m
    xs = np.zeros((n, 32), np.uint8)
    ks = np.zeros((n, 32), np.uint8)
    for j, (_, raw) in enumerate(EDGES):
        xs[j] = np.frombuffer(raw, np.uint8)
        ks[j] = np.frombuffer(O.scalar_bytes(random_scalar(b"edge-k", j)), np.uint8)
        xs[m + j] = np.frombuffer(O.scalar_bytes(random_scalar(b"edge-x", j)), np.uint8)
        ks[m + j] = np.frombuffer(raw, np.uint8)
    idx = ((np.arange(n) * 7 + 3) % 65).astype(np.uint32)
    idx[0], idx[m] = 64, 0                                           # the last pair and the first
    ctxs = [B._ctx(i) for i in range(n)]
    got = gpu.prove_pairs_many(pairs, idx, xs, ks, contexts=ctxs)
    names = [e[0] for e in EDGES]
    for i in range(n):
        one = gpu.prove(xs[i:i + 1], ks[i:i + 1], contexts=[ctxs[i]], params=pairs[int(idx[i])])
        for q in Q:
            assert got[q][i].tobytes() == one[q][0].tobytes(), (names[i % m], "x" if i < m else "k", q)
    zero = names.index("0")
    assert not got["y1"][zero].any() and not got["y2"][zero].any()          # x = 0: the identity's encoding
    assert not got["r1"][m + zero].any() and not got["r2"][m + zero].any()  # k = 0
    assert got["y1"][names.index("1")].tobytes() == pairs[int(idx[names.index("1")])].g     # x = 1: g itself


# ---- 3. block edges: 64 proofs per block -------------------------------------------------------------------

@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_block_edges(gpu, mix65, n):
    pairs, idx, ctxs, xs, ks, exp = mix65
    got = gpu.prove_pairs_many(pairs, idx[:n], xs[:n], ks[:n], contexts=ctxs[:n])
    _same(got, exp, n)


# ---- 4. npairs = 4096: the bound -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pairs4096(gpu):
    return BM._many_pairs(gpu, 4096, b"prove-many-4096")


def test_the_bound(gpu, pairs4096):
    """One entry per pair in a permuted order, then a sparse list in which most pairs have no entry."""
    pairs = pairs4096
    n = 4096
    idx = ((np.arange(n, dtype=np.int64) * 1237 + 11) % 4096).astype(np.uint32)     # 1237 is odd: a permutation
    assert len(set(idx.tolist())) == 4096
    ctxs = [B._ctx(i) for i in range(n)]
    xs, ks = _scalars(n, b"bound")
    got = gpu.prove_pairs_many(pairs, idx, xs, ks, contexts=ctxs)
    _same(got, _runs64(gpu, pairs, idx, xs, ks, ctxs))
    used = np.array([0, 63, 64, 2077, 4032, 4095], np.uint32)
    sparse = used[np.arange(90) % 6]
    got = gpu.prove_pairs_many(pairs, sparse, xs[:90], ks[:90], contexts=ctxs[:90])
    _same(got, _runs64(gpu, pairs, sparse, xs[:90], ks[:90], ctxs[:90]))


def test_4097_pairs_are_refused(gpu, pairs4096):
    pairs = pairs4096 + [pairs4096[0]]
    xs, ks = _scalars(4, b"over")
    with pytest.raises(_native.CpzError) as e:
        gpu.prove_pairs_many(pairs, [0, 1, 2, 4096], xs, ks)
    assert e.value.code == _native.CPZ_EINVAL and "CPZ_PROVE_PAIRS_MANY_MAX" in str(e.value) and "4097" in str(e.value)


# ---- 5. npairs <= 64: forwarding ------------------------------------------------------------------------------

CHILD = r"""
import sys
import numpy as np
import chaum_pedersen as cp
d = np.load(sys.argv[1])
pairs = [cp.Parameters(bytes(r[:32]), bytes(r[32:])) for r in d["gh"]]
ctxs = [None if not p else bytes(c[:k]) for p, c, k in zip(d["present"], d["ctx"], d["ctx_len"])]
with cp.Gpu(0) as g:
    g.set_timing(True)
    g.stage_times()
    out = g.prove_pairs_many(pairs, d["idx"], d["x"], d["k"], contexts=ctxs)
    times = g.stage_times()
    resident = g.pairs_resident(pairs)
np.savez(sys.argv[2], built=times.get("generators_varbase", (0.0, 0))[1], resident=resident, **out)
"""


@pytest.mark.parametrize("npairs", [64, 5])
def test_up_to_64_pairs_it_is_prove_pairs(gpu, pool, npairs, tmp_path):
    """The same rows and stage launches as prove_pairs on fresh contexts (the pairs' light sets are
    built and stay resident); with CPZ_PROVE_MANY_FORWARD=0 in a child process the same inputs give
    the same bytes through the small tables (npairs counted in one stage-13 span, no set resident
    afterwards)."""
    n = 200
    pairs = pool[100:100 + npairs]
    idx = (np.arange(n) % npairs).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    xs, ks = _scalars(n, b"fwd-%d" % npairs)
    seen = []
    for name in ("prove_pairs_many", "prove_pairs"):
        with cp.Gpu(0) as fresh:
            fresh.set_timing(True)
            fresh.stage_times()
            out = getattr(fresh, name)(pairs, idx, xs, ks, contexts=ctxs)
            times = fresh.stage_times()
            seen.append((b"".join(out[q].tobytes() for q in Q), {k: v[1] for k, v in times.items()},
                         _resident(fresh, pairs).tolist()))
    assert seen[0] == seen[1]
    assert seen[0][1][VARBASE] == npairs and seen[0][2] == [1] * npairs
    ctx_len = np.array([len(c or b"") for c in ctxs], np.int64)
    ctx = np.zeros((n, 32), np.uint8)
    for i, c in enumerate(ctxs):
        if c:
            ctx[i, :len(c)] = np.frombuffer(c, np.uint8)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, gh=_gh(pairs).reshape(npairs, 64), idx=idx, present=np.array([c is not None for c in ctxs]), ctx=ctx,
             ctx_len=ctx_len, x=xs, k=ks)
    env = dict(os.environ, CPZ_PROVE_MANY_FORWARD="0",
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "chaum-pedersen-zkp_amd")] +
                                          [p for p in [os.environ.get("PYTHONPATH")] if p]))
    r = subprocess.run([sys.executable, "-c", CHILD, src, dst], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(dst)
    assert b"".join(out[q].tobytes() for q in Q) == seen[0][0]
    assert int(out["built"]) == npairs and not out["resident"].any()


# ---- 6. the device form -----------------------------------------------------------------------------------------

def test_device_form(gpu, mix65):
    import torch
    pairs, idx, ctxs, xs, ks, exp = mix65
    n = 130
    host = gpu.prove_pairs_many(pairs, idx, xs, ks, contexts=ctxs)
    _same(host, exp)
    dev = torch.device("cuda:0")
    d_x, d_k = torch.from_numpy(xs).to(dev), torch.from_numpy(ks).to(dev)
    blob, off, present = cp._ctx_arrays(ctxs, n)
    d_blob = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_present = torch.from_numpy(present).to(dev)
    d_i32 = torch.from_numpy(idx.astype(np.int32)).to(dev)

    def poison():
        outs = [torch.full((n, 32), 0xAA, dtype=torch.uint8, device=dev) for _ in Q]
        torch.cuda.synchronize()
        return outs

    def untouched(outs):
        torch.cuda.synchronize()
        return all((o.cpu().numpy() == 0xAA).all() for o in outs)

    side = torch.cuda.Stream()                                      # a stream of the caller's, not the default one
    for d_idx in (d_i32, d_i32.view(torch.uint32)):
        outs = poison()
        gpu.prove_pairs_many_device(pairs, d_idx, d_x, d_k, *outs, stream=side.cuda_stream, ctx_bytes=d_blob,
                                    ctx_off=d_off, ctx_present=d_present)
        _same({q: o.cpu().numpy() for q, o in zip(Q, outs)}, host)      # the call returned synchronised
    # an index equal to npairs at 100 and at 3: found on the device, the lowest named, nothing written
    bad = d_i32.clone()
    bad[100] = 65
    bad[3] = 65
    outs = poison()
    with pytest.raises(_native.CpzError) as e:
        gpu.prove_pairs_many_device(pairs, bad, d_x, d_k, *outs, stream=side.cuda_stream, ctx_bytes=d_blob,
                                    ctx_off=d_off, ctx_present=d_present)
    assert e.value.code == _native.CPZ_EINVAL and "pair_idx[3] = 65" in str(e.value), str(e.value)
    assert untouched(outs)
    # a misaligned device row
    lib, h = gpu._lib, gpu._h
    gh = _gh(pairs)
    rc = lib.cpz_prove_pairs_many_device(h, 65, gh.ctypes.data, n - 1, d_i32.data_ptr(), d_x.data_ptr() + 4,
                                         d_k.data_ptr(), None, None, None, *[o.data_ptr() for o in outs], None)
    assert rc == _native.CPZ_EINVAL and b"16-byte aligned" in lib.cpz_last_error()
    assert untouched(outs)
    # a pair that does not decode: after the index scan, before any table or output
    ghb = gh.copy()
    ghb[64 * 40:64 * 40 + 32] = BAD_POINT
    rc = lib.cpz_prove_pairs_many_device(h, 65, ghb.ctypes.data, n, d_i32.data_ptr(), d_x.data_ptr(), d_k.data_ptr(),
                                         None, None, None, *[o.data_ptr() for o in outs], None)
    assert rc == _native.CPZ_EGENERATOR and b"pair 40" in lib.cpz_last_error()
    assert untouched(outs)


# ---- 7. errors ---------------------------------------------------------------------------------------------------

def test_errors_write_nothing_and_launch_nothing(gpu, pool):
    pairs = pool[:65]
    n = 16
    xs, ks = _scalars(n, b"errs")
    gh = _gh(pairs)
    idx = np.arange(n, dtype=np.uint32)
    outs = [np.full((n, 32), 255, np.uint8) for _ in Q]
    with cp.Gpu(0) as fresh:
        lib, h = fresh._lib, fresh._h
        fb = fresh.fallback_stats()
        fresh.set_timing(True)
        fresh.stage_times()

        def call(npairs, gh_, n_, idx_, rows=None, gh_ptr=True, ctx=(None, None, None)):
            rows = [xs, ks] + outs if rows is None else rows
            rc = lib.cpz_prove_pairs_many(h, npairs, gh_.ctypes.data if gh_ptr else None, n_,
                                          None if idx_ is None else idx_.ctypes.data,
                                          *[None if r is None else r.ctypes.data for r in rows[:2]],
                                          *[None if c is None else c.ctypes.data for c in ctx],
                                          *[None if r is None else r.ctypes.data for r in rows[2:]])
            err = lib.cpz_last_error()
            assert all((o == 255).all() for o in outs)                  # nothing was written
            times = fresh.stage_times()
            assert "prove" not in times and VARBASE not in times and "generators" not in times, times
            return rc, err, times

        assert call(65, gh, 0, idx)[0] == _native.CPZ_EEMPTY
        rc, err, _ = call(0, gh, n, idx)
        assert rc == _native.CPZ_EINVAL and b"npairs is 0" in err
        rc, err, _ = call(65, gh, _native.PROVE_PAIRS_MAX_PROOFS + 1, idx)
        assert rc == _native.CPZ_EINVAL and b"CPZ_PROVE_PAIRS_MAX_PROOFS" in err
        assert call(65, gh, n, idx, gh_ptr=False)[0] == _native.CPZ_EINVAL
        assert call(65, gh, n, None)[0] == _native.CPZ_EINVAL
        for k in range(7):                                              # a null input or output row
            rows = [xs, ks] + outs
            rows[k] = None
            rc, err, times = call(65, gh, n, idx, rows)
            assert rc == _native.CPZ_EINVAL and b"null input or output pointer" in err and times == {}
        # context offsets that decrease, and offsets without bytes
        blob = np.frombuffer(b"abcdefgh", np.uint8).copy()
        off = np.arange(n + 1, dtype=np.uint64)
        off[5] = 2
        present = np.ones(n, np.uint8)
        rc, err, times = call(65, gh, n, idx, ctx=(blob, off, present))
        assert rc == _native.CPZ_EINVAL and times == {}, err
        rc, err, times = call(65, gh, n, idx, ctx=(None, np.arange(n + 1, dtype=np.uint64), present))
        assert rc == _native.CPZ_EINVAL and times == {}, err
        # an index at npairs, the lowest offending entry named
        bad = idx.copy()
        bad[11], bad[13] = 65, 70
        rc, err, times = call(65, gh, n, bad)
        assert rc == _native.CPZ_EINVAL and b"pair_idx[11] = 65" in err and times == {}
        # the identity and g == h: the host's check, the lowest pair named, nothing launched at all
        ghb = gh.copy()
        ghb[64 * 50:64 * 50 + 32] = 0
        ghb[64 * 9 + 32:64 * 9 + 64] = ghb[64 * 9:64 * 9 + 32]
        rc, err, times = call(65, ghb, n, idx)
        assert rc == _native.CPZ_EGENERATOR and b"pair 9" in err and times == {}
        ghb = gh.copy()
        ghb[64 * 50:64 * 50 + 32] = 0
        rc, err, times = call(65, ghb, n, idx)
        assert rc == _native.CPZ_EGENERATOR and b"pair 50" in err and times == {}
        # pairs that do not decode: found by the descriptor launch, before any table is built
        ghb = gh.copy()
        ghb[64 * 64 + 32:64 * 65] = BAD_POINT
        ghb[64 * 30:64 * 30 + 32] = BAD_POINT
        rc, err, times = call(65, ghb, n, idx)
        assert rc == _native.CPZ_EGENERATOR and b"pair 30" in err and b"decode" in err
        assert fresh.fallback_stats() == fb
        # and the call itself still works on this context
        rc = lib.cpz_prove_pairs_many(h, 65, gh.ctypes.data, n, idx.ctypes.data, xs.ctypes.data, ks.ctypes.data, None,
                                      None, None, *[o.ctypes.data for o in outs])
        assert rc == _native.CPZ_OK and not any((o == 255).all() for o in outs)
        times = fresh.stage_times()
        assert times[VARBASE][1] == 65 and "generators" not in times, times
    _same(dict(zip(Q, outs)), _runs64(gpu, pairs, idx, xs, ks, None))

