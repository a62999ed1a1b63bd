"""The mixed-pair prover (cpz_prove_pairs, cpz_prove_pairs_device): one call proves entry i under
pairs[pair_idx[i]], every point from that pair's 128-entry Niels tables (k_prove_points_pairs),
the challenge with that pair's transcript prefix (k_challenge_pairs), and no comb is built.

Row i of every output must be byte for byte what cpz_prove writes for the same (x, k, context)
under that pair -- Gpu.prove per pair, code this feature does not touch -- and, for the edge
scalars of tests/prove_pairs_cases.py, what the Python oracle's prove gives
(tests/golden/prove_pairs.json).  Inputs are shaped as in tests/test_gpu_pairs_bulk.py."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import chaum_pedersen as cp
import pyoracle as O
from chaum_pedersen import _native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = ("y1", "y2", "r1", "r2", "s")


def _pairs(k, tag):
    """k distinct custom generator pairs (g_i = [a_i] B, h_i = [b_i] B)."""
    out = []
    for i in range(k):
        a = O.scalar_wide(hashlib.sha512(tag + b"-g-%d" % i).digest())
        b = O.scalar_wide(hashlib.sha512(tag + b"-h-%d" % i).digest())
        out.append(cp.Parameters(O.ristretto_encode(O.pt_mul(O.BASEPOINT, a)),
                                 O.ristretto_encode(O.pt_mul(O.BASEPOINT, b))))
    return out


def _ctx(i):
    """None, 32 bytes, 5 bytes, b"": the two fixed schedules and the byte-wise sponge."""
    return (None, hashlib.sha256(b"ctx-%d" % i).digest(), b"ctx%02d" % (i % 100), b"")[i % 4]


def _scalars(n, seed):
    xs = np.frombuffer(b"".join(O.scalar_bytes(O.bench_scalar(seed + b"x", i)) for i in range(n)), np.uint8)
    ks = np.frombuffer(b"".join(O.scalar_bytes(O.bench_scalar(seed + b"k", i)) for i in range(n)), np.uint8)
    return xs.reshape(n, 32).copy(), ks.reshape(n, 32).copy()


def _per_pair(gpu, pairs, groups, xs, ks, ctxs):
    """The same entries as one Gpu.prove call per pair (cpz_prove: the comb path)."""
    groups = np.asarray(groups)
    rows = {q: np.zeros((len(groups), 32), np.uint8) for q in Q}
    for p in sorted(set(groups.tolist())):
        idx = np.nonzero(groups == p)[0]
        out = gpu.prove(np.ascontiguousarray(xs[idx]), np.ascontiguousarray(ks[idx]),
                        contexts=[ctxs[i] for i in idx], params=pairs[p])
        for q in Q:
            rows[q][idx] = out[q]
    return rows


def _same(got, exp, n=None):
    for q in Q:
        g, e = got[q], exp[q] if n is None else exp[q][:n]
        bad = np.nonzero((g != e).any(axis=1))[0]
        assert bad.size == 0, (q, bad[:8].tolist())


# ---- the golden fixture: edge scalars against the Python oracle -----------------------------------
def test_golden_rows(gpu):
    with open(os.path.join(ROOT, "tests", "golden", "prove_pairs.json")) as f:
        fx = json.load(f)
    pairs = [cp.Parameters(bytes.fromhex(p["g"]), bytes.fromhex(p["h"])) for p in fx["pairs"]]
    assert pairs[0] == cp.Parameters() and len(pairs) == 3
    es = fx["entries"]
    n = len(es)
    xs = np.frombuffer(b"".join(bytes.fromhex(e["x"]) for e in es), np.uint8).reshape(n, 32)
    ks = np.frombuffer(b"".join(bytes.fromhex(e["k"]) for e in es), np.uint8).reshape(n, 32)
    ctxs = [None if e["ctx"] is None else bytes.fromhex(e["ctx"]) for e in es]
    out = gpu.prove_pairs(pairs, [e["pair"] for e in es], xs, ks, contexts=ctxs)
    for i, e in enumerate(es):
        for q in Q:
            assert out[q][i].tobytes().hex() == e[q], (i, e["what"], q)
    # x = 0 and k = 0: identity encodings
    assert any(e["what"] == "x = 0" and not out["y1"][i].any() and not out["y2"][i].any() for i, e in enumerate(es))
    assert any(e["what"] == "k = 0" and not out["r1"][i].any() and not out["r2"][i].any() for i, e in enumerate(es))


# ---- block edges: n = 255, 256, 257 over three pairs ---------------------------------------------
N3 = 257


@pytest.fixture(scope="module")
def mix3(gpu):
    """257 entries over the default pair and two custom ones, pair_idx[i] = i % 3, contexts of all
    four shapes; the expected rows from one Gpu.prove per pair, computed once."""
    pairs = [cp.Parameters()] + _pairs(2, b"prove3")
    groups = (np.arange(N3) % 3).astype(np.uint32)
    ctxs = [_ctx(i) for i in range(N3)]
    xs, ks = _scalars(N3, b"p3")
    return pairs, groups, ctxs, xs, ks, _per_pair(gpu, pairs, groups, xs, ks, ctxs)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_block_edges(gpu, mix3, n):
    """The last thread of a block (n = 256) and a second block holding one proof (n = 257)."""
    pairs, groups, ctxs, xs, ks, exp = mix3
    got = gpu.prove_pairs(pairs, groups[:n], xs[:n], ks[:n], contexts=ctxs[:n])
    _same(got, exp, n)


# ---- 64 pairs ------------------------------------------------------------------------------------
def test_sixty_four_pairs(gpu):
    pairs = _pairs(64, b"prove64")
    n = 192
    groups = (np.arange(n) % 64).astype(np.uint32)       # each pair three times, interleaved
    assert groups[191] == 63 and np.bincount(groups).tolist() == [3] * 64
    ctxs = [_ctx(i) for i in range(n)]
    xs, ks = _scalars(n, b"p64")
    got = gpu.prove_pairs(pairs, groups, xs, ks, contexts=ctxs)
    _same(got, _per_pair(gpu, pairs, groups, xs, ks, ctxs))
    st = gpu.verify_each_pairs(pairs, groups, *[got[q] for q in Q], contexts=ctxs)
    assert (st == cp.STATUS_OK).all(), np.nonzero(st)[0][:8].tolist()


# ---- repeated rows in `pairs`, the default pair among them ----------------------------------------
def test_repeated_rows_and_the_default_pair(gpu, mix3):
    pairs, groups, ctxs, xs, ks, exp = mix3
    n = 64
    rep = [pairs[1], pairs[0], pairs[1], pairs[2], pairs[0]]       # rows 0 = 2 and 1 = 4
    back = {0: (1, 4), 1: (0, 2), 2: (3, 3)}
    idx = np.array([back[int(g)][i % 2] for i, g in enumerate(groups[:n])], np.uint32)
    assert {1, 4, 0, 2, 3} == set(idx.tolist())
    got = gpu.prove_pairs(rep, idx, xs[:n], ks[:n], contexts=ctxs[:n])
    dedup = gpu.prove_pairs(pairs, groups[:n], xs[:n], ks[:n], contexts=ctxs[:n])
    _same(got, dedup)
    _same(got, exp, n)


# ---- a cold context builds light sets only ---------------------------------------------------------
def test_cold_context_builds_no_comb():
    pairs = _pairs(5, b"prove-cold")
    n = 40
    groups = (np.arange(n) % 5).astype(np.uint32)
    ctxs = [_ctx(i) for i in range(n)]
    xs, ks = _scalars(n, b"pc")
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        cold = fresh.prove_pairs(pairs, groups, xs, ks, contexts=ctxs)
        st = fresh.stage_times()
        assert "generators" not in st, st                          # no comb was built
        assert st.get("generators_varbase", (0.0, 0))[1] == 5, st   # one light set per pair
        assert st.get("prove", (0.0, 0))[1] >= 1, st
        warm = fresh.prove_pairs(pairs, groups, xs, ks, contexts=ctxs)
        st = fresh.stage_times()
        assert "generators_varbase" not in st and "generators" not in st and "prove" in st, st
        # one pair alone, one no context has seen: still its light set, still no comb
        lone = _pairs(1, b"prove-cold-one")
        one = fresh.prove_pairs(lone, np.zeros(n, np.uint32), xs, ks, contexts=ctxs)
        st = fresh.stage_times()
        assert "generators" not in st and st.get("generators_varbase", (0.0, 0))[1] == 1 and "prove" in st, st
        ok = fresh.verify_each_pairs(pairs, groups, *[cold[q] for q in Q], contexts=ctxs)
        ok1 = fresh.verify_each(*[one[q] for q in Q], contexts=ctxs, params=lone[0])
        assert "generators" not in fresh.stage_times()
    _same(warm, cold)
    assert (ok == cp.STATUS_OK).all() and (ok1 == cp.STATUS_OK).all()


# ---- the device form --------------------------------------------------------------------------------
def test_device_form(gpu, mix3):
    import torch
    pairs, groups, ctxs, xs, ks, exp = mix3
    n = N3
    host = gpu.prove_pairs(pairs, groups, xs, ks, contexts=ctxs)
    _same(host, exp)
    dev = torch.device("cuda:0")
    d_x, d_k = torch.from_numpy(xs).to(dev), torch.from_numpy(ks).to(dev)
    blob, off, present = cp._ctx_arrays(ctxs, n)
    d_blob = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_present = torch.from_numpy(present).to(dev)
    d_i32 = torch.from_numpy(groups.astype(np.int32)).to(dev)
    for d_idx in (d_i32, d_i32.view(torch.uint32)):
        outs = [torch.full((n, 32), 0xAA, dtype=torch.uint8, device=dev) for _ in Q]
        torch.cuda.synchronize()
        gpu.prove_pairs_device(pairs, d_idx, d_x, d_k, *outs, ctx_bytes=d_blob, ctx_off=d_off, ctx_present=d_present)
        _same({q: o.cpu().numpy() for q, o in zip(Q, outs)}, host)      # the call returned synchronised
    # on a stream of the caller's
    side = torch.cuda.Stream()
    outs = [torch.full((n, 32), 0xAA, dtype=torch.uint8, device=dev) for _ in Q]
    torch.cuda.synchronize()
    gpu.prove_pairs_device(pairs, d_i32, d_x, d_k, *outs, stream=side.cuda_stream, ctx_bytes=d_blob, ctx_off=d_off,
                           ctx_present=d_present)
    _same({q: o.cpu().numpy() for q, o in zip(Q, outs)}, host)
    # an index equal to npairs at 200 and at 3: found on the device, the lowest named, nothing written
    bad = d_i32.clone()
    bad[200] = 3
    bad[3] = 3
    outs = [torch.full((n, 32), 0xAA, dtype=torch.uint8, device=dev) for _ in Q]
    torch.cuda.synchronize()
    with pytest.raises(_native.CpzError) as e:
        gpu.prove_pairs_device(pairs, bad, d_x, d_k, *outs, ctx_bytes=d_blob, ctx_off=d_off, ctx_present=d_present)
    assert e.value.code == _native.CPZ_EINVAL and "pair_idx[3] = 3" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for o in outs:
        assert (o.cpu().numpy() == 0xAA).all()
    # a misaligned device row
    lib, h = gpu._lib, gpu._h
    gh = np.frombuffer(b"".join(p.g + p.h for p in pairs), np.uint8)
    rc = lib.cpz_prove_pairs_device(h, 3, gh.ctypes.data, n - 1, d_i32.data_ptr(), d_x.data_ptr() + 4, d_k.data_ptr(),
                                    None, None, None, *[o.data_ptr() for o in outs], None)
    assert rc == _native.CPZ_EINVAL and b"16-byte aligned" in lib.cpz_last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert (o.cpu().numpy() == 0xAA).all()


# ---- errors ---------------------------------------------------------------------------------------
def test_errors_write_nothing_and_launch_nothing():
    pairs = _pairs(64, b"prove-errs")          # pairs no context has seen: no set of theirs is resident
    n = 16
    xs, ks = _scalars(n, b"pe")
    gh = np.frombuffer(b"".join(p.g + p.h for p in pairs) + bytes(64), np.uint8).copy()   # 65 rows
    idx = np.arange(n, dtype=np.uint32)
    outs = [np.full((n, 32), 255, np.uint8) for _ in Q]
    with cp.Gpu(0) as fresh:
        lib, h = fresh._lib, fresh._h
        fresh.set_timing(True)
        fresh.stage_times()

        def call(npairs, gh_, n_, idx_, rows=None, gh_ptr=True):
            rows = [xs, ks] + outs if rows is None else rows
            rc = lib.cpz_prove_pairs(h, npairs, gh_.ctypes.data if gh_ptr else None, n_, idx_.ctypes.data,
                                     *[None if r is None else r.ctypes.data for r in rows[:2]], None, None, None,
                                     *[None if r is None else r.ctypes.data for r in rows[2:]])
            err = lib.cpz_last_error()
            assert all((o == 255).all() for o in outs)    # nothing was written
            assert fresh.stage_times() == {}              # and nothing was launched
            return rc, err

        assert call(64, gh, 0, idx)[0] == _native.CPZ_EEMPTY
        assert call(0, gh, n, idx)[0] == _native.CPZ_EINVAL
        rc, err = call(65, gh, n, idx)
        assert rc == _native.CPZ_EINVAL and b"CPZ_PAIRS_MAX" in err
        # n above the bound: refused on the count alone, before any row is read
        rc, err = call(64, gh, _native.PROVE_PAIRS_MAX_PROOFS + 1, idx)
        assert rc == _native.CPZ_EINVAL and b"CPZ_PROVE_PAIRS_MAX_PROOFS" in err
        assert call(64, gh, n, idx, gh_ptr=False)[0] == _native.CPZ_EINVAL
        for k in range(7):                                # a null input or output row
            rows = [xs, ks] + outs
            rows[k] = None
            assert call(64, gh, n, idx, rows)[0] == _native.CPZ_EINVAL
        bad = idx.copy()
        bad[11], bad[13] = 64, 70
        rc, err = call(64, gh, n, bad)
        assert rc == _native.CPZ_EINVAL and b"pair_idx[11] = 64" in err
        for what, g2, h2 in (("identity", bytes(32), pairs[2].h), ("equal", pairs[2].g, pairs[2].g),
                             ("undecodable", bytes.fromhex("01" + "00" * 31), pairs[2].h)):
            ghb = gh.copy()
            ghb[128:192] = np.frombuffer(g2 + h2, np.uint8)
            rc, err = call(64, ghb, n, idx)
            assert rc == _native.CPZ_EGENERATOR and b"pair 2" in err, (what, rc, err)
        # and the call itself still works on this context
        rc = lib.cpz_prove_pairs(h, 64, gh.ctypes.data, n, idx.ctypes.data, xs.ctypes.data, ks.ctypes.data, None, None,
                                 None, *[o.ctypes.data for o in outs])
        assert rc == _native.CPZ_OK and not any((o == 255).all() for o in outs)
        assert "generators" not in fresh.stage_times()
