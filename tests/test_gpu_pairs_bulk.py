"""Mixed-pair per-proof verification above the latency kernels' 2048 proofs
(cpz_verify_each_pairs_bulk, cpz_verify_each_pairs_device): chunks of at most 16384 proofs
(14080 on a 110-CU part), eight lanes per proof (k_verify_quad's mixed-pair arm), every proof
from the tables of pairs[pair_idx[i]] and with that pair's transcript prefix.  The batch check's
dense fallback (pairs_leaf) takes the same path above 2048 proofs.

Inputs are shaped as in tests/test_gpu_pairs.py: custom pairs [a]B, [b]B, proofs from Gpu.prove
per pair, contexts cycling through None, 32 bytes, 5 bytes and b"".  Expected statuses are the C
oracle's under each entry's own pair, and the same entries through one verify_each per pair
(code this feature does not touch) must give the same bytes."""
import ctypes
import hashlib

import numpy as np
import pytest

import chaum_pedersen as cp
import pyoracle as O
from chaum_pedersen import _native

pytestmark = pytest.mark.gpu

Q = ("y1", "y2", "r1", "r2", "s")
BAD_POINT = np.frombuffer(bytes.fromhex("01" + "00" * 31), np.uint8)
SEED = hashlib.sha256(b"pairs-bulk-weights").digest()
PREP_BLOCK = 256          # kRlcPrepBlock: the bisection's alignment
FANOUT = 8


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


def _prove(gpu, pairs, groups, ctxs, seed):
    """Valid proofs: entry i under pairs[groups[i]] with context ctxs[i]."""
    groups = np.asarray(groups)
    rows = {q: np.zeros((len(groups), 32), np.uint8) for q in Q}
    for p in sorted(set(groups.tolist())):
        idx = np.nonzero(groups == p)[0]
        out = gpu.prove([O.bench_scalar(seed + b"x", int(i)) for i in idx],
                        [O.bench_scalar(seed + b"k", int(i)) for i in idx],
                        contexts=[ctxs[i] for i in idx], params=pairs[p])
        for q in Q:
            rows[q][idx] = out[q]
    return rows


def _oracle(pairs, groups, rows, ctxs, sel=None):
    """coracle.verify_one under each entry's own pair, for every entry or for those in sel."""
    import coracle
    sel = range(len(groups)) if sel is None else sel
    return np.array([coracle.verify_one(pairs[int(groups[i])].g, pairs[int(groups[i])].h,
                                        *(rows[q][i].tobytes() for q in Q), ctx=ctxs[i]) for i in sel], np.uint8)


def _per_group(gpu, pairs, groups, rows, ctxs, equations_only=False):
    """The same entries as one verify_each call per pair."""
    groups = np.asarray(groups)
    out = np.full(len(groups), 255, np.uint8)
    for p in sorted(set(groups.tolist())):
        idx = np.nonzero(groups == p)[0]
        out[idx] = gpu.verify_each(*[np.ascontiguousarray(rows[q][idx]) for q in Q], contexts=[ctxs[i] for i in idx],
                                   params=pairs[p], equations_only=equations_only)
    return out


def _cols(rows, sel=slice(None)):
    return [np.ascontiguousarray(rows[q][sel]) for q in Q]


def _s_plus(rows, i, d):
    v = int.from_bytes(rows["s"][i].tobytes(), "little") + d
    rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)


def _diff(got, exp):
    bad = np.nonzero(got != exp)[0]
    return bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist()


# ---- n = 2049 over three pairs: the first size of the new path ------------------------------------
N3 = 2049
S_PLUS_1 = [0, 7, 8, 31, 32, 2048]
WRONG_PAIR = [100, 301, 1002]            # no context, a 32-byte context, a 5-byte context
FORGED = S_PLUS_1 + WRONG_PAIR + [130, 201, 262, 407]


@pytest.fixture(scope="module")
def mix3(gpu):
    """2049 entries over the default pair and two custom ones, pair_idx[i] = i % 3: the pair
    differs inside every wave (4 proofs) and every block (32), and the last block holds one
    proof.  Forged as the module's constants say; the oracle's statuses for all 2049 entries are
    computed once, here."""
    pairs = [cp.Parameters()] + _pairs(2, b"bulk3")
    groups = (np.arange(N3) % 3).astype(np.uint32)
    ctxs = [_ctx(i) for i in range(N3)]
    assert [ctxs[i] is None for i in WRONG_PAIR] == [True, False, False]
    assert [len(ctxs[i] or b"") for i in WRONG_PAIR] == [0, 32, 5]
    rows = _prove(gpu, pairs, groups, ctxs, b"b3")
    for i in S_PLUS_1:
        _s_plus(rows, i, 1)
    for i in WRONG_PAIR:                                   # proven under one pair, labelled the next
        groups[i] = (groups[i] + 1) % 3
    rows["r1"][130] = BAD_POINT                            # undecodable point
    _s_plus(rows, 201, O.L)                                # s + l: not canonical
    rows["s"][262] = 0                                     # zero s
    rows["r2"][407] = 0                                    # identity commitment
    exp = _oracle(pairs, groups, rows, ctxs)
    return pairs, groups, ctxs, rows, exp


def _expected(mix3, equations_only):
    exp = mix3[4].copy()
    assert np.nonzero(exp)[0].tolist() == sorted(FORGED)
    assert [int(exp[i]) for i in FORGED] == [1] * 9 + [2, 3, 5, 4]
    if equations_only:
        # commitment checks off: the zero s and the identity commitment are judged by the equations,
        # which a valid proof with its s or r2 replaced cannot satisfy (as tests/test_gpu_pairs.py)
        exp[[262, 407]] = 1
    return exp


@pytest.mark.parametrize("equations_only", [False, True])
def test_first_size_of_the_new_path_smallest_mix(gpu, mix3, equations_only):
    pairs, groups, ctxs, rows, _ = mix3
    exp = _expected(mix3, equations_only)
    got = gpu.verify_each_pairs_bulk(pairs, groups, *_cols(rows), contexts=ctxs, equations_only=equations_only)
    assert np.array_equal(got, exp), _diff(got, exp)
    assert got.tobytes() == _per_group(gpu, pairs, groups, rows, ctxs, equations_only).tobytes()


@pytest.mark.parametrize("n", [7, 521])
def test_below_the_bound_it_is_verify_each_pairs(gpu, mix3, n):
    pairs, groups, ctxs, rows, exp = mix3
    got = gpu.verify_each_pairs_bulk(pairs, groups[:n], *_cols(rows, slice(0, n)), contexts=ctxs[:n])
    ref = gpu.verify_each_pairs(pairs, groups[:n], *_cols(rows, slice(0, n)), contexts=ctxs[:n])
    assert got.tobytes() == ref.tobytes()
    assert got.tolist() == exp[:n].tolist() and got.any()


def test_the_old_cap_stands(gpu, mix3):
    pairs, groups, ctxs, rows, _ = mix3
    with pytest.raises(_native.CpzError) as e:
        gpu.verify_each_pairs(pairs, groups, *_cols(rows), contexts=ctxs)
    assert e.value.code == _native.CPZ_EINVAL and "CPZ_PAIRS_MAX_PROOFS" in str(e.value)


# ---- n = 16385 (+ 2) over 64 pairs: the chunk boundary ----------------------------------------------
N64 = 16385


@pytest.fixture(scope="module")
def big64(gpu):
    """16,387 valid proofs over 64 custom pairs, entry i under pair i % 64, contexts of all four
    shapes.  The chunk-boundary test uses the first 16,385; the two more give the last chunk of
    a 256-CU part entries that verify only from the right rows, indices and contexts."""
    pairs = _pairs(64, b"bulk64")
    n = N64 + 2
    groups = (np.arange(n) % 64).astype(np.uint32)
    ctxs = [_ctx(i) for i in range(n)]
    return pairs, groups, ctxs, _prove(gpu, pairs, groups, ctxs, b"b64")


def _forge_chunk_edges(big64, n):
    pairs, groups, ctxs, rows = big64
    groups = groups[:n].copy()
    ctxs = list(ctxs[:n])
    rows = {q: rows[q][:n].copy() for q in Q}
    # both sides of the chunk edge of a 256-CU part (16384) and of a 110-CU part (14080); 16384 is the
    # lone proof of the last chunk when n = 16385
    forged = [14079, 14080, 16383, 16384, 0]
    for i in forged:
        _s_plus(rows, i, 1)
    # a wrong-pair label below 16384; entry 16384 itself carries s + 1, so the label on the other side
    # of that edge is entry 16385 where n allows it, and on the other side of the 14080 edge otherwise
    wrong = [16382, 16385 if n > 16385 else 14081]
    for i in wrong:
        groups[i] = (groups[i] + 1) % 64
    forged += wrong
    exp = np.zeros(n, np.uint8)
    exp[forged] = 1
    near = [j for i in forged for j in (i - 1, i + 1) if 0 <= j < n]
    sample = sorted(set(forged + near + list(range(0, n, 997))))
    assert _oracle(pairs, groups, rows, ctxs, sample).tolist() == exp[sample].tolist()
    return pairs, groups, ctxs, rows, exp


def test_chunk_boundary(gpu, big64):
    pairs, groups, ctxs, rows, exp = _forge_chunk_edges(big64, N64)
    got = gpu.verify_each_pairs_bulk(pairs, groups, *_cols(rows), contexts=ctxs)
    assert np.array_equal(got, exp), _diff(got, exp)
    assert got.tobytes() == _per_group(gpu, pairs, groups, rows, ctxs).tobytes()


def test_last_chunk_reads_its_own_rows_indices_and_contexts(gpu, big64):
    """n = 16387: after the s + 1 of entry 16384 the last chunk of a 256-CU part holds a wrong-pair
    label (16385) and a valid proof (16386), which passes only with the chunk's offsets into the
    rows, pair_idx, ctx_off and ctx_present all right."""
    pairs, groups, ctxs, rows, exp = _forge_chunk_edges(big64, N64 + 2)
    assert exp[-3:].tolist() == [1, 1, 0]
    got = gpu.verify_each_pairs_bulk(pairs, groups, *_cols(rows), contexts=ctxs)
    assert np.array_equal(got, exp), _diff(got, exp)


def test_cold_context_builds_light_sets_and_no_comb(big64):
    pairs, groups, ctxs, rows = big64
    n = 2049
    cols = _cols(rows, slice(0, n))
    _s_plus({"s": cols[4]}, 2048, 1)
    exp = np.zeros(n, np.uint8)
    exp[2048] = 1
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        cold = fresh.verify_each_pairs_bulk(pairs, groups[:n], *cols, contexts=ctxs[:n])
        st = fresh.stage_times()
        assert st.get("generators_varbase", (0.0, 0))[1] == 64, st
        assert st.get("generators", (0.0, 0))[1] == 0, st
        assert st["verify_each"][1] == 1 and st["challenge"][1] == 1, st
        warm = fresh.verify_each_pairs_bulk(pairs, groups[:n], *cols, contexts=ctxs[:n])
        st = fresh.stage_times()
        assert "generators_varbase" not in st and "generators" not in st, st
    assert cold.tolist() == exp.tolist() and warm.tobytes() == cold.tobytes()


# ---- the device form ------------------------------------------------------------------------------
def test_device_form(gpu, mix3):
    import torch
    pairs, groups, ctxs, rows, _ = mix3
    exp = _expected(mix3, False)
    host = gpu.verify_each_pairs_bulk(pairs, groups, *_cols(rows), contexts=ctxs)
    assert np.array_equal(host, exp)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(c).to(dev) for c in _cols(rows)]
    blob, off, present = cp._ctx_arrays(ctxs, N3)
    d_blob = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_present = torch.from_numpy(present).to(dev)
    d_idx = torch.from_numpy(groups.astype(np.int32)).to(dev)
    out = torch.full((N3,), 0xff, dtype=torch.uint8, device=dev)
    gpu.verify_each_pairs_device(pairs, d_idx, *t, out, ctx_bytes=d_blob, ctx_off=d_off, ctx_present=d_present)
    got = out.cpu().numpy()                      # the call returned synchronised
    assert np.array_equal(got, host), _diff(got, host)
    # again on a stream of the caller's
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    out2 = torch.full((N3,), 0xff, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gpu.verify_each_pairs_device(pairs, d_idx, *t, out2, stream=side.cuda_stream, ctx_bytes=d_blob, ctx_off=d_off,
                                 ctx_present=d_present)
    assert np.array_equal(out2.cpu().numpy(), host)
    # an index outside the three pairs: found on the device, named, and nothing is written
    bad = d_idx.clone()
    bad[2048] = 3
    out3 = torch.full((N3,), 0xff, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(_native.CpzError) as e:
        gpu.verify_each_pairs_device(pairs, bad, *t, out3, ctx_bytes=d_blob, ctx_off=d_off, ctx_present=d_present)
    assert e.value.code == _native.CPZ_EINVAL and "pair_idx[2048] = 3" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert (out3.cpu().numpy() == 0xff).all()
    # the lowest offending entry is the one named
    bad[5] = 7
    with pytest.raises(_native.CpzError) as e:
        gpu.verify_each_pairs_device(pairs, bad, *t, out3, ctx_bytes=d_blob, ctx_off=d_off, ctx_present=d_present)
    assert "pair_idx[5] = 7" in str(e.value), str(e.value)
    assert (out3.cpu().numpy() == 0xff).all()


# ---- errors ---------------------------------------------------------------------------------------
def test_errors_write_nothing_and_launch_nothing(mix3):
    _, _, _, rows, _ = mix3
    pairs = _pairs(64, b"bulk-errs")          # pairs no context has seen: no set of theirs is resident
    n = 16
    cols = _cols(rows, slice(0, n))
    gh = np.frombuffer(b"".join(p.g + p.h for p in pairs) + bytes(64), np.uint8).copy()   # 65 rows
    idx = np.arange(n, dtype=np.uint32)
    out = np.full(n, 255, np.uint8)
    with cp.Gpu(0) as fresh:
        lib, h = fresh._lib, fresh._h
        fresh.set_timing(True)
        fresh.stage_times()

        def call(npairs, gh_, n_, idx_, cols_=cols, gh_ptr=True, ex=False):
            args = [npairs, gh_.ctypes.data if gh_ptr else None, n_, idx_.ctypes.data,
                    *[None if c is None else c.ctypes.data for c in cols_], None, None, None, out.ctypes.data]
            rc = lib.cpz_verify_each_pairs_bulk_ex(h, 0, *args) if ex else lib.cpz_verify_each_pairs_bulk(h, *args)
            err = lib.cpz_last_error()
            assert (out == 255).all()                     # nothing was written
            assert fresh.stage_times() == {}              # and nothing was launched
            return rc, err

        for ex in (False, True):
            assert call(64, gh, 0, idx, ex=ex)[0] == _native.CPZ_EEMPTY
            assert call(0, gh, n, idx, ex=ex)[0] == _native.CPZ_EINVAL
            rc, err = call(65, gh, n, idx, ex=ex)
            assert rc == _native.CPZ_EINVAL and b"CPZ_PAIRS_MAX" in err
            # n above the bound: refused on the count alone, before any row is read
            rc, err = call(64, gh, _native.PAIRS_BULK_MAX_PROOFS + 1, idx, ex=ex)
            assert rc == _native.CPZ_EINVAL and b"CPZ_PAIRS_BULK_MAX_PROOFS" in err
            assert call(64, gh, n, idx, gh_ptr=False, ex=ex)[0] == _native.CPZ_EINVAL
            for k in range(5):                            # a null row
                assert call(64, gh, n, idx, [None if j == k else c for j, c in enumerate(cols)], ex=ex)[0] == \
                    _native.CPZ_EINVAL
            bad = idx.copy()
            bad[11], bad[13] = 64, 70
            rc, err = call(64, gh, n, bad, ex=ex)
            assert rc == _native.CPZ_EINVAL and b"pair_idx[11] = 64" in err
            for what, g2, h2 in (("identity", bytes(32), pairs[2].h), ("equal", pairs[2].g, pairs[2].g),
                                 ("undecodable", bytes.fromhex("01" + "00" * 31), pairs[2].h)):
                ghb = gh.copy()
                ghb[128:192] = np.frombuffer(g2 + h2, np.uint8)
                rc, err = call(64, ghb, n, idx, ex=ex)
                assert rc == _native.CPZ_EGENERATOR and b"pair 2" in err, (what, rc, err)
        # the same refusals above the latency kernels' bound, where the new path would run
        big = [np.zeros((2049, 32), np.uint8) for _ in Q]
        bigidx = np.zeros(2049, np.uint32)
        bigidx[2048] = 64
        rc, err = call(64, gh, 2049, bigidx, big)
        assert rc == _native.CPZ_EINVAL and b"pair_idx[2048] = 64" in err
        ghb = gh.copy()
        ghb[128:160] = BAD_POINT
        rc, err = call(64, ghb, 2049, np.zeros(2049, np.uint32), big)
        assert rc == _native.CPZ_EGENERATOR and b"pair 2" in err and b"does not decode" in err


# ---- the batch check's dense fallback -------------------------------------------------------------------
def _cuts(lo, hi):
    """rlc_fallback's cut arithmetic (tests/test_gpu_batch_pairs.py): FANOUT parts aligned to the
    prepare block."""
    c = [(lo + ((hi - lo) * k) // FANOUT) // PREP_BLOCK * PREP_BLOCK for k in range(FANOUT + 1)]
    c[0], c[FANOUT] = lo, hi
    return c


def _partial(pairs, groups, rows, ctxs, sel):
    """The expected partial from the entries `sel` alone (every other entry is valid and contributes
    the identity): per pair, the C oracle's rlc_partial with the entries' global indices; summed."""
    import coracle
    groups = np.asarray(groups)
    acc = O.IDENTITY
    sel = np.asarray(sorted(sel), np.int64)
    for p in sorted(set(groups[sel].tolist())):
        idx = sel[groups[sel] == p]
        enc, _ = coracle.rlc_partial({q: np.ascontiguousarray(rows[q][idx]) for q in Q}, idx, SEED,
                                     [ctxs[i] for i in idx], g=pairs[p].g, h=pairs[p].h)
        acc = O.pt_add(acc, O.ristretto_decode(enc))
    return O.ristretto_encode(acc)


def test_dense_fallback_of_the_batch_check(gpu):
    """n = 4104 over 5 pairs with s + 1 in five of the eight top-level parts: more than half fail, so
    pairs_fallback hands the whole range to the leaf, which is above 2048 proofs and takes the
    chunked eight-lane path."""
    n = 4104
    pairs = [cp.Parameters()] + _pairs(4, b"bulk5")
    groups = (np.arange(n) % 5).astype(np.uint32)
    ctxs = [_ctx(i) for i in range(n)]
    rows = _prove(gpu, pairs, groups, ctxs, b"b5")
    forged = [10, 600, 1100, 2100, 4103]
    for i in forged:
        _s_plus(rows, i, 1)
    top = _cuts(0, n)
    hit = {max(k for k in range(FANOUT) if top[k] <= i) for i in forged}
    assert len(hit) == 5 and 2 * len(hit) > FANOUT
    exp = np.zeros(n, np.uint8)
    exp[forged] = 1
    near = [j for i in forged for j in (i - 1, i + 1) if 0 <= j < n]
    sample = sorted(set(forged + near + list(range(0, n, 97))))
    assert _oracle(pairs, groups, rows, ctxs, sample).tolist() == exp[sample].tolist()
    want = _partial(pairs, groups, rows, ctxs, forged)
    partial, ok, st = gpu.verify_batch_pairs(pairs, groups, *_cols(rows), SEED, contexts=ctxs)
    fb = gpu.fallback_stats()
    assert not ok and partial == want
    assert np.array_equal(st, exp), _diff(st, exp)
    assert st.tobytes() == gpu.verify_each_pairs_bulk(pairs, groups, *_cols(rows), contexts=ctxs).tobytes()
    assert fb["path"] == "bisection" and fb["bisection_msms"] == 8 and fb["per_proof"] == n, fb
