"""Per-proof verification over up to 4096 (g, h) pairs in one call (cpz_verify_each_pairs_many): above
CPZ_PAIRS_MAX pairs the descriptors are built on the device, every pair gets small tables (multiples
0..8 of g, 2^128 g, h, 2^128 h) in one launch, and the entries are verified in chunks on eight
lanes per proof from those tables; no 128-entry set is built and the light-set cache is not touched.

Pairs and proofs are made as in tests/test_gpu_batch_pairs_many.py (its helpers are used here), and
the expected statuses are the C oracle's verify_many_ctx under each entry's own pair
(tests/test_gpu_batch_pairs.py's _statuses)."""
import ctypes
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

pytestmark = pytest.mark.gpu

Q = B.Q
BAD_POINT = B.BAD_POINT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARBASE = "generators_varbase"


def _diff(got, exp):
    bad = np.nonzero(got != exp)[0]
    return bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist()


def _sample_ok(pairs, idx, rows, ctxs, exp, sample):
    """The C oracle's statuses on `sample` equal exp there."""
    sample = sorted(set(int(i) for i in sample if 0 <= i < len(idx)))
    got = B._statuses(pairs, idx[sample], {q: rows[q][sample] for q in Q}, [ctxs[i] for i in sample])
    assert got.tolist() == exp[sample].tolist()


def _resident(g, pairs):
    """pairs_resident over any number of rows (the call takes PAIRS_MAX at a time)."""
    return np.concatenate([g.pairs_resident(pairs[c:c + _native.PAIRS_MAX])
                           for c in range(0, len(pairs), _native.PAIRS_MAX)])


def _raw(g, flags, npairs, gh, n, idx, cols, out, ctxs=None):
    """The C entry point itself: its return code."""
    blob, off, present = cp._ctx_arrays(ctxs, n) if ctxs is not None else (None, None, None)
    return g._lib.cpz_verify_each_pairs_many(g._h, flags, npairs, cp._ptr(gh), n, cp._ptr(idx),
                                             *[cp._ptr(a) for a in cols], cp._ptr(blob), cp._ptr(off), cp._ptr(present),
                                             cp._ptr(out))


def _last_error(g):
    g._lib.cpz_last_error.restype = ctypes.c_char_p
    return g._lib.cpz_last_error().decode()


@pytest.fixture(scope="module")
def pool(gpu):
    """1000 distinct pairs."""
    return BM._many_pairs(gpu, 1000, b"each-pool")


# ---- n = 130 over 65 pairs: the smallest call that does not forward ------------------------------------

@pytest.fixture(scope="module")
def mix65(gpu, pool):
    """130 valid proofs over 65 pairs, entry i under pair i % 65, contexts cycling the four shapes."""
    pairs = pool[:65]
    idx = (np.arange(130) % 65).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(130)]
    return pairs, idx, ctxs, BM._prove_many(gpu, pairs, idx, ctxs, b"e65")


FORGED65 = {"s_plus_1": 3, "label": 10, "bad_y": 20, "bad_r": 33, "s_plus_l": 47, "identity_r1": 77, "zero_s": 129}


def _forge65(mix65):
    pairs, idx, ctxs, rows = mix65
    idx = idx.copy()
    rows = {q: rows[q].copy() for q in Q}
    B._s_plus(rows, FORGED65["s_plus_1"], 1)
    idx[FORGED65["label"]] = (idx[FORGED65["label"]] + 1) % 65      # proven under one pair, labelled the next
    rows["y1"][FORGED65["bad_y"]] = BAD_POINT
    rows["r2"][FORGED65["bad_r"]] = BAD_POINT
    B._s_plus(rows, FORGED65["s_plus_l"], O.L)                       # not canonical
    rows["r1"][FORGED65["identity_r1"]] = 0
    rows["s"][FORGED65["zero_s"]] = 0
    exp = B._statuses(pairs, idx, rows, ctxs)
    assert np.nonzero(exp)[0].tolist() == sorted(FORGED65.values())
    assert [int(exp[FORGED65[k]]) for k in ("s_plus_1", "label", "bad_y", "bad_r", "s_plus_l", "identity_r1", "zero_s")
            ] == [1, 1, 2, 2, 3, 4, 5]
    return pairs, idx, ctxs, rows, exp


def test_smallest_call_that_does_not_forward(mix65):
    pairs, idx, ctxs, rows = mix65
    assert [type(c) for c in ctxs[:4]] == [type(None), bytes, bytes, bytes] and [len(c) for c in ctxs[1:4]] == [32, 5, 0]
    with cp.Gpu(0) as fresh:
        assert not _resident(fresh, pairs).any()
        fb = fresh.fallback_stats()
        fresh.set_timing(True)
        fresh.stage_times()
        got = fresh.verify_each_pairs_many(pairs, idx, *B._cols(rows), contexts=ctxs)
        times = fresh.stage_times()
        assert got.tolist() == [0] * 130
        assert times[VARBASE][1] == 65, times                      # one span that counts the pairs
        assert "generators" not in times, times                    # no comb
        assert times["verify_each"][1] == 1, times
        fpairs, fidx, fctxs, frows, exp = _forge65(mix65)
        got = fresh.verify_each_pairs_many(fpairs, fidx, *B._cols(frows), contexts=fctxs)
        assert np.array_equal(got, exp), _diff(got, exp)
        # commitment checks off: the zero s and the identity commitment are judged by the equations,
        # which a valid proof with its s or r1 replaced cannot satisfy (as tests/test_gpu_pairs_bulk.py)
        exp_eq = exp.copy()
        exp_eq[[FORGED65["identity_r1"], FORGED65["zero_s"]]] = 1
        got = fresh.verify_each_pairs_many(fpairs, fidx, *B._cols(frows), contexts=fctxs, equations_only=True)
        assert np.array_equal(got, exp_eq), _diff(got, exp_eq)
        fresh.set_commitment_checks(False)                          # the context's mode does the same
        got = fresh.verify_each_pairs_many(fpairs, fidx, *B._cols(frows), contexts=fctxs)
        assert np.array_equal(got, exp_eq), _diff(got, exp_eq)
        fresh.set_commitment_checks(True)
        times = fresh.stage_times()
        assert times[VARBASE][1] == 3 * 65 and "generators" not in times, times    # rebuilt per call
        assert not _resident(fresh, pairs).any()                   # no set was built or cached
        assert fresh.fallback_stats() == fb


def test_the_light_set_cache_keeps_its_order(gpu, mix65, pool):
    """Sets made resident before the call are still resident after it, and the least recently used
    of them is still the first to go."""
    pairs, idx, ctxs, rows = mix65
    with cp.Gpu(0) as fresh:
        old = pool[100:164]
        assert fresh.load_pairs(old) == 64
        fresh.load_pairs(old[1:])                                    # old[0] is now the least recently used
        got = fresh.verify_each_pairs_many(pairs, idx, *B._cols(rows), contexts=ctxs)
        assert not got.any()
        assert _resident(fresh, old).all() and not _resident(fresh, pairs).any()
        assert fresh.load_pairs([pool[200]]) == 1
        assert _resident(fresh, old).tolist() == [0] + [1] * 63


# ---- n = npairs = 300: one pair per entry ---------------------------------------------------------------

def test_one_pair_per_entry(gpu, pool):
    """9 blocks of 32 proofs and one of 12, every proof of a wave under other tables.  The default
    pair at row 130, row 150 repeating row 20 with both labels used, forged entries first and last
    of a block and of the call."""
    n = 300
    pairs = list(pool[:n])
    pairs[130] = cp.Parameters()
    pairs[150] = pairs[20]
    idx = np.arange(n, dtype=np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    proven = idx.copy()
    proven[100] = 101                                   # proven under pair 101, labelled pair 100
    proven[20], proven[150] = 150, 20                   # the repeated row under both labels
    rows = BM._prove_many(gpu, pairs, proven, ctxs, b"e-own")
    for i in (0, 31, 32, 287, 288, 299):
        B._s_plus(rows, i, 1)
    rows["r1"][200] = BAD_POINT
    rows["y2"][280] = BAD_POINT
    exp = B._statuses(pairs, idx, rows, ctxs)
    assert np.nonzero(exp)[0].tolist() == [0, 31, 32, 100, 200, 280, 287, 288, 299]
    assert exp[[0, 31, 32, 100, 200, 280, 287, 288, 299]].tolist() == [1, 1, 1, 1, 2, 2, 1, 1, 1]
    got = gpu.verify_each_pairs_many(pairs, idx, *B._cols(rows), contexts=ctxs)
    assert np.array_equal(got, exp), _diff(got, exp)


def test_sparse_pair_list(gpu, pool):
    """200 rows of which 70 carry entries."""
    pairs = list(pool[:200])
    used = sorted(set(range(2, 200, 3)) | {0, 1, 130, 150})
    assert len(used) == 70
    n = 280
    idx = np.asarray([used[i % 70] for i in range(n)], np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    rows = BM._prove_many(gpu, pairs, idx, ctxs, b"e-sparse")
    assert not gpu.verify_each_pairs_many(pairs, idx, *B._cols(rows), contexts=ctxs).any()
    forged = [5, 140, 279]
    for i in forged:
        B._s_plus(rows, i, 1)
    exp = B._statuses(pairs, idx, rows, ctxs)
    assert np.nonzero(exp)[0].tolist() == forged
    got = gpu.verify_each_pairs_many(pairs, idx, *B._cols(rows), contexts=ctxs)
    assert np.array_equal(got, exp), _diff(got, exp)


# ---- n = 16,387 over 1000 pairs: the chunk edge --------------------------------------------------------

def test_chunk_edge(gpu, pool):
    """Both sides of the chunk edge of a 256-CU part (16384) and of a 110-CU part (14080); after the
    s + 1 of entry 16384 the last chunk holds a wrong-pair label (16385) and a valid proof (16386),
    which passes only with the chunk's offsets into the rows, pair_idx, ctx_off and ctx_present all
    right (as tests/test_gpu_pairs_bulk.py places them)."""
    n = 16387
    idx = (np.arange(n) % 1000).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    rows = BM._prove_many(gpu, pool, idx, ctxs, b"e-edge")
    forged = [0, 14079, 14080, 16383, 16384]
    for i in forged:
        B._s_plus(rows, i, 1)
    idx[16385] = (idx[16385] + 1) % 1000
    forged.append(16385)
    exp = np.zeros(n, np.uint8)
    exp[forged] = 1
    assert exp[-3:].tolist() == [1, 1, 0]
    near = [j for i in forged for j in (i - 1, i + 1)]
    _sample_ok(pool, idx, rows, ctxs, exp, forged + near + list(range(0, n, 97)))
    gpu.set_timing(True)
    gpu.stage_times()
    got = gpu.verify_each_pairs_many(pool, idx, *B._cols(rows), contexts=ctxs)
    times = gpu.stage_times()
    gpu.set_timing(False)
    assert np.array_equal(got, exp), _diff(got, exp)
    assert times[VARBASE][1] == 1000 and times["verify_each"][1] == 2, times


# ---- npairs = 4096: the bound ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def full4096(gpu):
    """4096 pairs and 4096 valid proofs, entry i under pair i."""
    pairs = BM._many_pairs(gpu, 4096, b"each-4096")
    idx = np.arange(4096, dtype=np.uint32)
    ctxs = [B._ctx(i) for i in range(4096)]
    return pairs, idx, ctxs, BM._prove_many(gpu, pairs, idx, ctxs, b"e4096")


def test_the_bound(gpu, full4096):
    pairs, idx, ctxs, rows = full4096
    rows = {q: rows[q].copy() for q in Q}
    forged = [0, 2077, 4095]
    for i in forged:
        B._s_plus(rows, i, 1)
    exp = np.zeros(4096, np.uint8)
    exp[forged] = 1
    near = [j for i in forged for j in (i - 1, i + 1)]
    _sample_ok(pairs, idx, rows, ctxs, exp, forged + near + list(range(0, 4096, 61)))
    got = gpu.verify_each_pairs_many(pairs, idx, *B._cols(rows), contexts=ctxs)
    assert np.array_equal(got, exp), _diff(got, exp)


def test_errors_write_nothing(gpu, full4096):
    pairs, idx, ctxs, rows = full4096
    n = 16
    cols = B._cols(rows, slice(0, n))
    gh = np.frombuffer(b"".join(p.g + p.h for p in pairs) + pairs[0].g + pairs[1].h, np.uint8).copy()   # 4097 rows
    small = np.arange(n, dtype=np.uint32)
    fb = gpu.fallback_stats()

    def call(npairs, gh_, n_, idx_, cols_=cols, ctxs_=None, out_=True):
        out = np.full(max(n_, 1), 255, np.uint8)
        rc = _raw(gpu, 0, npairs, gh_, n_, idx_, cols_, out if out_ else None, ctxs_)
        assert (out == 255).all()                                  # status_out is untouched
        return rc, _last_error(gpu)

    rc, msg = call(4097, gh, n, small)
    assert rc == _native.CPZ_EINVAL and "CPZ_EACH_PAIRS_MANY_MAX" in msg and "4097" in msg, msg
    assert call(4096, gh, 0, small)[0] == _native.CPZ_EEMPTY
    rc, msg = call(0, gh, n, small)
    assert rc == _native.CPZ_EINVAL and "npairs is 0" in msg, msg
    rc, msg = call(4096, gh, _native.PAIRS_BULK_MAX_PROOFS + 1, small)
    assert rc == _native.CPZ_EINVAL and "CPZ_PAIRS_BULK_MAX_PROOFS" in msg, msg
    for k in range(5):
        broken = list(cols)
        broken[k] = None
        assert call(4096, gh, n, small, broken)[0] == _native.CPZ_EINVAL
    assert call(4096, None, n, small)[0] == _native.CPZ_EINVAL
    assert call(4096, gh, n, None)[0] == _native.CPZ_EINVAL
    assert call(4096, gh, n, small, out_=False)[0] == _native.CPZ_EINVAL
    # an index at npairs, the lowest offending entry named
    bad_idx = small.copy()
    bad_idx[5] = 4096
    bad_idx[9] = 5000
    rc, msg = call(4096, gh, n, bad_idx)
    assert rc == _native.CPZ_EINVAL and "pair_idx[5] = 4096" in msg, msg
    # an undecodable pair at row 3000 and g == h at row 70: the host's check comes first, row 70 named
    gh2 = gh.copy()
    gh2[64 * 3000:64 * 3000 + 32] = BAD_POINT
    rc, msg = call(4096, gh2, n, small)
    assert rc == _native.CPZ_EGENERATOR and "pair 3000" in msg and "decode" in msg, msg
    gh2[64 * 70 + 32:64 * 70 + 64] = gh2[64 * 70:64 * 70 + 32]
    rc, msg = call(4096, gh2, n, small)
    assert rc == _native.CPZ_EGENERATOR and "pair 70" in msg, msg
    gh3 = gh.copy()
    gh3[64 * 9:64 * 9 + 32] = 0                                    # the identity
    rc, msg = call(4096, gh3, n, small)
    assert rc == _native.CPZ_EGENERATOR and "pair 9" in msg, msg
    assert gpu.fallback_stats() == fb
    # and the context still verifies (without their contexts only the entries proven without one pass)
    got = gpu.verify_each_pairs_many(pairs, small, *cols)
    exp = B._statuses(pairs, small, {q: rows[q][:n] for q in Q}, [None] * n)
    assert got.tolist() == exp.tolist() == [0, 1, 1, 1] * 4


# ---- npairs <= 64: forwarding ---------------------------------------------------------------------------

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
    st = g.verify_each_pairs_many(pairs, d["idx"], *[d[q] for q in ("y1", "y2", "r1", "r2", "s")], contexts=ctxs)
    times = g.stage_times()
    resident = g.pairs_resident(pairs)
np.savez(sys.argv[2], st=st, built=times.get("generators_varbase", (0.0, 0))[1], resident=resident)
"""


@pytest.mark.parametrize("npairs", [64, 5])
def test_up_to_64_pairs_it_is_the_bulk_call(gpu, mix65, pool, npairs, tmp_path):
    """Byte-identical statuses and stage launches to verify_each_pairs_bulk on fresh contexts; with
    CPZ_EACH_MANY_FORWARD=0 in a child process the same inputs give the same statuses through the
    small tables (npairs spans counted in stage 13, no set resident afterwards)."""
    n = 2100                                                         # above the latency kernels' range
    pairs = pool[300:300 + npairs]
    idx = (np.arange(n) % npairs).astype(np.uint32)
    ctxs = [B._ctx(i) for i in range(n)]
    rows = BM._prove_many(gpu, pairs, idx, ctxs, b"e-fwd-%d" % npairs)
    B._s_plus(rows, 7, 1)
    rows["y2"][2099] = BAD_POINT
    idx[1000] = (idx[1000] + 1) % npairs
    exp = np.zeros(n, np.uint8)
    exp[[7, 1000]] = 1
    exp[2099] = 2
    _sample_ok(pairs, idx, rows, ctxs, exp, [6, 7, 8, 999, 1000, 1001, 2098, 2099] + list(range(0, n, 53)))
    seen = []
    for name in ("verify_each_pairs_many", "verify_each_pairs_bulk"):
        with cp.Gpu(0) as fresh:
            fresh.set_timing(True)
            fresh.stage_times()
            st = getattr(fresh, name)(pairs, idx, *B._cols(rows), contexts=ctxs)
            times = fresh.stage_times()
            seen.append((st.tobytes(), {k: v[1] for k, v in times.items()}, _resident(fresh, pairs).tolist()))
    assert seen[0] == seen[1]
    assert seen[0][0] == exp.tobytes() and seen[0][1][VARBASE] == npairs and seen[0][2] == [1] * npairs
    # the same inputs through the small tables
    ctx_len = np.array([len(c or b"") for c in ctxs], np.int64)
    ctx = np.zeros((n, 32), np.uint8)
    for i, c in enumerate(ctxs):
        if c:
            ctx[i, :len(c)] = np.frombuffer(c, np.uint8)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, gh=np.frombuffer(b"".join(p.g + p.h for p in pairs), np.uint8).reshape(npairs, 64), idx=idx,
             present=np.array([c is not None for c in ctxs]), ctx=ctx, ctx_len=ctx_len, **rows)
    env = dict(os.environ, CPZ_EACH_MANY_FORWARD="0",
               PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "chaum-pedersen-zkp_amd")] +
                                          [p for p in [os.environ.get("PYTHONPATH")] if p]))
    r = subprocess.run([sys.executable, "-c", CHILD, src, dst], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(dst)
    assert out["st"].tobytes() == exp.tobytes(), _diff(out["st"], exp)
    assert int(out["built"]) == npairs and not out["resident"].any()


# ---- BatchVerifier ------------------------------------------------------------------------------------------

def test_batch_verifier_takes_one_call_for_65_groups(gpu, mix65):
    """130 entries over 65 Parameters, three forged: the oracle's statuses cold and warm, and a warm
    verify() is one verify launch."""
    pairs, idx, ctxs, rows = mix65
    rows = {q: rows[q].copy() for q in Q}
    for i in (3, 64, 129):
        B._s_plus(rows, i, 1)
    exp = B._statuses(pairs, idx, rows, ctxs)
    assert np.nonzero(exp)[0].tolist() == [3, 64, 129]
    with cp.Gpu(0) as fresh:
        b = cp.BatchVerifier(fresh)
        for i in range(130):
            b.add_with_context(pairs[int(idx[i])], cp.Statement(rows["y1"][i].tobytes(), rows["y2"][i].tobytes()),
                               cp.Proof(rows["r1"][i].tobytes(), rows["r2"][i].tobytes(), rows["s"][i].tobytes()),
                               ctxs[i])
        cold = [r.status for r in b.verify()]
        fresh.set_timing(True)
        fresh.stage_times()
        warm = [r.status for r in b.verify()]
        st = fresh.stage_times()
    assert cold == exp.tolist() and warm == exp.tolist()
    assert st["verify_each"][1] == 1, st
    assert st[VARBASE][1] == 65 and "generators" not in st, st
