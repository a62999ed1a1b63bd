"""Per-proof verification with a (g, h) pair per entry (cpz_verify_each_gh, its device form and
cpz_challenges_gh): every entry carries its own generator rows, the eight-lane kernel decodes them
beside Y and R and builds their small tables in the proof's own scratch, and a bad pair is a status
(6) of its entry, never an error of the call.

The pairs come from gpu.derive_pairs and the proofs from gpu.prove_pairs_many, in slices of at most
4096 pairs; scalars, contexts, columns and forgeries are those of tests/test_gpu_batch_pairs_many.py
and tests/test_gpu_batch_pairs.py, whose helpers are used here.  Expected statuses are the C oracle's
verify_one under the entry's own pair, and 6 where Parameters::with_generators would fail."""
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
SLICE = _native.EACH_PAIRS_MANY_MAX
ZERO = bytes(32)


def _diff(got, exp):
    bad = np.nonzero(got != exp)[0]
    return bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist()


def _derive(gpu, n, tag):
    """n distinct pairs as uint8[n, 64] rows (g then h), 4096 labels a call."""
    return np.concatenate([gpu.derive_pairs([tag + b"/%d" % i for i in range(c, min(c + SLICE, n))])
                           for c in range(0, n, SLICE)])


def _params(gh):
    return [cp.Parameters(r[:32].tobytes(), r[32:].tobytes()) for r in gh]


def _prove(gpu, gh, ctxs, tag):
    """Valid proofs, entry i under row i of gh, 4096 entries (and pairs) a prove_pairs_many call."""
    n = len(gh)
    xs, ks = BM._scalars(tag + b"-x", n), BM._scalars(tag + b"-k", n)
    rows = {q: np.zeros((n, 32), np.uint8) for q in Q}
    for c in range(0, n, SLICE):
        m = min(SLICE, n - c)
        out = gpu.prove_pairs_many(_params(gh[c:c + m]), np.arange(m, dtype=np.uint32), np.ascontiguousarray(xs[c:c + m]),
                                   np.ascontiguousarray(ks[c:c + m]), contexts=ctxs[c:c + m])
        for q in Q:
            rows[q][c:c + m] = out[q]
    return rows


def _expected(gh, rows, ctxs, sel):
    """{i: status} for the entries sel: 6 where with_generators(g_i, h_i) would fail (the oracle
    reports a generator that does not decode; the identity and g == h are decided by the bytes), else
    the C oracle's verify_one under (g_i, h_i)."""
    import coracle
    out = {}
    for i in sel:
        g, h = gh[i, :32].tobytes(), gh[i, 32:].tobytes()
        if g == ZERO or h == ZERO or g == h:
            out[i] = 6
            continue
        st = coracle.verify_one(g, h, *[rows[q][i].tobytes() for q in Q], ctxs[i])
        out[i] = 6 if st < 0 else st
    return out


def _call(g, gh, rows, ctxs, sel=slice(None), **kw):
    gh = gh[sel]
    return g.verify_each_gh(np.ascontiguousarray(gh[:, :32]), np.ascontiguousarray(gh[:, 32:]), *B._cols(rows, sel),
                            contexts=ctxs[sel], **kw)


def _chunk_max():
    """Proofs of one verify launch: half the eight-lane bound, which is 128 proofs per CU up to 16384."""
    import torch
    return min(16384, 128 * torch.cuda.get_device_properties(0).multi_processor_count) // 2


# ---- n = 1, 33, 130 and the special entries ---------------------------------------------------------------

NBASE = 130
# the entries after the valid ones, by offset: the seven forgeries of tests/test_gpu_each_pairs_many.py (the
# wrong pair: h swapped between two entries), the five bad-generator kinds, a bad generator with a bad y1, the
# default pair, two entries sharing one row
EXTRA = {"s_plus_1": 0, "swap_a": 1, "swap_b": 2, "bad_y": 3, "bad_r": 4, "s_plus_l": 5, "identity_r1": 6, "zero_s": 7,
         "g_undecodable": 8, "h_undecodable": 9, "g_identity": 10, "h_identity": 11, "g_equals_h": 12,
         "bad_g_and_bad_y1": 13, "default_pair": 14, "shared_a": 15, "shared_b": 16}
NEXTRA = len(EXTRA)
EXTRA_STATUS = {"s_plus_1": 1, "swap_a": 1, "swap_b": 1, "bad_y": 2, "bad_r": 2, "s_plus_l": 3, "identity_r1": 4,
                "zero_s": 5, "g_undecodable": 6, "h_undecodable": 6, "g_identity": 6, "h_identity": 6, "g_equals_h": 6,
                "bad_g_and_bad_y1": 6, "default_pair": 0, "shared_a": 0, "shared_b": 0}


@pytest.fixture(scope="module")
def pool(gpu):
    """NBASE + NEXTRA valid proofs, every entry under its own pair but the default-pair entry and the two
    that share a row; contexts cycling the four shapes."""
    n = NBASE + NEXTRA
    gh = _derive(gpu, n, b"each-gh-pool").copy()
    dg, dh = cp.default_generators()
    gh[NBASE + EXTRA["default_pair"]] = np.frombuffer(dg + dh, np.uint8)
    gh[NBASE + EXTRA["shared_b"]] = gh[NBASE + EXTRA["shared_a"]]
    ctxs = [B._ctx(i) for i in range(n)]
    return gh, ctxs, _prove(gpu, gh, ctxs, b"each-gh")


def _with_extras(pool, n):
    """The first n valid entries followed by the NEXTRA special ones: (gh, rows, ctxs, expected)."""
    gh0, ctxs0, rows0 = pool
    sel = list(range(n)) + list(range(NBASE, NBASE + NEXTRA))
    gh = gh0[sel].copy()
    rows = {q: rows0[q][sel].copy() for q in Q}
    ctxs = [ctxs0[i] for i in sel]
    at = {k: n + v for k, v in EXTRA.items()}
    B._s_plus(rows, at["s_plus_1"], 1)
    a, b = at["swap_a"], at["swap_b"]
    gh[[a, b], 32:] = gh[[b, a], 32:]
    rows["y1"][at["bad_y"]] = BAD_POINT
    rows["r2"][at["bad_r"]] = BAD_POINT
    B._s_plus(rows, at["s_plus_l"], O.L)
    rows["r1"][at["identity_r1"]] = 0
    rows["s"][at["zero_s"]] = 0
    gh[at["g_undecodable"], :32] = BAD_POINT
    gh[at["h_undecodable"], 32:] = BAD_POINT
    gh[at["g_identity"], :32] = 0
    gh[at["h_identity"], 32:] = 0
    gh[at["g_equals_h"], 32:] = gh[at["g_equals_h"], :32]
    gh[at["bad_g_and_bad_y1"], :32] = BAD_POINT
    rows["y1"][at["bad_g_and_bad_y1"]] = BAD_POINT
    exp = np.zeros(n + NEXTRA, np.uint8)
    for k, v in EXTRA_STATUS.items():
        exp[at[k]] = v
    want = _expected(gh, rows, ctxs, range(n + NEXTRA))
    assert [want[i] for i in range(n + NEXTRA)] == exp.tolist()
    return gh, rows, ctxs, exp, at


@pytest.mark.parametrize("n", [1, 33, 130])
def test_every_entry_under_its_own_pair(gpu, pool, n):
    gh0, ctxs0, rows0 = pool
    assert [type(c) for c in ctxs0[:4]] == [type(None), bytes, bytes, bytes] and [len(c) for c in ctxs0[1:4]] == [32, 5, 0]
    assert len({r.tobytes() for r in gh0[:n]}) == n
    want = _expected(gh0, rows0, ctxs0, range(n))
    assert set(want.values()) == {0}
    got = _call(gpu, gh0, rows0, ctxs0, slice(0, n))
    assert got.tolist() == [0] * n
    gh, rows, ctxs, exp, at = _with_extras(pool, n)
    got = _call(gpu, gh, rows, ctxs)
    assert np.array_equal(got, exp), _diff(got, exp)
    assert got[at["bad_g_and_bad_y1"]] == cp.STATUS_BAD_GENERATOR == 6
    assert cp.VerifyResult(6).error().args == ("Invalid generators",)
    # the default-pair entry is verify_each's
    d = at["default_pair"]
    one = gpu.verify_each(*[rows[q][d:d + 1] for q in Q], contexts=ctxs[d:d + 1])
    assert one.tolist() == [got[d]] == [0]
    # commitment checks off, for the call and for the context: the identity commitment and the zero s are
    # judged by the equations, which a valid proof with its r1 or s replaced cannot satisfy
    exp_eq = exp.copy()
    exp_eq[[at["identity_r1"], at["zero_s"]]] = 1
    got = _call(gpu, gh, rows, ctxs, equations_only=True)
    assert np.array_equal(got, exp_eq), _diff(got, exp_eq)
    gpu.set_commitment_checks(False)
    try:
        got = _call(gpu, gh, rows, ctxs)
    finally:
        gpu.set_commitment_checks(True)
    assert np.array_equal(got, exp_eq), _diff(got, exp_eq)


def test_challenges_gh(gpu, pool):
    import coracle
    gh, ctxs, rows = pool
    n = NBASE
    got = gpu.challenges_gh(np.ascontiguousarray(gh[:n, :32]), np.ascontiguousarray(gh[:n, 32:]),
                            *B._cols(rows, slice(0, n))[:4], contexts=ctxs[:n])
    assert got.shape == (n, 32)
    for i in range(n):
        want = coracle.challenge(gh[i, :32].tobytes(), gh[i, 32:].tobytes(), *[rows[q][i].tobytes() for q in Q[:4]], ctxs[i])
        assert got[i].tobytes() == want, i


# ---- the chunk edges -----------------------------------------------------------------------------------------

NBIG = 3 * 8192 + 1


@pytest.fixture(scope="module")
def big(gpu):
    """3 * 8192 + 1 valid proofs, every entry under its own pair."""
    gh = _derive(gpu, NBIG, b"each-gh-big")
    ctxs = [B._ctx(i) for i in range(NBIG)]
    return gh, ctxs, _prove(gpu, gh, ctxs, b"each-gh-big")


# 2 * 8192 + 4: the last chunk of a 256-CU part holds a forged entry, a wrong-pair one, a valid one and the last
@pytest.mark.parametrize("n", [8193, 2 * 8192 + 4, NBIG])
def test_chunk_edges(gpu, big, n):
    """Both sides of every chunk edge of a 256-CU part (multiples of 8192) and of a 110-CU part (of 7040),
    and the last entry, carry s + 1.  At the last chunk start with three entries before the last one (n = 8193:
    the 110-CU edge) the forged entry is followed by one whose h is its neighbour's and by a valid one: the three
    pass and fail as expected only with the chunk's offsets into g, h, the rows, the contexts and the challenges
    all right."""
    gh0, ctxs0, rows0 = big
    gh = gh0[:n].copy()
    ctxs = ctxs0[:n]
    rows = {q: rows0[q][:n].copy() for q in Q}
    edges = sorted(e for step in (8192, 7040) for e in range(step, n, step))
    forged = sorted({i for e in edges for i in (e - 1, e)} | {0, n - 1})
    for i in forged:
        B._s_plus(rows, i, 1)
    room = [e for e in edges if e + 3 <= n - 1]
    base = max([e for e in room if e % 8192 == 0] or room)
    assert base == {8193: 7040, 2 * 8192 + 4: 16384, NBIG: 16384}[n]
    wrong = [base + 1]
    gh[base + 1, 32:] = gh0[base + 2, 32:]              # proven under its own h, carries the next entry's
    exp = np.zeros(n, np.uint8)
    exp[forged + wrong] = 1
    assert exp[base:base + 3].tolist() == [1, 1, 0] and exp[n - 1] == 1
    near = [j for i in forged + wrong for j in (i - 1, i + 1) if 0 <= j < n]
    sample = sorted(set(forged + wrong + near))
    sample += [i for i in range(0, n, 211) if i not in sample][:300 - len(sample)]
    assert len(sample) <= 300
    want = _expected(gh, rows, ctxs, sample)
    assert [want[i] for i in sample] == exp[sample].tolist()
    gpu.set_timing(True)
    gpu.stage_times()
    got = _call(gpu, gh, rows, ctxs)
    times = gpu.stage_times()
    gpu.set_timing(False)
    assert np.array_equal(got, exp), _diff(got, exp)
    chunks = -(-n // _chunk_max())
    assert times["verify_each"][1] == chunks and times["challenge"][1] == chunks, times
    assert "generators" not in times and "generators_varbase" not in times, times


# ---- the device form -----------------------------------------------------------------------------------------

def test_device_form_on_a_stream(gpu, pool):
    import torch
    gh, rows, ctxs, exp, at = _with_extras(pool, NBASE)
    n = len(exp)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    g, h = t(gh[:, :32]), t(gh[:, 32:])
    cols = [t(rows[q]) for q in Q]
    blob, off, present = cp._ctx_arrays(ctxs, n)
    d_blob, d_off, d_present = t(blob), t(off.astype(np.int64)), t(present)
    status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    gpu.verify_each_gh_device(g, h, *cols, status, stream=stream.cuda_stream, ctx_bytes=d_blob, ctx_off=d_off,
                              ctx_present=d_present)
    stream.synchronize()
    got = status.cpu().numpy()
    assert np.array_equal(got, exp), _diff(got, exp)
    # a misaligned row: CPZ_EINVAL, the output untouched
    status.fill_(0xEE)
    torch.cuda.synchronize()
    shifted = torch.zeros(32 * n + 16, dtype=torch.uint8, device=dev)[8:8 + 32 * n]
    assert shifted.data_ptr() % 16 == 8
    for k in range(7):
        args = [g, h] + cols
        args[k] = shifted
        with pytest.raises(cp.CpzError) as err:
            gpu.verify_each_gh_device(*args, status, stream=stream.cuda_stream)
        assert err.value.code == _native.CPZ_EINVAL and "16-byte aligned" in str(err.value)
    stream.synchronize()
    assert (status.cpu().numpy() == 0xEE).all()
    # and later calls on the context are ordered after the device form's work
    gpu.verify_each_gh_device(g, h, *cols, status, stream=stream.cuda_stream, ctx_bytes=d_blob, ctx_off=d_off,
                              ctx_present=d_present)
    again = _call(gpu, gh, rows, ctxs)
    stream.synchronize()
    assert np.array_equal(again, exp) and np.array_equal(status.cpu().numpy(), exp)


# ---- no side effects -----------------------------------------------------------------------------------------

def test_no_side_effects(pool):
    gh, ctxs, rows = pool
    n = NBASE
    some, others = _params(gh[:64]), _params(gh[64:128])
    with cp.Gpu(0) as fresh:
        assert not fresh.pairs_resident(some).any()
        _call(fresh, gh, rows, ctxs, slice(0, n))
        assert not fresh.pairs_resident(some).any() and not fresh.pairs_resident(others).any()
        assert fresh.load_pairs(some) == 64
        before = fresh.pairs_resident(some)
        assert before.all()
        fb = fresh.fallback_stats()
        fresh.set_timing(True)
        fresh.stage_times()
        got = _call(fresh, gh, rows, ctxs, slice(0, n))
        times = fresh.stage_times()
        assert got.tolist() == [0] * n
        assert "generators" not in times and "generators_varbase" not in times, times
        assert times["verify_each"][1] == 1 and times["challenge"][1] == 1 and times["verify_span"][1] == 1, times
        assert fresh.pairs_resident(some).tolist() == before.tolist()
        assert fresh.fallback_stats() == fb
        # the least recently used of the resident sets is still the first to go
        fresh.load_pairs(some[1:])                                  # some[0] is now the least recently used
        _call(fresh, gh, rows, ctxs, slice(0, n))
        assert fresh.load_pairs(others[:1]) == 1
        assert fresh.pairs_resident(some).tolist() == [False] + [True] * 63


# ---- agreement with the existing path ---------------------------------------------------------------------------

def test_agrees_with_verify_each_pairs_many(gpu, big):
    gh0, ctxs0, rows0 = big
    n = 1000
    gh = gh0[:n].copy()
    ctxs = ctxs0[:n]
    rows = {q: rows0[q][:n].copy() for q in Q}
    B._s_plus(rows, 3, 1)
    gh[[10, 11], 32:] = gh[[11, 10], 32:]
    rows["y1"][20] = BAD_POINT
    rows["r2"][33] = BAD_POINT
    B._s_plus(rows, 47, O.L)
    rows["r1"][77] = 0
    rows["s"][999] = 0
    exp = np.zeros(n, np.uint8)
    exp[[3, 10, 11, 20, 33, 47, 77, 999]] = [1, 1, 1, 2, 2, 3, 4, 5]
    for kw in ({}, {"equations_only": True}):
        many = gpu.verify_each_pairs_many(_params(gh), np.arange(n, dtype=np.uint32), *B._cols(rows), contexts=ctxs, **kw)
        got = _call(gpu, gh, rows, ctxs, **kw)
        assert np.array_equal(got, many), _diff(got, many)
        if not kw:
            assert np.array_equal(got, exp), _diff(got, exp)
