"""Mixed-pair per-proof verification (cpz_verify_each_pairs): one call and one verify launch for
entries that carry their own (g, h), as every BatchVerifier entry does (batch.rs:52).  Proof i
reads pair_idx[i] and verifies from that pair's 128-entry tables, with that pair's transcript
prefix, generator words and challenge schedules (k_verify_wide_pairs up to 512 proofs,
k_verify_small_pairs up to 2048).  Expected statuses are the C oracle's verify_one under the
entry's own generators, and the same entries through per-group verify_each calls on the same
context must give the same bytes."""
import hashlib

import numpy as np
import pytest

import chaum_pedersen as cp
import pyoracle as O
from chaum_pedersen import _native

pytestmark = pytest.mark.gpu

Q = ("y1", "y2", "r1", "r2", "s")
NPAIRS = 64
N = 1000


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


def _oracle(pairs, groups, rows, ctxs):
    import coracle
    return np.array([coracle.verify_one(pairs[int(groups[i])].g, pairs[int(groups[i])].h,
                                        *(rows[q][i].tobytes() for q in Q), ctx=ctxs[i])
                     for i in range(len(groups))], np.uint8)


def _per_group(gpu, pairs, groups, rows, ctxs, equations_only=False):
    """The same entries as one verify_each call per pair (what a caller had to do before)."""
    groups = np.asarray(groups)
    out = np.full(len(groups), 255, np.uint8)
    for p in sorted(set(groups.tolist())):
        idx = np.nonzero(groups == p)[0]
        out[idx] = gpu.verify_each(*[np.ascontiguousarray(rows[q][idx]) for q in Q], contexts=[ctxs[i] for i in idx],
                                   params=pairs[p], equations_only=equations_only)
    return out


def _cols(rows, sel=slice(None)):
    return [rows[q][sel].copy() for q in Q]


def _s_plus(rows, i, d):
    v = int.from_bytes(rows["s"][i].tobytes(), "little") + d
    rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)


@pytest.fixture(scope="module")
def mixed(gpu):
    """1000 valid proofs over 64 custom pairs, entry i under pair i % 64 (so the 8 proofs of
    every k_verify_small workgroup carry 8 different pairs), contexts of all four shapes.
    Shared by the tests below, which copy what they forge."""
    pairs = _pairs(NPAIRS, b"mixed")
    groups = np.arange(N) % NPAIRS
    ctxs = [_ctx(i) for i in range(N)]
    rows = _prove(gpu, pairs, groups, ctxs, b"mx")
    return pairs, groups, ctxs, rows


def test_wide_kernel_smallest_mix(gpu):
    """n = 7 over the default pair and two custom ones; entry 4 has s + 1 and entry 5 is proven
    under pair 1 but labelled pair 2 (a wrong table or a wrong transcript prefix accepts it)."""
    pairs = [cp.Parameters()] + _pairs(2, b"wide")
    idx = np.array([0, 1, 2, 1, 0, 2, 1], np.uint32)
    ctxs = [_ctx(i) for i in range(7)]
    proven = idx.copy()
    proven[5] = 1
    rows = _prove(gpu, pairs, proven, ctxs, b"wd")
    _s_plus(rows, 4, 1)
    exp = _oracle(pairs, idx, rows, ctxs)
    assert exp.tolist() == [0, 0, 0, 0, 1, 1, 0]
    got = gpu.verify_each_pairs(pairs, idx, *_cols(rows), contexts=ctxs)
    assert got.tolist() == exp.tolist()
    assert got.tobytes() == _per_group(gpu, pairs, idx, rows, ctxs).tobytes()
    # duplicate rows in `pairs` are allowed: pair 3 repeats pair 1
    dup = gpu.verify_each_pairs(pairs + [pairs[1]], np.where(idx == 1, 3, idx), *_cols(rows), contexts=ctxs)
    assert dup.tolist() == exp.tolist()


@pytest.mark.parametrize("equations_only", [False, True])
def test_small_kernel_pairs_mixed_inside_a_workgroup(gpu, mixed, equations_only):
    """n = 521: above the 512-proof wide bound, 65 full workgroups of 8 different pairs and one
    proof plus 7 dead slots in the last.  Forgeries as above plus the decode-level statuses."""
    pairs, groups, ctxs, rows = mixed
    n = 521
    groups = groups[:n].copy()
    ctxs = list(ctxs[:n])
    rows = {q: rows[q][:n].copy() for q in Q}
    _s_plus(rows, 9, 1)                                    # s + 1
    _s_plus(rows, 520, 1)                                  # ... and in the last workgroup
    groups[77] = (groups[77] + 1) % NPAIRS                 # proven under pair 13, labelled pair 14
    groups[300] = (groups[300] + 8) % NPAIRS               # ... without a context (entry 77: 32 bytes)
    groups[302] = (groups[302] + 1) % NPAIRS               # ... with a 5-byte context (the byte-wise sponge)
    rows["r1"][130] = np.frombuffer(bytes.fromhex("01" + "00" * 31), np.uint8)   # undecodable point
    _s_plus(rows, 201, O.L)                                # s + l: not canonical
    rows["s"][262] = 0                                     # zero s
    rows["r2"][407] = 0                                    # identity commitment
    exp = _oracle(pairs, groups, rows, ctxs)
    assert [int(exp[i]) for i in (9, 520, 77, 300, 302, 130, 201, 262, 407)] == [1, 1, 1, 1, 1, 2, 3, 5, 4]
    assert (exp == 0).sum() == n - 9
    if equations_only:
        # commitment checks off: the zero s and the identity commitment are judged by the equations,
        # which a valid proof with its s or r2 replaced cannot satisfy (test_gpu_varbase asserts the same)
        exp[[262, 407]] = 1
    got = gpu.verify_each_pairs(pairs, groups, *_cols(rows), contexts=ctxs, equations_only=equations_only)
    assert np.array_equal(got, exp), (np.nonzero(got != exp)[0][:8], got[got != exp][:8], exp[got != exp][:8])
    assert got.tobytes() == _per_group(gpu, pairs, groups, rows, ctxs, equations_only).tobytes()


def test_residency_every_pair_of_a_call_is_cached_at_once(gpu, mixed):
    """A fresh context has 64 light-set slots, all empty.  Call A over 64 pairs fills them (64
    builds).  Call B over 64 other pairs evicts the least recently used set each time, which is
    always one of A's (B's own sets carry later stamps): 64 builds, and none of A's pairs is
    left.  Call C lists 32 of A's pairs, then 32 new ones: all 64 miss, and each build evicts one
    of B's sets (stamped before every set of C) -- 64 builds, never a set of the same call.
    No comb is built (stage 7)."""
    pairs_a, _, ctxs_a, rows_a = mixed
    others = _pairs(96, b"resident")
    ctxs_o = [_ctx(i + 1) for i in range(96)]
    rows_o = _prove(gpu, others, np.arange(96), ctxs_o, b"rs")
    idx = np.arange(64, dtype=np.uint32)

    def join(ra, sa, rb, sb):
        return [np.ascontiguousarray(np.concatenate([ra[q][sa], rb[q][sb]])) for q in Q]

    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        calls = (
            (pairs_a, _cols(rows_a, slice(0, 64)), ctxs_a[:64]),
            (others[:64], _cols(rows_o, slice(0, 64)), ctxs_o[:64]),
            (pairs_a[:32] + others[64:], join(rows_a, slice(0, 32), rows_o, slice(64, 96)), ctxs_a[:32] + ctxs_o[64:]),
        )
        for pairs, cols, ctxs in calls:
            cols[4][5] = cols[4][6]            # entry 5 takes entry 6's s: status 1
            exp = np.zeros(64, np.uint8)
            exp[5] = 1
            got = fresh.verify_each_pairs(pairs, idx, *cols, contexts=ctxs)
            st = fresh.stage_times()
            assert got.tolist() == exp.tolist()
            assert st.get("generators_varbase", (0.0, 0))[1] == 64, st
            assert st.get("generators", (0.0, 0))[1] == 0, st
        # the third call's pairs are all resident now: nothing is built
        fresh.verify_each_pairs(calls[2][0], idx, *calls[2][1], contexts=calls[2][2])
        assert "generators_varbase" not in fresh.stage_times()


def test_batch_verifier_issues_one_launch_for_64_groups(gpu, mixed):
    """1000 BatchVerifier entries over 64 Parameters: a warm verify() is one verify launch, not
    one per group, and returns the oracle's statuses."""
    pairs, groups, ctxs, rows = mixed
    rows = {q: rows[q].copy() for q in Q}
    for i in (3, 500, 999):
        _s_plus(rows, i, 1)
    exp = _oracle(pairs, groups, rows, ctxs)
    assert exp.sum() == 3
    with cp.Gpu(0) as fresh:
        b = cp.BatchVerifier(fresh)
        for i in range(N):
            b.add_with_context(pairs[int(groups[i])], cp.Statement(rows["y1"][i].tobytes(), rows["y2"][i].tobytes()),
                               cp.Proof(rows["r1"][i].tobytes(), rows["r2"][i].tobytes(), rows["s"][i].tobytes()),
                               ctxs[i])
        cold = [r.status for r in b.verify()]
        fresh.set_timing(True)
        fresh.stage_times()
        warm = [r.status for r in b.verify()]
        st = fresh.stage_times()
    assert cold == exp.tolist() and warm == exp.tolist()
    assert st["verify_each"][1] < NPAIRS, st
    assert st["verify_each"][1] == 1, st
    assert "generators_varbase" not in st and "generators" not in st


def test_errors_are_returned_before_any_launch(gpu, mixed):
    pairs, groups, ctxs, rows = mixed
    lib, h = gpu._lib, gpu._h
    n = 16
    cols = _cols(rows, slice(0, n))
    gh = np.frombuffer(b"".join(p.g + p.h for p in pairs) + bytes(64), np.uint8).copy()   # 65 rows
    idx = np.arange(n, dtype=np.uint32)
    out = np.full(n, 255, np.uint8)

    def call(npairs, gh_, n_, idx_, cols_=cols):
        return lib.cpz_verify_each_pairs(h, npairs, gh_.ctypes.data, n_, idx_.ctypes.data,
                                         *[c.ctypes.data for c in cols_], None, None, None, out.ctypes.data)

    assert call(0, gh, n, idx) == _native.CPZ_EINVAL
    assert call(65, gh, n, idx) == _native.CPZ_EINVAL
    assert b"CPZ_PAIRS_MAX" in lib.cpz_last_error()
    assert call(64, gh, 0, idx) == _native.CPZ_EEMPTY
    big = [np.zeros((2049, 32), np.uint8) for _ in Q]
    assert call(64, gh, 2049, np.zeros(2049, np.uint32), big) == _native.CPZ_EINVAL
    bad = idx.copy()
    bad[11] = 64
    assert call(64, gh, n, bad) == _native.CPZ_EINVAL
    assert b"pair_idx[11]" in lib.cpz_last_error()
    assert lib.cpz_verify_each_pairs(h, 64, None, n, idx.ctypes.data, *[c.ctypes.data for c in cols], None, None,
                                     None, out.ctypes.data) == _native.CPZ_EINVAL
    for what, g2, h2 in (("identity", bytes(32), pairs[2].h), ("equal", pairs[2].g, pairs[2].g),
                         ("undecodable", bytes.fromhex("01" + "00" * 31), pairs[2].h)):
        ghb = gh.copy()
        ghb[128:192] = np.frombuffer(g2 + h2, np.uint8)
        assert call(64, ghb, n, idx) == _native.CPZ_EGENERATOR, what
        assert b"pair 2" in lib.cpz_last_error(), what
    assert (out == 255).all()                              # nothing was written by the refused calls
    # the context still serves a valid call
    exp = _oracle(pairs, groups[:n], {q: rows[q][:n] for q in Q}, ctxs[:n])
    got = gpu.verify_each_pairs(pairs, idx, *cols, contexts=ctxs[:n])
    assert got.tolist() == exp.tolist() == [0] * n
    with pytest.raises(_native.CpzError) as e:
        gpu.verify_each_pairs(pairs + [cp.Parameters()], idx, *cols, contexts=ctxs[:n])
    assert e.value.code == _native.CPZ_EINVAL
