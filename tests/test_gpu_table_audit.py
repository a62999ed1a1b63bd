"""GPU audit of the precomputed tables and of the digit handling of every per-proof kernel.

a. The 2 x 16 x 32769-entry fixed-base combs (k_comb_bases, k_comb_fill), of the default pair
   and of a custom pair: the prover multiplies by scalars that select every entry a canonical
   scalar can reach (tests/digit_vectors.py comb_audit_scalars) and the C oracle verifies every
   proof; a stride is compared byte for byte with the Python oracle.
b. Digit extremes of s' = v s mod l -- comb slot 32768, tab[127], the carry out of byte 15, the
   largest top digits -- with one challenge of every class of the split, through k_verify_wide,
   k_verify_small, k_verify_quad and k_verify_each, on the combs (default pair) and on the
   128-entry Niels tables (k_niels_bases, k_build_niels: a custom pair on a fresh context).
c. Degenerate relations between a proof's points through the same kernels.

Every expected status is the Python oracle's verify_response under the entry's pair; every
comparison is exact."""
import os
import random

import numpy as np
import pytest

import chaum_pedersen as cp
import digit_vectors as DV
import pyoracle as O
from test_gpu_varbase import _pairs

pytestmark = pytest.mark.gpu

L = O.L
KERNEL_SIZES = [(480, "wide"), (513, "small"), (2049, "quad"), (16385, "each")]
FIELDS = ("y1", "y2", "r1", "r2", "s")


def _pair(which):
    """(Parameters, g, h as points)."""
    params = cp.Parameters() if which == "default" else _pairs(1, tag=b"table-audit")[0]
    return params, O.ristretto_decode(params.g), O.ristretto_decode(params.h)


def _rows32(values):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), np.uint8).reshape(-1, 32)


def _enc(p, k):
    return O.ristretto_encode(O.pt_mul(p, k))


# ---- a. the combs, through the prover -----------------------------------------------------------

@pytest.fixture(scope="module")
def audit_scalars():
    """x = comb_audit_scalars(); k = the same values permuted: k_i = x_((40503 i + 1) mod 65536)
    on the 65,536 enumerating values (40503 is odd, and 40502 i = -1 has no solution, so k_i is
    never x_i) and the five tail values rotated by one."""
    xs = DV.comb_audit_scalars()
    body = DV.COMB_AUDIT_BODY
    tail = list(xs[body:])
    ks = [xs[(40503 * i + 1) % body] for i in range(body)] + tail[1:] + tail[:1]
    assert sorted(ks) == sorted(xs) and all(a != b for a, b in zip(xs, ks))
    return xs, ks, _rows32(xs), _rows32(ks)


def _report_comb_failures(bad, xs, ks, rows, g, h):
    """The rejected proofs' (window, digit) pairs, which of their four points differ from the
    Python oracle's (that names the base and the scalar whose digits met the wrong entry), and
    the pairs that no accepted proof uses."""
    users = {}
    for i in range(len(xs)):
        for w, d in enumerate(DV.recode16(xs[i])):
            users.setdefault((w, d), []).append(i)
        for w, d in enumerate(DV.recode16(ks[i])):
            users.setdefault((w, d), []).append(i)
    failing = set(int(i) for i in bad)
    suspects = sorted(wd for wd, idx in users.items() if wd[1] != 0 and set(idx) <= failing)
    print("comb audit: %d proofs rejected, first indices %r" % (len(failing), sorted(failing)[:16]))
    for i in sorted(failing)[:4]:
        want = (_enc(g, xs[i]), _enc(h, xs[i]), _enc(g, ks[i]), _enc(h, ks[i]))
        wrong = [q for q, w in zip(FIELDS[:4], want) if rows[q][i].tobytes() != w]
        print("  proof %d: points differing from the oracle's: %r" % (i, wrong))
        print("  proof %d: x (window, digit) %r" % (i, list(enumerate(DV.recode16(xs[i])))))
        print("  proof %d: k (window, digit) %r" % (i, list(enumerate(DV.recode16(ks[i])))))
    print("  (window, digit) pairs used only by rejected proofs: %r" % suspects[:32])
    return suspects


@pytest.mark.parametrize("which", ["default", "custom"])
def test_comb_audit_through_prover(gpu, audit_scalars, which):
    """Every comb entry of both bases that a canonical scalar selects is read by exactly one
    witness and one nonce of 65,541 proofs (2^16 signed digits per window: no smaller batch
    enumerates the comb).  A wrong entry breaks one equation of the proof that read it: the C
    oracle must accept all of them; on a stride of 1024 and the tail the five fields equal the
    Python oracle's."""
    import coracle
    params, g, h = _pair(which)
    xs, ks, xrows, krows = audit_scalars
    rows = gpu.prove(xrows, krows, params=params)
    threads = min(16, len(os.sched_getaffinity(0)))
    st = coracle.verify_many(rows, g=params.g, h=params.h, threads=threads)
    bad = np.nonzero(st)[0]
    suspects = _report_comb_failures(bad, xs, ks, rows, g, h) if bad.size else []
    assert bad.size == 0, (which, bad[:16].tolist(), st[bad[:16]].tolist(), suspects[:8])
    sample = list(range(0, DV.COMB_AUDIT_BODY, 1024)) + list(range(DV.COMB_AUDIT_BODY, len(xs)))
    for i in sample:
        x, k = xs[i], ks[i]
        want = (_enc(g, x), _enc(h, x), _enc(g, k), _enc(h, k))
        got = tuple(rows[q][i].tobytes() for q in FIELDS[:4])
        assert got == want, (which, i, [a == b for a, b in zip(got, want)], list(enumerate(DV.recode16(x))),
                             list(enumerate(DV.recode16(k))))
        c = O.challenge(params.g, params.h, *want)
        assert int.from_bytes(rows["s"][i].tobytes(), "little") == (k + c * x) % L, (which, i)


@pytest.mark.parametrize("which", ["default", "custom"])
def test_prover_takes_scalars_mod_l(gpu, which):
    """cpz_prove: witnesses and nonces at and above l (l, l + 1, 2^255 - 19, 2^256 - 1) are taken
    mod l: the proofs are the oracle's for the reduced values (l itself gives the identity)."""
    params, g, h = _pair(which)
    big = [L, L + 1, 2**255 - 19, 2**256 - 1]
    xs = big + [5, L - 1, big[2]]
    ks = big[1:] + big[:1] + [big[3], big[0] + 7, 9]
    rows = gpu.prove(_rows32(xs), _rows32(ks), params=params)
    for i, (x, k) in enumerate(zip(xs, ks)):
        want = O.prove(x % L, k % L, None, g, h)
        for q in FIELDS:
            assert rows[q][i].tobytes() == getattr(want, q), (which, i, q)
    assert rows["y1"][0].tobytes() == bytes(32) and rows["r1"][3].tobytes() == bytes(32)


# ---- b. digit edges through every per-proof kernel and both table forms -------------------------

def _tile(a, n):
    return np.ascontiguousarray(a[np.arange(n) % len(a)])


def _cols(recs, cbytes):
    cols = [np.frombuffer(b"".join(getattr(r, q) for r in recs), np.uint8).reshape(-1, 32) for q in FIELDS]
    return cols + [np.frombuffer(b"".join(cbytes), np.uint8).reshape(-1, 32)]


def _edge_entries(which):
    """Valid entries whose s' runs over comb_edge_scalars() and table_audit_scalars(), paired
    round-robin with one challenge per class of the split; on every eighth, two forged copies --
    y1 alone replaced by [x + 1] g (equation 1 wrong) and y2 alone by [x + 1] h (equation 2
    wrong).  Expected statuses: the Python oracle's under the pair, computed once."""
    params, g, h = _pair(which)
    rnd = random.Random(31)
    cs = DV.challenge_list()
    witnesses = [rnd.randrange(1, L) for _ in range(4)]
    ys = {x: (_enc(g, x), _enc(h, x)) for x in witnesses}
    off = {x: (_enc(g, x + 1), _enc(h, x + 1)) for x in witnesses}
    recs, cb, labels = [], [], []
    for j, sigma in enumerate(DV.comb_edge_scalars() + DV.table_audit_scalars()):
        c = cs[j % len(cs)]
        x = witnesses[j % 4]
        rec, cbytes, x2, _ = DV.build_entry(sigma, c, g, h, x, ys[x])
        assert x2 == x
        recs.append(rec)
        cb.append(cbytes)
        labels.append(("valid", sigma, c))
        if j % 8 == 7:
            recs.append(O.ProofRecord(off[x][0], rec.y2, rec.r1, rec.r2, rec.s))
            recs.append(O.ProofRecord(rec.y1, off[x][1], rec.r1, rec.r2, rec.s))
            cb += [cbytes, cbytes]
            labels += [("equation 1 wrong", sigma, c), ("equation 2 wrong", sigma, c)]
    assert len(recs) <= KERNEL_SIZES[0][0]   # the smallest launch holds every entry
    want = np.array([O.verify_response(r, c, params.g, params.h) for r, c in zip(recs, cb)], np.uint8)
    for (kind, _, _), w in zip(labels, want):
        assert w == (O.ST_OK if kind == "valid" else O.ST_EQ_FAIL)
    return params, _cols(recs, cb), want, labels


@pytest.fixture(scope="module")
def edge_default():
    return _edge_entries("default")


@pytest.fixture(scope="module")
def edge_custom():
    return _edge_entries("custom")


def _describe(labels, i):
    kind, sigma, c = labels[i]
    return {"entry": i, "kind": kind, "s'": hex(sigma), "class": DV.challenge_class(c), "c": hex(c),
            "radix-2^16 digits": DV.recode16(sigma), "radix-2^8 digits": DV.recode8(sigma)}


def _check_statuses(ctx, params, cols, want, labels, n, kernel, **kw):
    m = len(want)
    st = ctx.verify_response(*[_tile(a, n) for a in cols], params=params, **kw)
    wrong = np.nonzero(st[:m] != want)[0]
    for i in wrong[:6]:
        print("%s (n = %d): status %d, oracle %d: %r" % (kernel, n, st[i], want[i], _describe(labels, int(i))))
    assert wrong.size == 0, (kernel, n, wrong[:16].tolist())
    assert np.array_equal(st, _tile(st[:m], n)), "%s: repeats of one entry got different statuses" % kernel


@pytest.mark.parametrize("n,kernel", KERNEL_SIZES, ids=[k for _, k in KERNEL_SIZES])
def test_digit_edges_default_pair(gpu, edge_default, n, kernel):
    """The combs of the default pair (radix 2^16 digits) under every kernel."""
    params, cols, want, labels = edge_default
    _check_statuses(gpu, params, cols, want, labels, n, kernel)


def test_digit_edges_custom_pair(edge_custom):
    """A pair with no cached comb, on a fresh context: up to 2049 proofs read the 128-entry Niels
    tables (radix 2^8 digits: k_verify_wide's eight levels, k_verify_small, k_verify_quad<kVar>),
    built once; 16385 proofs build the pair's comb for k_verify_each."""
    params, cols, want, labels = edge_custom
    builds = {"generators": 0, "generators_varbase": 0}
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        fresh.stage_times()
        for n, kernel in KERNEL_SIZES:
            _check_statuses(fresh, params, cols, want, labels, n, kernel)
            st = fresh.stage_times()
            for k in builds:
                builds[k] += st.get(k, (0.0, 0))[1]
            if n <= 2049:
                assert builds == {"generators": 0, "generators_varbase": 1}, (n, builds)
            else:
                assert builds == {"generators": 1, "generators_varbase": 1}, (n, builds)


# ---- c. degenerate relations between a proof's points ------------------------------------------

def _degenerate_entries(which):
    """(columns, labels) of entries whose points coincide, double or cancel -- the cases in which
    an incomplete addition formula or a table builder that assumes distinct points goes wrong --
    each valid and with equation 2 alone spoiled (y2 = [x + 1] h; with c = 0, where the statement
    does not enter, r2 = [k + 1] h)."""
    params, g, h = _pair(which)
    rnd = random.Random(41)
    a, b = rnd.randrange(2, L // 2), rnd.randrange(2, L // 2)
    prev_x = rnd.randrange(1, L)
    cases = [("k = x", a, a), ("k = -x", a, L - a), ("k = 2 x", a, 2 * a % L), ("x = 2 k", 2 * b % L, b),
             ("x = 1", 1, b), ("x = l - 1", L - 1, b), ("k = 1", a, 1), ("x = 0", 0, b), ("k = 0", a, 0),
             ("c = 0", a, b), ("previous y1 as r1", b, prev_x)]
    recs, cb, labels = [], [], []
    # the entry whose y1 the last case's r1 repeats
    lead = (prev_x, rnd.randrange(1, L), rnd.randrange(1, L))
    for name, x, k in [("lead", lead[0], lead[1])] + cases:
        c = 0 if name == "c = 0" else rnd.randrange(1, L)
        s = (k + c * x) % L
        y1, y2, r1, r2 = _enc(g, x), _enc(h, x), _enc(g, k), _enc(h, k)
        spoiled = (y2, _enc(h, k + 1)) if c == 0 else (_enc(h, x + 1), r2)
        for kind, (y2v, r2v) in (("valid", (y2, r2)), ("equation 2 wrong", spoiled)):
            recs.append(O.ProofRecord(y1, y2v, r1, r2v, O.scalar_bytes(s)))
            cb.append(c.to_bytes(32, "little"))
            labels.append((name, kind))
    i_lead, i_last = 0, 2 * len(cases)
    assert labels[i_last] == ("previous y1 as r1", "valid") and recs[i_last].r1 == recs[i_lead].y1
    return params, recs, cb, labels


@pytest.fixture(scope="module")
def degenerate():
    """Per pair: the entries and the Python oracle's statuses with commitment checks on and with
    the equations alone, computed once."""
    out = {}
    for which in ("default", "custom"):
        params, recs, cb, labels = _degenerate_entries(which)
        want = {eq: np.array([O.verify_response(r, c, params.g, params.h, commitment_checks=not eq)
                              for r, c in zip(recs, cb)], np.uint8) for eq in (False, True)}
        by = {lab: (int(want[False][i]), int(want[True][i])) for i, lab in enumerate(labels)}
        # what the oracle says of the special ones: an identity commitment is refused by the
        # checks and judged by the equations without them; everything else is plain
        assert by[("k = 0", "valid")] == (O.ST_IDENTITY, O.ST_OK)
        assert by[("k = 0", "equation 2 wrong")] == (O.ST_IDENTITY, O.ST_EQ_FAIL)
        for lab, w in by.items():
            if lab[0] != "k = 0":
                assert w == ((O.ST_OK,) * 2 if lab[1] == "valid" else (O.ST_EQ_FAIL,) * 2), (lab, w)
        out[which] = (params, _cols(recs, cb), want, labels)
    return out


def _check_degenerate(ctx, params, cols, want, labels, eq_only):
    m = len(labels)
    # n = 1: each entry alone
    for i in range(m):
        st = ctx.verify_response(*[np.ascontiguousarray(a[i:i + 1]) for a in cols], params=params,
                                 equations_only=eq_only)
        assert int(st[0]) == want[i], ("n = 1", labels[i], int(st[0]), int(want[i]))
    for n, kernel in KERNEL_SIZES:
        st = ctx.verify_response(*[_tile(a, n) for a in cols], params=params, equations_only=eq_only)
        wrong = np.nonzero(st[:m] != want)[0]
        assert wrong.size == 0, (kernel, n, [(labels[i], int(st[i]), int(want[i])) for i in wrong[:8]])
        assert np.array_equal(st, _tile(st[:m], n)), "%s: repeats of one entry got different statuses" % kernel


@pytest.mark.parametrize("eq_only", [False, True], ids=["checks", "equations_only"])
def test_degenerate_relations_default_pair(gpu, degenerate, eq_only):
    """R' = +-Y', R' = 2 Y', Y' = 2 R', a statement or commitment equal to a generator, the
    identity statement and commitment, c = 0, and one entry's y1 as the next one's r1: the
    device-only table builders and adders (quad_table / ge_add_quad, the 16-lane rows of
    k_verify_wide and k_verify_small, build_joint_table in k_verify_each) on the combs."""
    params, cols, want, labels = degenerate["default"]
    _check_degenerate(gpu, params, cols, want[eq_only], labels, eq_only)


@pytest.mark.parametrize("eq_only", [False, True], ids=["checks", "equations_only"])
def test_degenerate_relations_custom_pair(degenerate, eq_only):
    """The same on a fresh context and a custom pair: the Niels tables up to 2049 proofs, then the
    pair's comb."""
    params, cols, want, labels = degenerate["custom"]
    with cp.Gpu(0) as fresh:
        _check_degenerate(fresh, params, cols, want[eq_only], labels, eq_only)
