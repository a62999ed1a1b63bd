"""GPU tests of the RLC batch check's prepare stage and of the device scalar arithmetic on chosen
inputs (csrc/rlc.hip: k_rlc_prepare, k_rlc_prepare_pairs, k_rlc_prepare4, k_rlc_prepare4_pairs,
k_rlc_bsum4, k_rlc_extra, k_rlc_extra_pairs and both prepare launchers; rlc_dev.h: rlc_weight,
recode16; scalar25519.h: sc_mul, sc_add, sc_neg, sc_reduce_wide, sc_is_canonical).

The whole-call tests see this stage through one 32-byte partial or a status list, on random
proofs, which cannot reach a full carry ripple in recode16, a tree of additions that all wrap past
l, a weight counter that crosses 2^32, the status precedence as a table, or the zero-weight rule
per digit slot.  tests/native/prepprobe.hip includes rlc.hip unchanged and returns everything the
stage writes; tests/prep_model.py holds the cases and the Python-integer model,
tests/scalar_vectors.py the scalar vectors the host build runs as well
(tests/test_device_arith.py::test_scalars), and tests/test_prep_model.py proves on the CPU that
every case reaches the edge it names.  All comparisons are exact: integers and bytes.

CPZ_PREPPROBE=<path> loads another build of the probe (over a mutated copy of csrc)."""
import random

import numpy as np
import pytest

import prep_model as M
import pyoracle as O
import scalar_vectors as SV

pytestmark = pytest.mark.gpu

L = O.L
FF32 = 0xffffffff


@pytest.fixture(scope="module")
def probe():
    return M.load_probe()


@pytest.fixture(autouse=True)
def _stop_after_hip_error():
    """Once an entry point has returned a HIP error nothing more is launched from this process."""
    if M.hip_failure:
        pytest.exit("stopping after " + M.hip_failure, returncode=3)


def test_constants(probe):
    k = M.probe_consts()
    assert (k["kRlcWindows"], k["kRlcPrepBlock"], k["kRlcSumBlock"]) == (16, M.PREP_BLOCK, M.SUM_BLOCK)
    assert k["kRlcPrepWideMax"] == M.WIDE_MAX and k["sizeof_ge_niels"] == M.NIELS_BYTES
    assert (k["kStOk"], k["kStBadPoint"], k["kStBadScalar"], k["kStIdentity"], k["kStZeroS"]) == (
        M.ST_OK, M.ST_BAD_POINT, M.ST_BAD_SCALAR, M.ST_IDENTITY, M.ST_ZERO_S)
    assert k["kStBadChallenge"] not in (0, 3, 5)   # never an input of the prepare (prep_model.prepare_model)
    assert k["kNielsEntriesRlc"] >= 1


# ---- device scalar arithmetic -----------------------------------------------------------------------------

def _differ(got, want):
    return [i for i, (g, w) in enumerate(zip(got, want)) if g != w]


def test_sc_reduce_wide(probe):
    xs = SV.reduce_wide_cases()
    got = M.ints_of(M.probe_scalar("reduce_wide", M.words_of(xs, 64)))
    bad = _differ(got, [x % L for x in xs])
    assert not bad, "%d of %d differ, first input %#x" % (len(bad), len(xs), xs[bad[0]])


@pytest.mark.parametrize("op", ["mul", "add"])
def test_sc_mul_add(probe, op):
    pairs = SV.grid_pairs()
    a, b = M.words_of([p[0] for p in pairs]), M.words_of([p[1] for p in pairs])
    got = M.ints_of(M.probe_scalar(op, a, b))
    want = [(x * y if op == "mul" else x + y) % L for x, y in pairs]
    bad = _differ(got, want)
    assert not bad, "%d of %d differ, first operands %#x, %#x" % ((len(bad), len(pairs)) + pairs[bad[0]])


def test_sc_neg(probe):
    v = SV.grid_values()
    got = M.ints_of(M.probe_scalar("neg", M.words_of(v)))
    assert got == [(-x) % L for x in v]


def test_sc_is_canonical(probe):
    v = SV.CANONICAL_CASES + SV.grid_values()
    out = M.probe_scalar("is_canonical", M.words_of(v))
    assert out[:, 0].tolist() == [1 if x < L else 0 for x in v]
    assert np.all(out[:, 1:] == FF32)


def test_rlc_weight(probe):
    """rlc_weight over the half-word edges: sum int16(half) 2^(16 k) mod l, pyoracle.rlc_weights'
    definition."""
    cases = SV.weight_cases()
    words = M.words_of([SV.from_windows(h) for h in cases], 16)
    got = M.ints_of(M.probe_scalar("weight", words))
    bad = _differ(got, [SV.weight_value(h) for h in cases])
    assert not bad, "%d differ, first halves %r" % (len(bad), [hex(x) for x in cases[bad[0]]])


def test_recode16(probe):
    """Each digit in [-2^15, 2^15), the digits sum back to the scalar, and they are the model's."""
    cases = SV.recode16_cases()
    out = M.probe_scalar("recode16", M.words_of(cases)).view(np.int16).reshape(len(cases), 16)
    for s, row in zip(cases, out.tolist()):
        assert M.digit_value(row) == s, hex(s)
        assert row == SV.recode16_model(s), hex(s)


# ---- the prepare kernels ------------------------------------------------------------------------------------

def _all_ff(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == 0xff))


def check_prepare(o, b, m, form, pairs):
    """Everything one prepare wrote, against the model `m` of case `b`.  form 0: the one-lane
    kernel, 1: the four-lane one."""
    n = b.n
    want_st = np.array([m.status[i] for i in range(n)], np.uint8)
    bad = np.nonzero(o.status != want_st)[0]
    assert bad.size == 0, "status differs at %r: got %r, want %r" % (
        bad[:8].tolist(), o.status[bad[:8]].tolist(), want_st[bad[:8]].tolist())
    assert int(o.any_bad[0]) == int(not all(m.live.values())), "any_bad"
    # digits: the model's on the 4 n columns (zero on all 64 slots of a rejected entry), 0xff beyond
    want_d = M.model_digit_array(m)
    diff = np.argwhere(o.digits[:, :4 * n] != want_d)
    assert diff.size == 0, "digits differ at (window, column) %r ... (entry %d, point %d)" % (
        diff[:4].tolist(), diff[0][1] // 4, diff[0][1] % 4)
    assert _all_ff(o.digits[:, 4 * n:]), "digit columns beyond 4 n were written"
    # points: (y - x, y + x, -2 d x y) mod p wherever the encoding decodes
    f = M.niels_ints(o.pts)
    for j in range(4 * n):
        if m.niels[j] is not None:
            assert (f[0][j], f[1][j], f[2][j]) == m.niels[j], "Niels entry of proof %d, point %d" % (j // 4, j % 4)
    if pairs:
        got = M.ints_of(o.prod)
        want = [v for i in range(n) for v in m.prod[i]]
        bad = _differ(got, want)
        assert not bad, "prod differs at entries %r" % [k // 2 for k in bad[:8]]
        assert _all_ff(o.block_sums) and _all_ff(o.quarter_sums), "pair mode wrote block or quarter sums"
    else:
        got = M.ints_of(o.block_sums)
        want = [v for s in m.block_sums for v in s]
        bad = _differ(got, want)
        assert not bad, "block sums differ at (block, a/b) %r" % [(k // 2, k % 2) for k in bad[:8]]
        assert _all_ff(o.prod), "single-pair mode wrote prod"
        if form == 0:
            assert _all_ff(o.quarter_sums), "the one-lane form wrote quarter_sums"
        else:
            assert M.ints_of(o.quarter_sums) == [v for s in m.quarter_sums for v in s], "quarter sums"


@pytest.mark.parametrize("form", [0, 1], ids=["one_lane", "four_lanes"])
@pytest.mark.parametrize("pairs", [0, 1], ids=["single", "pairs"])
@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_prepare(probe, name, pairs, form):
    """Every named case through k_rlc_prepare / k_rlc_prepare_pairs (launched directly, whatever the
    size) and through k_rlc_prepare4 + k_rlc_bsum4 / k_rlc_prepare4_pairs: statuses, any_bad, all 64
    digit slots per proof, the four negated Niels points mod p, the block sums or per-proof
    products, and what must stay untouched."""
    b = M.case(name)
    check_prepare(M.probe_prepare(b, form, pairs), b, M.model(name), form, pairs)


@pytest.mark.parametrize("pairs", [0, 1], ids=["single", "pairs"])
@pytest.mark.parametrize("name", ["size_257", "mixed300", "status_table_eq1"])
def test_launcher_small(probe, name, pairs):
    """launch_rlc_prepare / launch_rlc_prepare_pairs below the size switch: the four-lane form's
    outputs, quarter sums included."""
    b = M.case(name)
    check_prepare(M.probe_prepare(b, 2, pairs), b, M.model(name), 1, pairs)


# ---- cross-form and routing at the size switch ------------------------------------------------------------------

TILE_FIRST = 5 << 20


def _tiled_entry(b, i):
    """the model of entry i of mixed300 tiled: row i % 300 under the weights of index TILE_FIRST + i"""
    r = i % b.n
    m = M.prepare_model(b, first_index=TILE_FIRST + i - r, rows=[r])
    return m.status[r], m.digits[r], m.prod[r]


@pytest.mark.parametrize("pairs", [0, 1], ids=["single", "pairs"])
@pytest.mark.parametrize("over", [0, 1], ids=["wide_max", "wide_max_plus_1"])
def test_forms_agree_at_the_size_switch(probe, over, pairs):
    """n = kRlcPrepWideMax and kRlcPrepWideMax + 1, rows tiled from mixed300: the one-lane form, the
    four-lane form and the launcher give byte-identical digits, statuses and sums and equal points
    mod p; quarter_sums shows which form the launcher took; 64 sampled entries and three sum
    blocks are checked against the model."""
    b = M.case("mixed300")
    n = M.WIDE_MAX + over
    rows = [i % b.n for i in range(n)]
    o0, o1, o2 = (M.probe_prepare(b, form, pairs, rows=rows, first_index=TILE_FIRST) for form in (0, 1, 2))
    row_status = np.array([M.model("mixed300").status[r] for r in range(b.n)], np.uint8)
    want_st = row_status[np.array(rows)]
    decodes = np.repeat(want_st != M.ST_BAD_POINT, 4)
    for tag, o in (("four-lane", o1), ("launcher", o2)):
        assert np.array_equal(o.status, o0.status), tag
        assert o.digits.tobytes() == o0.digits.tobytes(), tag
        assert o.block_sums.tobytes() == o0.block_sums.tobytes(), tag
        assert o.prod.tobytes() == o0.prod.tobytes(), tag
        assert int(o.any_bad[0]) == int(o0.any_bad[0]) == 1, tag
        differ = np.nonzero(np.any(o.pts[:, :30] != o0.pts[:, :30], axis=1) & decodes)[0]
        if differ.size:   # other limbs: the values mod p must still agree
            assert M.niels_ints(o.pts[differ]) == M.niels_ints(o0.pts[differ]), tag
    assert np.array_equal(o0.status, want_st)
    assert _all_ff(o0.digits[:, 4 * n:]) and _all_ff(o0.quarter_sums)
    if pairs:
        assert _all_ff(o2.quarter_sums) and _all_ff(o2.block_sums)
    else:
        assert not _all_ff(o1.quarter_sums)
        assert _all_ff(o2.quarter_sums) == bool(over), "the launcher's form at n = %d" % n
        if not over:
            assert o2.quarter_sums.tobytes() == o1.quarter_sums.tobytes()
    rnd = random.Random(n + pairs)
    sample = sorted({0, 1, 299, 300, M.WIDE_MAX - 1, n - 1} | {rnd.randrange(n) for _ in range(58)})
    assert len(sample) >= 60
    for i in sample:
        st, dig, prod = _tiled_entry(b, i)
        assert int(o0.status[i]) == st, i
        assert o0.digits[:, 4 * i:4 * i + 4].T.tolist() == dig, "digits of entry %d" % i
        if pairs:
            assert tuple(M.ints_of(o0.prod[i])) == prod, "prod of entry %d" % i
    if not pairs:
        nsum = (n + M.SUM_BLOCK - 1) // M.SUM_BLOCK
        for k in (0, 117, nsum - 1):
            part = [_tiled_entry(b, i)[2] for i in range(M.SUM_BLOCK * k, min(n, M.SUM_BLOCK * (k + 1)))]
            want = (sum(p[0] for p in part) % L, sum(p[1] for p in part) % L)
            assert tuple(M.ints_of(o0.block_sums[k])) == want, "block sum %d" % k
        assert M.ints_of(o0.block_sums[nsum:]) == [0] * (2 * (o0.block_sums.shape[0] - nsum))


# ---- k_rlc_extra / k_rlc_extra_pairs ---------------------------------------------------------------------------------

def _check_columns(dig, e0, cols):
    """digit columns e0 .. e0 + len(cols) - 1 are `cols`; every other slot stays 0xff"""
    k = len(cols)
    assert dig[:, e0:e0 + k].T.tolist() == cols
    assert _all_ff(dig[:, :e0]) and _all_ff(dig[:, e0 + k:]), "digit columns outside the extras were written"


@pytest.mark.parametrize("b0,b1", M.EXTRA_RANGES)
def test_extra(probe, b0, b1):
    """k_rlc_extra: g and h byte for byte (pad words included) from entries 0 and
    kNielsEntriesRlc of the table, digits recode16 of the sums over [b0, b1) mod l."""
    sums = M.extra_sums()
    g = M.niels_bytes(O.BASEPOINT, pad=0x11223344)
    h = M.niels_bytes(O.generator_h(), pad=0x55667788)
    e0, dstride = 13, 32
    pts, dig = M.probe_extra(sums, b0, b1, e0, dstride, g, h)
    assert pts[0].tobytes() == g and pts[1].tobytes() == h
    _check_columns(dig, e0, M.extra_model(sums, b0, b1))


@pytest.mark.parametrize("lo,hi", M.PAIR_RANGES)
@pytest.mark.parametrize("npairs", M.PAIR_COUNTS)
def test_extra_pairs(probe, npairs, lo, hi):
    """k_rlc_extra_pairs: pair p's points byte for byte, digits recode16 of the sum of the products
    of the entries of [lo, hi) under p; a pair without entry in range gets all-zero digits."""
    pc = M.pair_case(npairs)
    e0 = 4 * M.PAIR_N
    dstride = M.dstride_of(M.PAIR_N) + 2 * npairs
    pts, dig = M.probe_extra_pairs(pc, lo, hi, e0, dstride)
    assert pts.tobytes() == pc.gh
    cols = [c for pair in M.pair_model(pc, lo, hi) for c in pair]
    _check_columns(dig, e0, cols)
    if npairs == 64:
        for p in M.PAIR_EMPTY:
            assert not dig[:, e0 + 2 * p:e0 + 2 * p + 2].any()


# ---- closure with the oracle ----------------------------------------------------------------------------------------

def test_closure_with_the_oracle(probe):
    """n = 24 with three forged and two rejected entries: the points rebuilt from the returned Niels
    triples (xy2d = 2 d x y checked), times the returned digits, plus k_rlc_extra's two entries over
    the returned block sums, encode to pyoracle.rlc_partial of the same records."""
    b = M.case("closure24")
    n = b.n
    o = M.probe_prepare(b, 1, 0)
    sums = M.ints_of(o.block_sums)
    sums = [(sums[2 * k], sums[2 * k + 1]) for k in range(len(sums) // 2)]
    g, h = M.niels_bytes(O.BASEPOINT), M.niels_bytes(O.generator_h())
    epts, edig = M.probe_extra(sums, 0, len(sums), 4 * n, o.dstride, g, h)
    f = M.niels_ints(np.concatenate([o.pts, epts]))
    cols, pts = [], []
    for i in range(n):
        if o.status[i] != M.ST_OK:
            assert not o.digits[:, 4 * i:4 * i + 4].any()
            continue
        for j in range(4 * i, 4 * i + 4):
            cols.append(o.digits[:, j].tolist())
            pts.append(M.point_of_niels(f[0][j], f[1][j], f[2][j]))
    assert sorted(set(range(n)) - {j for j in range(n) if o.status[j] == M.ST_OK}) == sorted(
        (M.CLOSURE_BAD_POINT, M.CLOSURE_ZERO_S))
    for k in range(2):
        cols.append(edig[:, 4 * n + k].tolist())
        pts.append(M.point_of_niels(f[0][4 * n + k], f[1][4 * n + k], f[2][4 * n + k]))
    want = O.rlc_partial(b.facts["recs"], b.seed, b.first_index)
    assert O.ristretto_encode(M.weighted_sum(cols, pts)) == O.ristretto_encode(want)
