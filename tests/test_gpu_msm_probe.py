"""GPU tests of the Pippenger MSM's sort and reduction (csrc/rlc.hip) on chosen digits and sizes.

The public ABI reaches these kernels only through scalars (cpz_msm: p0 = 0, two extras with zero
digits) or seed-derived weights (the batch checks), so tests/native/msmprobe.hip includes rlc.hip
unchanged and runs the sort alone (k_rlc_hist .. k_rlc_fine) on hand-made digit rows, ranges and
extras, and the accumulation and reduction alone (k_rlc_bucket, k_rlc_bucket_fix, k_rlc_segment +
k_rlc_window or k_rlc_window_sparse, k_rlc_final and k_rlc_final16) on the MODEL's offsets and
sorted ids, so a sort bug can neither mask nor cause a reduction failure.  Every point is a known
multiple of the basepoint, so each window sum and the total are one pt_mul on a Python integer
(tests/msm_model.py, which holds the case list; tests/test_msm_model.py proves on the CPU that
every case reaches the edge it names).  Offsets are compared exactly, sorted ids per bucket as
multisets, window sums and partials as 32-byte encodings.  The cases a scalar can express also run
through cpz_msm.

CPZ_MSMPROBE=<path> loads another build of the probe (over a mutated copy of csrc)."""
import numpy as np
import pytest

import msm_model as M
import pyoracle as O

pytestmark = pytest.mark.gpu

K, L = M.K, O.L


@pytest.fixture(scope="module")
def probe():
    return M.load_probe()


# ---- the sort ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_sort(probe, name):
    """k_rlc_hist, k_rlc_bscan, k_rlc_scan, k_rlc_coarse, k_rlc_fine: the offsets exactly, every
    bucket's ids as a multiset, bit 31 the digit's sign, no slot left unwritten, none written
    past a row's end."""
    c = M.case(name)
    moff, midx = c.sorted
    off, idx = M.probe_sort(c)
    badw = [w for w in range(16) if not np.array_equal(off[w].astype(np.int64), moff[w])]
    assert not badw, "offsets differ in windows %r" % badw
    D = c.digits
    for w in range(16):
        tot = int(moff[w, -1])
        row = idx[w, :tot].astype(np.int64)
        holes = np.nonzero(row == 0xffffffff)[0]
        assert holes.size == 0, "window %d: %d slots unwritten, first at %d" % (w, holes.size, holes[0])
        assert np.all(idx[w, tot:] == 0xffffffff), "window %d: written past its end" % w
        pid = row & 0x7fffffff
        inside = ((pid >= c.p0) & (pid < c.p0 + c.np)) | ((pid >= c.e0) & (pid < c.e0 + c.nextra))
        assert inside.all(), "window %d: ids outside the MSM's ranges, e.g. %d" % (w, pid[~inside][0])
        sign_bad = np.nonzero((D[w, pid] < 0) != (row >> 31 == 1))[0]
        assert sign_bad.size == 0, "window %d: bit 31 is not the digit's sign at slots %r" % (w, sign_bad[:8].tolist())
        diff = np.nonzero(c.canonical(w, idx[w]) != midx[w, :tot].astype(np.int64))[0]
        assert diff.size == 0, "window %d: %d slots differ from the model, first at %d" % (w, diff.size, diff[0])


# ---- accumulation and reduction -----------------------------------------------------------------------

def check_reduce(probe, c, sparse):
    rc, win, part, ident, part16, ident16 = M.probe_reduce(c, sparse)
    assert rc == 0, "msmprobe_reduce: hipError %d" % rc
    want = [M.enc_mul(v) for v in c.window_ints]
    badw = [w for w in range(16) if win[w].tobytes() != want[w]]
    assert not badw, "window sums differ in windows %r" % badw
    tot, flag = M.enc_mul(c.total_int), int(c.total_int == 0)
    assert part.tobytes() == tot and int(ident[0]) == flag, "k_rlc_final"
    assert part16.tobytes() == tot and int(ident16[0]) == flag, "k_rlc_final16"


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_reduce(probe, name):
    """k_rlc_bucket and k_rlc_bucket_fix at the case's echunk, then the reduction its size
    selects, then both finals, on the model's offsets and ids: T_w = [sum_i d_iw m_i] B for every
    window, both partials [sum] B with the right identity flag."""
    c = M.case(name)
    check_reduce(probe, c, c.facts["sparse"])


@pytest.mark.parametrize("name", M.BOTH_CASES)
def test_reduce_dense_on_small(probe, name):
    """The cases of at most kRlcSparsePts points through k_rlc_segment + k_rlc_window as well."""
    check_reduce(probe, M.case(name), False)


# ---- end to end: cpz_msm --------------------------------------------------------------------------------

def _points(c):
    raw = c.enc[:c.np].tobytes()
    return [raw[32 * i:32 * i + 32] for i in range(c.np)]


@pytest.mark.parametrize("name", M.SCALAR_CASES)
def test_msm_end_to_end(gpu, name):
    """The cases a scalar can express through the public cpz_msm: the oracle's [sum s_i m_i] B."""
    c = M.case(name)
    assert gpu.msm(_points(c), c.scalars) == M.enc_mul(c.total_int)


def test_msm_undecodable_point(gpu):
    """One point that does not decode, at index 256 + 3 (the second block of k_msm_load):
    CPZ_EINVAL; the same call with the point put right gives the oracle's sum."""
    import chaum_pedersen as cp
    m = M.pool()[0]
    n = 300
    raw = M.pool()[1][np.arange(n) % M.POOL].tobytes()
    pts = [raw[32 * i:32 * i + 32] for i in range(n)]
    scal = [(i * 0x10001 + 1) for i in range(n)]
    bad = list(pts)
    bad[256 + 3] = bytes.fromhex("01" + "00" * 31)
    with pytest.raises(cp._native.CpzError) as ei:
        gpu.msm(bad, scal)
    assert ei.value.code == cp._native.CPZ_EINVAL
    assert gpu.msm(pts, scal) == M.enc_mul(sum(s * m[i % M.POOL] for i, s in enumerate(scal)))
