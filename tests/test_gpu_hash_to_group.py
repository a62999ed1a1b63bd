"""Hash-to-group on the device (csrc/h2g.hip: k_sha512_rows, k_from_uniform) through
cpz_from_uniform_bytes, cpz_hash_to_group, cpz_derive_pairs and the device forms, against the Python
oracle (tests/h2g_cases.py computes every expected encoding once).

k_from_uniform gives a lane pair to a point, so the sizes run over the pair tails and the wave
boundaries (n = 1, 2, 63, 64, 65, 127, 129, 257: an odd n leaves half a pair, 65 and 129 a wave with one
pair); k_sha512_rows gives a lane to a message, so one call mixes every block count among
neighbouring lanes.  Derived rows go into the mixed-pair prover and both verifiers as they are."""
import ctypes
import hashlib

import numpy as np
import pytest

import chaum_pedersen as cp
import h2g_cases as C
import pyoracle as O
from chaum_pedersen import _native

pytestmark = pytest.mark.gpu

POOL = [row for _, row in C.EDGE_ROWS] + C.random_rows(256)       # 275 rows, the edges first
LONGEST = _native.HASH_MAX_MSG - len(_native.PAIR_DST_G)
SENTINEL = 0xEE


def _expected(rows):
    return np.frombuffer(b"".join(C.expected_point(r) for r in rows), np.uint8).reshape(len(rows), 32)


def _same_rows(got, exp):
    bad = np.nonzero((np.asarray(got) != exp).any(axis=1))[0]
    assert bad.size == 0, bad[:8].tolist()


# ---- from_uniform_bytes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 129, 257, len(POOL)])
def test_from_uniform_bytes_sizes(gpu, n):
    rows = POOL[:n]
    got = gpu.from_uniform_bytes(rows)
    assert got.shape == (n, 32)
    _same_rows(got, _expected(rows))


def test_from_uniform_bytes_edges(gpu):
    names = [name for name, _ in C.EDGE_ROWS]
    got = dict(zip(names, (r.tobytes() for r in gpu.from_uniform_bytes([row for _, row in C.EDGE_ROWS]))))
    assert got["zero"] == bytes(32) and got["bits 255 only"] == bytes(32)
    for a, b in C.SAME_POINT:
        assert got[a] == got[b], (a, b)
    assert got["p+1 alone"].hex().startswith("7c1f61e9") and got["p+1 alone"].hex().endswith("02608560")
    # a row alone, and the same row as the last of an odd count, give one point
    for name, row in C.EDGE_ROWS:
        assert gpu.from_uniform_bytes(row).tobytes() == got[name], name


# ---- hash_to_group ---------------------------------------------------------------------------------------

def _hash_messages():
    msgs = [C.message(n) for n in C.HASH_LENGTHS] + [C.message(n, 1) for n in C.HASH_LENGTHS]
    msgs += [C.RFC_A3_MSG, O.GENERATOR_H_DST]
    order = np.random.default_rng(20264).permutation(len(msgs))     # neighbouring lanes run different block counts
    return [msgs[i] for i in order]


def test_hash_to_group_lengths_shuffled_in_one_call(gpu):
    msgs = _hash_messages()
    assert sorted({len(m) for m in msgs} - {len(C.RFC_A3_MSG), len(O.GENERATOR_H_DST)}) == C.HASH_LENGTHS
    got = gpu.hash_to_group(msgs)
    exp = np.frombuffer(b"".join(C.expected_hash(m) for m in msgs), np.uint8).reshape(len(msgs), 32)
    _same_rows(got, exp)
    assert got[msgs.index(C.RFC_A3_MSG)].tobytes() == C.RFC_A3_POINT              # RFC 9496 A.3
    assert got[msgs.index(O.GENERATOR_H_DST)].tobytes() == C.DEFAULT_H == cp.default_generators()[1]


# ---- the device forms ------------------------------------------------------------------------------------

def test_device_forms_equal_the_host_forms_on_another_stream(gpu):
    import torch
    dev = torch.device("cuda", 0)
    msgs = _hash_messages()
    host_pts = gpu.hash_to_group(msgs)
    blob = b"".join(msgs)
    off = np.zeros(len(msgs) + 1, np.int64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    big = torch.zeros(len(blob) + 1, dtype=torch.uint8, device=dev)
    d_blob = big[1:]                                                  # the blob starts at an odd address
    d_blob.copy_(torch.from_numpy(np.frombuffer(blob, np.uint8).copy()))
    assert d_blob.data_ptr() % 2 == 1
    d_off = torch.from_numpy(off).to(dev)
    d_out = torch.full((len(msgs), 32), SENTINEL, dtype=torch.uint8, device=dev)
    rows = POOL[:65]
    host_uni = gpu.from_uniform_bytes(rows)
    flat = np.frombuffer(b"".join(rows), np.uint8).copy()
    d_uni = torch.from_numpy(flat).to(dev)
    big_u = torch.zeros(flat.size + 1, dtype=torch.uint8, device=dev)
    d_uni_odd = big_u[1:]
    d_uni_odd.copy_(d_uni)
    assert d_uni.data_ptr() % 16 == 0 and d_uni_odd.data_ptr() % 2 == 1
    d_pts = torch.full((65, 32), SENTINEL, dtype=torch.uint8, device=dev)
    d_pts_odd = torch.full((65, 32), SENTINEL, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    assert side.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    gpu.hash_to_group_device(d_blob, d_off, d_out, stream=side.cuda_stream)
    gpu.from_uniform_bytes_device(d_uni, d_pts, stream=side.cuda_stream)
    gpu.from_uniform_bytes_device(d_uni_odd, d_pts_odd, stream=side.cuda_stream)
    side.synchronize()
    _same_rows(d_out.cpu().numpy(), host_pts)
    _same_rows(d_pts.cpu().numpy(), host_uni)
    _same_rows(d_pts_odd.cpu().numpy(), host_uni)
    # a host call after the unsynchronised device calls orders after them and still agrees
    _same_rows(gpu.hash_to_group(msgs), host_pts)


# ---- derive_pairs ----------------------------------------------------------------------------------------

def _labels(n):
    base = [b"", b"t", b"x" * LONGEST]                               # the empty label, one byte, the longest allowed
    return (base + [b"tenant-%d" % i for i in range(n)])[:n] if n >= 3 else [b"tenant-%d" % i for i in range(n)]


@pytest.mark.parametrize("n", [1, 64, 65, 130])
def test_derive_pairs_in_full_against_the_oracle(gpu, n):
    labels = _labels(n)
    rows = gpu.derive_pairs(labels)
    assert rows.shape == (n, 64) and rows.dtype == np.uint8
    exp = np.frombuffer(b"".join(C.expected_pair(lb) for lb in labels), np.uint8).reshape(n, 64)
    _same_rows(rows, exp)
    params = cp.Parameters.from_labels(labels, gpu=gpu)
    assert b"".join(p.g + p.h for p in params) == rows.tobytes()
    assert cp.Parameters.from_label(labels[-1], gpu=gpu) == params[-1]


def test_the_empty_label_does_not_give_the_default_h(gpu):
    row = gpu.derive_pairs([b""])[0].tobytes()
    g, h = cp.default_generators()
    assert row[32:] != h and row[:32] != g and row[32:] == C.expected_hash(O.GENERATOR_H_DST + b"/")


def test_derive_4096_pairs(gpu):
    labels = _labels(4096)
    rows = gpu.derive_pairs(labels)
    assert rows.shape == (4096, 64)
    for p in np.random.default_rng(20265).choice(4096, 32, replace=False).tolist() + [0, 2, 4095]:
        assert rows[p].tobytes() == C.expected_pair(labels[p]), p
    pts = rows.reshape(8192, 32)
    ok, enc = gpu.decode_points(pts)
    assert ok.all() and np.array_equal(enc, pts)                      # every row decodes, canonically
    assert len({r.tobytes() for r in pts}) == 8192                    # pairwise distinct


# ---- end to end ------------------------------------------------------------------------------------------

def test_derived_pairs_serve_the_prover_and_both_verifiers(gpu):
    labels = [b"tenant/%d" % i for i in range(65)]
    pairs = cp.Parameters.from_labels(labels, gpu=gpu)
    assert b"".join(p.g + p.h for p in pairs) == gpu.derive_pairs(labels).tobytes()    # the rows as they are
    n = 130
    idx = (np.arange(n) % 65).astype(np.uint32)

    def scalars(tag):
        vals = [int.from_bytes(hashlib.sha512(tag + b"%d" % i).digest(), "little") % O.L for i in range(n)]
        return np.frombuffer(b"".join(O.scalar_bytes(v) for v in vals), np.uint8).reshape(n, 32).copy()

    out = gpu.prove_pairs_many(pairs, idx, scalars(b"h2g-x"), scalars(b"h2g-k"))
    q = [out[k] for k in ("y1", "y2", "r1", "r2", "s")]
    assert gpu.verify_each_pairs_many(pairs, idx, *q).tolist() == [cp.STATUS_OK] * n
    _, batch_ok, st = gpu.verify_batch_pairs_many(pairs, idx, *q, seed=hashlib.sha256(b"h2g-seed").digest())
    assert batch_ok and st.tolist() == [cp.STATUS_OK] * n


# ---- error cases: nothing is written ---------------------------------------------------------------------

def _last_error():
    return _native.load().cpz_last_error().decode()


def _u64(vals):
    return np.asarray(vals, dtype=np.uint64)


def test_errors_leave_the_outputs_untouched(gpu):
    lib, h = gpu._lib, gpu._h
    p = lambda a: a.ctypes.data
    out = np.full((8, 64), SENTINEL, np.uint8)
    blob = np.zeros(3 * 4097 + 16, np.uint8)
    uni = np.zeros((8, 64), np.uint8)

    def untouched():
        return bool((out == SENTINEL).all())

    # n == 0
    assert lib.cpz_from_uniform_bytes(h, 0, p(uni), p(out)) == _native.CPZ_EEMPTY and untouched()
    assert lib.cpz_hash_to_group(h, 0, p(blob), p(_u64([0])), p(out)) == _native.CPZ_EEMPTY and untouched()
    assert lib.cpz_derive_pairs(h, 0, p(blob), p(_u64([0])), p(out)) == _native.CPZ_EEMPTY and untouched()
    # decreasing offsets: the lowest offending entry is named
    assert lib.cpz_hash_to_group(h, 4, p(blob), p(_u64([0, 5, 3, 2, 9])), p(out)) == _native.CPZ_EINVAL and untouched()
    assert _last_error().startswith("message 1:"), _last_error()
    assert lib.cpz_derive_pairs(h, 3, p(blob), p(_u64([4, 5, 9, 8])), p(out)) == _native.CPZ_EINVAL and untouched()
    assert _last_error().startswith("label 2:"), _last_error()
    # one message of 4097 bytes among good ones (4096 is accepted: the shuffled call above)
    off = _u64([0, 10, 10 + 4096, 10 + 4096 + 4097, 10 + 4096 + 4097 + 1])
    assert lib.cpz_hash_to_group(h, 4, p(blob), p(off), p(out)) == _native.CPZ_EINVAL and untouched()
    assert _last_error().startswith("message 2:") and "4097" in _last_error(), _last_error()
    # a label that exceeds the bound only once prefixed (LONGEST is accepted: the derive tests above)
    assert LONGEST + 1 <= _native.HASH_MAX_MSG
    off = _u64([0, 1, 1 + LONGEST + 1, 3 + LONGEST])
    assert lib.cpz_derive_pairs(h, 3, p(blob), p(off), p(out)) == _native.CPZ_EINVAL and untouched()
    assert _last_error().startswith("label 1:") and "4097" in _last_error(), _last_error()
    # null pointers
    assert lib.cpz_from_uniform_bytes(h, 1, None, p(out)) == _native.CPZ_EINVAL
    assert lib.cpz_hash_to_group(h, 1, p(blob), None, p(out)) == _native.CPZ_EINVAL and untouched()
    assert lib.cpz_derive_pairs(h, 1, None, p(_u64([0, 1])), p(out)) == _native.CPZ_EINVAL and untouched()
    assert lib.cpz_derive_pairs(h, 1, p(blob), p(_u64([0, 1])), None) == _native.CPZ_EINVAL
    # n above the bound
    big_n = _native.HASH_MAX_N + 1
    big_out = np.full((big_n, 32), SENTINEL, np.uint8)
    assert lib.cpz_from_uniform_bytes(h, big_n, p(np.zeros((big_n, 64), np.uint8)), p(big_out)) == _native.CPZ_EINVAL
    assert lib.cpz_hash_to_group(h, big_n, p(blob), p(np.zeros(big_n + 1, np.uint64)), p(big_out)) == _native.CPZ_EINVAL
    assert (big_out == SENTINEL).all()
    many = _native.EACH_PAIRS_MANY_MAX + 1
    many_out = np.full((many, 64), SENTINEL, np.uint8)
    assert lib.cpz_derive_pairs(h, many, p(blob), p(np.zeros(many + 1, np.uint64)), p(many_out)) == _native.CPZ_EINVAL
    assert (many_out == SENTINEL).all()
    # the context still works
    assert gpu.hash_to_group([O.GENERATOR_H_DST])[0].tobytes() == C.DEFAULT_H


def test_device_form_errors_leave_the_outputs_untouched(gpu):
    import torch
    dev = torch.device("cuda", 0)
    lib, h = gpu._lib, gpu._h
    d_uni = torch.zeros(4 * 64, dtype=torch.uint8, device=dev)
    d_blob = torch.zeros(64, dtype=torch.uint8, device=dev)
    d_off = torch.tensor([0, 8, 16, 24, 32], dtype=torch.int64, device=dev)
    raw = torch.full((4 * 32 + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    mis = raw[8:8 + 128]                                              # 8 bytes past a 16-byte boundary
    assert raw.data_ptr() % 16 == 0 and mis.data_ptr() % 16 == 8
    st = torch.cuda.current_stream(dev).cuda_stream
    assert lib.cpz_from_uniform_bytes_device(h, 4, d_uni.data_ptr(), mis.data_ptr(), st) == _native.CPZ_EINVAL
    assert "16-byte aligned" in _last_error()
    assert lib.cpz_hash_to_group_device(h, 4, d_blob.data_ptr(), d_off.data_ptr(), mis.data_ptr(), st) == _native.CPZ_EINVAL
    assert "16-byte aligned" in _last_error()
    assert lib.cpz_from_uniform_bytes_device(h, 0, d_uni.data_ptr(), raw.data_ptr(), st) == _native.CPZ_EEMPTY
    assert lib.cpz_hash_to_group_device(h, 0, d_blob.data_ptr(), d_off.data_ptr(), raw.data_ptr(), st) == _native.CPZ_EEMPTY
    assert lib.cpz_from_uniform_bytes_device(h, _native.HASH_MAX_N + 1, d_uni.data_ptr(), raw.data_ptr(), st) == _native.CPZ_EINVAL
    assert lib.cpz_hash_to_group_device(h, _native.HASH_MAX_N + 1, d_blob.data_ptr(), d_off.data_ptr(), raw.data_ptr(),
                                        st) == _native.CPZ_EINVAL
    assert lib.cpz_hash_to_group_device(h, 4, d_blob.data_ptr(), None, raw.data_ptr(), st) == _native.CPZ_EINVAL
    torch.cuda.synchronize(dev)
    assert bool((raw == SENTINEL).all())
    with pytest.raises(cp.InvalidParams):                             # the wrapper refuses the same row first
        gpu.from_uniform_bytes_device(d_uni, mis)
