"""cpz_verify_each with the joint-table build's state in LDS columns (CPZ_BUILD_LDS: csrc/kernels.hip
verify_one_row, csrc/verify.h check_equation, csrc/scalarmul.h build_joint_table_cols) and the folded
doublings, on synthetic proofs at n = 2049, 4096 + 37 and 65,536 + 1: one partial block, and two
launches on two streams with their own slabs (the second of one thread).  Rows spoiled with the
benchmark's four kinds sit in the first and last thread of a block and of a wave; every status is
the C oracle's.  A thread's LDS column holds first its equation's encodings, then the build state
over them, for two equations and, in the next call, for another proof: the last test runs a call
twice on one context."""
import hashlib
import os

import numpy as np
import pytest

import coracle as C
import pyoracle as O

pytestmark = pytest.mark.gpu

SX = hashlib.sha256(b"cpz-bench-x").digest()
SK = hashlib.sha256(b"cpz-bench-k").digest()
KEYS = ("y1", "y2", "r1", "r2", "s")
SIZES = (2049, 4096 + 37, 65536 + 1)
NMAX = max(SIZES)
WANT = (1, 1, 2, 5)  # s + 1, swapped y1, undecodable r1, s = 0


def _threads():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return max(1, min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def base(gpu):
    """NMAX valid proofs (every size takes a prefix) and the C oracle's verdicts on them, once."""
    torch = pytest.importorskip("torch")
    t = {k: torch.empty((NMAX, 32), dtype=torch.uint8, device="cuda:0") for k in KEYS}
    gpu.prove_synthetic_device(NMAX, SX, SK, t["y1"], t["y2"], t["r1"], t["r2"], t["s"])
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in t.items()}
    for v in r.values():
        v.setflags(write=False)
    oracle = C.verify_many(r, threads=_threads())
    oracle.setflags(write=False)
    assert not oracle.any()
    return r, oracle


def _edge_rows(n):
    """First and last thread of a block and of a wave: in the first block, around the first block
    edge, in the last whole block, in the last (partial) block, and the launch edge at 2^16."""
    last = n - 1
    blk = 256 * (last // 256)          # first thread of the last (partial) block
    whole = blk - 256                  # first thread of the last whole block
    rows = {0, 63, 64, 127, 192, 255, 256, 319, 320, 511,
            whole, whole + 63, whole + 64, whole + 255, blk, last,
            64 * (last // 64), 64 * (last // 64) - 1}
    if n > 65536:
        rows |= {65535 - 255, 65535 - 63, 65535, 65536}
    return sorted(i for i in rows if 0 <= i < n)


def _spoil(base_rows, n, shift):
    """A copy of the first n proofs with the edge rows spoiled, the four kinds in turn from
    `shift` on, and {row: expected status}."""
    r = {k: v[:n].copy() for k, v in base_rows.items()}
    want = {}
    for j, i in enumerate(_edge_rows(n)):
        kind = (j + shift) % 4
        if kind == 0:
            v = (int.from_bytes(r["s"][i].tobytes(), "little") + 1) % O.L
            r["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
        elif kind == 1:
            r["y1"][i] = base_rows["y1"][(i + 7) % n]
        elif kind == 2:
            r["r1"][i] = 0
            r["r1"][i, 0] = 1
        else:
            r["s"][i] = 0
        want[i] = WANT[kind]
    return r, want


def _oracle(base_oracle, r, want, n):
    """The C oracle's per-proof verdicts on r: the spoiled rows verified now, the others (the
    unchanged valid proofs; a verdict depends on its own row only) taken from the shared run."""
    idx = np.array(sorted(want))
    sub = C.verify_many({k: np.ascontiguousarray(r[k][idx]) for k in KEYS}, threads=_threads())
    out = base_oracle[:n].copy()
    out[idx] = sub
    return out


@pytest.mark.parametrize("n,shift", [(SIZES[0], 0), (SIZES[1], 1), (SIZES[2], 2), (SIZES[2], 3)])
def test_verify_each_statuses_equal_the_oracle(gpu, base, n, shift):
    rows, base_oracle = base
    r, want = _spoil(rows, n, shift)
    got = gpu.verify_each(*[r[k] for k in KEYS])
    oracle = _oracle(base_oracle, r, want, n)
    assert got.tobytes() == oracle.tobytes(), np.nonzero(got != oracle)[0][:10].tolist()
    assert {int(i): int(got[i]) for i in np.nonzero(got)[0]} == want
    kinds = {(j + shift) % 4 for j in range(len(want))}
    assert kinds == {0, 1, 2, 3}


def test_second_call_on_the_same_context(gpu, base):
    """The same call twice on one context, then a call whose spoiled rows are other kinds: no
    thread reads build state or encodings that an earlier launch left in its LDS column."""
    rows, base_oracle = base
    n = SIZES[0]
    r, want = _spoil(rows, n, 0)
    first = gpu.verify_each(*[r[k] for k in KEYS])
    second = gpu.verify_each(*[r[k] for k in KEYS])
    assert first.tobytes() == second.tobytes()
    assert first.tobytes() == _oracle(base_oracle, r, want, n).tobytes()
    r2, want2 = _spoil(rows, n, 2)
    third = gpu.verify_each(*[r2[k] for k in KEYS])
    assert third.tobytes() == _oracle(base_oracle, r2, want2, n).tobytes()
