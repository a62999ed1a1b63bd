"""k_verify_each / k_verify_prepared with the lazy window sign and the lean joint table, at the
smallest launch that reaches them (16,640 proofs: 65 blocks of 256, above the eight-lane kernel's
16,384): statuses byte-equal to the C oracle's with one row in 16 spoiled."""
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
N = 16640  # 65 blocks: the last one lies wholly above verify_quad_max


def _threads():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return max(1, min(16, os.cpu_count() or 1))


@pytest.fixture(scope="module")
def rows(gpu):
    """The valid proofs both tests start from (each test spoils a copy)."""
    torch = pytest.importorskip("torch")
    t = {k: torch.empty((N, 32), dtype=torch.uint8, device="cuda:0") for k in KEYS}
    gpu.prove_synthetic_device(N, SX, SK, t["y1"], t["y2"], t["r1"], t["r2"], t["s"])
    r = {k: v.cpu().numpy() for k, v in t.items()}
    for v in r.values():
        v.setflags(write=False)
    return r


def _bump_s(rows, i):
    v = (int.from_bytes(rows["s"][i].tobytes(), "little") + 1) % O.L
    rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)


def test_verify_each_one_row_in_16_spoiled(gpu, rows):
    """One row in 16 spoiled, the benchmark's four kinds in turn (s + 1, the y1 of the row seven
    further on, an r1 that decodes to no point, s = 0), the last block included: every status is
    the C oracle's."""
    torch = pytest.importorskip("torch")
    r = {k: v.copy() for k, v in rows.items()}
    y1 = rows["y1"]
    idx = list(range(5, N, 16))
    assert idx[-1] >= N - 256 and len([i for i in idx if i >= N - 256]) == 16  # the tail block is covered
    want = {}
    for j, i in enumerate(idx):
        kind = j % 4
        if kind == 0:
            _bump_s(r, i)
        elif kind == 1:
            r["y1"][i] = y1[(i + 7) % N]
        elif kind == 2:
            r["r1"][i] = 0
            r["r1"][i, 0] = 1
        else:
            r["s"][i] = 0
        want[i] = (1, 1, 2, 5)[kind]
    dev = {k: torch.from_numpy(r[k]).to("cuda:0") for k in KEYS}
    st = torch.full((N,), 0xee, dtype=torch.uint8, device="cuda:0")
    gpu.verify_each_device(dev["y1"], dev["y2"], dev["r1"], dev["r2"], dev["s"], st)
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    oracle = C.verify_many(r, threads=_threads())
    assert got.tobytes() == oracle.tobytes(), np.nonzero(got != oracle)[0][:10].tolist()
    assert {int(i): int(got[i]) for i in np.nonzero(got)[0]} == want


def test_fallback_reports_the_forged_set(gpu, rows):
    """A failing batch of the same size with 8 forged rows: the fallback verifies every proof from
    the prepared points (k_verify_prepared) and reports exactly the forged ones, status 1."""
    torch = pytest.importorskip("torch")
    r = {k: v.copy() for k, v in rows.items()}
    bad = [0, 255, 256, 8191, 8192, 16383, 16384, N - 1]  # block edges, the eight-lane limit, both ends
    for i in bad:
        _bump_s(r, i)
    dev = {k: torch.from_numpy(r[k]).to("cuda:0") for k in KEYS}
    st = torch.full((N,), 0xee, dtype=torch.uint8, device="cuda:0")
    seed = hashlib.sha256(b"cpz-weights-v1").digest()
    partial, ok = gpu.verify_batch_device(dev["y1"], dev["y2"], dev["r1"], dev["r2"], dev["s"], st, seed, fallback=True)
    assert not ok
    assert gpu.fallback_stats()["per_proof"] == N  # the per-proof kernel saw the whole range
    got = st.cpu().numpy()
    assert np.nonzero(got)[0].tolist() == bad and got[bad].tolist() == [1] * 8
    sub = {k: r[k][bad] for k in KEYS}
    assert C.verify_many(sub).tolist() == [1] * 8
