"""k_verify_each / k_verify_prepared with the joint table, at the smallest shapes that reach them
(launches above the eight-lane kernel's 16,384 proofs): statuses byte-equal to the C oracle's,
with spoiled rows at the first, middle and last index of every launch."""
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
LAUNCH = 1 << 16  # proofs per k_verify_each launch on MI355X (half the occupancy grid x 256)


def _threads():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return max(1, min(16, os.cpu_count() or 1))


def _synthetic(gpu, torch, n):
    t = {k: torch.empty((n, 32), dtype=torch.uint8, device="cuda:0") for k in KEYS}
    gpu.prove_synthetic_device(n, SX, SK, t["y1"], t["y2"], t["r1"], t["r2"], t["s"])
    return {k: v.cpu().numpy() for k, v in t.items()}


def _spoil(rows, idx):
    """The benchmark's four kinds of spoiled row, in turn: s + 1, the y1 of the row seven
    further on, an r1 that decodes to no point (01 00 .. 00), s = 0."""
    n = len(rows["s"])
    y1 = rows["y1"].copy()
    want = {}
    for j, i in enumerate(idx):
        kind = j % 4
        if kind == 0:
            v = (int.from_bytes(rows["s"][i].tobytes(), "little") + 1) % O.L
            rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
        elif kind == 1:
            rows["y1"][i] = y1[(i + 7) % n]
        elif kind == 2:
            rows["r1"][i] = 0
            rows["r1"][i, 0] = 1
        else:
            rows["s"][i] = 0
        want[int(i)] = (1, 1, 2, 5)[kind]
    return want


@pytest.mark.parametrize("n", [16385, LAUNCH + 257])
def test_verify_each_launch_edges(gpu, n):
    """n = 16,385: one launch whose last block holds one live thread.  n = 65,536 + 257: two
    launches on two streams with a slab each, and a ragged tail."""
    torch = pytest.importorskip("torch")
    rows = _synthetic(gpu, torch, n)
    idx = []
    for lo in range(0, n, LAUNCH):
        hi = min(n, lo + LAUNCH)
        mid = (lo + hi) // 2
        # every kind at the first, the middle and the last indices of the launch
        idx += [lo, lo + 1, lo + 2, lo + 3, mid - 2, mid - 1, mid, mid + 1, hi - 4, hi - 3, hi - 2, hi - 1]
    # shifted so that the first index of a launch is not always s + 1, nor the last always s = 0
    idx = sorted(set(idx))
    idx = idx[1:] + idx[:1]
    want = _spoil(rows, idx)
    dev = {k: torch.from_numpy(rows[k]).to("cuda:0") for k in KEYS}
    st = torch.full((n,), 0xee, dtype=torch.uint8, device="cuda:0")
    gpu.verify_each_device(dev["y1"], dev["y2"], dev["r1"], dev["r2"], dev["s"], st)
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    oracle = C.verify_many(rows, threads=_threads())
    assert got.tobytes() == oracle.tobytes(), np.nonzero(got != oracle)[0][:10].tolist()
    assert {int(i): int(got[i]) for i in np.nonzero(got)[0]} == want


def test_rlc_fallback_reaches_prepared_kernel(gpu):
    """A failing batch just above 16,384 proofs with two forgeries: the fallback verifies the
    whole range per proof from the prepared points (k_verify_prepared), and reports exactly the
    two."""
    torch = pytest.importorskip("torch")
    n = 16384 + 129
    rows = _synthetic(gpu, torch, n)
    bad = [0, n - 1]
    for i in bad:
        v = (int.from_bytes(rows["s"][i].tobytes(), "little") + 1) % O.L
        rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    dev = {k: torch.from_numpy(rows[k]).to("cuda:0") for k in KEYS}
    st = torch.full((n,), 0xee, dtype=torch.uint8, device="cuda:0")
    seed = hashlib.sha256(b"cpz-weights-v1").digest()
    partial, ok = gpu.verify_batch_device(dev["y1"], dev["y2"], dev["r1"], dev["r2"], dev["s"], st, seed, fallback=True)
    assert not ok and partial != bytes(32)
    got = st.cpu().numpy()
    assert gpu.fallback_stats()["per_proof"] == n
    assert np.nonzero(got)[0].tolist() == bad and got[bad].tolist() == [1, 1]
    sub = {k: rows[k][bad] for k in KEYS}
    assert C.verify_many(sub).tolist() == [1, 1]
