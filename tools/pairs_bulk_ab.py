#!/usr/bin/env python3
"""A/B of the bulk mixed-pair per-proof call against what a caller had before it, in one process.

    tools/pairs_bulk_ab.py [--out FILE] [--reps K] [--sizes 2049,16384,131072,1048576] [--dense LOG2N]

64 custom pairs, entry i under pair i % 64, no contexts, three forged entries; every size warm
(one context, every pair resident) and cold (a fresh context per call):

  A   host    Gpu.verify_each_pairs_bulk on host rows
      device  Gpu.verify_each_pairs_device on rows, indices and statuses resident on the device
  B   (a)     Gpu.verify_each_pairs in 2048-entry calls
      (b)     one Gpu.verify_each per pair on the rows the caller gathers for it; the gather and
              the scatter of the statuses are part of the span and are also timed alone

and the batch check's dense fallback (tests/test_gpu_pairs_bulk.py's shape scaled to 2^LOG2N: five
pairs, s + 1 in five of the eight top-level parts) with the leaf's eight-lane path and, through
CPZ_PAIRS_LEAF_QUAD=0, with the serial 2048-proof latency launches it replaces.

The sides alternate inside every repetition, every shape is warmed up first (a throw-away context
loads the code objects before any cold time is taken), and the times are host clocks around calls
that return synchronised.  Writes medians and spreads (min, max) in milliseconds, the ratios
B / A of the medians and B's own run-to-run spread as JSON."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "chaum-pedersen-zkp_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import chaum_pedersen as cp  # noqa: E402
import pyoracle as O  # noqa: E402
from chaum_pedersen import _native  # noqa: E402

Q = ("y1", "y2", "r1", "r2", "s")
SEED = hashlib.sha256(b"pairs-bulk-ab").digest()
K = 64


def pairs_of(k, tag):
    out = []
    for i in range(k):
        a = O.scalar_wide(hashlib.sha512(tag + b"-g-%d" % i).digest())
        b = O.scalar_wide(hashlib.sha512(tag + b"-h-%d" % i).digest())
        out.append(cp.Parameters(O.ristretto_encode(O.pt_mul(O.BASEPOINT, a)),
                                 O.ristretto_encode(O.pt_mul(O.BASEPOINT, b))))
    return out


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "runs": len(xs)}


def proofs(gpu, pairs, n, forged):
    """n entries, entry i under pair i % len(pairs); `forged` get s + 1."""
    k = len(pairs)
    groups = (np.arange(n) % k).astype(np.uint32)
    rows = {q: np.zeros((n, 32), np.uint8) for q in Q}
    for p in range(k):
        idx = np.nonzero(groups == p)[0]
        out = gpu.prove_synthetic(len(idx), SEED, SEED[::-1], first_index=p * n, params=pairs[p])
        for q in Q:
            rows[q][idx] = out[q]
    for i in forged:
        v = int.from_bytes(rows["s"][i].tobytes(), "little") + 1
        rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    want = np.zeros(n, np.uint8)
    want[list(forged)] = 1
    return groups, rows, want


def size_case(gpu, pairs, n, reps):
    import torch
    forged = (0, n // 2, n - 1)
    groups, rows, want = proofs(gpu, pairs, n, forged)
    cols = [rows[q] for q in Q]
    dev = torch.device("cuda:0")
    d_cols = [torch.from_numpy(c).to(dev) for c in cols]
    d_idx = torch.from_numpy(groups.astype(np.int32)).to(dev)
    d_out = torch.empty(n, dtype=torch.uint8, device=dev)
    member = [np.nonzero(groups == p)[0] for p in range(K)]
    torch.cuda.synchronize()

    def a_host(g):
        assert np.array_equal(g.verify_each_pairs_bulk(pairs, groups, *cols), want)

    def a_device(g):
        g.verify_each_pairs_device(pairs, d_idx, *d_cols, d_out)

    def b_calls(g):
        out = np.empty(n, np.uint8)
        for lo in range(0, n, _native.PAIRS_MAX_PROOFS):
            hi = min(n, lo + _native.PAIRS_MAX_PROOFS)
            out[lo:hi] = g.verify_each_pairs(pairs, groups[lo:hi], *[c[lo:hi] for c in cols])
        assert np.array_equal(out, want)

    def gather():
        return [[np.ascontiguousarray(c[idx]) for c in cols] for idx in member]

    def b_groups(g):
        out = np.empty(n, np.uint8)
        for p, part in enumerate(gather()):
            out[member[p]] = g.verify_each(*part, params=pairs[p])
        assert np.array_equal(out, want)

    def b_gather_alone(g):
        out = np.empty(n, np.uint8)
        for p, part in enumerate(gather()):
            out[member[p]] = 0

    sides = (("A_host", a_host), ("A_device", a_device), ("B_a_2048_entry_calls", b_calls),
             ("B_b_one_call_per_pair", b_groups), ("B_b_gather_alone", b_gather_alone))
    res = {"warm": {nm: [] for nm, _ in sides}, "cold": {nm: [] for nm, _ in sides if nm != "B_b_gather_alone"}}
    for nm, fn in sides:                      # every shape once, untimed
        fn(gpu)
    assert np.array_equal(d_out.cpu().numpy(), want)
    for _ in range(reps):
        for nm, fn in sides:
            res["warm"][nm].append(timed(lambda: fn(gpu))[0])
    for _ in range(reps):
        for nm, fn in sides:
            if nm == "B_b_gather_alone":
                continue
            with cp.Gpu(0) as fresh:
                res["cold"][nm].append(timed(lambda: fn(fresh))[0])
    out = {c: {nm: stats(v) for nm, v in d.items()} for c, d in res.items()}
    for c in ("warm", "cold"):
        d = out[c]
        for a in ("A_host", "A_device"):
            for b in ("B_a_2048_entry_calls", "B_b_one_call_per_pair"):
                d["ratio_%s_over_%s" % (b, a)] = round(d[b]["median_ms"] / d[a]["median_ms"], 3)
        for b in ("B_a_2048_entry_calls", "B_b_one_call_per_pair"):
            d["spread_" + b] = round((d[b]["max_ms"] - d[b]["min_ms"]) / d[b]["median_ms"], 4)
        # A wins when its slowest run is faster than B's fastest: more than B's own spread
        d["A_host_wins"] = d["A_host"]["max_ms"] < min(d["B_a_2048_entry_calls"]["min_ms"],
                                                       d["B_b_one_call_per_pair"]["min_ms"])
        d["A_device_wins"] = d["A_device"]["max_ms"] < min(d["B_a_2048_entry_calls"]["min_ms"],
                                                           d["B_b_one_call_per_pair"]["min_ms"])
    out["shape"] = {"n": n, "pairs": K, "forged": list(forged), "contexts": "none"}
    return out


def dense_case(gpu, log2n, reps):
    n = 1 << log2n
    pairs = [cp.Parameters()] + pairs_of(4, b"ab-dense")
    forged = tuple(int(n * f) for f in (0.002, 0.146, 0.268, 0.512, 0.9998))   # parts 0, 1, 2, 4, 7 of 8
    groups, rows, want = proofs(gpu, pairs, n, forged)
    cols = [rows[q] for q in Q]

    def run(quad):
        os.environ["CPZ_PAIRS_LEAF_QUAD"] = "1" if quad else "0"
        partial, ok, st = gpu.verify_batch_pairs(pairs, groups, *cols, SEED)
        fb = gpu.fallback_stats()
        assert not ok and np.array_equal(st, want)
        assert fb["path"] == "bisection" and fb["bisection_msms"] == 8 and fb["per_proof"] == n, fb

    res = {"leaf_eight_lane_chunks": [], "leaf_serial_2048_proof_launches": []}
    try:
        run(True)
        run(False)
        for _ in range(reps):
            res["leaf_eight_lane_chunks"].append(timed(lambda: run(True))[0])
            res["leaf_serial_2048_proof_launches"].append(timed(lambda: run(False))[0])
    finally:
        os.environ.pop("CPZ_PAIRS_LEAF_QUAD", None)
    out = {nm: stats(v) for nm, v in res.items()}
    out["ratio_serial_over_chunks"] = round(out["leaf_serial_2048_proof_launches"]["median_ms"] /
                                            out["leaf_eight_lane_chunks"]["median_ms"], 3)
    out["shape"] = {"n": n, "pairs": 5, "forged": list(forged), "call": "verify_batch_pairs, statuses, whole call"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="2049,16384,131072,1048576")
    ap.add_argument("--dense", type=int, default=20)
    a = ap.parse_args()
    if a.reps < 3:
        ap.error("at least three repetitions")
    result = {"device": "MI355X (gfx950)", "clock": "host perf_counter around calls that return synchronised",
              "reps": a.reps}
    pairs = pairs_of(K, b"ab-bulk")
    with cp.Gpu(0) as gpu:
        with cp.Gpu(0) as warm:  # code objects, allocator: before any cold time
            w = pairs_of(2, b"ab-warm")
            g3, r3, _ = proofs(warm, w, 2049, ())
            warm.verify_each_pairs_bulk(w, g3, *[r3[q] for q in Q])
            warm.verify_each_pairs(w, g3[:8], *[r3[q][:8] for q in Q])
            warm.verify_each(*[r3[q][:8:2] for q in Q], params=w[0])
        for n in [int(x) for x in a.sizes.split(",") if x]:
            result["n_%d" % n] = size_case(gpu, pairs, n, a.reps)
        if a.dense:
            result["dense_fallback_2pow%d" % a.dense] = dense_case(gpu, a.dense, a.reps)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
