#!/usr/bin/env python3
"""A/B of the mixed-pair batch check against what a caller had before it, in one process.

    tools/batch_pairs_ab.py [--out FILE] [--reps K] [--cases a,b,c] [--big LOG2N]

  (a) 1000 entries over 64 custom pairs, all valid: Gpu.verify_batch_pairs against
      Gpu.verify_each_pairs, cold (the first call on a fresh context) and warm.
  (b) the same with 3 forged entries, the fallback included.
  (c) 2^20 entries over 64 pairs, all valid: one verify_batch_pairs call against 64 verify_batch
      calls (one per pair, 16,384 entries each) on one context.

The two sides alternate, each shape is warmed up first (a throw-away context loads the code
objects before any cold time is taken), and the times are host clocks around the synchronous
calls.  Writes medians and spreads (min, max) in milliseconds as JSON."""
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

Q = ("y1", "y2", "r1", "r2", "s")
SEED = hashlib.sha256(b"batch-pairs-ab").digest()


def pairs_of(k, tag):
    out = []
    for i in range(k):
        a = O.scalar_wide(hashlib.sha512(tag + b"-g-%d" % i).digest())
        b = O.scalar_wide(hashlib.sha512(tag + b"-h-%d" % i).digest())
        out.append(cp.Parameters(O.ristretto_encode(O.pt_mul(O.BASEPOINT, a)),
                                 O.ristretto_encode(O.pt_mul(O.BASEPOINT, b))))
    return out


def ctx_of(i):
    return (None, hashlib.sha256(b"ctx-%d" % i).digest(), b"ctx%02d" % (i % 100), b"")[i % 4]


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "runs": len(xs)}


def small_cases(gpu, reps, forged):
    n, k = 1000, 64
    pairs = pairs_of(k, b"ab-small")
    groups = (np.arange(n) % k).astype(np.uint32)
    ctxs = [ctx_of(i) for i in range(n)]
    rows = {q: np.zeros((n, 32), np.uint8) for q in Q}
    for p in range(k):
        idx = np.nonzero(groups == p)[0]
        out = gpu.prove_synthetic(len(idx), SEED, SEED[::-1], first_index=1000 * p, contexts=[ctxs[i] for i in idx],
                                  params=pairs[p])
        for q in Q:
            rows[q][idx] = out[q]
    for i in forged:
        v = int.from_bytes(rows["s"][i].tobytes(), "little") + 1
        rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    cols = [rows[q] for q in Q]
    want = np.zeros(n, np.uint8)
    want[list(forged)] = 1

    def batch(g):
        partial, ok, st = g.verify_batch_pairs(pairs, groups, *cols, SEED, contexts=ctxs)
        assert ok == (not forged) and np.array_equal(st, want)

    def each(g):
        assert np.array_equal(g.verify_each_pairs(pairs, groups, *cols, contexts=ctxs), want)

    res = {"cold": {"verify_batch_pairs": [], "verify_each_pairs": []},
           "warm": {"verify_batch_pairs": [], "verify_each_pairs": []}}
    for _ in range(reps):
        for name, fn in (("verify_batch_pairs", batch), ("verify_each_pairs", each)):
            with cp.Gpu(0) as fresh:
                res["cold"][name].append(timed(lambda: fn(fresh))[0])
    with cp.Gpu(0) as g:
        for _ in range(3):
            batch(g)
            each(g)
        for _ in range(max(reps, 10)):
            res["warm"]["verify_batch_pairs"].append(timed(lambda: batch(g))[0])
            res["warm"]["verify_each_pairs"].append(timed(lambda: each(g))[0])
    out = {c: {nm: stats(v) for nm, v in d.items()} for c, d in res.items()}
    out["shape"] = {"n": n, "pairs": k, "forged": list(forged)}
    return out


def big_case(gpu, reps, log2n):
    k = 64
    n = 1 << log2n
    per = n // k
    pairs = pairs_of(k, b"ab-big")
    rows = {q: np.zeros((n, 32), np.uint8) for q in Q}
    for p in range(k):
        out = gpu.prove_synthetic(per, SEED, SEED[::-1], first_index=p * per, params=pairs[p])
        for q in Q:
            rows[q][p * per:(p + 1) * per] = out[q]
    groups = np.repeat(np.arange(k, dtype=np.uint32), per)
    cols = [rows[q] for q in Q]

    def one(g):
        partial, ok, st = g.verify_batch_pairs(pairs, groups, *cols, SEED)
        assert ok and partial == bytes(32) and not st.any()

    def many(g):
        for p in range(k):
            lo, hi = p * per, (p + 1) * per
            partial, ok, st = g.verify_batch(*[c[lo:hi] for c in cols], SEED, first_index=lo, params=pairs[p])
            assert ok and partial == bytes(32)

    res = {"verify_batch_pairs": [], "verify_batch_x64": []}
    with cp.Gpu(0) as g:
        one(g)
        many(g)
        for _ in range(reps):
            res["verify_batch_pairs"].append(timed(lambda: one(g))[0])
            res["verify_batch_x64"].append(timed(lambda: many(g))[0])
    out = {nm: stats(v) for nm, v in res.items()}
    out["shape"] = {"n": n, "pairs": k, "one_lane_prepare": os.environ.get("CPZ_RLC_PAIRS_WIDE") != "1"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--big", type=int, default=20)
    a = ap.parse_args()
    cases = a.cases.split(",")
    result = {"device": "MI355X (gfx950)", "clock": "host perf_counter around synchronous calls", "reps": a.reps}
    with cp.Gpu(0) as gpu:
        with cp.Gpu(0) as warm:  # code objects, allocator: before any cold time
            w = pairs_of(2, b"ab-warm")
            r = warm.prove_synthetic(8, SEED, SEED, params=w[0])
            warm.verify_batch_pairs(w, np.zeros(8, np.uint32), *[r[q] for q in Q], SEED)
            warm.verify_each_pairs(w, np.zeros(8, np.uint32), *[r[q] for q in Q])
        if "a" in cases:
            result["a_1000_entries_64_pairs_valid"] = small_cases(gpu, a.reps, ())
        if "b" in cases:
            result["b_1000_entries_64_pairs_3_forged"] = small_cases(gpu, a.reps, (3, 500, 999))
        if "c" in cases:
            result["c_2pow%d_entries_64_pairs_valid" % a.big] = big_case(gpu, a.reps, a.big)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
