#!/usr/bin/env python3
"""A/B of the mixed-pair prover against one cpz_prove per pair, in one process.

    tools/prove_pairs_ab.py [--out profiles/prove_pairs_ab.json] [--reps K] [--cold K]

n in {2048, 2^17, 2^20} over 64 custom pairs (entry i under pair i % 64) and n = 2^20 over one
custom pair, no contexts, random witnesses and nonces:

  A   one Gpu.prove (cpz_prove) per pair, on inputs gathered per pair beforehand (the gather and
      the scatter of the rows are not in the span): each pair's proofs from its comb, which the
      context builds when the pair is not among its CPZ_GEN_CACHE = 4 cached full sets
  B   one Gpu.prove_pairs (cpz_prove_pairs): every proof from its pair's 128-entry tables, no comb

each cold (a fresh context per run) and warm (one context, the sides alternating inside every
repetition, after one untimed run of each).  Also B's stage-6 kernel time (a run of its own with
the stage timers on) and the single-pair cpz_prove rate at 2^20 proofs on the default pair, the
comb-based yardstick.  B's rows are compared with A's at every size.  Times are host clocks around
calls that return synchronised; medians and spreads (min, max) in milliseconds as JSON."""
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


def case(gpu, pairs, n, reps, cold):
    k = len(pairs)
    rng = np.random.default_rng(n + k)
    xs = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32)   # any 32 bytes: taken mod l
    ks = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32)
    groups = (np.arange(n) % k).astype(np.uint32)
    member = [np.nonzero(groups == p)[0] for p in range(k)]
    parts = [(np.ascontiguousarray(xs[m]), np.ascontiguousarray(ks[m])) for m in member]

    def side_a(g):
        return [g.prove(px, pk, params=pairs[p]) for p, (px, pk) in enumerate(parts)]

    def side_b(g):
        return g.prove_pairs(pairs, groups, xs, ks)

    a0, b0 = side_a(gpu), side_b(gpu)            # untimed; and B's rows are A's
    for p, m in enumerate(member):
        for q in Q:
            assert np.array_equal(b0[q][m], a0[p][q]), (n, p, q)
    del a0, b0
    res = {"warm": {"A": [], "B": []}, "cold": {"A": [], "B": []}}
    for _ in range(reps):
        res["warm"]["A"].append(timed(lambda: side_a(gpu))[0])
        res["warm"]["B"].append(timed(lambda: side_b(gpu))[0])
    for _ in range(cold):
        for nm, fn in (("A", side_a), ("B", side_b)):
            with cp.Gpu(0) as fresh:
                res["cold"][nm].append(timed(lambda: fn(fresh))[0])
    out = {c: {nm: stats(v) for nm, v in d.items()} for c, d in res.items()}
    for c in ("warm", "cold"):
        d = out[c]
        d["ratio_A_over_B"] = round(d["A"]["median_ms"] / d["B"]["median_ms"], 3)
        d["B_ahead"] = d["B"]["max_ms"] < d["A"]["min_ms"]      # by more than either side's spread
        d["B_proofs_per_s"] = round(n / d["B"]["median_ms"] * 1e3)
        d["A_proofs_per_s"] = round(n / d["A"]["median_ms"] * 1e3)
    gpu.set_timing(True)
    gpu.stage_times()
    side_b(gpu)
    st = gpu.stage_times()
    gpu.set_timing(False)
    assert "generators" not in st, st
    out["B_stage6_prove_ms"] = round(st["prove"][0], 4)
    out["B_stage6_launches"] = st["prove"][1]
    out["B_stage6_proofs_per_s"] = round(n / st["prove"][0] * 1e3)
    out["shape"] = {"n": n, "pairs": k, "contexts": "none"}
    return out


def yardstick(gpu, n, reps):
    rng = np.random.default_rng(7)
    xs = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32)
    ks = np.frombuffer(rng.bytes(32 * n), np.uint8).reshape(n, 32)
    gpu.prove(xs, ks)
    t = [timed(lambda: gpu.prove(xs, ks))[0] for _ in range(reps)]
    gpu.set_timing(True)
    gpu.stage_times()
    gpu.prove(xs, ks)
    st = gpu.stage_times()
    gpu.set_timing(False)
    out = stats(t)
    out["proofs_per_s"] = round(n / out["median_ms"] * 1e3)
    out["stage6_prove_ms"] = round(st["prove"][0], 4)
    out["stage6_proofs_per_s"] = round(n / st["prove"][0] * 1e3)
    out["shape"] = {"n": n, "pair": "default", "call": "cpz_prove, warm"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cold", type=int, default=3)
    ap.add_argument("--sizes", default="2048,131072,1048576")
    a = ap.parse_args()
    if a.reps < 5 or a.cold < 1:
        ap.error("at least five warm repetitions and one cold pass")
    result = {"device": "MI355X (gfx950)", "clock": "host perf_counter around calls that return synchronised",
              "warm_reps": a.reps, "cold_passes": a.cold,
              "A": "one cpz_prove per pair on inputs gathered beforehand", "B": "one cpz_prove_pairs"}
    pairs = pairs_of(64, b"ab-prove")
    with cp.Gpu(0) as gpu:
        with cp.Gpu(0) as warm:  # code objects, allocator: before any cold time
            w = pairs_of(2, b"ab-prove-warm")
            warm.prove_pairs(w, [0, 1, 0, 1], [1, 2, 3, 4], [5, 6, 7, 8])
            warm.prove([1, 2], [3, 4], params=w[0])
        sizes = [int(x) for x in a.sizes.split(",") if x]
        for n in sizes:
            result["n_%d_pairs_64" % n] = case(gpu, pairs, n, a.reps, a.cold)
        big = max(sizes)
        result["n_%d_pairs_1" % big] = case(gpu, pairs[:1], big, a.reps, a.cold)
        result["yardstick_default_pair_n_%d" % big] = yardstick(gpu, big, a.reps)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
