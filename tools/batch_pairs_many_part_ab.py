#!/usr/bin/env python3
"""A/B of the routes a caller has for a FAILING batch over more than 64 pairs, in one process.

    tools/batch_pairs_many_part_ab.py [--out FILE] [--reps K] [--sizes small,17,20] [--slow-ms MS]
                                      [--densities one,0.001,0.01,0.1] [--shapes uniform,skewed]

  small   1000 entries over 1000 pairs, 3 forged.
  17, 20  2^17 / 2^20 entries over 4096 pairs, uniform and with 90 % of the entries in one pair,
          with 1 forged entry and with 0.1 %, 1 % and 10 % forged.

Routes compared on the same rows, alternating, after one warm-up call each:
  flagged    verify_batch_pairs_many(..., locate="partitioned")  (CPZ_CALL_PARTITIONED_MANY)
  unflagged  verify_batch_pairs_many(...)                         (bisection, then runs)
  each       verify_each_pairs_many(...)                          (everything per proof)
Every call's statuses are checked against the forged set.  A route whose warm-up call takes longer
than --slow-ms is not repeated: its cell holds that one run ("runs": 1).  The GPU times of stages
13 (small tables / sets built), 14 (the block walk) and 15 (the locate pass's walk) of the flagged
and unflagged routes are reported on the side, from one more timed call each.

The times are host clocks around the synchronous calls.  Writes medians with min and max in
milliseconds as JSON, flushed after every cell; an exception ends the run (nothing is started after
a failed call)."""
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

Q = ("y1", "y2", "r1", "r2", "s")
SEED = hashlib.sha256(b"batch-pairs-many-part-ab").digest()
K = 64
SIDE_STAGES = ("generators_varbase", "part_acc", "part_acc_locate")   # stages 13, 14, 15


def scalars(tag, n):
    rs = np.random.RandomState(int.from_bytes(hashlib.sha256(tag).digest()[:4], "little"))
    a = rs.randint(0, 256, size=(n, 32)).astype(np.uint8)
    a[:, 31] &= 0x0f
    return a


def many_pairs(gpu, k, tag):
    out = gpu.prove(scalars(tag + b"-a", k), scalars(tag + b"-k", k))
    return [cp.Parameters(out["y1"][i].tobytes(), out["y2"][i].tobytes()) for i in range(k)]


def prove_many(gpu, pairs, idx, tag):
    idx = np.asarray(idx, np.int64)
    n = len(idx)
    xs, ks = scalars(tag + b"-x", n), scalars(tag + b"-k", n)
    rows = {q: np.zeros((n, 32), np.uint8) for q in Q}
    for c in range(0, len(pairs), K):
        sel = np.nonzero((idx >= c) & (idx < c + K))[0]
        if len(sel):
            out = gpu.prove_pairs(pairs[c:c + K], idx[sel] - c, np.ascontiguousarray(xs[sel]),
                                  np.ascontiguousarray(ks[sel]))
            for q in Q:
                rows[q][sel] = out[q]
    return rows


def forged_rows(rows, entries):
    """A copy of the s column with s + 1 at `entries` (s < 2^252, so no carry leaves the row)."""
    s = rows["s"].copy()
    for i in entries:
        v = int.from_bytes(s[i].tobytes(), "little") + 1
        s[i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    out = dict(rows)
    out["s"] = s
    return out


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "runs": len(xs)}


def routes(pairs, idx, rows, want):
    idx = np.ascontiguousarray(idx, np.uint32)
    cols = [rows[q] for q in Q]

    def flagged(g):
        partial, ok, st = g.verify_batch_pairs_many(pairs, idx, *cols, SEED, locate="partitioned")
        assert not ok and np.array_equal(st, want)
        assert g.fallback_stats()["path"] == "partitioned"

    def unflagged(g):
        partial, ok, st = g.verify_batch_pairs_many(pairs, idx, *cols, SEED)
        assert not ok and np.array_equal(st, want)
        assert g.fallback_stats()["path"] == "bisection"

    def each(g):
        assert np.array_equal(g.verify_each_pairs_many(pairs, idx, *cols), want)

    return [("flagged", flagged), ("unflagged", unflagged), ("each", each)]


def cell(g, pairs, idx, rows, forged, reps, slow_ms):
    want = np.zeros(len(idx), np.uint8)
    want[forged] = 1
    named = routes(pairs, idx, forged_rows(rows, forged), want)
    res, live = {}, []
    for nm, fn in named:                                    # warm-up; a slow route is not repeated
        ms = timed(lambda: fn(g))
        if ms > slow_ms:
            res[nm] = [ms]
        else:
            res[nm] = []
            live.append((nm, fn))
    for _ in range(reps):
        for nm, fn in live:
            res[nm].append(timed(lambda: fn(g)))
    out = {nm: stats(v) for nm, v in res.items()}
    g.set_timing(True)
    for nm, fn in named[:2]:                                # stages 13 / 14 / 15, GPU time, one call
        if len(res[nm]) == 1 and reps > 1:
            continue                                        # the slow route is not run again
        g.stage_times()
        fn(g)
        t = g.stage_times()
        out[nm]["stage_ms"] = {s: [round(t.get(s, (0.0, 0))[0], 4), t.get(s, (0.0, 0))[1]] for s in SIDE_STAGES}
        out[nm]["fallback_stats"] = g.fallback_stats()
    g.set_timing(False)
    out["forged"] = len(forged)
    return out


def pick_forged(n, density, rs):
    if density == "one":
        return [n // 2 + 77]
    k = max(1, int(round(n * float(density))))
    return sorted(rs.choice(n, size=k, replace=False).tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="small,17,20")
    ap.add_argument("--densities", default="one,0.001,0.01,0.1")
    ap.add_argument("--shapes", default="uniform,skewed")
    ap.add_argument("--slow-ms", type=float, default=2000.0)
    a = ap.parse_args()
    result = {"device": "MI355X (gfx950)", "clock": "host perf_counter around synchronous calls", "reps": a.reps,
              "slow_ms": a.slow_ms, "routes": {"flagged": "verify_batch_pairs_many locate=partitioned",
                                               "unflagged": "verify_batch_pairs_many (bisection, runs)",
                                               "each": "verify_each_pairs_many"},
              "stage_ms": "GPU ms and launch count of stages 13, 14, 15 in one call", "cells": {}}

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    with cp.Gpu(0) as g:
        for size in a.sizes.split(","):
            if size == "small":
                n = 1000
                pairs = many_pairs(g, n, b"small")
                idx = np.arange(n, dtype=np.uint32)
                rows = prove_many(g, pairs, idx, b"small-rows")
                result["cells"]["1000_entries_1000_pairs_3_forged"] = cell(g, pairs, idx, rows, [3, 500, 999],
                                                                           max(a.reps, 10), a.slow_ms)
                flush()
                continue
            n = 1 << int(size)
            pairs = many_pairs(g, 4096, b"big")
            for shape in a.shapes.split(","):
                rs = np.random.RandomState(5)
                idx = rs.randint(0, 4096, size=n).astype(np.uint32)
                if shape == "skewed":
                    idx[rs.rand(n) < 0.9] = 0
                rows = prove_many(g, pairs, idx, b"big-rows-" + shape.encode() + size.encode())
                for d in a.densities.split(","):
                    key = "2pow%s_entries_4096_pairs_%s_forged_%s" % (size, shape, d)
                    result["cells"][key] = cell(g, pairs, idx, rows, pick_forged(n, d, rs), a.reps, a.slow_ms)
                    flush()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
