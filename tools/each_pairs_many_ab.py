#!/usr/bin/env python3
"""A/B of cpz_verify_each_pairs_many against what a caller with more than 64 pairs had before it,
in one process.

    tools/each_pairs_many_ab.py [--out FILE] [--reps K] [--cases a,b,p,t] [--big 17,20]

  (a) 1000 entries over 1000 pairs, all valid, cold (the first call on a fresh context) and warm:
      one verify_each_pairs_many call against 16 verify_each_pairs calls of 64 pairs
      (BatchVerifier's route before this call existed).
  (b) 2^17 and 2^20 entries over 4096 pairs, all valid, uniform and with 90 % of the entries in one
      pair, warm: one call against 64 verify_each_pairs_bulk calls of 64 pairs on rows gathered by
      pair (the gathering is not timed).
  (p) the price of the small tables at equal pair count: 64 pairs, 16,384 and 2^20 entries,
      CPZ_EACH_MANY_FORWARD=0 (read at every call) against the forwarded call, warm and cold.
      Reported only.
  (t) stage 13 (the span of the table build, GPU time) of a call over 65, 1000 and 4096 pairs, and
      stage 5 (the verify launches) of the 1000-entry call beside it.

The sides alternate, each shape is warmed up first, and the times are host clocks around the
synchronous calls.  Writes medians and spreads (min, max) in milliseconds as JSON."""
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
K = 64
KNOB = "CPZ_EACH_MANY_FORWARD"


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


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "runs": len(xs)}


def ratio(res, old, new):
    """old / new by the medians, and whether the two ranges are apart (new's max below old's min)."""
    return {"speedup_by_medians": round(res[old]["median_ms"] / res[new]["median_ms"], 2),
            "ranges_apart": res[new]["max_ms"] < res[old]["min_ms"]}


def gathered(pairs, idx, rows):
    """Per chunk of 64 pairs: (pairs, local indices, columns) of its entries."""
    idx = np.asarray(idx, np.int64)
    out = []
    for c in range(0, len(pairs), K):
        sel = np.nonzero((idx >= c) & (idx < c + K))[0]
        if len(sel):
            out.append((pairs[c:c + K], (idx[sel] - c).astype(np.uint32), [np.ascontiguousarray(rows[q][sel]) for q in Q]))
    return out


def sides(pairs, idx, rows, bulk):
    """The new call and the route of 64 pairs a call; each checks that every entry passes."""
    idx = np.ascontiguousarray(idx, np.uint32)
    cols = [rows[q] for q in Q]
    chunks = gathered(pairs, idx, rows)

    def many(g):
        assert not g.verify_each_pairs_many(pairs, idx, *cols).any()

    def per64(g):
        for pr, li, cl in chunks:
            assert not (g.verify_each_pairs_bulk if bulk else g.verify_each_pairs)(pr, li, *cl).any()

    return many, per64


def case_small(gpu, reps):
    n = 1000
    pairs = many_pairs(gpu, n, b"small")
    idx = np.arange(n, dtype=np.uint32)
    rows = prove_many(gpu, pairs, idx, b"small-rows")
    many, per64 = sides(pairs, idx, rows, False)
    named = [("verify_each_pairs_many", many), ("verify_each_pairs_x16", per64)]
    res = {"cold": {nm: [] for nm, _ in named}, "warm": {nm: [] for nm, _ in named}}
    for _ in range(reps):
        for nm, fn in named:
            with cp.Gpu(0) as fresh:
                res["cold"][nm].append(timed(lambda: fn(fresh))[0])
    with cp.Gpu(0) as g:
        for _, fn in named:
            fn(g)
        for _ in range(max(reps, 10)):
            for nm, fn in named:
                res["warm"][nm].append(timed(lambda: fn(g))[0])
    out = {c: {nm: stats(v) for nm, v in d.items()} for c, d in res.items()}
    for c in ("cold", "warm"):
        out[c]["new_against_x16"] = ratio(out[c], "verify_each_pairs_x16", "verify_each_pairs_many")
    out["shape"] = {"n": n, "pairs": n}
    return out


def case_big(gpu, reps, log2n):
    out = {}
    n = 1 << log2n
    for name, skew in (("uniform", False), ("skewed_90pct_in_one_pair", True)):
        rs = np.random.RandomState(5)
        idx = rs.randint(0, 4096, size=n).astype(np.uint32)
        if skew:
            idx[rs.rand(n) < 0.9] = 0
        pairs = many_pairs(gpu, 4096, b"big")
        rows = prove_many(gpu, pairs, idx, b"big-rows")
        many, per64 = sides(pairs, idx, rows, True)
        res = {"verify_each_pairs_many": [], "verify_each_pairs_bulk_x64": []}
        with cp.Gpu(0) as g:
            many(g)
            per64(g)
            for _ in range(reps):
                res["verify_each_pairs_many"].append(timed(lambda: many(g))[0])
                res["verify_each_pairs_bulk_x64"].append(timed(lambda: per64(g))[0])
        out[name] = {nm: stats(v) for nm, v in res.items()}
        out[name]["new_against_x64"] = ratio(out[name], "verify_each_pairs_bulk_x64", "verify_each_pairs_many")
        out[name]["largest_pair_share"] = round(float(np.bincount(idx).max()) / n, 4)
    out["shape"] = {"n": n, "pairs": 4096}
    return out


def case_price(gpu, reps, n):
    pairs = many_pairs(gpu, 64, b"price")
    idx = np.random.RandomState(9).randint(0, 64, size=n).astype(np.uint32)
    rows = prove_many(gpu, pairs, idx, b"price-rows")
    cols = [rows[q] for q in Q]

    def call(g, knob):
        if knob:
            os.environ[KNOB] = "0"
        try:
            assert not g.verify_each_pairs_many(pairs, idx, *cols).any()
        finally:
            os.environ.pop(KNOB, None)

    named = [("forwarded_128_entry_tables", False), ("small_tables", True)]
    res = {"cold": {nm: [] for nm, _ in named}, "warm": {nm: [] for nm, _ in named}}
    for _ in range(reps):
        for nm, knob in named:
            with cp.Gpu(0) as fresh:
                res["cold"][nm].append(timed(lambda: call(fresh, knob))[0])
    with cp.Gpu(0) as g:
        for _, knob in named:
            call(g, knob)
        for _ in range(reps):
            for nm, knob in named:
                res["warm"][nm].append(timed(lambda: call(g, knob))[0])
    out = {c: {nm: stats(v) for nm, v in d.items()} for c, d in res.items()}
    for c in ("cold", "warm"):
        out[c]["small_over_forwarded"] = round(out[c]["small_tables"]["median_ms"] /
                                               out[c]["forwarded_128_entry_tables"]["median_ms"], 3)
    out["shape"] = {"n": n, "pairs": 64}
    return out


def case_build(gpu, reps):
    pairs = many_pairs(gpu, 4096, b"build")
    out = {}
    with cp.Gpu(0) as g:
        for npairs in (65, 1000, 4096):
            n = max(npairs, 1000) if npairs != 65 else 130
            idx = (np.arange(n) % npairs).astype(np.uint32)
            rows = prove_many(gpu, pairs[:npairs], idx, b"build-rows-%d" % npairs)
            cols = [rows[q] for q in Q]
            g.set_timing(True)
            g.verify_each_pairs_many(pairs[:npairs], idx, *cols)
            g.stage_times()
            build, verify, desc = [], [], []
            for _ in range(max(reps, 10)):
                assert not g.verify_each_pairs_many(pairs[:npairs], idx, *cols).any()
                t = g.stage_times()
                assert t["generators_varbase"][1] == npairs
                build.append(t["generators_varbase"][0])
                verify.append(t["verify_span"][0] if "verify_span" in t else t["verify_each"][0])
                desc.append(t.get("rlc_prepare", (0.0, 0))[0])
            g.set_timing(False)
            out["%d_pairs" % npairs] = {"n": n, "stage13_table_build": stats(build), "stage5_verify": stats(verify),
                                        "stage2_descriptors": stats(desc)}
    out["note"] = "GPU time between events on the call's stream"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="a,b,p,t")
    ap.add_argument("--big", default="17,20")
    a = ap.parse_args()
    cases = a.cases.split(",")
    result = {"device": "MI355X (gfx950)", "clock": "host perf_counter around synchronous calls", "reps": a.reps}

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    with cp.Gpu(0) as gpu:
        with cp.Gpu(0) as warm:  # code objects, allocator: before any cold time
            w = many_pairs(warm, 70, b"warm")
            i70 = (np.arange(2100) % 70).astype(np.uint32)
            r = prove_many(warm, w, i70, b"warm-rows")
            warm.verify_each_pairs_many(w, i70, *[r[q] for q in Q])
            warm.verify_each_pairs_bulk(w[:64], i70 % 64, *[r[q] for q in Q])
            warm.verify_each_pairs(w[:64], i70[:140] % 64, *[r[q][:140] for q in Q])
        if "a" in cases:
            result["a_1000_entries_1000_pairs"] = case_small(gpu, a.reps)
            flush()
        if "t" in cases:
            result["t_table_build"] = case_build(gpu, a.reps)
            flush()
        if "p" in cases:
            for n in (16384, 1 << 20):
                result["p_%d_entries_64_pairs" % n] = case_price(gpu, a.reps, n)
                flush()
        if "b" in cases:
            for log2n in [int(x) for x in a.big.split(",") if x]:
                result["b_2pow%d_entries_4096_pairs" % log2n] = case_big(gpu, a.reps, log2n)
                flush()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
