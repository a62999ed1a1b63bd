#!/usr/bin/env python3
"""A/B of cpz_prove_pairs_many against what a caller with more than 64 pairs had before it, in one
process.

    tools/prove_pairs_many_ab.py [--out FILE] [--reps K] [--cases a,b,p,t] [--big 17,20]

  (a) 1000 entries over 1000 pairs, cold (the first call on a fresh context) and warm: one
      prove_pairs_many call against 16 prove_pairs calls of at most 64 pairs on rows gathered by
      pair (the gathering is not timed).
  (b) 2^17 and 2^20 entries over 4096 pairs, cold and warm, the latter uniform and with 90 % of the
      entries in one pair: one call against 64 prove_pairs calls of 64 pairs on gathered rows.
  (p) the price of the small tables at equal pair count: 64 pairs, 16,384 and 2^20 entries,
      CPZ_PROVE_MANY_FORWARD=0 (read at every call) against the forwarded call, warm and cold.
  (t) GPU time by stage of one call: stage 2 (the descriptors), stage 13 (the table build) and stage 6
      (the point kernel, then challenges + responses) at 130 entries over 65 pairs, 1000 over 1000
      and 4096 over 4096 -- what the small call's time is made of.

The sides alternate, each shape is warmed up first, both sides' rows are compared once, and the
times are host clocks around the synchronous calls.  Writes medians and spreads (min, max) in
milliseconds as JSON."""
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
KNOB = "CPZ_PROVE_MANY_FORWARD"
NEW, OLD = "prove_pairs_many", "prove_pairs_runs_of_64"


def scalars(tag, n):
    rs = np.random.RandomState(int.from_bytes(hashlib.sha256(tag).digest()[:4], "little"))
    a = rs.randint(0, 256, size=(n, 32)).astype(np.uint8)
    a[:, 31] &= 0x0f
    return a


def many_pairs(gpu, k, tag):
    out = gpu.prove(scalars(tag + b"-a", k), scalars(tag + b"-k", k))
    return [cp.Parameters(out["y1"][i].tobytes(), out["y2"][i].tobytes()) for i in range(k)]


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "runs": len(xs)}


def ratio(res, old, new):
    """old / new by the medians, and whether the two ranges are apart (and which side is below)."""
    apart = res[new]["max_ms"] < res[old]["min_ms"] or res[old]["max_ms"] < res[new]["min_ms"]
    return {"speedup_by_medians": round(res[old]["median_ms"] / res[new]["median_ms"], 2), "ranges_apart": apart,
            "faster": (new if res[new]["median_ms"] < res[old]["median_ms"] else old) if apart else "ranges overlap"}


def sides(pairs, idx, xs, ks):
    """The new call and the route of at most 64 pairs a call on gathered rows."""
    idx = np.ascontiguousarray(idx, np.uint32)
    wide = np.asarray(idx, np.int64)
    chunks = []
    for c in range(0, len(pairs), K):
        sel = np.nonzero((wide >= c) & (wide < c + K))[0]
        if len(sel):
            chunks.append((pairs[c:c + K], (wide[sel] - c).astype(np.uint32), np.ascontiguousarray(xs[sel]),
                           np.ascontiguousarray(ks[sel]), sel))

    def many(g):
        return g.prove_pairs_many(pairs, idx, xs, ks)

    def per64(g):
        return [(sel, g.prove_pairs(pr, li, x, k)) for pr, li, x, k, sel in chunks]

    def check(g):
        a, b = many(g), per64(g)
        for sel, out in b:
            for q in Q:
                assert np.array_equal(a[q][sel], out[q]), q

    return many, per64, check


def alternate(named, reps, cold):
    res = {nm: [] for nm, _ in named}
    if cold:
        for _ in range(reps):
            for nm, fn in named:
                with cp.Gpu(0) as fresh:
                    res[nm].append(timed(lambda: fn(fresh))[0])
    else:
        with cp.Gpu(0) as g:
            for _, fn in named:
                fn(g)
            for _ in range(reps):
                for nm, fn in named:
                    res[nm].append(timed(lambda: fn(g))[0])
    out = {nm: stats(v) for nm, v in res.items()}
    return out


def case_shape(gpu, reps, n, npairs, skew=False, tag=b"shape"):
    pairs = many_pairs(gpu, npairs, tag)
    rs = np.random.RandomState(5)
    idx = np.arange(n, dtype=np.uint32) if n == npairs else rs.randint(0, npairs, size=n).astype(np.uint32)
    if skew:
        idx[rs.rand(n) < 0.9] = 0
    xs, ks = scalars(tag + b"-x", n), scalars(tag + b"-k", n)
    many, per64, check = sides(pairs, idx, xs, ks)
    check(gpu)
    named = [(NEW, many), (OLD, per64)]
    out = {}
    for c in ("cold", "warm"):
        out[c] = alternate(named, reps if c == "cold" else max(reps, 5), c == "cold")
        out[c]["new_against_runs_of_64"] = ratio(out[c], OLD, NEW)
    out["shape"] = {"n": n, "pairs": npairs, "largest_pair_share": round(float(np.bincount(idx).max()) / n, 4)}
    return out


def case_price(gpu, reps, n):
    pairs = many_pairs(gpu, 64, b"price")
    idx = np.random.RandomState(9).randint(0, 64, size=n).astype(np.uint32)
    xs, ks = scalars(b"price-x", n), scalars(b"price-k", n)

    def call(g, knob):
        if knob:
            os.environ[KNOB] = "0"
        try:
            return g.prove_pairs_many(pairs, idx, xs, ks)
        finally:
            os.environ.pop(KNOB, None)

    a, b = call(gpu, False), call(gpu, True)
    for q in Q:
        assert np.array_equal(a[q], b[q]), q
    named = [("forwarded_128_entry_tables", lambda g: call(g, False)), ("small_tables", lambda g: call(g, True))]
    out = {}
    for c in ("cold", "warm"):
        out[c] = alternate(named, reps, c == "cold")
        out[c]["small_over_forwarded"] = round(out[c]["small_tables"]["median_ms"] /
                                               out[c]["forwarded_128_entry_tables"]["median_ms"], 3)
        out[c]["forwarded_against_small"] = ratio(out[c], "small_tables", "forwarded_128_entry_tables")
    out["shape"] = {"n": n, "pairs": 64}
    return out


def case_stages(gpu, reps):
    pairs = many_pairs(gpu, 4096, b"stages")
    out = {}
    with cp.Gpu(0) as g:
        for n, npairs in ((130, 65), (1000, 1000), (4096, 4096)):
            idx = (np.arange(n) % npairs).astype(np.uint32)
            xs, ks = scalars(b"st-x-%d" % n, n), scalars(b"st-k-%d" % n, n)
            g.prove_pairs_many(pairs[:npairs], idx, xs, ks)
            g.set_timing(True)
            g.stage_times()
            desc, build, prove, host = [], [], [], []
            for _ in range(max(reps, 10)):
                host.append(timed(lambda: g.prove_pairs_many(pairs[:npairs], idx, xs, ks))[0])
                t = g.stage_times()
                assert t["generators_varbase"][1] == npairs and t["prove"][1] == 2
                desc.append(t.get("rlc_prepare", (0.0, 0))[0])
                build.append(t["generators_varbase"][0])
                prove.append(t["prove"][0])
            g.set_timing(False)
            out["%d_entries_%d_pairs" % (n, npairs)] = {
                "stage2_descriptors": stats(desc), "stage13_table_build": stats(build),
                "stage6_points_challenges_responses": stats(prove), "host_call_with_timing_on": stats(host)}
    out["note"] = "stages: GPU time between events on the call's stream; stage 6 sums the point kernel's span and the " \
                  "span of challenges + responses"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="a,t,p,b")
    ap.add_argument("--big", default="17,20")
    a = ap.parse_args()
    cases = a.cases.split(",")
    result = {"device": "MI355X (gfx950)", "clock": "host perf_counter around synchronous calls", "reps": a.reps}
    if a.out and os.path.exists(a.out):      # cases run one at a time add to the same file
        with open(a.out) as f:
            result.update(json.load(f))

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    with cp.Gpu(0) as gpu:
        with cp.Gpu(0) as warm:  # code objects, allocator: before any cold time
            w = many_pairs(warm, 70, b"warm")
            i70 = (np.arange(2100) % 70).astype(np.uint32)
            x, k = scalars(b"warm-x", 2100), scalars(b"warm-k", 2100)
            warm.prove_pairs_many(w, i70, x, k)
            warm.prove_pairs(w[:64], i70 % 64, x, k)
        if "a" in cases:
            result["a_1000_entries_1000_pairs"] = case_shape(gpu, a.reps, 1000, 1000, tag=b"small")
            flush()
        if "t" in cases:
            result["t_stages"] = case_stages(gpu, a.reps)
            flush()
        if "p" in cases:
            for n in (16384, 1 << 20):
                result["p_%d_entries_64_pairs" % n] = case_price(gpu, a.reps, n)
                flush()
        if "b" in cases:
            for log2n in [int(x) for x in a.big.split(",") if x]:
                n = 1 << log2n
                result["b_2pow%d_entries_4096_pairs_uniform" % log2n] = case_shape(gpu, a.reps, n, 4096, tag=b"big")
                flush()
                if log2n == 20:
                    result["b_2pow20_entries_4096_pairs_90pct_in_one_pair"] = case_shape(gpu, a.reps, n, 4096, skew=True,
                                                                                        tag=b"skew")
                    flush()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
