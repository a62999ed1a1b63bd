#!/usr/bin/env python3
"""A/B of cpz_verify_batch_pairs_many against what a caller with more than 64 pairs had before it,
in one process.

    tools/batch_pairs_many_ab.py [--out FILE] [--reps K] [--cases a,b,c,d,s] [--big LOG2N]

  (a) 1000 entries over 1000 pairs, all valid, cold (the first call on a fresh context) and warm:
      one verify_batch_pairs_many call against 16 verify_each_pairs calls of 64 pairs
      (BatchVerifier's route) and against 16 verify_batch_pairs calls.
  (b) 2^20 entries over 4096 pairs, all valid, uniform and with 90 % of the entries in one pair:
      one call against 64 verify_batch_pairs calls of 64 pairs on rows gathered by pair (the
      gathering is not timed).
  (c) the batch of (a) and the uniform batch of (b) with 3 forged entries, under both leaf policies
      of the bisection (CPZ_PAIRS_MANY_DEEP, read at every call) and against the baselines.
  (d) 64 pairs at 2^20 entries: stage 3 (the sort phase's accounting holds the extras) through
      k_rlc_extra_pairs (verify_batch_pairs, 64 pairs) and through the bucketed sums (65 pairs, one
      without entries, bucketing included).  Reported only.
  (s) stage 2 at 4096 pairs: stage 2 (the descriptor build and the prepare) of a 4096-entry call
      over 4096 listed pairs and of the same entries over 65, whose difference is what the
      device build of 4031 more rows costs, beside the host loop of the 64-pair call's recording
      sponge extrapolated to 4096 pairs (the CPU-test build of the same function, timed on this
      host).

The sides alternate, each shape is warmed up first, and the times are host clocks around the
synchronous calls.  Writes medians and spreads (min, max) in milliseconds as JSON."""
import argparse
import ctypes
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
SEED = hashlib.sha256(b"batch-pairs-many-ab").digest()
K = 64


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


def forge(rows, entries):
    for i in entries:
        v = int.from_bytes(rows["s"][i].tobytes(), "little") + 1
        rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "runs": len(xs)}


def gathered(pairs, idx, rows):
    """Per chunk of 64 pairs: (pairs, local indices, columns, global positions) of its entries."""
    idx = np.asarray(idx, np.int64)
    out = []
    for c in range(0, len(pairs), K):
        sel = np.nonzero((idx >= c) & (idx < c + K))[0]
        if len(sel):
            out.append((pairs[c:c + K], (idx[sel] - c).astype(np.uint32),
                        [np.ascontiguousarray(rows[q][sel]) for q in Q], sel))
    return out


def sides(pairs, idx, rows, want):
    """The three routes over one batch; each checks the statuses it returns."""
    idx = np.ascontiguousarray(idx, np.uint32)
    cols = [rows[q] for q in Q]
    chunks = gathered(pairs, idx, rows)
    bad = bool(want.any())

    def many(g):
        partial, ok, st = g.verify_batch_pairs_many(pairs, idx, *cols, SEED)
        assert ok == (not bad) and np.array_equal(st, want)

    def each(g):
        for pr, li, cl, sel in chunks:
            assert np.array_equal(g.verify_each_pairs(pr, li, *cl), want[sel])

    def batch(g):
        for pr, li, cl, sel in chunks:
            partial, ok, st = g.verify_batch_pairs(pr, li, *cl, SEED)
            assert np.array_equal(st, want[sel])

    return many, each, batch


def case_small(gpu, reps, forged):
    n = 1000
    pairs = many_pairs(gpu, n, b"small")
    idx = np.arange(n, dtype=np.uint32)
    rows = prove_many(gpu, pairs, idx, b"small-rows")
    forge(rows, forged)
    want = np.zeros(n, np.uint8)
    want[list(forged)] = 1
    many, each, batch = sides(pairs, idx, rows, want)
    named = [("verify_batch_pairs_many", many), ("verify_each_pairs_x16", each), ("verify_batch_pairs_x16", batch)]
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
    if forged:
        out["warm"].update(policies(many, max(reps, 10)))
    out["shape"] = {"n": n, "pairs": n, "forged": list(forged)}
    return out


def policies(many, reps):
    """The failing call under both leaf policies, alternating."""
    res = {"many_deep": [], "many_stop_at_2048": []}
    with cp.Gpu(0) as g:
        many(g)
        for _ in range(reps):
            for nm, v in (("many_deep", "1"), ("many_stop_at_2048", "0")):
                os.environ["CPZ_PAIRS_MANY_DEEP"] = v
                res[nm].append(timed(lambda: many(g))[0])
        os.environ.pop("CPZ_PAIRS_MANY_DEEP", None)
    return {nm: stats(v) for nm, v in res.items()}


def big_batch(gpu, log2n, npairs, skew, tag):
    n = 1 << log2n
    rs = np.random.RandomState(5)
    idx = rs.randint(0, npairs, size=n).astype(np.uint32)
    if skew:
        idx[rs.rand(n) < 0.9] = 0
    pairs = many_pairs(gpu, npairs, tag)
    return pairs, idx, prove_many(gpu, pairs, idx, tag + b"-rows")


def case_big(gpu, reps, log2n):
    out = {}
    kept = None
    for name, skew in (("uniform", False), ("skewed_90pct_in_one_pair", True)):
        pairs, idx, rows = big_batch(gpu, log2n, 4096, skew, b"big")
        want = np.zeros(len(idx), np.uint8)
        many, _, batch = sides(pairs, idx, rows, want)
        res = {"verify_batch_pairs_many": [], "verify_batch_pairs_x64": []}
        with cp.Gpu(0) as g:
            many(g)
            batch(g)
            for _ in range(reps):
                res["verify_batch_pairs_many"].append(timed(lambda: many(g))[0])
                res["verify_batch_pairs_x64"].append(timed(lambda: batch(g))[0])
        out[name] = {nm: stats(v) for nm, v in res.items()}
        out[name]["largest_pair_share"] = round(float(np.bincount(idx).max()) / len(idx), 4)
        if not skew:
            kept = (pairs, idx, rows)
    out["shape"] = {"n": 1 << log2n, "pairs": 4096}
    return out, kept


def case_big_forged(kept, reps):
    pairs, idx, rows = kept
    n = len(idx)
    forged = [3, n // 2 + 77, n - 1]
    rows = {q: rows[q].copy() for q in Q}
    forge(rows, forged)
    want = np.zeros(n, np.uint8)
    want[forged] = 1
    many, _, batch = sides(pairs, idx, rows, want)
    res = {"verify_batch_pairs_x64": []}
    with cp.Gpu(0) as g:
        batch(g)
        for _ in range(reps):
            res["verify_batch_pairs_x64"].append(timed(lambda: batch(g))[0])
    out = {nm: stats(v) for nm, v in res.items()}
    out.update(policies(many, reps))
    out["shape"] = {"n": n, "pairs": 4096, "forged": forged}
    return out


def stage(g, name, fn, reps):
    g.set_timing(True)
    fn(g)
    g.stage_times()
    xs = []
    for _ in range(reps):
        fn(g)
        xs.append(g.stage_times().get(name, (0.0, 0))[0])
    g.set_timing(False)
    return stats(xs)


def case_extras(gpu, reps, log2n):
    n = 1 << log2n
    pairs = many_pairs(gpu, 65, b"extras")
    idx = np.random.RandomState(9).randint(0, 64, size=n).astype(np.uint32)
    rows = prove_many(gpu, pairs, idx, b"extras-rows")
    cols = [rows[q] for q in Q]

    def old(g):
        assert g.verify_batch_pairs(pairs[:64], idx, *cols, SEED, statuses=False)[1]

    def new(g):
        assert g.verify_batch_pairs_many(pairs, idx, *cols, SEED, statuses=False)[1]

    with cp.Gpu(0) as g:
        return {"stage3_64_pairs_k_rlc_extra_pairs": stage(g, "rlc_msm", old, reps),
                "stage3_65_pairs_bucketed_sums": stage(g, "rlc_msm", new, reps),
                "shape": {"n": n, "note": "GPU time of stage 3 (extras, sort, MSM); the second side includes the bucketing"}}


def case_stage2(gpu, reps):
    import build_native
    n = 4096
    pairs = many_pairs(gpu, 4096, b"stage2")
    rows = prove_many(gpu, pairs, np.arange(n) % 65, b"stage2-rows")
    cols = [rows[q] for q in Q]
    idx65 = (np.arange(n) % 65).astype(np.uint32)
    # the same entries under 4096 listed pairs: rows 0 .. 64 carry them, the rest have no entry

    def few(g):
        assert g.verify_batch_pairs_many(pairs[:65], idx65, *cols, SEED, statuses=False)[1]

    def all_(g):
        assert g.verify_batch_pairs_many(pairs, idx65, *cols, SEED, statuses=False)[1]

    with cp.Gpu(0) as g:
        s65 = stage(g, "rlc_prepare", few, reps)
        s4096 = stage(g, "rlc_prepare", all_, reps)
        w65 = stats([timed(lambda: few(g))[0] for _ in range(reps)])
        w4096 = stats([timed(lambda: all_(g))[0] for _ in range(reps)])
    lib = ctypes.CDLL(build_native.build_hosttest())
    lib.pairsum_host_masks_ms.restype = ctypes.c_double
    lib.pairsum_host_masks_ms.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    gh = np.frombuffer(b"".join(p.g + p.h for p in pairs[:64]), np.uint32).copy()
    acc = np.zeros(1, np.uint32)
    host = [lib.pairsum_host_masks_ms(64, gh.ctypes.data, acc.ctypes.data) for _ in range(max(reps, 10))]
    h = stats(host)
    return {"stage2_gpu_65_pairs": s65, "stage2_gpu_4096_pairs": s4096,
            "stage2_4096_minus_65_pairs_ms": round(s4096["median_ms"] - s65["median_ms"], 4),
            "call_wall_65_pairs": w65, "call_wall_4096_pairs": w4096,
            "host_recording_sponge_64_pairs": h,
            "host_loop_extrapolated_to_4096_pairs_ms": round(64 * h["median_ms"], 3),
            "shape": {"n": n, "note": "host figure: the CPU-test build (-O2, bounds checks) of challenge_masks_ctx32"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="a,b,c,d,s")
    ap.add_argument("--big", type=int, default=20)
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
            r = prove_many(warm, w, np.arange(140) % 70, b"warm-rows")
            warm.verify_batch_pairs_many(w, (np.arange(140) % 70).astype(np.uint32), *[r[q] for q in Q], SEED)
            warm.verify_batch_pairs(w[:64], (np.arange(140) % 64).astype(np.uint32), *[r[q] for q in Q], SEED)
            warm.verify_each_pairs(w[:64], (np.arange(140) % 64).astype(np.uint32), *[r[q] for q in Q])
        if "a" in cases:
            result["a_1000_entries_1000_pairs_valid"] = case_small(gpu, a.reps, ())
            flush()
        if "c" in cases:
            result["c_1000_entries_1000_pairs_3_forged"] = case_small(gpu, a.reps, (3, 500, 999))
            flush()
        if "b" in cases or "c" in cases:
            big, kept = case_big(gpu, a.reps, a.big)
            result["b_2pow%d_entries_4096_pairs_valid" % a.big] = big
            flush()
            if "c" in cases:
                result["c_2pow%d_entries_4096_pairs_3_forged" % a.big] = case_big_forged(kept, a.reps)
                flush()
        if "d" in cases:
            result["d_2pow%d_entries_64_pairs_extras" % a.big] = case_extras(gpu, a.reps, a.big)
            flush()
        if "s" in cases:
            result["stage2_4096_pairs"] = case_stage2(gpu, a.reps)
            flush()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
