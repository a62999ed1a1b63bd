#!/usr/bin/env python3
"""A/B of the mixed-pair batch check's search for invalid entries: this tree's library against
another build of it (the parent commit's, built into a path of its own), one configuration per
fresh child process.

    tools/batch_pairs_part_ab.py --parent-lib PATH [--out FILE] [--reps K] [--rounds R]
                                 [--sizes 13,14,15,17,20] [--shares one,0.001,0.01,0.1]

64 custom pairs (entry i under pair i % 64), n = 2^13 .. 2^20 entries, of which one entry, 0.1 %,
1 % or 10 % have s + 1 (evenly spread).  A child loads one library (CPZ_LIB), proves the entries,
runs Gpu.verify_batch_pairs twice to warm up -- tables, buffers and code objects are then resident
-- and times `reps` further calls with the host clock around the synchronous call, checking the
statuses every time.  Every cell runs `rounds` children per library, the two libraries alternating,
so the parent's own run-to-run spread (max - min over all of its timings of a cell) is known.

Writes, per cell, both sides' medians and spreads, the ratio new / parent of the medians, the
verdict against the parent's spread, and what the fallback did (cpz_ctx_fallback_stats)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "chaum-pedersen-zkp_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

Q = ("y1", "y2", "r1", "r2", "s")
SEED = hashlib.sha256(b"batch-pairs-part-ab").digest()
PAIRS = 64


def forged_of(n, share):
    if share == "one":
        return [n // 3]
    k = max(1, round(n * float(share)))
    return sorted({(i * n) // k + (7 * i) % max(1, n // k) for i in range(k)})


def child(a):
    import numpy as np

    import chaum_pedersen as cp
    import pyoracle as O

    n = 1 << a.log2n
    pairs = []
    for i in range(PAIRS):
        x = O.scalar_wide(hashlib.sha512(b"part-ab-g-%d" % i).digest())
        y = O.scalar_wide(hashlib.sha512(b"part-ab-h-%d" % i).digest())
        pairs.append(cp.Parameters(O.ristretto_encode(O.pt_mul(O.BASEPOINT, x)),
                                   O.ristretto_encode(O.pt_mul(O.BASEPOINT, y))))
    groups = (np.arange(n) % PAIRS).astype(np.uint32)
    rows = {q: np.zeros((n, 32), np.uint8) for q in Q}
    forged = forged_of(n, a.share)
    with cp.Gpu(0) as gpu:
        per = n // PAIRS
        for p in range(PAIRS):
            out = gpu.prove_synthetic(per, SEED, SEED[::-1], first_index=p * per, params=pairs[p])
            for q in Q:
                rows[q][p::PAIRS] = out[q]
        for i in forged:
            v = int.from_bytes(rows["s"][i].tobytes(), "little") + 1
            rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
        cols = [rows[q] for q in Q]
        want = np.zeros(n, np.uint8)
        want[forged] = 1
        times = []
        for k in range(2 + a.reps):
            t0 = time.perf_counter()
            partial, ok, st = gpu.verify_batch_pairs(pairs, groups, *cols, SEED)
            dt = (time.perf_counter() - t0) * 1e3
            assert not ok and np.array_equal(st, want), "wrong statuses"
            if k >= 2:
                times.append(dt)
        fb = gpu.fallback_stats()
    print("RESULT " + json.dumps({"ms": times, "forged": len(forged), "fallback": fb}))


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3),
            "spread_ms": round(max(xs) - min(xs), 3), "runs": len(xs)}


def run_child(lib, log2n, share, reps):
    env = dict(os.environ)
    if lib:
        env["CPZ_LIB"] = lib
    else:
        env.pop("CPZ_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--log2n", str(log2n), "--share", share,
                        "--reps", str(reps)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError("child failed (%s, 2^%d, %s): rc %d\n%s" % (lib or "new", log2n, share, r.returncode,
                                                                    r.stdout[-2000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--log2n", type=int, default=13)
    ap.add_argument("--share", default="one")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sizes", default="13,14,15,17,20")
    ap.add_argument("--shares", default="one,0.001,0.01,0.1")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the parent commit's libcpz.so, built into a path of its own")
    result = {"device": "MI355X (gfx950)", "clock": "host perf_counter around the synchronous call, warm",
              "pairs": PAIRS, "reps": a.reps, "rounds": a.rounds, "cells": []}
    for log2n in [int(x) for x in a.sizes.split(",")]:
        for share in a.shares.split(","):
            ms = {"parent": [], "new": []}
            fb = {}
            nforged = 0
            for _ in range(a.rounds):
                for side, lib in (("parent", os.path.abspath(a.parent_lib)), ("new", "")):
                    r = run_child(lib, log2n, share, a.reps)
                    ms[side] += r["ms"]
                    fb[side] = r["fallback"]
                    nforged = r["forged"]
            par, new = stats(ms["parent"]), stats(ms["new"])
            diff = new["median_ms"] - par["median_ms"]
            cell = {"n": 1 << log2n, "share": share, "forged": nforged, "parent": par, "new": new,
                    "ratio_new_over_parent": round(new["median_ms"] / par["median_ms"], 4),
                    "verdict": "faster" if -diff > par["spread_ms"] else ("slower" if diff > par["spread_ms"]
                                                                         else "within the parent's spread"),
                    "fallback_parent": fb["parent"], "fallback_new": fb["new"]}
            result["cells"].append(cell)
            print("2^%d %-5s parent %.2f ms (spread %.2f)  new %.2f ms  ratio %.3f  %s  [%s]" % (
                log2n, share, par["median_ms"], par["spread_ms"], new["median_ms"], cell["ratio_new_over_parent"],
                cell["verdict"], fb["new"]["path"]), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
