#!/usr/bin/env python3
"""A/B of cpz_verify_each_gh against what a caller with a (g, h) pair per entry had before it, in
one process.

    tools/each_gh_ab.py [--out FILE] [--reps K] [--shapes 1000,4096,131072,1048576] [--few 131072]

Every shape has a distinct pair per entry (gpu.derive_pairs, proofs from cpz_prove_pairs_many in
slices of 4096 pairs, no contexts):
  old  cpz_verify_each_pairs_many over consecutive slices of 4096 entries, pairs = the slice's rows,
       indices 0..: n / 4096 synchronous calls;
  new  one cpz_verify_each_gh call on the same rows.
--few: the same number of entries over only 16 distinct pairs, where the old route is ONE
cpz_verify_each_pairs_many call over the 16 pairs (resident 128-entry tables, amortised) and should
win; reported so that the header can say when not to use the new call.

Both sides are the C entry points themselves (no wrapper work is timed).  The two sides' statuses
are compared before timing (three entries carry s + 1), the sides alternate, each shape is warmed up
first, and the times are host clocks around the synchronous calls: medians with (min - max), in
milliseconds.  At the largest shape the GPU time of the verify launches (stage 5) of the new call is
recorded too, with the proofs per second it gives."""
import argparse
import ctypes
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
from chaum_pedersen import _native  # noqa: E402

Q = ("y1", "y2", "r1", "r2", "s")
SLICE = _native.EACH_PAIRS_MANY_MAX
FEW = 16


def scalars(seed, n):
    a = np.random.RandomState(seed).randint(0, 256, size=(n, 32)).astype(np.uint8)
    a[:, 31] &= 0x0f
    return a


def derive(gpu, n, tag):
    return np.concatenate([gpu.derive_pairs([tag + b"/%d" % i for i in range(c, min(c + SLICE, n))])
                           for c in range(0, n, SLICE)])


def prove(gpu, gh, n):
    """Entry i under row i % len(gh) of gh: cpz_prove_pairs_many itself, 4096 entries a call."""
    xs, ks = scalars(1, n), scalars(2, n)
    rows = {q: np.zeros((n, 32), np.uint8) for q in Q}
    for c in range(0, n, SLICE):
        m = min(SLICE, n - c)
        if len(gh) >= n:
            pairs, idx = np.ascontiguousarray(gh[c:c + m]), np.arange(m, dtype=np.uint32)
        else:
            pairs, idx = np.ascontiguousarray(gh), ((c + np.arange(m)) % len(gh)).astype(np.uint32)
        out = {q: np.empty((m, 32), np.uint8) for q in Q}
        x, k = np.ascontiguousarray(xs[c:c + m]), np.ascontiguousarray(ks[c:c + m])
        _native.check(gpu._lib.cpz_prove_pairs_many(gpu._h, len(pairs), cp._ptr(pairs), m, cp._ptr(idx), cp._ptr(x),
                                                    cp._ptr(k), None, None, None, *[cp._ptr(out[q]) for q in Q]))
        for q in Q:
            rows[q][c:c + m] = out[q]
    return rows


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "runs": len(xs)}


def sides(g, gh, rows, n, few):
    """(old, new): each returns the n statuses."""
    cols = [rows[q] for q in Q]
    if few:
        full = np.ascontiguousarray(gh[np.arange(n) % len(gh)])
        idx_all = (np.arange(n) % len(gh)).astype(np.uint32)
    else:
        full = gh
    gg, hh = np.ascontiguousarray(full[:, :32]), np.ascontiguousarray(full[:, 32:])
    idx = np.arange(SLICE, dtype=np.uint32)
    st_old, st_new = np.empty(n, np.uint8), np.empty(n, np.uint8)
    lib, h = g._lib, g._h

    def old():
        if few:
            _native.check(lib.cpz_verify_each_pairs_many(h, 0, len(gh), cp._ptr(gh), n, cp._ptr(idx_all),
                                                         *[cp._ptr(c) for c in cols], None, None, None, cp._ptr(st_old)))
            return st_old
        for c in range(0, n, SLICE):
            m = min(SLICE, n - c)
            _native.check(lib.cpz_verify_each_pairs_many(
                h, 0, m, gh.ctypes.data + 64 * c, m, cp._ptr(idx), *[col.ctypes.data + 32 * c for col in cols], None, None,
                None, st_old.ctypes.data + c))
        return st_old

    def new():
        _native.check(lib.cpz_verify_each_gh(h, 0, n, cp._ptr(gg), cp._ptr(hh), *[cp._ptr(c) for c in cols], None, None,
                                             None, cp._ptr(st_new)))
        return st_new

    return old, new


def case(gpu, n, reps, few=False, stage5=False):
    gh = derive(gpu, FEW if few else n, b"each-gh-ab-%d" % n)
    rows = prove(gpu, gh, n)
    forged = sorted({0, n // 2, n - 1})
    for i in forged:
        v = int.from_bytes(rows["s"][i].tobytes(), "little") + 1
        rows["s"][i] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)
    exp = np.zeros(n, np.uint8)
    exp[forged] = 1
    names = ("old_pairs_many_one_call" if few else "old_pairs_many_slices_of_4096", "new_verify_each_gh")
    res = {nm: [] for nm in names}
    out = {"shape": {"n": n, "distinct_pairs": FEW if few else n, "old_calls": 1 if few else -(-n // SLICE)}}
    with cp.Gpu(0) as g:
        old, new = sides(g, gh, rows, n, few)
        a, b = old().copy(), new().copy()              # warm-up, and the comparison before any timing
        assert np.array_equal(a, b) and np.array_equal(a, exp), "the two sides disagree"
        out["statuses_compared"] = True
        for _ in range(reps):
            for nm, fn in zip(names, (old, new)):
                res[nm].append(timed(fn)[0])
        if stage5:
            g.set_timing(True)
            g.stage_times()
            span, launches = [], 0
            for _ in range(reps):
                new()
                t = g.stage_times()
                span.append(t["verify_span"][0])
                launches = t["verify_each"][1]
            g.set_timing(False)
            out["new_stage5_verify_launches_gpu"] = stats(span)
            out["new_stage5_verify_launches_gpu"]["launches"] = launches
            out["new_stage5_proofs_per_s"] = round(n / (statistics.median(span) * 1e-3))
    for nm in names:
        out[nm] = stats(res[nm])
    o, w = out[names[0]], out[names[1]]
    out["old_over_new_by_medians"] = round(o["median_ms"] / w["median_ms"], 3)
    out["new_faster_ranges_apart"] = w["max_ms"] < o["min_ms"]
    out["old_faster_ranges_apart"] = o["max_ms"] < w["min_ms"]
    out["new_proofs_per_s_host_clock"] = round(n / (w["median_ms"] * 1e-3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="1000,4096,131072,1048576")
    ap.add_argument("--few", default="131072")
    a = ap.parse_args()
    shapes = [int(x) for x in a.shapes.split(",") if x]
    result = {"device": "MI355X (gfx950)", "clock": "host perf_counter around synchronous C calls; stage 5: GPU events",
              "reps": a.reps, "contexts": "none", "method": "one process, the two sides alternate, warmed up first"}

    def flush():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    with cp.Gpu(0) as gpu:
        for n in shapes:
            result["distinct_pairs_n_%d" % n] = case(gpu, n, a.reps, stage5=(n == max(shapes)))
            flush()
        for n in [int(x) for x in a.few.split(",") if x]:
            result["16_pairs_n_%d" % n] = case(gpu, n, a.reps, few=True)
            flush()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
