#!/usr/bin/env python3
"""A/B of the one-pass light-set build (load_pairs) against one build per pair, in one process.

    tools/load_pairs_ab.py [--out profiles/load_pairs_ab.json] [--reps K]

The knob CPZ_PAIRS_BUILD_BATCH is read by the library at every call: "0" restores the one-by-one
builds (side `off`, the parent's behaviour), unset is the one pass (side `on`).  Every repetition
runs each case on both sides, off then on, each on a fresh context:

  load_k            Gpu.load_pairs of k = 1, 8, 64 custom pairs
  cold_verify       Gpu.verify_each_pairs, 1000 entries over 64 pairs (entry i under pair i % 64)
  cold_prove        Gpu.prove_pairs, 2048 proofs over 64 pairs
  rotation          192 pairs in three 64-pair verify_each_pairs calls of 1000 entries on ONE
                    context, twice round: the first round allocates the 64 sets, the second
                    rebuilds them in place (every call evicts the previous call's 64 sets), so
                    the two rounds differ by the allocations

For each: the host clock around the call (which returns synchronised) and the stage-13 span (HIP
events on the stream around the build: copies in, kernels, copies back -- the allocations come
before the span on side `on` and inside it on side `off`), with the sets it counted.  Medians and
spreads (min, max) in milliseconds as JSON; `on_ahead` is true when side on's slowest run beats
side off's fastest."""
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
KNOB = "CPZ_PAIRS_BUILD_BATCH"
VARBASE = "generators_varbase"


def pairs_of(k, tag):
    out = []
    for i in range(k):
        a = O.scalar_wide(hashlib.sha512(tag + b"-g-%d" % i).digest())
        b = O.scalar_wide(hashlib.sha512(tag + b"-h-%d" % i).digest())
        out.append(cp.Parameters(O.ristretto_encode(O.pt_mul(O.BASEPOINT, a)),
                                 O.ristretto_encode(O.pt_mul(O.BASEPOINT, b))))
    return out


def set_side(side):
    if side == "off":
        os.environ[KNOB] = "0"
    else:
        os.environ.pop(KNOB, None)


def timed(gpu, fn):
    """(host ms, stage-13 ms, sets counted) of one call on a context with the stage timers on."""
    gpu.stage_times()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    ms, cnt = gpu.stage_times().get(VARBASE, (0.0, 0))
    return host, ms, cnt


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "runs": len(xs)}


def summarise(runs):
    """runs: {side: [(host, stage13, count)]} -> the case's JSON."""
    out = {}
    for side, v in runs.items():
        out[side] = {"host": stats([r[0] for r in v]), "stage13": stats([r[1] for r in v]),
                     "host_minus_stage13_median_ms": round(statistics.median([r[0] - r[1] for r in v]), 4),
                     "sets_built": sorted(set(r[2] for r in v))}
    for key in ("host", "stage13"):
        off, on = out["off"][key], out["on"][key]
        out[key + "_ratio_off_over_on"] = round(off["median_ms"] / on["median_ms"], 3)
        out[key + "_on_ahead"] = on["max_ms"] < off["min_ms"]
        out[key + "_on_behind"] = on["min_ms"] > off["max_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least five repetitions")
    pairs = pairs_of(192, b"ab-load")
    rng = np.random.default_rng(11)
    nv, npr = 1000, 2048
    idx_v = (np.arange(nv) % 64).astype(np.uint32)
    idx_p = (np.arange(npr) % 64).astype(np.uint32)
    xs = np.frombuffer(rng.bytes(32 * npr), np.uint8).reshape(npr, 32)   # any 32 bytes: taken mod l
    ks = np.frombuffer(rng.bytes(32 * npr), np.uint8).reshape(npr, 32)
    set_side("on")
    with cp.Gpu(0) as warm:  # code objects, allocator, and the entries to verify: before any timed run
        thirds = [pairs[64 * j:64 * j + 64] for j in range(3)]
        rows = [warm.prove_pairs(t, idx_v, xs[:nv], ks[:nv]) for t in thirds]
        for t, r in zip(thirds, rows):
            assert not warm.verify_each_pairs(t, idx_v, *[r[q] for q in Q]).any()
        ref_prove = warm.prove_pairs(thirds[0], idx_p, xs, ks)
    set_side("off")
    with cp.Gpu(0) as warm:
        warm.load_pairs(pairs[:2])
    cases = ["load_1", "load_8", "load_64", "cold_verify_1000x64", "cold_prove_2048x64", "rotation_round_1",
             "rotation_round_2"]
    runs = {c: {"off": [], "on": []} for c in cases}
    for _ in range(a.reps):
        for side in ("off", "on"):
            set_side(side)
            for k in (1, 8, 64):
                with cp.Gpu(0) as g:
                    g.set_timing(True)
                    r = timed(g, lambda: g.load_pairs(pairs[:k]))
                    assert r[2] == k, r
                    runs["load_%d" % k][side].append(r)
            with cp.Gpu(0) as g:
                g.set_timing(True)
                st = []
                r = timed(g, lambda: st.append(g.verify_each_pairs(thirds[0], idx_v, *[rows[0][q] for q in Q])))
                assert r[2] == 64 and not st[0].any(), r
                runs["cold_verify_1000x64"][side].append(r)
            with cp.Gpu(0) as g:
                g.set_timing(True)
                got = []
                r = timed(g, lambda: got.append(g.prove_pairs(thirds[0], idx_p, xs, ks)))
                assert r[2] == 64 and all(np.array_equal(got[0][q], ref_prove[q]) for q in Q), r
                runs["cold_prove_2048x64"][side].append(r)
            with cp.Gpu(0) as g:
                g.set_timing(True)
                for rnd in (1, 2):
                    tot = [0.0, 0.0, 0]
                    for t, rw in zip(thirds, rows):
                        st = []
                        r = timed(g, lambda: st.append(g.verify_each_pairs(t, idx_v, *[rw[q] for q in Q])))
                        assert not st[0].any()
                        tot = [tot[0] + r[0], tot[1] + r[1], tot[2] + r[2]]
                    assert tot[2] == 192, tot
                    runs["rotation_round_%d" % rnd][side].append(tuple(tot))
    set_side("on")
    result = {"device": "MI355X (gfx950)",
              "clock": "host perf_counter around calls that return synchronised; stage13: HIP events around the build",
              "reps": a.reps, "off": KNOB + "=0: one build per pair (ensure_generators)",
              "on": "default: one pass for all of a call's missing pairs (load_pairs)",
              "rotation": "three verify_each_pairs calls (1000 entries, 64 pairs each) over 192 pairs, summed per round",
              "cases": {c: summarise(runs[c]) for c in cases}}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
