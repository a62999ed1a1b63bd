#!/usr/bin/env python3
"""Hash-to-group on the device against the Python oracle's map, in one process.

    tools/hash_to_group_ab.py [--out FILE] [--reps K] [--shapes 64,1000,4096] [--big 16]

  derive_pairs   64, 1000 and 4096 labels ("tenant-<i>"): one cpz_derive_pairs call, which is 2 points
                 per label (one hash launch, one map launch, the rows checked and copied back).
  hash_to_group  2^16 short messages ("message-<i>") in one cpz_hash_to_group call.

The other side is the Python oracle (oracle/pyoracle.py: SHA-512 by hashlib, then
ristretto_from_uniform_bytes and ristretto_encode), the only other implementation of the map in
the project: it is timed in the same run on a sample of 64 points, and its time for a shape is
that sample's time per point times the shape's point count -- scaled, not run, and marked so in
the file.  The device side is warmed up first, its rows are compared with the oracle's on the
sample, and the times are host clocks around the synchronous calls.  Writes medians and spreads
(min, max) in milliseconds as JSON; a shape that was not run is absent from the file."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "chaum-pedersen-zkp_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import chaum_pedersen as cp  # noqa: E402
import pyoracle as O  # noqa: E402
from chaum_pedersen import _native  # noqa: E402

SAMPLE = 64


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "runs": len(xs)}


def oracle_point(msg):
    return O.ristretto_encode(O.ristretto_from_uniform_bytes(hashlib.sha512(msg).digest()))


def oracle_sample(reps):
    """Milliseconds per point of the oracle over SAMPLE short messages, `reps` times."""
    msgs = [_native.PAIR_DST_H + b"tenant-%d" % i for i in range(SAMPLE)]
    runs = [timed(lambda: [oracle_point(m) for m in msgs])[0] / SAMPLE for _ in range(reps)]
    return stats(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="64,1000,4096")
    ap.add_argument("--big", default="16")
    a = ap.parse_args()
    result = {"device": "MI355X (gfx950)", "clock": "host perf_counter around synchronous calls", "reps": a.reps,
              "other_side": "Python oracle (hashlib SHA-512, pyoracle.ristretto_from_uniform_bytes and "
                            "ristretto_encode) timed in this run on %d points; its time for a shape is SCALED "
                            "from that sample (time per point x points), not run" % SAMPLE}
    per_point = oracle_sample(max(3, a.reps // 3))
    result["oracle_ms_per_point"] = per_point
    with cp.Gpu(0) as gpu:
        gpu.derive_pairs([b"warm-%d" % i for i in range(130)])      # code objects, buffers
        for n in [int(x) for x in a.shapes.split(",") if x]:
            labels = [b"tenant-%d" % i for i in range(n)]
            rows = gpu.derive_pairs(labels)
            for i in range(0, n, max(1, n // 16)):                  # a sample of the rows against the oracle
                want = oracle_point(_native.PAIR_DST_G + labels[i]) + oracle_point(_native.PAIR_DST_H + labels[i])
                assert rows[i].tobytes() == want, i
            dev = stats([timed(lambda: gpu.derive_pairs(labels))[0] for _ in range(a.reps)])
            scaled = round(per_point["median_ms"] * 2 * n, 2)
            result["derive_pairs_%d_labels" % n] = {
                "points": 2 * n, "device": dev, "oracle_scaled_ms": scaled,
                "oracle_scaled_over_device": round(scaled / dev["median_ms"], 1)}
        for log2n in [int(x) for x in a.big.split(",") if x]:
            n = 1 << log2n
            msgs = [b"message-%d" % i for i in range(n)]
            pts = gpu.hash_to_group(msgs)
            for i in range(0, n, n // 16):
                assert pts[i].tobytes() == oracle_point(msgs[i]), i
            dev = stats([timed(lambda: gpu.hash_to_group(msgs))[0] for _ in range(a.reps)])
            scaled = round(per_point["median_ms"] * n, 2)
            result["hash_to_group_2pow%d_messages" % log2n] = {
                "points": n, "device": dev, "oracle_scaled_ms": scaled,
                "oracle_scaled_over_device": round(scaled / dev["median_ms"], 1),
                "note": "the device time includes the wrapper's joining of the messages into one blob"}
    text = json.dumps(result, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
