#!/usr/bin/env python3
"""The route a failing batch takes through the batch check, per scenario of
tests/route_scenarios.py: the fallback stats, the launches per stage, the verdict, the partial and
the entries reported invalid (a long list as its length and digest).  Every route gives exact
statuses, so only these show that host-side routing code still sends each batch where it went before.

  tools/route_trace.py --record           run every scenario, write tests/golden/route_trace.json
  tools/route_trace.py --scenario NAME    run one, print its trace as one JSON line

tests/test_gpu_route_trace.py compares trace() of each scenario with the recorded file."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "chaum-pedersen-zkp_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import chaum_pedersen as cp  # noqa: E402
from route_scenarios import SCENARIOS  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "route_trace.json")
KEYS = ("y1", "y2", "r1", "r2", "s")
SX = hashlib.sha256(b"cpz-route-x").digest()
SK = hashlib.sha256(b"cpz-route-k").digest()
WSEED = hashlib.sha256(b"cpz-route-weights").digest()
PAIRS_MAX = 64


def device_info():
    import torch
    p = torch.cuda.get_device_properties(0)
    return {"name": p.name, "cus": int(p.multi_processor_count)}


def forged_entries(scn):
    if "forged" in scn:
        return np.asarray(sorted(scn["forged"]), np.int64)
    rng = np.random.default_rng(scn["seed"])
    return np.sort(rng.choice(scn["n"], int(scn["n"] * scn["density"]), replace=False)).astype(np.int64)


def invalid_record(entries):
    """The sorted entries reported invalid as the fixture holds them: the list itself up to 64 of
    them, above that their number and the SHA-256 of the indices as little-endian int64."""
    e = np.asarray(entries, np.int64)
    if e.size <= 64:
        return [int(i) for i in e]
    return {"count": int(e.size), "sha256": hashlib.sha256(e.astype("<i8").tobytes()).hexdigest()}


def _scalars(seed, n):
    a = np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)
    a[:, 31] &= 0x0f  # below 2^252 < l
    return a


def _plus_one(rows):
    """s := s + 1 on (m, 32) little-endian rows, in place."""
    for r in range(rows.shape[0]):
        v = int.from_bytes(rows[r].tobytes(), "little") + 1
        rows[r] = np.frombuffer(v.to_bytes(32, "little"), np.uint8)


def make_pairs(maker, k):
    """The default pair, then k - 1 distinct ones from one prove under it: ([a] g, [a] h)."""
    if k == 1:
        return [cp.Parameters()]
    out = maker.prove(_scalars(11, k - 1), _scalars(12, k - 1))
    return [cp.Parameters()] + [cp.Parameters(out["y1"][i].tobytes(), out["y2"][i].tobytes()) for i in range(k - 1)]


def _prove_mixed(maker, pairs, idx, n):
    """Valid proofs, entry i under pairs[idx[i]]: prove_pairs_device, PAIRS_MAX pairs a call."""
    import torch
    dev = "cuda:0"
    x, k = _scalars(21, n), _scalars(22, n)
    rows = {q: np.zeros((n, 32), np.uint8) for q in KEYS}
    for c in range(0, len(pairs), PAIRS_MAX):
        sel = np.nonzero((idx >= c) & (idx < c + PAIRS_MAX))[0]
        if not len(sel):
            continue
        outs = [torch.empty((len(sel), 32), dtype=torch.uint8, device=dev) for _ in KEYS]
        maker.prove_pairs_device(pairs[c:c + PAIRS_MAX], torch.from_numpy((idx[sel] - c).astype(np.int32)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(x[sel])).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(k[sel])).to(dev), *outs)
        for q, o in zip(KEYS, outs):
            rows[q][sel] = o.cpu().numpy()
    return rows


def trace(scn, maker):
    """Run one scenario (in this process, whatever scn["env"] says): proofs from `maker`, the
    check on a context of its own with timing on."""
    import torch
    n, forged = scn["n"], forged_entries(scn)
    with cp.Gpu(0) as fresh:
        fresh.set_timing(True)
        if scn["api"] == "device":
            dev = "cuda:0"
            t = {q: torch.empty((n, 32), dtype=torch.uint8, device=dev) for q in KEYS}
            maker.prove_synthetic_device(n, SX, SK, *[t[q] for q in KEYS])
            sel = torch.from_numpy(forged).to(dev)
            bumped = t["s"].index_select(0, sel).cpu().numpy()
            _plus_one(bumped)
            t["s"].index_copy_(0, sel, torch.from_numpy(bumped).to(dev))
            st = torch.full((n,), 0xAA, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            fresh.stage_times()
            partial, ok = fresh.verify_batch_device(*[t[q] for q in KEYS], st, WSEED, fallback=True)
            torch.cuda.synchronize()
            status = st.cpu().numpy()
        else:
            pairs = make_pairs(maker, scn["npairs"])
            idx = (np.arange(n) % scn["npairs"]).astype(np.uint32)
            rows = _prove_mixed(maker, pairs, idx, n)
            bumped = rows["s"][forged]
            _plus_one(bumped)
            rows["s"][forged] = bumped
            torch.cuda.synchronize()
            fresh.stage_times()
            cols = [rows[q] for q in KEYS]
            if scn["api"] == "pairs":
                partial, ok, status = fresh.verify_batch_pairs(pairs, idx, *cols, WSEED,
                                                               locate=scn.get("locate", "auto"))
            else:
                partial, ok, status = fresh.verify_batch_pairs_many(pairs, idx, *cols, WSEED)
        stages = fresh.stage_times()
        stats = fresh.fallback_stats()
    return {"fallback_stats": stats, "launches": {k: int(v[1]) for k, v in sorted(stages.items())},
            "batch_ok": bool(ok), "partial": partial.hex(),
            "invalid": invalid_record(np.nonzero(status)[0]),
            "invalid_statuses": sorted(set(int(v) for v in status[status != 0]))}


def trace_in_child(scn):
    """trace() of a scenario with an environment of its own, in a fresh process."""
    env = dict(os.environ)
    env.update(scn["env"])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--scenario", scn["name"]], capture_output=True,
                       text=True, timeout=300, env=env, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError("scenario %s failed in its child process:\n%s" % (scn["name"], r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def run(scn, maker):
    return trace_in_child(scn) if scn.get("env") else trace(scn, maker)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", action="store_true", help="write tests/golden/route_trace.json")
    ap.add_argument("--scenario", help="run this scenario here and print its trace")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    by_name = {s["name"]: s for s in SCENARIOS}
    with cp.Gpu(0) as maker:
        if args.scenario:
            print(json.dumps(trace(by_name[args.scenario], maker), separators=(",", ":")))
            return
        if not args.record:
            ap.error("--record or --scenario NAME")
        out = {"device": device_info(), "scenarios": {}}
        for scn in SCENARIOS:
            out["scenarios"][scn["name"]] = run(scn, maker)
            t = out["scenarios"][scn["name"]]
            print(scn["name"], t["fallback_stats"], t["launches"], flush=True)
    with open(args.out, "w") as f:  # a scenario per line
        f.write('{"device":%s,"scenarios":{\n' % json.dumps(out["device"], separators=(",", ":")))
        f.write(",\n".join('%s:%s' % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                           for k, v in out["scenarios"].items()))
        f.write("\n}}\n")


if __name__ == "__main__":
    main()
