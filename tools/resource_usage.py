#!/usr/bin/env python3
"""Per-kernel resource usage of the product's HIP units, as a table.

    tools/resource_usage.py [--csrc DIR] [--units a.hip,b.hip] [--match REGEX]

Compiles each unit of DIR (default: the tree's csrc) for gfx950 with
-Rpass-analysis=kernel-resource-usage, as build_native.py compiles it, and prints one line per
kernel: SGPRs, VGPRs, AGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes per block and
waves per SIMD.  Run it on two checkouts to compare them (profiles/batch_pairs_resource_usage.txt).
No GPU is needed."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "chaum-pedersen-zkp_amd"))

FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("VGPRs Spill", "vspill"), ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ"))


def demangle(names):
    try:
        out = subprocess.run(["c++filt", "-p"], input="\n".join(names), text=True, capture_output=True, check=True)
        return out.stdout.split("\n")[:len(names)]
    except Exception:
        return names


def usage(csrc, unit):
    import build_native
    flags = build_native.UNIT_FLAGS.get(unit, [])
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([build_native._hipcc(), "--offload-arch=" + build_native.ARCH, "-O3", "-std=c++17", "-fPIC",
                            "-I", csrc, "-I", os.path.join(os.path.dirname(os.path.dirname(csrc)), "include"),
                            "-Rpass-analysis=kernel-resource-usage"] + flags +
                           ["-c", os.path.join(csrc, unit), "-o", os.path.join(tmp, "u.o")],
                           text=True, capture_output=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr[-4000:])
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {"name": val}
            rows.append(cur)
        elif cur is not None:
            for field, short in FIELDS:
                if key == field:
                    cur[short] = int(val)
    for row, name in zip(rows, demangle([r_["name"] for r_ in rows])):
        row["name"] = re.sub(r"^cpz::", "", name)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "chaum-pedersen-zkp_amd", "csrc"))
    ap.add_argument("--units", default="kernels.hip,rlc.hip")
    ap.add_argument("--match", default="")
    a = ap.parse_args()
    print("%-46s %5s %5s %5s %8s %7s %7s %4s" % ("kernel", "sgpr", "vgpr", "agpr", "scratch", "vspill", "lds", "occ"))
    for unit in a.units.split(","):
        for row in usage(os.path.abspath(a.csrc), unit):
            if a.match and not re.search(a.match, row["name"]):
                continue
            print("%-46s %5d %5d %5d %8d %7d %7d %4d" % ((row["name"][:46],) + tuple(row.get(s, -1) for _, s in FIELDS)))


if __name__ == "__main__":
    main()
