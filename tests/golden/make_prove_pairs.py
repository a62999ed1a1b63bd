"""Generate tests/golden/prove_pairs.json from the CPU oracle (oracle/pyoracle.py prove).

Run:  python tests/golden/make_prove_pairs.py
Data only: three (g, h) pairs -- the default pair and two custom [a] B, [b] B -- and one entry per
edge scalar of tests/prove_pairs_cases.py crossed with the four context shapes (None, 32 bytes,
5 bytes, b""), cycling over the pairs, each edge once as the witness x with a random nonce k and
once as the nonce with a random witness.  The oracle decides every expected row (x = 0 and k = 0
give identity encodings, 32 zero bytes).  tests/test_gpu_prove_pairs.py proves the same inputs
with Gpu.prove_pairs and compares the bytes.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyoracle as O  # noqa: E402
from prove_pairs_cases import CONTEXTS, EDGES, custom_pairs_scalars, random_scalar  # noqa: E402


def main():
    pts = [(O.BASEPOINT, O.generator_h())]
    for a, b in custom_pairs_scalars(2, b"prove-pairs-golden"):
        pts.append((O.pt_mul(O.BASEPOINT, a), O.pt_mul(O.BASEPOINT, b)))
    pairs = [{"g": O.ristretto_encode(g).hex(), "h": O.ristretto_encode(h).hex()} for g, h in pts]
    assert pairs[0] == {"g": O.G_BYTES.hex(), "h": O.H_BYTES.hex()}
    entries = []
    for role in ("x", "k"):
        for e, (name, raw) in enumerate(EDGES):
            for c, ctx in enumerate(CONTEXTS):
                i = len(entries)
                p = i % len(pts)
                other = O.scalar_bytes(random_scalar(role.encode(), i))
                x, k = (raw, other) if role == "x" else (other, raw)
                rec = O.prove(int.from_bytes(x, "little") % O.L, int.from_bytes(k, "little") % O.L, ctx, *pts[p])
                entries.append({"what": "%s = %s" % (role, name), "pair": p, "x": x.hex(), "k": k.hex(),
                                "ctx": None if ctx is None else ctx.hex(), "y1": rec.y1.hex(), "y2": rec.y2.hex(),
                                "r1": rec.r1.hex(), "r2": rec.r2.hex(), "s": rec.s.hex()})
    zero = bytes(32).hex()
    assert all(e["y1"] == zero and e["y2"] == zero for e in entries if e["what"] == "x = 0")
    assert all(e["r1"] == zero and e["r2"] == zero for e in entries if e["what"] == "k = 0")
    assert {e["pair"] for e in entries} == {0, 1, 2}
    out = os.path.join(HERE, "prove_pairs.json")
    with open(out, "w") as f:
        json.dump({"pairs": pairs, "entries": entries}, f, indent=0)
        f.write("\n")
    print("wrote", out, len(entries), "entries")


if __name__ == "__main__":
    main()
