#!/usr/bin/env python3
"""Hop-count histogram of the LZ4 origin chase (juicefs_amd/csrc/lz4_chase.h),
from its Python restatement (tests/lz4_chase_cases.py hop_depths): per output
byte, the steps from the byte to its literal.  4 MiB blocks of every blockgen
class and a mixed block, from the exact LZ4 oracle encoder and from the fast
parse's host twin.  CPU only.  CHASE_HOPS is the smallest power of two that is
at least twice the largest depth printed here.

  python scripts/lz4_chase_hops.py [--size BYTES] [--out profiles/lz4_chase/hops.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from juicefs_amd import compress as C  # noqa: E402
from juicefs_amd.blockgen import gen_block  # noqa: E402
from tests import lz4_chase_cases as K  # noqa: E402
from tests.oracle_ctypes import Oracle  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lz4_chase", "hops.json"))
    a = ap.parse_args()
    oracle = Oracle(os.path.join(ROOT, "oracle", "_build", "liboracle.so"))
    blocks = [("T", gen_block("T", 4100, a.size)), ("T2", gen_block("T", 4101, a.size)), ("Z", gen_block("Z", 0, a.size)),
              ("R", gen_block("R", 4102, a.size)), ("mixed", K.mixed_block(11, a.size)), ("mixed2", K.mixed_block(12, a.size))]
    rows, top = [], 0
    for name, src in blocks:
        for enc, comp in (("exact", oracle.lz4_compress(src)[1]), ("fast", C.lz4_fast_host(src))):
            hist, mx = K.hop_histogram(comp)
            n = sum(hist.values())
            mean = sum(k * v for k, v in hist.items()) / max(n, 1)
            # bytes at depth >= 1, 2, 4, 8, ...
            tail = {str(1 << b): sum(v for k, v in hist.items() if k >= (1 << b)) for b in range(0, 8) if (1 << b) <= max(mx, 1)}
            rows.append({"block": name, "encoder": enc, "bytes": n, "compressed": len(comp), "max_depth": mx,
                         "mean_depth": round(mean, 3), "bytes_at_depth_ge": tail, "histogram": hist})
            top = max(top, mx)
            print(f"{name:7s} {enc:5s} comp={len(comp):8d} max={mx:3d} mean={mean:6.3f}", flush=True)
    out = {"size": a.size, "max_depth": top, "chase_hops": K.hops_cap(top), "rows": rows}
    print(f"largest depth {top}: CHASE_HOPS = {K.hops_cap(top)}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
