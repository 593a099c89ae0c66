#!/usr/bin/env python3
"""One leg of the LZ4 window measurement: reads of 4 KiB and
128 KiB from the head, the middle or the tail of 4 MiB text blocks, from the
fast encoder and again from the exact encoder, 1 and 128 sources per call, one
read per source.

  --leg prefix   JFS_READ_DECODE=prefix and nothing else: run it from a checkout
                 of the commit to compare against (--tree), whose library knows
                 no window switch -- the code under test is never its own yardstick
  --leg window   JFS_READ_DECODE=prefix with JFS_READ_LZ4_WINDOW on: this tree

Per cell: the wall time of Compressor.ReadBatch (host buffers in, host buffers
out) and the device time, by events, of the decode call alone on resident
buffers (jfs_lz4_decompress_prefix_device_small with want = the read's end, or
jfs_lz4_decompress_window_device_small with the read's range).  Median, minimum
and the 10th..90th percentile spread of --reps calls after --warmup; one JSON
file per run.  Run the legs alternately, twice each, every run under its own
time limit, and report the medians as lower..upper of the two runs."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=["prefix", "window"], required=True)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", required=True)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sources", default="1,128")
ap.add_argument("--sizes", default="4096,131072")
ap.add_argument("--encoders", default="fast,exact")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
os.environ["JFS_READ_DECODE"] = "prefix"

import numpy as np  # noqa: E402
import torch  # noqa: E402

from juicefs_amd import compress as C  # noqa: E402
from juicefs_amd import device as D  # noqa: E402
from juicefs_amd.blockgen import gen_block  # noqa: E402
from tests.oracle_ctypes import Oracle  # noqa: E402

BLOCK = 4 << 20
ROOT = os.path.abspath(args.tree)
oracle = Oracle(os.path.join(ROOT, "oracle", "_build", "liboracle.so"))
raws = [gen_block("T", 8800 + i, BLOCK) for i in range(2)]
dev = torch.device("cuda:0")
if args.leg == "window":
    C.set_read_lz4_window_mode("on")


def stats(ts):
    ts = sorted(ts)
    q = lambda p: ts[min(len(ts) - 1, int(p * len(ts)))]  # noqa: E731
    return {"median_us": round(statistics.median(ts) * 1e6, 1), "min_us": round(ts[0] * 1e6, 1),
            "p10_us": round(q(0.1) * 1e6, 1), "p90_us": round(q(0.9) * 1e6, 1), "n": len(ts)}


def offset(pos, size):
    return {"head": 0, "middle": (BLOCK - size) // 2 // 4096 * 4096, "tail": BLOCK - size}[pos]


rows = []
for enc in args.encoders.split(","):
    stored = [C.lz4_fast_host(r) if enc == "fast" else oracle.lz4_compress(r)[1] for r in raws]
    for nsrc in [int(x) for x in args.sources.split(",")]:
        srcs = [(stored[i % 2], BLOCK) for i in range(nsrc)]
        # resident copies for the device-time leg
        offs, o = [], 0
        for s, _ in srcs:
            offs.append(o)
            o = (o + len(s) + 63) & ~63
        host = np.zeros(o + 64, dtype=np.uint8)
        for (s, _), so in zip(srcs, offs):
            host[so:so + len(s)] = np.frombuffer(s, dtype=np.uint8)
        src_t = torch.from_numpy(host).to(dev)
        dst_t = torch.zeros(nsrc * BLOCK, dtype=torch.uint8, device=dev)
        lens = [len(s) for s, _ in srcs]
        desc = D.make_desc(src_t, offs, lens, dst_t, [i * BLOCK for i in range(nsrc)], [BLOCK] * nsrc)
        ret = torch.zeros(nsrc, dtype=torch.int32, device=dev)
        for size in [int(x) for x in args.sizes.split(",")]:
            for pos in ("head", "middle", "tail"):
                lo = offset(pos, size)
                seg_first = list(range(nsrc + 1))
                seg = [(i, lo, 0, size) for i in range(nsrc)]
                outs = [bytearray(size) for _ in range(nsrc)]
                wall = []
                for it in range(args.warmup + args.reps):
                    t0 = time.perf_counter()
                    sres, rres, _ = C.LZ4().ReadBatch(srcs, outs, (seg_first, seg))
                    t1 = time.perf_counter()
                    if it >= args.warmup:
                        wall.append(t1 - t0)
                assert all(r == (size, None) for r in rres), rres[:2]
                assert all(bytes(outs[i]) == raws[i % 2][lo:lo + size] for i in (0, nsrc - 1))
                # the decode call alone, on the device
                hi_t = torch.full((nsrc,), lo + size, dtype=torch.int32, device=dev)
                if args.leg == "prefix":
                    call = lambda: D.lz4_decompress_prefix_small(desc, hi_t, ret, lens, [BLOCK] * nsrc)  # noqa: E731
                else:
                    lo_t = torch.full((nsrc,), lo, dtype=torch.int32, device=dev)
                    call = lambda: D.lz4_decompress_window(desc, lo_t, hi_t, ret, lens, [BLOCK] * nsrc)  # noqa: E731
                    D.lz4_window_counts(reset=True)
                devt = []
                for it in range(args.warmup + args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call()
                    e1.record()
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        devt.append(e0.elapsed_time(e1) * 1e-3)
                assert ret.cpu().tolist() == [lo + size] * nsrc
                assert dst_t[lo:lo + size].cpu().numpy().tobytes() == raws[0][lo:lo + size]
                row = {"leg": args.leg, "encoder": enc, "sources": nsrc, "read_bytes": size, "position": pos,
                       "wall": stats(wall), "device": stats(devt)}
                if args.leg == "window":
                    row["window_counts"] = list(D.lz4_window_counts())
                rows.append(row)
                print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"leg": args.leg, "block": BLOCK, "class": "T", "reps": args.reps, "rows": rows}, f, indent=1)
    f.write("\n")
