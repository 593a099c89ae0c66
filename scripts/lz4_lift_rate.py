#!/usr/bin/env python3
"""One leg of the LZ4 lift measurement: compaction of 1, 20 and 128
text blocks of 4 MiB, each output its source with one 4 KiB piece overwritten,
so 63 of an output's 64 chunks are candidates.

  --leg parent    fast parse; run it from a checkout of the commit to compare
                  against (--tree), whose library knows no lift -- the code under
                  test is never its own yardstick
  --leg off       this tree, fast parse, JFS_COMPACT_LZ4_LIFT off
  --leg on-fast   this tree, the switch on, sources from the fast encoder
  --leg on-exact  this tree, the switch on, sources from the exact encoder: every
                  candidate but a chunk 0 here and there is refused, so this is
                  the cost of the index and the lift walk when they buy nothing

Per row: the wall time of Compressor.CompactBatch (host buffers in and out) and
the device time, by events, of decode -> gather -> encode on resident buffers
(jfs_lz4_decompress_device, jfs_gather_device, then
jfs_lz4_compress_fast_device or jfs_lz4_compress_fast_lift_device), and of the
encode step alone.  Median, minimum and the 10th..90th percentile spread of
--reps calls after --warmup; one JSON file per run.  Run the legs alternately,
twice each, every run under its own time limit, and report the medians as
lower..upper of the two runs.  --no-wall leaves the host calls out (for a
kernel trace of the device chain)."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--leg", choices=["parent", "off", "on-fast", "on-exact"], required=True)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", required=True)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--blocks", default="1,20,128")
ap.add_argument("--no-wall", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from juicefs_amd import compress as C  # noqa: E402
from juicefs_amd import device as D  # noqa: E402
from juicefs_amd.blockgen import gen_block  # noqa: E402

BLOCK, CH, NCH = 4 << 20, 65536, 64
LIFT = args.leg.startswith("on")
dev = torch.device("cuda:0")
raws = [gen_block("T", 9900 + i, BLOCK) for i in range(2)]
Z = C.NewCompressor("lz4")


def stats(ts):
    ts = sorted(ts)
    q = lambda p: ts[min(len(ts) - 1, int(p * len(ts)))]  # noqa: E731
    return {"median_us": round(statistics.median(ts) * 1e6, 1), "min_us": round(ts[0] * 1e6, 1),
            "p10_us": round(q(0.1) * 1e6, 1), "p90_us": round(q(0.9) * 1e6, 1), "n": len(ts)}


def exact_stream(raw):
    src = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev)
    cap = D.lz4_bound(len(raw))
    dst = torch.zeros(cap, dtype=torch.uint8, device=dev)
    ret = torch.zeros(1, dtype=torch.int32, device=dev)
    D.lz4_compress(D.make_desc(src, [0], [len(raw)], dst, [0], [cap]), ret)
    torch.cuda.synchronize()
    return dst[:int(ret.cpu()[0])].cpu().numpy().tobytes()


def timed(call, reps, warmup):
    out = []
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) * 1e-3)
    return out


stored2 = [exact_stream(r) if args.leg == "on-exact" else C.lz4_fast_host(r) for r in raws]
rows = []
for nblk in [int(x) for x in args.blocks.split(",")]:
    stored = [stored2[i % 2] for i in range(nblk)]
    # output k: source k, 4 KiB at `cut` from the next source (a lone block: from another place of itself)
    seg_first, seg, lift = [0], [], []
    for k in range(nblk):
        cut = (k * 37 % 60 + 1) * CH + 1000
        seg += [(k, 0, 0, cut), ((k + 1) % nblk, cut + 8 * CH if nblk == 1 else cut, cut, 4096),
                (k, cut + 4096, cut + 4096, BLOCK - cut - 4096)]
        seg_first.append(len(seg))
        lift += [(k, j) if j != cut // CH and (j + 1) * CH + 12 <= BLOCK else (-1, 0) for j in range(NCH)]
    planned = sum(s >= 0 for s, _ in lift)
    row = {"leg": args.leg, "blocks": nblk, "planned": planned}
    with C.lz4_parse_mode("fast"):
        if LIFT:
            C.set_compact_lz4_lift_mode("on")
            C.compact_lz4_lift_counts(reset=True)
        if not args.no_wall:
            srcs = [(s, BLOCK) for s in stored]
            outs = [bytearray(Z.CompressBound(BLOCK)) for _ in range(nblk)]
            wall = []
            for it in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                sres, ores = Z.CompactBatch(srcs, outs, (seg_first, seg))[:2]
                t1 = time.perf_counter()
                if it >= args.warmup:
                    wall.append(t1 - t0)
            assert all(e is None for _, e in sres) and all(e is None and n > 0 for n, e in ores), (sres[:2], ores[:2])
            row["wall"] = stats(wall)
            row["out_bytes"] = sum(n for n, _ in ores)
            if LIFT:
                row["lift_counts"] = list(C.compact_lz4_lift_counts(reset=True))
    # the chain's kernels on resident buffers
    offs, o = [], 0
    for s in stored:
        offs.append(o)
        o = (o + len(s) + 63) & ~63
    host = np.zeros(o + 64, dtype=np.uint8)
    for s, so in zip(stored, offs):
        host[so:so + len(s)] = np.frombuffer(s, dtype=np.uint8)
    d_stored = torch.from_numpy(host).to(dev)
    d_dec = torch.zeros(nblk * BLOCK, dtype=torch.uint8, device=dev)
    d_gat = torch.zeros(nblk * BLOCK, dtype=torch.uint8, device=dev)
    cap = D.lz4_bound(BLOCK)
    ostep = (cap + 63) & ~63
    d_out = torch.zeros(nblk * ostep, dtype=torch.uint8, device=dev)
    lens = [len(s) for s in stored]
    sdesc = D.make_desc(d_stored, offs, lens, d_dec, [i * BLOCK for i in range(nblk)], [BLOCK] * nblk)
    src_n = torch.zeros(nblk, dtype=torch.int32, device=dev)
    odesc, dseg = D.make_compact_desc(d_gat, [i * BLOCK for i in range(nblk)], [BLOCK] * nblk, seg_first, seg)
    gret = torch.zeros(nblk, dtype=torch.int32, device=dev)
    edesc = D.make_desc(d_gat, [i * BLOCK for i in range(nblk)], [BLOCK] * nblk, d_out, [i * ostep for i in range(nblk)],
                        [cap] * nblk)
    eret = torch.zeros(nblk, dtype=torch.int32, device=dev)
    if LIFT:
        flat = np.array(lift, dtype=D.LIFT_DTYPE)
        d_lift = torch.from_numpy(flat.view(np.uint8).copy()).to(dev)
        lifted = torch.zeros(nblk, dtype=torch.int32, device=dev)

    def encode():
        if LIFT:
            D.lz4_compress_fast_lift(edesc, eret, [BLOCK] * nblk, d_lift, sdesc, src_n, lens, [BLOCK] * nblk, lifted)
        else:
            D.lz4_compress_fast(edesc, eret, [BLOCK] * nblk)

    def chain():
        D.lz4_decompress(sdesc, src_n)
        D.gather(sdesc, src_n, odesc, dseg, BLOCK, gret)
        encode()

    row["device_chain"] = stats(timed(chain, args.reps, args.warmup))
    row["device_encode"] = stats(timed(encode, args.reps, args.warmup))
    assert src_n.cpu().tolist() == [BLOCK] * nblk and gret.cpu().tolist() == [BLOCK] * nblk
    assert all(r > 0 for r in eret.cpu().tolist())
    row["device_out_bytes"] = int(eret.sum().cpu())
    if LIFT:
        row["device_lifted"] = int(lifted.sum().cpu())
    rows.append(row)
    print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump({"leg": args.leg, "block": BLOCK, "class": "T", "reps": args.reps, "rows": rows}, f, indent=1)
    f.write("\n")
