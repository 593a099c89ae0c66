#!/usr/bin/env python3
"""What splicing untouched frames buys the Zstd compaction call:
64 text-class sources of 4 MiB stored as seekable objects, one output per
source, jfs_compact_batch from host buffers on one GPU, under three plans:

  (a) overwrite  one 4 KiB overwrite per block: 31 of 32 frames pass;
  (b) identity   every frame passes, nothing is decoded or encoded;
  (c) shifted    every block read from 4 KiB on: nothing passes, so the switch
                 on must cost what the switch off costs.

Per plan the switch off and on are interleaved call by call; medians of --reps
calls after --warmup calls, with min and max, the counters of one call, and the
ratio off / on.  --root DIR imports juicefs_amd from another checkout (the
parent commit, for the baseline): a package without the switch runs only the
"off" legs.  Needs a GPU; writes one JSON file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 4 << 20
NSRC = 64
K4 = 4 << 10


def plans():
    over, ident, shift = ([0], []), ([0], []), ([0], [])
    for i in range(NSRC):
        at = (i % 32) * (128 << 10) + 8 * K4  # inside frame i mod 32
        over[1].extend([(i, 0, 0, at), (NSRC + i, 0, at, K4), (i, at + K4, at + K4, U - at - K4)])
        ident[1].append((i, 0, 0, U))
        shift[1].append((i, K4, 0, U - K4))
        for p in (over, ident, shift):
            p[0].append(len(p[1]))
    return {"overwrite": over, "identity": ident, "shifted": shift}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--root", default=ROOT, help="the checkout whose juicefs_amd is measured")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seekable", "rates_splice.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from juicefs_amd import compress as C
    from juicefs_amd import device as D
    assert torch.cuda.is_available(), "compact_splice_rate.py measures on a GPU"
    has_switch = hasattr(C, "set_compact_splice_mode")
    dev = torch.device("cuda:0")
    raw_t = torch.empty(NSRC * U, dtype=torch.uint8, device=dev)
    D.gen_blocks(raw_t, NSRC, U, "T", 7000)
    torch.cuda.synchronize()
    raw = raw_t.cpu().numpy()
    rng = np.random.default_rng(5)
    small = [rng.integers(0, 256, K4, dtype=np.uint8).tobytes() for _ in range(NSRC)]
    z = C.NewCompressor("zstd")
    C.set_zstd_parse_mode("seekable")
    blocks = [raw[i * U:(i + 1) * U] for i in range(NSRC)] + small
    sd = [bytearray(z.CompressBound(len(b))) for b in blocks]
    r = z.CompressBatch(list(zip(sd, blocks)))
    assert all(e is None for _, e in r)
    stored = [bytes(sd[i][:r[i][0]]) for i in range(len(blocks))]
    sources = [(s, U) for s in stored[:NSRC]] + [(s, K4) for s in stored[NSRC:]]
    dst = [bytearray(z.CompressBound(U)) for _ in range(NSRC)]
    res = {"label": a.label, "shape": {"sources": NSRC, "block_bytes": U, "frame_bytes": 128 << 10,
                                       "stored_source_bytes": sum(len(s) for s in stored[:NSRC])},
           "reps": a.reps, "warmup": a.warmup, "plans": {}}
    for name, plan in plans().items():
        t = {"off": [], "on": []}
        counts, sizes = None, {}
        for it in range(a.warmup + a.reps):
            for mode in (("off", "on") if has_switch else ("off",)):
                if has_switch:
                    C.set_compact_splice_mode(mode)
                    C.compact_splice_counts(reset=True)
                t0 = time.perf_counter()
                sres, ores = z.CompactBatch(sources, dst, plan)
                dt = (time.perf_counter() - t0) * 1e3
                assert all(e is None for _, e in sres + ores), (name, mode)
                sizes[mode] = sum(n for n, _ in ores)
                if has_switch and mode == "on":
                    counts = C.compact_splice_counts()
                if it >= a.warmup:
                    t[mode].append(dt)
        leg = {"stored_output_bytes": sizes}
        for mode, xs in t.items():
            if xs:
                leg[mode] = {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs),
                             "gib_s_gathered": NSRC * U / 2**30 / (statistics.median(xs) / 1e3)}
        if t["on"]:
            leg["counts_of_one_call"] = dict(zip(("outputs_spliced", "frames_passed", "frames_reencoded", "bytes_passed"), counts))
            leg["off_over_on"] = leg["off"]["median_ms"] / leg["on"]["median_ms"]
        res["plans"][name] = leg
    if has_switch:
        C.set_compact_splice_mode("off")
    C.set_zstd_parse_mode("exact")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
