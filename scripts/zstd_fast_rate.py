#!/usr/bin/env python3
"""Rates of the fast Zstd encoder next to the exact one, same device,
same process: medians of REPS timed repetitions after 2 warm-ups, device legs
under device events, host legs on the wall clock.  Writes
profiles/round9/zstd_fast_rate.json.

  python scripts/zstd_fast_rate.py            # every leg
  python scripts/zstd_fast_rate.py --max-blocks 20   # skip the larger batches

The exact encoder is not touched by the fast mode, so its figures here are the
parent's, measured in the same session.  Device legs: jfs_zstd_compress_device
against jfs_zstd_compress_fast_device on blocks generated in HBM.  Host legs:
Compress and CompressBatch with the parse mode held at exact, then fast."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from juicefs_amd import compress as C  # noqa: E402
from juicefs_amd import device as D  # noqa: E402
from juicefs_amd.blockgen import gen_block  # noqa: E402

U = 4 << 20
GIB = float(1 << 30)


def dev_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def wall_ms(fn, reps):
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def device_leg(nblk, cls, reps):
    dev = torch.device("cuda:0")
    raw = torch.empty(nblk * U, dtype=torch.uint8, device=dev)
    D.gen_blocks(raw, nblk, U, cls, 1)
    slot = (D.zstd_bound(U) + 255) // 256 * 256
    comp = torch.empty(nblk * slot, dtype=torch.uint8, device=dev)
    offs = np.arange(nblk, dtype=np.int64)
    desc = D.make_desc(raw, offs * U, [U] * nblk, comp, offs * slot, [slot] * nblk)
    ret = torch.empty(nblk, dtype=torch.int32, device=dev)
    legs = {"nblk": nblk, "cls": cls}
    sizes = {}
    for mode, fn in (("exact", D.zstd_compress), ("fast", D.zstd_compress_fast)):
        legs[f"{mode}_ms"] = dev_ms(lambda: fn(desc, ret), reps)
        torch.cuda.synchronize()
        r = ret.cpu().numpy().astype("int64")
        assert (r > 0).all(), (mode, int(r.min()))
        sizes[mode] = int(r.sum())
    # the fast frames of the last repetition decode back to the blocks
    back = torch.empty_like(raw)
    ddesc = D.make_desc(comp, offs * slot, ret.cpu().tolist(), back, offs * U, [U] * nblk)
    dret = torch.empty(nblk, dtype=torch.int32, device=dev)
    D.zstd_decompress_sync(ddesc, dret)
    assert (dret.cpu().numpy() == U).all() and torch.equal(back, raw), "fast frames do not decode to the input"
    gib = nblk * U / GIB
    legs.update(exact_gibs=gib / legs["exact_ms"] * 1e3, fast_gibs=gib / legs["fast_ms"] * 1e3,
                speedup=legs["exact_ms"] / legs["fast_ms"], size_ratio=sizes["fast"] / sizes["exact"],
                fast_compression=nblk * U / sizes["fast"])
    del raw, comp, back
    torch.cuda.empty_cache()
    return legs


def host_legs(reps):
    c = C.ZStandard()
    blocks = [gen_block("T", 100 + i, U) for i in range(20)]
    out = {}
    for mode in ("exact", "fast"):
        with C.zstd_parse_mode(mode):
            d = bytearray(c.CompressBound(U))
            out[f"lone_{mode}_ms"] = wall_ms(lambda: c.Compress(d, blocks[0]), reps)
            dsts = [bytearray(c.CompressBound(U)) for _ in blocks]

            def burst():
                ts = [threading.Thread(target=c.Compress, args=(dsts[i], blocks[i])) for i in range(20)]
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()
            ms = wall_ms(burst, reps)
            out[f"concurrent20_{mode}_ms"] = ms
            out[f"concurrent20_{mode}_gibs"] = 20 * U / GIB / ms * 1e3
    return out


def host_batch_leg(nblk, reps):
    c = C.ZStandard()
    uniq = [gen_block("T", 200 + i, U) for i in range(16)]
    pairs = [(bytearray(c.CompressBound(U)), uniq[i % 16]) for i in range(nblk)]
    out = {"nblk": nblk}
    for mode in ("exact", "fast"):
        with C.zstd_parse_mode(mode):
            ms = wall_ms(lambda: c.CompressBatch(pairs), reps)
            out[f"{mode}_ms"], out[f"{mode}_gibs"] = ms, nblk * U / GIB / ms * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-blocks", type=int, default=1024)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round9", "zstd_fast_rate.json"))
    a = ap.parse_args()
    assert a.reps >= 7, "medians of at least 7 repetitions"
    res = {"block_bytes": U, "reps": a.reps, "device": torch.cuda.get_device_name(0), "device_legs": []}
    for nblk, cls in [(1, "T"), (1, "Z"), (1, "R"), (20, "T"), (1024, "T"), (1024, "Z"), (1024, "R")]:
        if nblk > a.max_blocks:
            res.setdefault("skipped", []).append([nblk, cls])
            continue
        leg = device_leg(nblk, cls, a.reps)
        print(json.dumps(leg), flush=True)
        res["device_legs"].append(leg)
    if not a.no_host:
        res["host"] = host_legs(a.reps)
        print(json.dumps(res["host"]), flush=True)
        if a.max_blocks >= 1024:
            res["host_batch"] = host_batch_leg(1024, a.reps)
            print(json.dumps(res["host_batch"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
