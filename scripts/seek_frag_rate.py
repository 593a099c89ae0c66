#!/usr/bin/env python3
"""What checksummed seek tables and fragment decode cost and buy,
in the method of 12e: one process, medians of --reps after --warmup, the sides
of a comparison interleaved call by call, min and max beside every median.

  (a) jfs_xxh64_device alone: 1, 32 and 32,768 pieces of 128 KiB in HBM, under
      device events; GB/s and, for one piece, microseconds per 32-byte step;
  (b) jfs_zstd_compress_seekable_device against
      jfs_zstd_compress_seekable_csum_device, 1 and 1,024 text objects of 4 MiB
      in HBM, wall time (both calls are host-synchronous; the checksummed one
      includes a copy of the descriptors to the host and of the piece list back);
  (c) 12e's read table: 64 text sources of 4 MiB from host buffers, one 128 KiB
      read each, at seeded uniform offsets and at the last 128 KiB:
      ReadBatch with JFS_READ_SEEK=on on seekable objects (12e's column (b))
      against LoadRangeBatch from table + planned fragment, 8-byte and 12-byte
      tables.  The difference between the last two is the price of verification.

Needs a GPU; writes one JSON file (default profiles/seekable/rates_frag.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U = 4 << 20
B = 128 << 10


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def interleaved(a, sides):
    """sides = {name: fn}; every round calls each once, in order -> {name: summary}"""
    ms = {k: [] for k in sides}
    for it in range(a.warmup + a.reps):
        for k, fn in sides.items():
            t = fn()
            if it >= a.warmup:
                ms[k].append(t)
    return {k: summary(v) for k, v in ms.items()}


def xxh_alone(a, torch, D, dev):
    out = {}
    for n in (1, 32, 32768):
        src = torch.empty(n * B + 1, dtype=torch.uint8, device=dev)
        D.gen_blocks(src, max(1, n * B // U), min(U, n * B), "T", 9000)
        offs = [1 + k * B for k in range(n)]  # unaligned starts, the normal case
        desc = D.make_desc(src, offs, [B] * n, src, [0] * n, [0] * n)
        h = torch.zeros(n, dtype=torch.int64, device=dev)

        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            D.xxh64(desc, h)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        r = interleaved(a, {"xxh64": run})["xxh64"]
        r["gb_per_s"] = n * B / r["median_ms"] / 1e6
        if n == 1:
            r["us_per_step"] = r["median_ms"] * 1e3 / (B // 32)
        out[f"pieces_{n}"] = r
        del src, desc, h
    return out


def encode(a, torch, D, dev):
    out = {}
    for n in (1, 1024):
        src = torch.empty(n * U, dtype=torch.uint8, device=dev)
        D.gen_blocks(src, n, U, "T", 9100)
        cap = D.zstd_bound(U)
        dst = torch.empty(n * cap, dtype=torch.uint8, device=dev)
        desc = D.make_desc(src, [k * U for k in range(n)], [U] * n, dst, [k * cap for k in range(n)], [cap] * n)
        ret = torch.zeros(n, dtype=torch.int32, device=dev)

        def side(fn):
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(desc, ret)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            return run
        r = interleaved(a, {"seekable": side(D.zstd_compress_seekable), "checksummed": side(D.zstd_compress_seekable_csum)})
        r["extra_ms"] = r["checksummed"]["median_ms"] - r["seekable"]["median_ms"]
        out[f"objects_{n}"] = r
        del src, dst, desc, ret
    return out


def reads(a, torch, C, D, dev):
    nsrc = 64
    raw_t = torch.empty(nsrc * U, dtype=torch.uint8, device=dev)
    D.gen_blocks(raw_t, nsrc, U, "T", 7000)
    torch.cuda.synchronize()
    raw = raw_t.cpu().numpy()
    del raw_t
    z = C.ZStandard()
    objs = {}
    prev = C.set_zstd_parse_mode("seekable")
    try:
        for name, mode in (("8", "off"), ("12", "on")):
            C.set_zstd_seek_csum_mode(mode)
            sd = [bytearray(z.CompressBound(U)) for _ in range(nsrc)]
            r = z.CompressBatch([(sd[i], raw[i * U:(i + 1) * U]) for i in range(nsrc)])
            assert all(e is None for _, e in r)
            objs[name] = [bytes(sd[i][:r[i][0]]) for i in range(nsrc)]
    finally:
        C.set_zstd_seek_csum_mode("off")
        C.set_zstd_parse_mode(prev)
    rng = np.random.default_rng(2025)
    out = {}
    for wname, offs in (("uniform", [int(rng.integers(0, U - B + 1)) for _ in range(nsrc)]), ("last_128k", [U - B] * nsrc)):
        want = [raw[i * U + o:i * U + o + B] for i, o in enumerate(offs)]
        dst = [np.empty(B, dtype=np.uint8) for _ in range(nsrc)]
        seg_first, seg = list(range(nsrc + 1)), [(i, o, 0, B) for i, o in enumerate(offs)]
        srcs = [(o, U) for o in objs["8"]]
        frag = {}
        for name in ("8", "12"):
            rr = []
            for i, o in enumerate(offs):
                obj = objs[name][i]
                p = C.seek_plan(obj[-4096:], len(obj), o, o + B)  # (the table is cached per key: not timed)
                assert p["status"] == "ok"
                rr.append((dst[i], obj[p["table_off"]:], len(obj), obj[p["get_off"]:p["get_off"] + p["get_len"]],
                           p["get_off"], o, o + B, U))
            frag[name] = rr

        def check():
            for j in range(nsrc):
                assert np.array_equal(dst[j], want[j]), (wname, j)
                dst[j][:] = 0

        def read_batch():
            old = C.set_read_seek_mode("on")
            try:
                t0 = time.perf_counter()
                sres, rres, _ = z.ReadBatch(srcs, dst, (seg_first, seg))
                t = (time.perf_counter() - t0) * 1e3
            finally:
                C.set_read_seek_mode(old)
            assert all(e is None for _, e in sres + rres)
            check()
            return t

        def load_range(name):
            def run():
                t0 = time.perf_counter()
                res = z.LoadRangeBatch(frag[name])
                t = (time.perf_counter() - t0) * 1e3
                assert all(e is None and n == B for n, e in res)
                check()
                return t
            return run
        r = interleaved(a, {"read_batch_seek_on": read_batch, "load_range_8": load_range("8"), "load_range_12": load_range("12")})
        r["bytes_up"] = {"read_batch": sum(len(o) for o in objs["8"]),
                         "load_range_8": sum(len(x[1]) + len(x[3]) for x in frag["8"]),
                         "load_range_12": sum(len(x[1]) + len(x[3]) for x in frag["12"])}
        r["verification_ms"] = r["load_range_12"]["median_ms"] - r["load_range_8"]["median_ms"]
        out[wname] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seekable", "rates_frag.json"))
    ap.add_argument("--only", choices=["xxh64", "encode", "reads"], action="append")
    a = ap.parse_args()
    import torch
    from juicefs_amd import compress as C
    from juicefs_amd import device as D
    dev = torch.device("cuda:0")
    parts = a.only or ["xxh64", "encode", "reads"]
    res = {"method": f"one process, medians of {a.reps} after {a.warmup} warm-ups, sides interleaved", "device": torch.cuda.get_device_name(0)}
    if "xxh64" in parts:
        res["xxh64"] = xxh_alone(a, torch, D, dev)
    if "encode" in parts:
        res["encode"] = encode(a, torch, D, dev)
    if "reads" in parts:
        res["reads"] = reads(a, torch, C, D, dev)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
