"""Measurements of DESIGN.md 12e (seekable Zstd objects): sizes, encode rates,
reads from the middle of 4 MiB objects, and a lone whole-object decode.

    python scripts/seek_rate.py [--out profiles/seekable/rates.json] [--frames 1024]

Everything runs in one process on device 0: medians of 7 repetitions after 2
warm-ups, the two sides of every comparison interleaved, wall clock around
calls that end synchronised.  Every decoded byte is compared with the input
once, outside the timed region."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from juicefs_amd import _lib as L  # noqa: E402
from juicefs_amd import compress as C  # noqa: E402
from juicefs_amd import device as D  # noqa: E402
from juicefs_amd.blockgen import gen_block  # noqa: E402

MIB4 = 4 << 20
REPS, WARM = 7, 2


def text(seed, n=MIB4):
    buf = ctypes.create_string_buffer(n)
    L.load().jfs_gen_block_host(ctypes.addressof(buf), n, b"T", seed)
    return buf.raw


def med(samples):
    s = sorted(samples)
    return {"median_ms": round(statistics.median(s) * 1e3, 3), "min_ms": round(s[0] * 1e3, 3),
            "max_ms": round(s[-1] * 1e3, 3)}


def interleaved(fns):
    """fns: name -> callable that ends synchronised; -> name -> med()"""
    t = {k: [] for k in fns}
    for r in range(WARM + REPS):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            if r >= WARM:
                t[k].append(time.perf_counter() - t0)
    return {k: med(v) for k, v in t.items()}


def device_encode(dev, n):
    """n text blocks in HBM (16 different ones, repeated) and room for their objects"""
    base = torch.from_numpy(np.frombuffer(b"".join(text(1 + i) for i in range(min(n, 16))), dtype=np.uint8).copy()).to(dev)
    src = base.repeat(-(-n // 16))[:n * MIB4].contiguous() if n > 16 else base
    cap = D.zstd_bound(MIB4)
    dst = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
    desc = D.make_desc(src, [i * MIB4 for i in range(n)], [MIB4] * n, dst, [i * cap for i in range(n)], [cap] * n)
    ret = torch.zeros(n, dtype=torch.int32, device=dev)

    def run(fn):
        fn(desc, ret)
        torch.cuda.synchronize()
    return run, ret, dst, cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seekable", "rates.json"))
    ap.add_argument("--frames", type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    z = C.ZStandard()
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmups": WARM}

    # ---- sizes
    sizes = {}
    for name, raw in (("T 4 MiB seed 1", text(1)), ("T-200003", gen_block("T", 21, 200003))):
        out = {}
        for mode in ("fast", "seekable"):
            with C.zstd_parse_mode(mode):
                d = bytearray(z.CompressBound(len(raw)))
                n, err = z.Compress(d, raw)
            assert err is None
            back = bytearray(len(raw))
            m, err = z.Decompress(back, bytes(d[:n]))
            assert err is None and bytes(back) == raw
            out[mode] = n
        nb = -(-len(raw) // (128 << 10))
        out["ratio"] = round(out["seekable"] / out["fast"], 5)
        out["bytes_per_extra_frame"] = round((out["seekable"] - out["fast"] - 17 - 8) / max(nb - 1, 1), 2)
        sizes[name] = out
    res["sizes"] = sizes

    # ---- encode rates, in HBM
    enc = {}
    for nfr in (1, a.frames):
        run, ret, dst, cap = device_encode(dev, nfr)
        r = interleaved({"fast": lambda: run(D.zstd_compress_fast), "seekable": lambda: run(D.zstd_compress_seekable)})
        for k in r:
            r[k]["GiB_s"] = round(nfr * MIB4 / (r[k]["median_ms"] / 1e3) / 2**30, 2)
        enc[f"{nfr} frames T"] = r
        assert (ret > 0).all()
        del dst
    res["encode"] = enc

    # ---- reads: 64 sources x 4 MiB, one 128 KiB read per source
    ns, rd = 64, 128 << 10
    raws = [text(100 + i) for i in range(ns)]

    def stored(mode):
        with C.zstd_parse_mode(mode):
            pairs = [(bytearray(z.CompressBound(MIB4)), r) for r in raws]
            out = z.CompressBatch(pairs)
        return [bytes(d[:n]) for (d, _), (n, e) in zip(pairs, out)]
    fast, seek = stored("fast"), stored("seekable")
    rng = random.Random(12)
    reads = {}
    for where, offs in (("uniform offset", [rng.randrange(0, MIB4 - rd + 1) for _ in range(ns)]),
                        ("last 128 KiB", [MIB4 - rd] * ns)):
        plan = (list(range(ns + 1)), [(i, offs[i], 0, rd) for i in range(ns)])
        bufs = [bytearray(rd) for _ in range(ns)]

        def call(objs, dmode, smode):
            C.set_read_decode_mode(dmode)
            C.set_read_seek_mode(smode)
            try:
                sres, rres, _ = z.ReadBatch([(o, MIB4) for o in objs], bufs, plan)
            finally:
                C.set_read_decode_mode("full")
                C.set_read_seek_mode("off")
            assert all(e is None for _, e in rres)
            return sres
        for objs, dm, sm in ((fast, "prefix-all", "off"), (seek, "full", "on"), (fast, "full", "off")):
            call(objs, dm, sm)
            assert all(bytes(b) == raws[i][offs[i]:offs[i] + rd] for i, b in enumerate(bufs))
        r = interleaved({"fast frames, prefix-all": lambda: call(fast, "prefix-all", "off"),
                         "seekable, seek on": lambda: call(seek, "full", "on"),
                         "fast frames, full": lambda: call(fast, "full", "off")})
        reads[where] = r
    res["reads"] = reads
    res["reads_stored_bytes"] = {"fast": sum(map(len, fast)), "seekable": sum(map(len, seek))}

    # ---- a lone whole-object decode
    raw, so, fo = raws[0], seek[0], fast[0]
    out = bytearray(MIB4)
    src_t = torch.from_numpy(np.frombuffer(so, dtype=np.uint8).copy()).to(dev)
    dst_t = torch.zeros(MIB4, dtype=torch.uint8, device=dev)
    desc = D.make_desc(src_t, [0], [len(so)], dst_t, [0], [MIB4])
    ret = torch.zeros(1, dtype=torch.int32, device=dev)
    lo = torch.zeros(1, dtype=torch.int32, device=dev)
    hi = torch.full((1,), MIB4, dtype=torch.int32, device=dev)

    def one_call(obj):
        m, err = z.Decompress(out, obj)
        assert err is None and m == MIB4

    def ranged():
        D.zstd_decompress_range(desc, lo, hi, ret)
        torch.cuda.synchronize()

    def full_dev():
        D.zstd_decompress_sync(desc, ret)
    ranged()
    assert int(ret[0]) == MIB4 and dst_t.cpu().numpy().tobytes() == raw
    res["lone decode"] = interleaved({"seekable, jfs_decompress": lambda: one_call(so),
                                      "seekable, range_device [0, cap), in HBM": ranged,
                                      "seekable, jfs_zstd_decompress_device, in HBM": full_dev,
                                      "fast frame, jfs_decompress": lambda: one_call(fo)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
