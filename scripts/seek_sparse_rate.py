"""Measurements of DESIGN.md 12g (sparse range decode in the read calls): 64
text sources of 4 MiB from host buffers, read with JFS_READ_SEEK = off, on and
sparse in the same run, for 8-byte and 12-byte seekable objects.

    python scripts/seek_sparse_rate.py [--out profiles/seekable/rates_sparse.json]

Two plans: two 4 KiB reads per source, one in its first frame and one in its
last (the fragmented batch), and one contiguous 128 KiB read per source (where
sparse should cost no more than on).  One process on device 0: medians of 7
repetitions after 2 warm-ups, the sides interleaved, wall clock around calls
that end synchronised, min and max recorded.  Every read is compared with the
input once, outside the timed region, and jfs_zstd_sparse_counts is recorded
for one sparse call of every case."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from juicefs_amd import _lib as L  # noqa: E402
from juicefs_amd import compress as C  # noqa: E402
from juicefs_amd import device as D  # noqa: E402

MIB4 = 4 << 20
REPS, WARM = 7, 2
NS, KIB4, KIB128 = 64, 4 << 10, 128 << 10


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seekable", "rates_sparse.json"))
    a = ap.parse_args()
    z = C.ZStandard()
    res = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmups": WARM, "sources": NS}
    raws = [text(300 + i) for i in range(NS)]

    def stored(csum):
        prev = C.set_zstd_seek_csum_mode("on" if csum else "off")
        try:
            with C.zstd_parse_mode("seekable"):
                pairs = [(bytearray(z.CompressBound(MIB4)), r) for r in raws]
                out = z.CompressBatch(pairs)
        finally:
            C.set_zstd_seek_csum_mode(prev)
        assert all(e is None for _, e in out)
        return [bytes(d[:n]) for (d, _), (n, _) in zip(pairs, out)]
    objs = {"8-byte tables": stored(False), "12-byte tables": stored(True)}
    res["stored_bytes"] = {k: sum(map(len, v)) for k, v in objs.items()}

    plans = {
        # read 2 i: source i's first frame; read 2 i + 1: its last
        "two 4 KiB reads per source, first and last frame":
            (list(range(2 * NS + 1)), [(i // 2, 1000 if i % 2 == 0 else MIB4 - KIB4 - 1000, 0, KIB4) for i in range(2 * NS)],
             KIB4),
        "one contiguous 128 KiB read per source":
            (list(range(NS + 1)), [(i, 17 * KIB128 + 5000, 0, KIB128) for i in range(NS)], KIB128),
    }
    res["reads"] = {}
    for pname, (seg_first, seg, rd) in plans.items():
        bufs = [bytearray(rd) for _ in range(len(seg))]
        for oname, oo in objs.items():
            def call(smode):
                C.set_read_seek_mode(smode)
                try:
                    sres, rres, _ = z.ReadBatch([(o, MIB4) for o in oo], bufs, (seg_first, seg), device_mask=1)
                finally:
                    C.set_read_seek_mode("off")
                assert all(e is None for _, e in rres) and all(e is None for _, e in sres)
            counts = {}
            for sm in ("off", "on", "sparse"):
                for b in bufs:
                    b[:] = bytes(rd)
                D.zstd_sparse_counts(reset=True)
                call(sm)
                counts[sm] = D.zstd_sparse_counts()
                assert all(bytes(b) == raws[s[0]][s[1]:s[1] + rd] for b, s in zip(bufs, seg)), (pname, oname, sm)
            r = interleaved({"off": lambda: call("off"), "on": lambda: call("on"), "sparse": lambda: call("sparse")})
            r["sparse_counts"] = {"inputs through a table": counts["sparse"][0], "frames selected": counts["sparse"][1],
                                  "frames compared": counts["sparse"][2]}
            r["sparse_over_on"] = round(r["sparse"]["median_ms"] / r["on"]["median_ms"], 3)
            res["reads"][f"{pname}; {oname}"] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
