#!/usr/bin/env python3
"""What splicing untouched frames buys the sealed Zstd compaction call (DESIGN
11e): scripts/compact_splice_rate.py's three plans -- one 4 KiB overwrite per
block, identity, shifted by 4 KiB -- over 64 text-class sources of 4 MiB stored
as seekable objects inside AES-256-GCM envelopes, one output per source,
jfs_compact_seal_batch from host buffers on one GPU.

Per plan the switch off and all are interleaved call by call; medians of --reps
calls after --warmup calls, with min and max, the counters of one call, and the
ratio off / all.  --root DIR imports juicefs_amd from another checkout (the
parent commit, for the baseline): a package that does not know "all" runs only
the "off" legs.  Needs a GPU; writes one JSON file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from compact_splice_rate import K4, NSRC, U, plans  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--root", default=ROOT, help="the checkout whose juicefs_amd is measured")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seekable", "rates_splice_seal.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from juicefs_amd import _lib as L
    from juicefs_amd import compress as C
    from juicefs_amd import device as D
    from juicefs_amd import encrypt as E
    assert torch.cuda.is_available(), "compact_splice_seal_rate.py measures on a GPU"
    has_all = hasattr(L, "COMPACT_SPLICE_ALL")
    algo = E.AES256GCM_RSA
    dev = torch.device("cuda:0")
    raw_t = torch.empty(NSRC * U, dtype=torch.uint8, device=dev)
    D.gen_blocks(raw_t, NSRC, U, "T", 7000)
    torch.cuda.synchronize()
    raw = raw_t.cpu().numpy()
    rng = np.random.default_rng(5)
    small = [rng.integers(0, 256, K4, dtype=np.uint8).tobytes() for _ in range(NSRC)]
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    C.set_zstd_parse_mode("seekable")
    blocks = [raw[i * U:(i + 1) * U] for i in range(NSRC)] + small
    sp = [(rb(32), rb(12), rb(256)) for _ in blocks]  # an RSA-2048 wrapped key
    op = [(rb(32), rb(12), rb(256)) for _ in range(NSRC)]
    sd = [bytearray(E.envelope_bound(L.ALGO_ZSTD, len(b), 256)) for b in blocks]
    r = E.compress_seal_batch(L.ALGO_ZSTD, algo, list(zip(sd, blocks)), sp)
    assert all(e is None for _, e in r)
    envs = [bytes(sd[i][:r[i][0]]) for i in range(len(blocks))]
    sources = [(e, U) for e in envs[:NSRC]] + [(e, K4) for e in envs[NSRC:]]
    keys = [p[0] for p in sp]
    dst = [bytearray(E.envelope_bound(L.ALGO_ZSTD, U, 256)) for _ in range(NSRC)]
    res = {"label": a.label, "cipher": "aes256gcm",
           "shape": {"sources": NSRC, "block_bytes": U, "frame_bytes": 128 << 10,
                     "stored_source_bytes": sum(len(s) for s in envs[:NSRC])},
           "reps": a.reps, "warmup": a.warmup, "plans": {}}
    modes = ("off", "all") if has_all else ("off",)
    for name, plan in plans().items():
        t = {m: [] for m in modes}
        counts, sizes = None, {}
        for it in range(a.warmup + a.reps):
            for mode in modes:
                if has_all:
                    C.set_compact_splice_mode(mode)
                    C.compact_splice_counts(reset=True)
                t0 = time.perf_counter()
                sres, ores = E.compact_seal_batch(L.ALGO_ZSTD, algo, sources, keys, dst, op, plan)
                dt = (time.perf_counter() - t0) * 1e3
                assert all(e is None for _, e in sres + ores), (name, mode)
                sizes[mode] = sum(n for n, _ in ores)
                if mode == "all":
                    counts = C.compact_splice_counts()
                if it >= a.warmup:
                    t[mode].append(dt)
        leg = {"stored_output_bytes": sizes}
        for mode, xs in t.items():
            leg[mode] = {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs),
                         "gib_s_gathered": NSRC * U / 2**30 / (statistics.median(xs) / 1e3)}
        if has_all:
            leg["counts_of_one_call"] = dict(zip(("outputs_spliced", "frames_passed", "frames_reencoded", "bytes_passed"), counts))
            leg["off_over_all"] = leg["off"]["median_ms"] / leg["all"]["median_ms"]
        res["plans"][name] = leg
    if has_all:
        C.set_compact_splice_mode("off")
    C.set_zstd_parse_mode("exact")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
