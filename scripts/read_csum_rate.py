#!/usr/bin/env python3
"""What the read calls' disk-cache checksums cost and save: the
workload of read_rate.py (64 text-class source blocks x 4 MiB, fragmented reads
of 128 KiB, fixed seed) with 16 of the 256 reads replaced by whole-block cache
fills that want their checksums, on one GPU.

  (a) the single call: jfs_read_batch_csum (ReadBatch(with_csum=...)), LZ4 and
      Zstd, and jfs_read_open_batch_csum for LZ4 under AES-256-GCM;
  (b) what an adapter does without it: jfs_read_batch for the 240 reads plus
      jfs_decompress_batch_csum for the 16 blocks (sealed: jfs_read_open_batch
      plus jfs_open_decompress_batch, the 16 blocks' checksums on a host core
      NOT counted);
  (c) the kernel alone under device events: read_csum_flat_kernel
      (jfs_read_csum_device) against jfs_crc32c_device with seg_bytes = 32768,
      one workgroup per read, over the same packed bytes in HBM:
      16 x 4 MiB plus 240 x 128 KiB.

Wall times are medians of --reps calls after --warmup calls, one process.
Needs a GPU; writes one JSON file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.read_rate import NREAD, NSRC, READ, U, plan, slice_reads  # noqa: E402

NFILL = 16
PIECE = 32 << 10


def med(xs):
    return statistics.median(xs)


def stats(xs):
    return {"ms": med(xs), "min_ms": min(xs), "max_ms": max(xs)}


def fill_plan():
    """read_rate's plan with its last NFILL reads replaced by whole blocks 0 .. NFILL-1"""
    seg_first, seg = plan()
    nfrag = NREAD - NFILL
    seg = list(seg[:seg_first[nfrag]])
    seg_first = list(seg_first[:nfrag + 1])
    for i in range(NFILL):
        seg.append((i, 0, 0, U))
        seg_first.append(len(seg))
    return seg_first, seg, nfrag


def host_legs(a, res, oracle, raw):
    from juicefs_amd import compress as C
    from juicefs_amd import encrypt as E
    seg_first, seg, nfrag = fill_plan()
    blocks = [raw[i * U:(i + 1) * U] for i in range(NSRC)]
    want = [np.empty(READ, dtype=np.uint8) for _ in range(NREAD)]
    slice_reads(blocks, seg_first[:nfrag + 1] + [seg_first[nfrag]] * NFILL, seg, want)  # the fragmented reads only
    want_cs = [oracle.crc32c_segments(blocks[i].tobytes()) for i in range(NFILL)]
    flags = [False] * nfrag + [True] * NFILL
    frag_plan = (seg_first[:nfrag + 1], seg[:seg_first[nfrag]])
    rng = np.random.default_rng(11)
    for name in ("lz4", "zstd", "lz4_aes256gcm"):
        sealed = name.endswith("aes256gcm")
        c = C.NewCompressor(name.split("_")[0])
        if sealed:
            algo = E.AES256GCM_RSA
            params = [(rng.bytes(32), rng.bytes(12), rng.bytes(256)) for _ in range(NSRC)]
            sd = [bytearray(E.envelope_bound(c.algo, U, 256)) for _ in range(NSRC)]
            r = E.compress_seal_batch(c.algo, algo, list(zip(sd, blocks)), params)
            keys = [p[0] for p in params]
        else:
            sd = [bytearray(c.CompressBound(U)) for _ in range(NSRC)]
            r = c.CompressBatch(list(zip(sd, blocks)))
        assert all(e is None for _, e in r)
        stored = [bytes(sd[i][:r[i][0]]) for i in range(NSRC)]
        srcs = [(s, U) for s in stored]
        dst_a = [np.empty(READ, dtype=np.uint8) for _ in range(nfrag)] + [np.empty(U, dtype=np.uint8) for _ in range(NFILL)]
        dst_b = [np.empty(READ, dtype=np.uint8) for _ in range(nfrag)]
        fill_b = [np.empty(U, dtype=np.uint8) for _ in range(NFILL)]
        ta, tb, tb_read, tb_fill = [], [], [], []
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            if sealed:
                sres, rres, _, cs = E.read_open_batch(c.algo, algo, srcs, keys, dst_a, (seg_first, seg), with_csum=flags)
            else:
                sres, rres, _, cs = c.ReadBatch(srcs, dst_a, (seg_first, seg), with_csum=flags)
            t1 = time.perf_counter()
            if sealed:
                sres2, rres2, _ = E.read_open_batch(c.algo, algo, srcs, keys, dst_b, frag_plan)
                t2 = time.perf_counter()
                back = E.open_decompress_batch(c.algo, algo, list(zip(fill_b, stored[:NFILL])), keys[:NFILL])
                cs_b = None
            else:
                sres2, rres2, _ = c.ReadBatch(srcs, dst_b, frag_plan)
                t2 = time.perf_counter()
                full = c.DecompressBatchChecksum(list(zip(fill_b, stored[:NFILL])))
                back, cs_b = [(n, e) for n, e, _ in full], [x for _, _, x in full]
            t3 = time.perf_counter()
            assert all(e is None for _, e in sres + rres + sres2 + rres2 + back)
            if it == 0:  # the same bytes and checksums either way, and the oracle's
                for j in range(nfrag):
                    assert np.array_equal(dst_a[j], want[j]) and np.array_equal(dst_b[j], want[j]), (name, j)
                for i in range(NFILL):
                    assert np.array_equal(dst_a[nfrag + i], blocks[i]) and np.array_equal(fill_b[i], blocks[i]), (name, i)
                assert cs[:nfrag] == [None] * nfrag and cs[nfrag:] == want_cs, name
                assert cs_b is None or cs_b == want_cs, name
            if it >= a.warmup:
                ta.append((t1 - t0) * 1e3)
                tb.append((t3 - t1) * 1e3)
                tb_read.append((t2 - t1) * 1e3)
                tb_fill.append((t3 - t2) * 1e3)
        res[name] = {"a_single_call": stats(ta), "b_two_calls": stats(tb), "b_read_batch_ms": med(tb_read),
                     "b_fill_batch_ms": med(tb_fill), "a_over_b": med(ta) / med(tb),
                     "b_counts_host_checksums": False if sealed else None,
                     "stored_source_bytes": sum(len(s) for s in stored)}


def kernel_leg(res, oracle, dev):
    """(c): both checksum kernels over 16 x 4 MiB + 240 x 128 KiB packed in HBM"""
    import torch
    from juicefs_amd import device as D
    totals = [U] * NFILL + [READ] * (NREAD - NFILL)
    offs = np.concatenate([[0], np.cumsum(totals[:-1])]).astype(np.int64)  # multiples of 128 KiB: 16-aligned
    gat = torch.empty(-(-sum(totals) // U) * U, dtype=torch.uint8, device=dev)
    D.gen_blocks(gat, len(gat) // U, U, "T", 9100)
    torch.cuda.synchronize()
    words = [(t - 1) // PIECE + 1 for t in totals]
    pf = np.concatenate([[0], np.cumsum(words)]).astype(np.int32)
    npiece = int(pf[-1])
    no = len(totals)
    odesc, _ = D.make_compact_desc(gat, offs, totals, list(range(no + 1)), [(-1, 0, 0, t) for t in totals])
    ret = torch.tensor(totals, dtype=torch.int32, device=dev)
    pf_t = torch.from_numpy(pf).to(dev)
    cs_flat = torch.zeros(4 * npiece, dtype=torch.uint8, device=dev)
    cs_blk = torch.zeros(4 * npiece, dtype=torch.uint8, device=dev)
    bdesc = D.make_desc(gat, offs, totals, cs_blk, 4 * pf[:-1].astype(np.int64), [4 * w for w in words])
    crc = torch.zeros(no, dtype=torch.int32, device=dev)
    bret = torch.zeros(no, dtype=torch.int32, device=dev)

    def timed(fn, reps=20, warm=3):
        ms = []
        for it in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warm:
                ms.append(e0.elapsed_time(e1))
        return ms

    flat = timed(lambda: D.read_csum(odesc, ret, pf_t, npiece, cs_flat))
    blk = timed(lambda: D.crc32c(bdesc, crc, bret, seg_bytes=PIECE))
    a, b = cs_flat.cpu().numpy(), cs_blk.cpu().numpy()
    assert bret.cpu().tolist() == [4 * w for w in words]
    assert np.array_equal(a, b), "the flat kernel and crc32c_kernel disagree"
    host = gat.cpu().numpy()
    for j in (0, NFILL - 1, NFILL, no - 1):  # and both are the oracle's
        assert a[4 * pf[j]:4 * pf[j + 1]].tobytes() == oracle.crc32c_segments(host[offs[j]:offs[j] + totals[j]].tobytes())
    gib = sum(totals) / 2**30
    res["kernel"] = {"reads": no, "pieces": npiece, "bytes": sum(totals),
                     "c_flat": stats(flat), "c_per_block": stats(blk), "c_flat_over_per_block": med(flat) / med(blk),
                     "flat_gib_s": gib / (med(flat) / 1e3), "per_block_gib_s": gib / (med(blk) / 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_csum", "read_rate.json"))
    a = ap.parse_args()
    import torch
    from juicefs_amd import device as D
    from tests.oracle_ctypes import Oracle
    assert torch.cuda.is_available(), "read_csum_rate.py measures on a GPU"
    dev = torch.device("cuda:0")
    oracle = Oracle(os.path.join(ROOT, "oracle", "_build", "liboracle.so"))
    raw_t = torch.empty(NSRC * U, dtype=torch.uint8, device=dev)
    D.gen_blocks(raw_t, NSRC, U, "T", 7000)
    torch.cuda.synchronize()
    raw = raw_t.cpu().numpy()
    del raw_t
    res = {"shape": {"sources": NSRC, "block_bytes": U, "reads": NREAD, "fragmented_reads": NREAD - NFILL,
                     "read_bytes": READ, "cache_fills": NFILL, "fill_bytes": U},
           "reps": a.reps, "warmup": a.warmup,
           "not_measured": ["concurrent callers", "data classes other than text", "more than one GPU"]}
    host_legs(a, res, oracle, raw)
    kernel_leg(res, oracle, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
