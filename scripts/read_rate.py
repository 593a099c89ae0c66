#!/usr/bin/env python3
"""What on-device read assembly buys: 256 fragmented reads of
128 KiB (2 to 4 segments each, at random offsets of random blocks, fixed seed)
out of 64 text-class source blocks x 4 MiB, on one GPU.

  (a) jfs_read_batch (ReadBatch), LZ4 and Zstd: wall time per call, with and
      without the CRC-32C check of every source;
  (b) the same reads on the batch ABI without it: DecompressBatch of the 64
      blocks, then numpy slicing on the host -- with the two stage times;
  (c) the flat-grid gather kernel alone (jfs_read_gather_device) against the
      2-D grid (jfs_gather_device) on the same plan, sources already decoded
      in HBM, under device events.

Medians of --reps calls after --warmup calls, one process.  Needs a GPU;
writes one JSON file."""
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
NSRC, NREAD, READ = 64, 256, 128 << 10


def plan(seed=2025):
    rng = np.random.default_rng(seed)
    seg_first, seg = [0], []
    for _ in range(NREAD):
        k = int(rng.integers(2, 5))
        cuts = sorted(int(x) for x in rng.choice(np.arange(1, READ), size=k - 1, replace=False))
        at = 0
        for end in cuts + [READ]:
            n = end - at
            seg.append((int(rng.integers(0, NSRC)), int(rng.integers(0, U - n + 1)), at, n))
            at = end
        seg_first.append(len(seg))
    return seg_first, seg


def slice_reads(dec, seg_first, seg, outs):
    for j in range(NREAD):
        o = outs[j]
        for src, so, do, n in seg[seg_first[j]:seg_first[j + 1]]:
            o[do:do + n] = dec[src][so:so + n]


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_assembly", "read_rate.json"))
    a = ap.parse_args()
    import torch
    from juicefs_amd import compress as C
    from juicefs_amd import device as D
    from juicefs_amd import _lib as L
    assert torch.cuda.is_available(), "read_rate.py measures on a GPU"
    dev = torch.device("cuda:0")
    raw_t = torch.empty(NSRC * U, dtype=torch.uint8, device=dev)
    D.gen_blocks(raw_t, NSRC, U, "T", 7000)
    torch.cuda.synchronize()
    raw = raw_t.cpu().numpy()
    seg_first, seg = plan()
    want = [np.empty(READ, dtype=np.uint8) for _ in range(NREAD)]
    slice_reads([raw[i * U:(i + 1) * U] for i in range(NSRC)], seg_first, seg, want)
    res = {"shape": {"sources": NSRC, "block_bytes": U, "reads": NREAD, "read_bytes": READ, "segments": len(seg),
                     "gathered_bytes": NREAD * READ}, "reps": a.reps, "warmup": a.warmup}
    for name in ("lz4", "zstd"):
        c = C.NewCompressor(name)
        bound = c.CompressBound(U)
        sd = [bytearray(bound) for _ in range(NSRC)]
        r = c.CompressBatchChecksum([(sd[i], raw[i * U:(i + 1) * U]) for i in range(NSRC)])
        assert all(e is None for _, e, _ in r)
        stored = [bytes(sd[i][:r[i][0]]) for i in range(NSRC)]
        crcs = [x[2] for x in r]
        dst_a = [np.empty(READ, dtype=np.uint8) for _ in range(NREAD)]
        dst_b = [np.empty(READ, dtype=np.uint8) for _ in range(NREAD)]
        dec = [np.empty(U, dtype=np.uint8) for _ in range(NSRC)]
        srcs = [(s, U) for s in stored]
        ta, tac, tb, tdec, tsl = [], [], [], [], []
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            sres, rres, _ = c.ReadBatch(srcs, dst_a, (seg_first, seg))
            t1 = time.perf_counter()
            sres2, rres2, got = c.ReadBatch(srcs, dst_a, (seg_first, seg), crcs=crcs)
            t2 = time.perf_counter()
            dres = c.DecompressBatch(list(zip(dec, stored)))
            t3 = time.perf_counter()
            slice_reads(dec, seg_first, seg, dst_b)
            t4 = time.perf_counter()
            assert all(e is None for _, e in sres + rres + sres2 + rres2 + dres) and got == crcs
            if it == 0:  # same bytes either way
                for j in range(NREAD):
                    assert np.array_equal(dst_a[j], want[j]) and np.array_equal(dst_b[j], want[j]), (name, j)
            if it >= a.warmup:
                ta.append((t1 - t0) * 1e3)
                tac.append((t2 - t1) * 1e3)
                tb.append((t4 - t2) * 1e3)
                tdec.append((t3 - t2) * 1e3)
                tsl.append((t4 - t3) * 1e3)
        res[name] = {
            "a_read_batch_ms": med(ta), "a_min_ms": min(ta), "a_max_ms": max(ta),
            "a_with_crc_ms": med(tac), "a_with_crc_min_ms": min(tac), "a_with_crc_max_ms": max(tac),
            "b_parent_abi_ms": med(tb), "b_min_ms": min(tb), "b_max_ms": max(tb),
            "b_decompress_batch_ms": med(tdec), "b_numpy_slicing_ms": med(tsl),
            "a_over_b": med(ta) / med(tb), "a_with_crc_over_b": med(tac) / med(tb),
            "stored_source_bytes": sum(len(s) for s in stored),
        }
    # (c) the two gather grids alone, sources already decoded in HBM
    offs = np.arange(NSRC, dtype=np.int64) * U
    sdesc = D.make_desc(raw_t, offs, [U] * NSRC, raw_t, offs, [U] * NSRC)
    src_n = torch.full((NSRC,), U, dtype=torch.int32, device=dev)
    gat = torch.empty(NREAD * READ, dtype=torch.uint8, device=dev)
    caps = [READ] * NREAD
    odesc, sdev = D.make_compact_desc(gat, np.arange(NREAD, dtype=np.int64) * READ, caps, seg_first, seg)
    ret = torch.empty(NREAD, dtype=torch.int32, device=dev)

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

    def check():
        assert ret.cpu().tolist() == caps
        assert np.array_equal(gat.cpu().numpy(), np.concatenate(want))
        gat.zero_()

    flat = timed(lambda: D.read_gather(sdesc, src_n, odesc, sdev, caps, ret))
    check()
    grid = timed(lambda: D.gather(sdesc, src_n, odesc, sdev, READ, ret))
    check()
    # the mixed shape the flat grid is for: the same reads plus one of 4 MiB
    big = torch.empty(U, dtype=torch.uint8, device=dev)
    o2 = np.frombuffer(odesc.cpu().numpy().tobytes(), dtype=D.COMPACT_OUT_DTYPE).copy()
    extra = np.zeros(1, dtype=D.COMPACT_OUT_DTYPE)
    extra["dst"], extra["dst_cap"], extra["seg_first"], extra["seg_count"] = big.data_ptr(), U, len(seg), 1
    o2 = torch.from_numpy(np.concatenate([o2, extra]).view(np.uint8).copy()).to(dev)
    s2 = np.frombuffer(sdev.cpu().numpy().tobytes(), dtype=D.SEG_DTYPE)[:len(seg)].copy()
    one = np.zeros(1, dtype=D.SEG_DTYPE)
    one["src"], one["src_off"], one["dst_off"], one["len"] = 3, 0, 0, U
    s2 = torch.from_numpy(np.concatenate([s2, one]).view(np.uint8).copy()).to(dev)
    ret2 = torch.empty(NREAD + 1, dtype=torch.int32, device=dev)
    caps2 = caps + [U]
    flat2 = timed(lambda: D.read_gather(sdesc, src_n, o2, s2, caps2, ret2))
    grid2 = timed(lambda: D.gather(sdesc, src_n, o2, s2, U, ret2))
    assert ret2.cpu().tolist() == caps2 and np.array_equal(big.cpu().numpy(), raw[3 * U:4 * U])
    gib = NREAD * READ / 2**30
    res["gather"] = {
        "c_flat_ms": med(flat), "c_flat_min_ms": min(flat), "c_flat_max_ms": max(flat),
        "c_grid2d_ms": med(grid), "c_grid2d_min_ms": min(grid), "c_grid2d_max_ms": max(grid),
        "c_flat_over_grid2d": med(flat) / med(grid), "flat_gib_s_out": gib / (med(flat) / 1e3),
        "mixed_flat_ms": med(flat2), "mixed_flat_min_ms": min(flat2), "mixed_flat_max_ms": max(flat2),
        "mixed_grid2d_ms": med(grid2), "mixed_grid2d_min_ms": min(grid2), "mixed_grid2d_max_ms": max(grid2),
        "mixed_flat_over_grid2d": med(flat2) / med(grid2),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
