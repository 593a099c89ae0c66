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
      in HBM, under device events;
  (d) --decode full|prefix [...]: jfs_read_batch (LZ4, no checksums) in each
      listed decode mode (JFS_READ_DECODE), in the order given, on three
      workloads: (a)'s 64 sources (the small-batch decoder), the same reads out
      of 256 sources (more than JFS_LZ4_SPLIT_MAX: the one-workgroup kernel),
      and 64 sources with every segment ending at its block's last byte
      (need == dst_cap everywhere: prefix mode takes the full launchers).
      --only-decode skips (a)-(c).
  (e) --zstd-front (with --decode full prefix-all): Zstd sources, modes
      alternating call by call in one process, on two workloads: "front" -- one
      128 KiB read from offset 0 of each of 64 sources x 4 MiB, what sequential
      readers and the prefetcher produce -- and (a)'s random reads.  Beside the
      call's wall time: the decode stage alone under device events
      (jfs_zstd_decompress_device against jfs_zstd_decompress_prefix_device on
      the staged sources), and the Zstd blocks walked against the blocks in the
      frames (jfs_zstd_plan_host_prefix).  Runs alone, like --only-decode.

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


def plan(seed=2025, nsrc=NSRC, tail=False):
    """tail: every segment ends at its block's last byte, and the sources take turns"""
    rng = np.random.default_rng(seed)
    seg_first, seg = [0], []
    for _ in range(NREAD):
        k = int(rng.integers(2, 5))
        cuts = sorted(int(x) for x in rng.choice(np.arange(1, READ), size=k - 1, replace=False))
        at = 0
        for end in cuts + [READ]:
            n = end - at
            if tail:
                seg.append((len(seg) % nsrc, U - n, at, n))
            else:
                seg.append((int(rng.integers(0, nsrc)), int(rng.integers(0, U - n + 1)), at, n))
            at = end
        seg_first.append(len(seg))
    return seg_first, seg


def decode_modes(a, res):
    """(d): ReadBatch (LZ4) per workload and decode mode"""
    import torch
    from juicefs_amd import compress as C
    from juicefs_amd import device as D
    dev = torch.device("cuda:0")
    c = C.NewCompressor("lz4")
    out = {}
    for wname, nsrc, tail in (("sources_64", 64, False), ("sources_256", 256, False), ("tail_64", 64, True)):
        raw_t = torch.empty(nsrc * U, dtype=torch.uint8, device=dev)
        D.gen_blocks(raw_t, nsrc, U, "T", 7000)
        torch.cuda.synchronize()
        raw = raw_t.cpu().numpy()
        del raw_t
        seg_first, seg = plan(nsrc=nsrc, tail=tail)
        want = [np.empty(READ, dtype=np.uint8) for _ in range(NREAD)]
        slice_reads([raw[i * U:(i + 1) * U] for i in range(nsrc)], seg_first, seg, want)
        sd = [bytearray(c.CompressBound(U)) for _ in range(nsrc)]
        r = c.CompressBatch([(sd[i], raw[i * U:(i + 1) * U]) for i in range(nsrc)])
        assert all(e is None for _, e in r)
        srcs = [(bytes(sd[i][:r[i][0]]), U) for i in range(nsrc)]
        need = [0] * nsrc
        for src, so, _, n in seg:
            need[src] = max(need[src], so + n)
        dst = [np.empty(READ, dtype=np.uint8) for _ in range(NREAD)]
        w = {"sources": nsrc, "segments": len(seg), "decoded_bytes_full": nsrc * U, "decoded_bytes_needed": sum(need)}
        for mode in a.decode:
            prev = C.set_read_decode_mode(mode)
            try:
                ms = []
                for it in range(a.warmup + a.reps):
                    t0 = time.perf_counter()
                    sres, rres, _ = c.ReadBatch(srcs, dst, (seg_first, seg))
                    t1 = time.perf_counter()
                    assert all(e is None for _, e in sres + rres)
                    if it == 0:
                        assert [n for n, _ in sres] == (need if mode != "full" else [U] * nsrc)
                        for j in range(NREAD):
                            assert np.array_equal(dst[j], want[j]), (wname, mode, j)
                    if it >= a.warmup:
                        ms.append((t1 - t0) * 1e3)
            finally:
                C.set_read_decode_mode(prev)
            w[mode] = {"read_batch_ms": med(ms), "min_ms": min(ms), "max_ms": max(ms)}
        if "full" in w and "prefix" in w:
            w["prefix_over_full"] = w["prefix"]["read_batch_ms"] / w["full"]["read_batch_ms"]
        out[wname] = w
    res["decode_modes"] = out


def zstd_front(a, res):
    """(e): ReadBatch on Zstd sources, full and prefix-all alternating"""
    import ctypes
    import struct
    import torch
    from juicefs_amd import compress as C
    from juicefs_amd import device as D
    from juicefs_amd import _lib as L
    lib = L.load()
    lib.jfs_zstd_plan_host_prefix.restype = None
    dev = torch.device("cuda:0")
    c = C.NewCompressor("zstd")
    raw_t = torch.empty(NSRC * U, dtype=torch.uint8, device=dev)
    D.gen_blocks(raw_t, NSRC, U, "T", 7000)
    torch.cuda.synchronize()
    raw = raw_t.cpu().numpy()
    del raw_t
    sd = [bytearray(c.CompressBound(U)) for _ in range(NSRC)]
    r = c.CompressBatch([(sd[i], raw[i * U:(i + 1) * U]) for i in range(NSRC)])
    assert all(e is None for _, e in r)
    stored = [bytes(sd[i][:r[i][0]]) for i in range(NSRC)]
    srcs = [(s, U) for s in stored]
    modes = [m for m in a.decode if m in ("full", "prefix-all")]
    assert modes, "--zstd-front measures the modes full and prefix-all"
    out = {}
    for wname in ("front", "random"):
        if wname == "front":
            seg_first, seg = list(range(NSRC + 1)), [(i, 0, 0, READ) for i in range(NSRC)]
        else:
            seg_first, seg = plan()
        nread = len(seg_first) - 1
        need = [0] * NSRC
        for src, so, _, n in seg:
            need[src] = max(need[src], so + n)
        dst = [np.empty(READ, dtype=np.uint8) for _ in range(nread)]
        want = [np.empty(READ, dtype=np.uint8) for _ in range(nread)]
        for j in range(nread):
            for src, so, do, n in seg[seg_first[j]:seg_first[j + 1]]:
                want[j][do:do + n] = raw[src * U + so:src * U + so + n]
        # blocks walked against blocks in the frames (host plan)
        walked = total = 0
        for s, nd in zip(stored, need):
            buf = ctypes.create_string_buffer(s, len(s))
            for w, acc in ((nd, "walked"), (U, "total")):
                info, tot = ctypes.create_string_buffer(64), (ctypes.c_uint64 * 6)()
                lib.jfs_zstd_plan_host_prefix((ctypes.c_void_p * 1)(ctypes.addressof(buf)), (ctypes.c_int32 * 1)(len(s)),
                                              (ctypes.c_int32 * 1)(U), (ctypes.c_int32 * 1)(w), 1, info, tot)
                nb = struct.unpack_from("<I", info.raw, 52)[0]
                if acc == "walked":
                    walked += nb
                else:
                    total += nb
        w = {"sources": NSRC, "reads": nread, "segments": len(seg), "decoded_bytes_full": NSRC * U,
             "decoded_bytes_needed": sum(need), "zstd_blocks_in_frames": total, "zstd_blocks_walked": walked}
        ms = {m: [] for m in modes}
        for it in range(a.warmup + a.reps):
            for mode in modes:  # alternating
                prev = C.set_read_decode_mode(mode)
                try:
                    t0 = time.perf_counter()
                    sres, rres, _ = c.ReadBatch(srcs, dst, (seg_first, seg))
                    t1 = time.perf_counter()
                finally:
                    C.set_read_decode_mode(prev)
                assert all(e is None for _, e in sres + rres)
                if it == 0:
                    assert [n for n, _ in sres] == ([min(U, x) for x in need] if mode == "prefix-all" else [U] * NSRC)
                    for j in range(nread):
                        assert np.array_equal(dst[j], want[j]), (wname, mode, j)
                if it >= a.warmup:
                    ms[mode].append((t1 - t0) * 1e3)
        for m in modes:
            w[m] = {"read_batch_ms": med(ms[m]), "min_ms": min(ms[m]), "max_ms": max(ms[m])}
        # the decode stage alone, sources staged in HBM, device events
        offs, o = [], 0
        for s in stored:
            offs.append(o)
            o = (o + len(s) + 15) & ~15
        host = np.zeros(o + 64, dtype=np.uint8)
        for s, q in zip(stored, offs):
            host[q:q + len(s)] = np.frombuffer(s, dtype=np.uint8)
        src_t = torch.from_numpy(host).to(dev)
        dst_t = torch.empty(NSRC * U, dtype=torch.uint8, device=dev)
        desc = D.make_desc(src_t, offs, [len(s) for s in stored], dst_t, np.arange(NSRC, dtype=np.int64) * U, [U] * NSRC)
        ret = torch.empty(NSRC, dtype=torch.int32, device=dev)
        want_t = torch.tensor(need, dtype=torch.int32, device=dev)
        ev = {"full": [], "prefix-all": []}
        for it in range(a.warmup + a.reps):
            for mode in modes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if mode == "full":
                    D.zstd_decompress(desc, ret)
                else:
                    D.zstd_decompress_prefix(desc, want_t, ret)
                e1.record()
                torch.cuda.synchronize()
                assert ret.cpu().tolist() == ([U] * NSRC if mode == "full" else [min(U, x) for x in need])
                if it >= a.warmup:
                    ev[mode].append(e0.elapsed_time(e1))
        for m in modes:
            w[m].update({"decode_stage_ms": med(ev[m]), "decode_stage_min_ms": min(ev[m]), "decode_stage_max_ms": max(ev[m])})
        if len(modes) == 2:
            w["prefix_all_over_full"] = w["prefix-all"]["read_batch_ms"] / w["full"]["read_batch_ms"]
            w["decode_stage_prefix_all_over_full"] = w["prefix-all"]["decode_stage_ms"] / w["full"]["decode_stage_ms"]
        out[wname] = w
    res["zstd_front"] = out


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
    ap.add_argument("--decode", nargs="+", choices=["full", "prefix", "prefix-all"], default=["full"],
                    help="decode modes of the read calls to measure in (d), in this order")
    ap.add_argument("--only-decode", action="store_true", help="measure (d) alone")
    ap.add_argument("--zstd-front", action="store_true", help="measure (e) alone: Zstd, full against prefix-all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_assembly", "read_rate.json"))
    a = ap.parse_args()
    import torch
    from juicefs_amd import compress as C
    from juicefs_amd import device as D
    from juicefs_amd import _lib as L
    assert torch.cuda.is_available(), "read_rate.py measures on a GPU"
    dev = torch.device("cuda:0")
    if a.zstd_front:
        res = {"shape": {"block_bytes": U, "read_bytes": READ}, "reps": a.reps, "warmup": a.warmup}
        zstd_front(a, res)
        return write(a, res)
    if a.only_decode:
        res = {"shape": {"block_bytes": U, "reads": NREAD, "read_bytes": READ, "gathered_bytes": NREAD * READ},
               "reps": a.reps, "warmup": a.warmup}
        decode_modes(a, res)
        return write(a, res)
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
    decode_modes(a, res)
    write(a, res)


def write(a, res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
