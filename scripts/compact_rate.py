#!/usr/bin/env python3
"""What on-device compaction buys: one synthetic compaction of 16
output blocks x 4 MiB out of 64 text-class source blocks x 4 MiB (about 25 % of
every source survives; segments of 4 KiB - 1 MiB from a fixed seed), on one GPU.

  (a) jfs_compact_batch (CompactBatch), LZ4 and Zstd: wall time per call;
  (b) the same work on the batch ABI without it: DecompressBatch, a numpy
      stitch on the host, CompressBatch -- with the three stage times;
  (c) the gather kernel alone under device events against a
      hipMemcpyDtoDAsync of the same number of bytes.

With --cipher NAME (aes256gcm-rsa, chacha20-rsa, sm4gcm) the same workload on
an encrypted volume instead: every stored object is an envelope,

  (a) jfs_compact_seal_batch (encrypt.compact_seal_batch): wall time per call;
  (b) open_decompress_batch, the numpy stitch, compress_seal_batch -- with the
      three stage times;

and (c) is left out (the gather kernel is the same).

Medians of --reps calls after --warmup calls.  Needs a GPU; writes one JSON file."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U = 4 << 20
NSRC, NOUT = 64, 16


def plan(seed=2024):
    rng = np.random.default_rng(seed)
    seg_first, seg = [0], []
    k = 0
    for _ in range(NOUT):
        at = 0
        while at < U:
            n = int(min(U - at, rng.integers(4 << 10, (1 << 20) + 1)))
            src = k % NSRC  # every source is used, about a quarter of each
            seg.append((src, int(rng.integers(0, U - n + 1)), at, n))
            at += n
            k += 1
        seg_first.append(len(seg))
    return seg_first, seg


def stitch(dec, seg_first, seg):
    outs = []
    for j in range(NOUT):
        o = np.empty(U, dtype=np.uint8)
        for src, so, do, n in seg[seg_first[j]:seg_first[j + 1]]:
            o[do:do + n] = dec[src][so:so + n]
        outs.append(o)
    return outs


def med(xs):
    return statistics.median(xs)


def sealed(a, raw, seg_first, seg, res):
    """legs (a) and (b) on an encrypted volume"""
    from juicefs_amd import _lib as L
    from juicefs_amd import encrypt as E
    rng = np.random.default_rng(99)
    klen = E.key_size(a.cipher)

    def params(n):  # (data key, nonce, wrapped key): a 256-byte wrap as RSA-2048 gives
        return [(rng.bytes(klen), rng.bytes(12), rng.bytes(256)) for _ in range(n)]
    res["cipher"] = a.cipher
    for name, algo in (("lz4", L.ALGO_LZ4), ("zstd", L.ALGO_ZSTD)):
        bound = E.envelope_bound(algo, U, 256)
        sp, op = params(NSRC), params(NOUT)
        keys = [p[0] for p in sp]
        sd = [bytearray(bound) for _ in range(NSRC)]
        r = E.compress_seal_batch(algo, a.cipher, [(sd[i], raw[i * U:(i + 1) * U]) for i in range(NSRC)], sp)
        assert all(e is None for _, e in r)
        stored = [bytes(sd[i][:r[i][0]]) for i in range(NSRC)]
        dst_a = [bytearray(bound) for _ in range(NOUT)]
        dst_b = [bytearray(bound) for _ in range(NOUT)]
        dec = [np.empty(U, dtype=np.uint8) for _ in range(NSRC)]
        ta, tb, tdec, tst, tenc = [], [], [], [], []
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            sres, ores = E.compact_seal_batch(algo, a.cipher, [(s, U) for s in stored], keys, dst_a, op,
                                              (seg_first, seg))
            t1 = time.perf_counter()
            dres = E.open_decompress_batch(algo, a.cipher, list(zip(dec, stored)), keys)
            t2 = time.perf_counter()
            outs = stitch(dec, seg_first, seg)
            t3 = time.perf_counter()
            eres = E.compress_seal_batch(algo, a.cipher, list(zip(dst_b, outs)), op)
            t4 = time.perf_counter()
            assert all(e is None for _, e in sres + ores + dres + eres)
            if it == 0:  # same bytes either way
                for j in range(NOUT):
                    assert ores[j][0] == eres[j][0] and dst_a[j][:ores[j][0]] == dst_b[j][:eres[j][0]], (name, j)
            if it >= a.warmup:
                ta.append((t1 - t0) * 1e3)
                tb.append((t4 - t1) * 1e3)
                tdec.append((t2 - t1) * 1e3)
                tst.append((t3 - t2) * 1e3)
                tenc.append((t4 - t3) * 1e3)
        res[name] = {
            "a_compact_seal_batch_ms": med(ta), "a_min_ms": min(ta), "a_max_ms": max(ta),
            "b_three_calls_ms": med(tb), "b_min_ms": min(tb), "b_max_ms": max(tb),
            "b_open_decompress_batch_ms": med(tdec), "b_numpy_stitch_ms": med(tst),
            "b_compress_seal_batch_ms": med(tenc), "a_over_b": med(ta) / med(tb),
            "stored_source_bytes": sum(len(s) for s in stored), "stored_output_bytes": sum(n for n, _ in ores),
        }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cipher", default=None, help="measure the encrypted-volume legs with this data cipher")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", *(("round10", "compact_seal_rate.json") if a.cipher else
                                                 ("round7", "compact_rate.json")))
    import torch
    from juicefs_amd import compress as C
    from juicefs_amd import device as D
    assert torch.cuda.is_available(), "compact_rate.py measures on a GPU"
    dev = torch.device("cuda:0")
    raw_t = torch.empty(NSRC * U, dtype=torch.uint8, device=dev)
    D.gen_blocks(raw_t, NSRC, U, "T", 7000)
    torch.cuda.synchronize()
    raw = raw_t.cpu().numpy()
    seg_first, seg = plan()
    res = {"shape": {"sources": NSRC, "outputs": NOUT, "block_bytes": U, "segments": len(seg),
                     "gathered_bytes": NOUT * U}, "reps": a.reps, "warmup": a.warmup}
    if a.cipher:
        sealed(a, raw, seg_first, seg, res)
        write(a, res)
        return
    for name in ("lz4", "zstd"):
        c = C.NewCompressor(name)
        bound = c.CompressBound(U)
        sd = [bytearray(bound) for _ in range(NSRC)]
        r = c.CompressBatch([(sd[i], raw[i * U:(i + 1) * U]) for i in range(NSRC)])
        assert all(e is None for _, e in r)
        stored = [bytes(sd[i][:r[i][0]]) for i in range(NSRC)]
        dst_a = [bytearray(bound) for _ in range(NOUT)]
        dst_b = [bytearray(bound) for _ in range(NOUT)]
        dec = [np.empty(U, dtype=np.uint8) for _ in range(NSRC)]
        ta, tb, tdec, tst, tenc = [], [], [], [], []
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            sres, ores = c.CompactBatch([(s, U) for s in stored], dst_a, (seg_first, seg))
            t1 = time.perf_counter()
            dres = c.DecompressBatch(list(zip(dec, stored)))
            t2 = time.perf_counter()
            outs = stitch(dec, seg_first, seg)
            t3 = time.perf_counter()
            eres = c.CompressBatch(list(zip(dst_b, outs)))
            t4 = time.perf_counter()
            assert all(e is None for _, e in sres + ores + dres + eres)
            if it == 0:  # same bytes either way
                for j in range(NOUT):
                    assert ores[j][0] == eres[j][0] and dst_a[j][:ores[j][0]] == dst_b[j][:eres[j][0]], (name, j)
            if it >= a.warmup:
                ta.append((t1 - t0) * 1e3)
                tb.append((t4 - t1) * 1e3)
                tdec.append((t2 - t1) * 1e3)
                tst.append((t3 - t2) * 1e3)
                tenc.append((t4 - t3) * 1e3)
        res[name] = {
            "a_compact_batch_ms": med(ta), "a_min_ms": min(ta), "a_max_ms": max(ta),
            "b_parent_abi_ms": med(tb), "b_min_ms": min(tb), "b_max_ms": max(tb),
            "b_decompress_batch_ms": med(tdec), "b_numpy_stitch_ms": med(tst), "b_compress_batch_ms": med(tenc),
            "a_over_b": med(ta) / med(tb),
            "stored_source_bytes": sum(len(s) for s in stored), "stored_output_bytes": sum(n for n, _ in ores),
        }
    # (c) the gather kernel alone, sources already decoded in HBM
    offs = np.arange(NSRC, dtype=np.int64) * U
    sdesc = D.make_desc(raw_t, offs, [U] * NSRC, raw_t, offs, [U] * NSRC)
    src_n = torch.full((NSRC,), U, dtype=torch.int32, device=dev)
    gat = torch.empty(NOUT * U, dtype=torch.uint8, device=dev)
    odesc, sdev = D.make_compact_desc(gat, np.arange(NOUT, dtype=np.int64) * U, [U] * NOUT, seg_first, seg)
    ret = torch.empty(NOUT, dtype=torch.int32, device=dev)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    st = torch.cuda.current_stream().cuda_stream

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

    g = timed(lambda: D.gather(sdesc, src_n, odesc, sdev, U, ret))
    assert ret.cpu().tolist() == [U] * NOUT
    want = stitch([raw[i * U:(i + 1) * U] for i in range(NSRC)], seg_first, seg)
    assert np.array_equal(gat.cpu().numpy(), np.concatenate(want))

    def memcpy():
        assert hip.hipMemcpyDtoDAsync(gat.data_ptr(), raw_t.data_ptr(), NOUT * U, st) == 0
    m = timed(memcpy)
    gib = NOUT * U / 2**30
    res["gather"] = {"c_gather_ms": med(g), "c_min_ms": min(g), "c_max_ms": max(g), "memcpy_dtod_ms": med(m),
                     "memcpy_min_ms": min(m), "memcpy_max_ms": max(m), "c_over_memcpy": med(g) / med(m),
                     "gather_gib_s_out": gib / (med(g) / 1e3), "memcpy_gib_s": gib / (med(m) / 1e3)}
    write(a, res)


def write(a, res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
