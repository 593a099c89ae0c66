#!/usr/bin/env python3
"""Headline benchmark (BASELINE.json): device-resident GiB/s of LZ4 block
decompression, 4 MiB blocks, 4096 blocks in HBM per GPU (configs[1]).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  torchrun --nproc-per-node N bench.py --gpus N ...   (one process per GPU)

A plain run does what the headline figure needs and nothing else: it builds
the batch, warms up, times exactly K steps, writes its outputs when
--dump-outputs is given, and prints one JSON result line.  --full adds the
check of the decoded output, every sub-record below and the CPU legs (minutes
of run time), and prints a compact summary record after the result line.

--dump-outputs DIR writes what the last timed step left in the caller's
buffers, as float32 / float64 .npy files: decoded.npy (a fixed, seeded sample
of the decoded bytes, every byte when the output is small) and sizes.npy (the
decoder's return value per block).  The inputs depend on the arguments alone,
so two builds can be compared file for file.

`python bench.py --gpus N` with N > 1 and no torchrun environment starts the N
ranks itself (torch.distributed.run as a child process, before anything here
touches a GPU) and exits with its status.

A step = one launch of the LZ4 decode kernel over the rank's whole batch.
Blocks are independent, so ranks shard them with no data-path collective
(weak scaling: every rank decodes its own 4096 blocks); torch.distributed is
used only for the barrier and the max-over-ranks time.  Inputs are synthetic
text-like blocks generated on the GPU and compressed by the GPU
encoder (byte-identical to LZ4_compress_default) before timing; with --full
the decoded output is checked against the original on the device after timing.

Sub-records of the same JSON line with --full (each names its BASELINE config):
  configs_3        Zstd level-3 decode, 4096 x 4 MiB frames in HBM, every rank
  configs_2        LZ4 compress + decompress, 2048 blocks per GPU, block i on
                   rank i % N (round robin), every block verified, every rank
  configs_0        LZ4 round trip of 1024 x 4 MiB host blocks through the C ABI
                   batch entry points (rank 0, N = 1)
  host_path        PCIe-inclusive LZ4 decompress/compress (rank 0, N = 1)
  mixed_host_path  configs[4] shape on one GPU (rank 0, N = 1)
  roofline         HIP-event timed decode kernel vs 8 TB/s; `traffic` from
                   profiles/traffic.json only while its kernel-source stamp
                   matches the sources built here
  cpu_baseline     liblz4 LZ4_decompress_safe (the C code pkg/compress's
                   go-lz4 wraps) on this host's cores; 1-core figure and the
                   CPU oracle beside it
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ZSTD_FRAMES = []  # configs[3]'s distinct frames (host copies) for its CPU leg
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
METRIC = "device-resident GiB/s (de)compress, 4 MiB blocks, LZ4+Zstd, 1/2/4/8 MI355X"
KERNEL_SOURCES = ("juicefs_amd/csrc/lz4_decode.hip", "juicefs_amd/csrc/wave.cuh", "juicefs_amd/csrc/jfs_internal.h")
ZSTD_KERNEL_SOURCES = ("juicefs_amd/csrc/zstd_decode.hip", "juicefs_amd/csrc/zstd_split.inc",
                       "juicefs_amd/csrc/wave.cuh", "juicefs_amd/csrc/jfs_internal.h")



def _mark(name):
    """(JFS_HOST_TRACE) a leg marker on stderr, on the library's trace clock"""
    if os.environ.get("JFS_HOST_TRACE"):
        print(f"[bench] t={time.monotonic() * 1e3:.2f} leg {name}", file=sys.stderr, flush=True)

def kernel_src_sha256(sources=KERNEL_SOURCES) -> str:
    """Stamp of a kernel's sources (profiles/traffic*.json carry it): the LZ4
    decode kernel by default, ZSTD_KERNEL_SOURCES for the Zstd decoder."""
    h = hashlib.sha256()
    for p in sources:
        with open(os.path.join(ROOT, p), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--full", action="store_true",
                   help="also verify the decoded output and run every sub-record and CPU leg (the --no-* and "
                        "sub-record options below apply only with --full)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's outputs to DIR/<name>.npy (float32/float64, <= 64 MB)")
    p.add_argument("--blocks", type=int, default=4096)
    p.add_argument("--block-bytes", type=int, default=4 << 20)
    p.add_argument("--cls", default="T")
    p.add_argument("--codec", default="lz4", choices=["lz4", "zstd"],
                   help="headline codec: lz4 = configs[1] (default); zstd = level-3 decode (configs[3])")
    p.add_argument("--level", type=int, default=3, help="zstd level of the generated frames")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-host-path", action="store_true", help="skip the PCIe-inclusive legs (host_path, mixed, configs_0)")
    p.add_argument("--host-blocks", type=int, default=2048, help="blocks in the host_path sample")
    p.add_argument("--no-extras", action="store_true", help="skip every sub-record (headline only)")
    p.add_argument("--no-mixed", action="store_true", help="skip configs[4] (mixed LZ4/Zstd 64 KiB-4 MiB, host path)")
    p.add_argument("--mixed-blocks", type=int, default=4096)
    p.add_argument("--c0-blocks", type=int, default=1024, help="configs[0] blocks (host round trip)")
    p.add_argument("--c2-blocks", type=int, default=2048, help="configs[2] blocks per GPU (one full LZ4 encoder round: 8 blocks per CU)")
    p.add_argument("--zstd-steps", type=int, default=3, help="timed launches of the configs[3] sub-record")
    p.add_argument("--extra-blocks", type=int, default=1024, help="blocks in the Zstd compress sample")
    p.add_argument("--cpu-seconds", type=float, default=6.0, help="wall budget per CPU baseline leg")
    p.add_argument("--traffic-file", default=os.path.join(ROOT, "profiles", "traffic.json"))
    p.add_argument("--zstd-traffic-file", default=os.path.join(ROOT, "profiles", "traffic_zstd.json"))
    return p.parse_args()


def host_threads() -> int:
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    return max(1, min(16, n))  # the GPU box's CPU share is 16


def _spawn_ranks(n: int) -> int:
    """`--gpus N` without a torchrun environment: run N ranks (one per GPU)
    under torch.distributed.run as a child process; nothing in this process has
    touched a GPU yet."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=dict(os.environ)).returncode


# ---------------------------------------------------------------------------
# CPU legs (bounded samples, rank 0 at N = 1)
# ---------------------------------------------------------------------------
def _timed_threads(work_one, T, seconds):
    """Run work_one(t, k) on T threads until `seconds` elapse; returns (calls, wall)."""
    counts = [0] * T
    stop = [False]

    def work(t):
        k = t
        while not stop[0]:
            work_one(t, k)
            counts[t] += 1
            k += T

    th = [threading.Thread(target=work, args=(t,)) for t in range(T)]
    t0 = time.perf_counter()
    [x.start() for x in th]
    time.sleep(seconds)
    stop[0] = True
    [x.join() for x in th]
    return sum(counts), time.perf_counter() - t0


def _liblz4():
    for path in ("/opt/conda/lib/liblz4.so.1", "/usr/lib/x86_64-linux-gnu/liblz4.so.1"):
        if os.path.exists(path):
            lz = ctypes.CDLL(path)
            lz.path = path
            return lz
    return None


def liblz4_baseline(comp_blocks, U, seconds, threads):
    """LZ4_decompress_safe from the host's liblz4 -- the C routine pkg/compress
    reaches through go-lz4 (compress.go:120-125; this image has 1.9.3, the
    reference vendors a 2017 copy).  ctypes releases the GIL, so the threads
    decode in parallel; one block stream per thread."""
    lz = _liblz4()
    if lz is None:
        return None
    bufs = [ctypes.create_string_buffer(c, len(c)) for c in comp_blocks]
    outs = [ctypes.create_string_buffer(U) for _ in range(threads)]

    def one(t, k):
        c = bufs[k % len(bufs)]
        r = lz.LZ4_decompress_safe(c, outs[t], len(c), U)
        assert r == U

    nb, dt = _timed_threads(one, threads, seconds)
    return {"value": nb * U / dt / 2**30, "unit": "GiB/s", "cores": threads, "kind": "reference",
            "library": f"{lz.path} v{lz.LZ4_versionNumber()}",
            "sample": f"{nb} LZ4_decompress_safe calls over {len(bufs)} distinct 4 MiB text blocks (the headline's "
                      f"own compressed blocks), {threads} threads, {dt:.1f} s wall"}


def oracle_baseline(comp_blocks, U, seconds, codec="lz4"):
    """The CPU oracle (test infrastructure, oracle/*.c at -O2) on the same
    sample: reported beside the library, never the thing measured."""
    from tests.oracle_ctypes import Oracle
    so = os.path.join(ROOT, "oracle", "_build", "liboracle.so")
    if not os.path.exists(so):
        return None
    orc = Oracle(so)
    T = host_threads()
    bufs = [ctypes.create_string_buffer(c, len(c)) for c in comp_blocks]
    outs = [ctypes.create_string_buffer(U) for _ in range(T)]

    def one(t, k):
        c = bufs[k % len(bufs)]
        if codec == "lz4":
            r = orc.lib.oracle_lz4_decompress_safe(c, outs[t], len(c), U)
        else:
            r = orc.lib.oracle_zstd_decompress(c, len(c), outs[t], U)
        assert r == U

    nb, dt = _timed_threads(one, T, seconds)
    return {"value": nb * U / dt / 2**30, "unit": "GiB/s", "cores": T, "kind": "port",
            "sample": f"{nb} decodes of {len(bufs)} distinct 4 MiB text blocks (oracle/{codec}_oracle.c), {T} threads"}


def libzstd_baseline(comp_blocks, U, seconds):
    """ZSTD_decompress from the host's libzstd (the C library DataDog/zstd
    wraps; this image has 1.4.9, the reference pins 1.5.6)."""
    from juicefs_amd.device import _libzstd
    z = _libzstd()
    if z is None:
        return None
    z.ZSTD_versionNumber.restype = ctypes.c_uint
    T = host_threads()
    bufs = [ctypes.create_string_buffer(c, len(c)) for c in comp_blocks]
    outs = [ctypes.create_string_buffer(U) for _ in range(T)]

    def one(t, k):
        c = bufs[k % len(bufs)]
        assert z.ZSTD_decompress(outs[t], U, c, len(c)) == U

    nb, dt = _timed_threads(one, T, seconds)
    return {"value": nb * U / dt / 2**30, "unit": "GiB/s", "cores": T, "kind": "reference",
            "library": f"{z.path} v{z.ZSTD_versionNumber()}"}


def cpu_codec_legs(raw_blocks, comp_blocks, zstd_frames, U, seconds):
    """The C routines pkg/compress reaches, on this host's cores (one block
    stream per thread; 16 threads and 1 core), beside every GPU leg -- the
    reference's own harness times both directions of both codecs
    (pkg/compress/compress_test.go:78-151): LZ4_compress_default,
    ZSTD_compress(level 1), ZSTD_decompress (the configs[3] level-3 frames).
    GiB/s of uncompressed bytes."""
    from juicefs_amd.device import _libzstd
    lz, z = _liblz4(), _libzstd()
    out = {}
    T = host_threads()
    bound = U + U // 255 + 16
    zbound = U + (U >> 8) + 64
    raws = [ctypes.create_string_buffer(r, len(r)) for r in raw_blocks]

    def leg(one, threads, secs):
        nb, dt = _timed_threads(one, threads, secs)
        return nb * U / dt / 2**30

    if lz is not None:
        outs = [ctypes.create_string_buffer(bound) for _ in range(T)]

        def lz4c(t, k):
            r = raws[k % len(raws)]
            assert lz.LZ4_compress_default(r, outs[t], U, bound) > 0
        out["lz4_compress"] = {"value": leg(lz4c, T, seconds), "unit": "GiB/s", "cores": T,
                               "one_core": leg(lz4c, 1, seconds / 3), "library": f"{lz.path}"}
    if z is not None:
        z.ZSTD_compress.restype = ctypes.c_size_t
        zouts = [ctypes.create_string_buffer(zbound) for _ in range(T)]

        def zc(t, k):
            r = raws[k % len(raws)]
            assert z.ZSTD_compress(zouts[t], zbound, r, U, 1) < (1 << 40)
        out["zstd1_compress"] = {"value": leg(zc, T, seconds), "unit": "GiB/s", "cores": T,
                                 "one_core": leg(zc, 1, seconds / 3), "library": f"{z.path}"}
        if zstd_frames:
            fr = [ctypes.create_string_buffer(f, len(f)) for f in zstd_frames]
            douts = [ctypes.create_string_buffer(U) for _ in range(T)]

            def zd(t, k):
                f = fr[k % len(fr)]
                assert z.ZSTD_decompress(douts[t], U, f, len(f)) == U
            out["zstd_decompress_configs3"] = {"value": leg(zd, T, seconds), "unit": "GiB/s", "cores": T,
                                               "one_core": leg(zd, 1, seconds / 3), "library": f"{z.path}",
                                               "sample": f"{len(fr)} distinct level-3 frames of configs[3]"}
    out["note"] = ("host C libraries (liblz4 1.9.3 / libzstd 1.4.9 of this image; the reference pins go-lz4 2017 "
                   "and zstd 1.5.6), bounded samples of 32 distinct 4 MiB text blocks")
    return out


# ---------------------------------------------------------------------------
# host-buffer legs (C ABI batch entry points: what the cgo drop-in calls)
# ---------------------------------------------------------------------------
def host_path_rate(comp_blocks, raw_blocks, U, nblk, reps=2, device_mask=0):
    """PCIe-inclusive: Go-heap-like host buffers -> pinned -> HBM -> kernel ->
    pinned -> host buffers, via the C ABI batch entry points, chunked and
    pipelined over two streams (capi.hip run_batch).  Host clock around the
    whole call; best of `reps`."""
    from juicefs_amd import compress as C
    c = C.LZ4()
    k = max(1, nblk // len(comp_blocks))
    srcs = (comp_blocks * k)[:nblk]
    pairs = [(bytearray(U), cb) for cb in srcs]
    c.DecompressBatch(pairs[:4], device_mask=device_mask)
    res_d = 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        res = c.DecompressBatch(pairs, device_mask=device_mask)
        dt = time.perf_counter() - t0
        assert all(n == U and e is None for n, e in res)
        res_d = max(res_d, len(pairs) * U / dt / 2**30)
    del pairs
    bound = c.CompressBound(U)
    ncb = min(nblk, 1024)
    raws = (raw_blocks * (ncb // len(raw_blocks) + 1))[:ncb]
    cpairs = [(bytearray(bound), rb) for rb in raws]
    res_c = 0.0
    for _ in range(reps):  # best of reps: the first call may grow the staging (4 GiB LZ4-compress chunks)
        t0 = time.perf_counter()
        res = c.CompressBatch(cpairs, device_mask=device_mask)
        dt = time.perf_counter() - t0
        assert all(n > 0 and e is None for n, e in res)
        res_c = max(res_c, len(cpairs) * U / dt / 2**30)
    return {"lz4_decompress": {"value": res_d, "unit": "GiB/s"},
            "lz4_compress": {"value": res_c, "unit": "GiB/s"},
            "blocks": nblk, "compress_blocks": ncb, "chunk_mb": int(os.environ.get("JFS_HOST_CHUNK_MB", "2048")),
            "chunk_mb_lz4_compress": int(os.environ.get("JFS_HOST_CHUNK_MB_LZ4C", "4096")),
            "path": "jfs_{de,}compress_batch: host buffers -> pinned (16 threads) -> H2D -> kernel -> D2H -> "
                    "host buffers, 2-stream chunk pipeline, 1 GPU, GiB/s of uncompressed bytes"}


def oneshot_concurrency(comp_blocks, raw_blocks, U, n_dec=200, n_enc=20, rounds=2):
    """The drop-in shape: pkg/chunk's one-call-per-block Compress/Decompress
    from many goroutines at once (max-downloads 200, max-uploads 20,
    cmd/flags.go:133-139), here Python threads calling the C ABI (the GIL is
    released inside each call; the library's coalescer batches whatever is
    queued).  Per-call latency percentiles and aggregate throughput; a lone
    call's latency for comparison.  Every output is checked."""
    import threading
    from juicefs_amd import compress as C
    c = C.LZ4()
    bound = c.CompressBound(U)

    def pct(v, q):
        v = sorted(v)
        return v[min(len(v) - 1, int(q * len(v)))] * 1e3

    from juicefs_amd import _lib as L

    def batches():  # device batches the coalescer ran so far (LZ4 and Zstd, both directions)
        arr = (L.JfsOpStats * L.STATS_N)()
        L.load().jfs_stats(arr, L.STATS_N)
        return int(sum(arr[a * 2 + d].batches for a in (L.ALGO_LZ4, L.ALGO_ZSTD) for d in (0, 1)))

    def run(n, k, fn, check):
        """n threads x k calls of fn(t, r) -> result; every result is checked
        with check(t, r, result) after the clock stops (a 4 MiB compare holds
        the GIL: inside the timed region 400 of them alone cap the rate)."""
        lat, res = [[] for _ in range(n)], [[None] * k for _ in range(n)]
        bar = threading.Barrier(n + 1)
        b0 = batches()

        def worker(t):
            bar.wait()
            for r in range(k):
                t0 = time.perf_counter()
                res[t][r] = fn(t, r)
                lat[t].append(time.perf_counter() - t0)
        th = [threading.Thread(target=worker, args=(t,)) for t in range(n)]
        for x in th:
            x.start()
        bar.wait()
        t0 = time.perf_counter()
        for x in th:
            x.join()
        wall = time.perf_counter() - t0
        b1 = batches()
        errs = sum(1 for t in range(n) for r in range(k) if not check(t, r, res[t][r]))
        flat = [v for row in lat for v in row]
        return {"calls": n * k, "p50_ms": pct(flat, 0.5), "p99_ms": pct(flat, 0.99),
                "value": n * k * U / wall / 2**30, "unit": "GiB/s", "errors": errs, "device_batches": b1 - b0}

    def bursts(n, k, fn, check, nb=5):
        """nb bursts of run(n, k): the median value / p50 / p99 over the bursts
        (one burst alone swings with what the coalescer gathers), each burst's
        record (device batches = how many device batches its calls formed)."""
        rs = [run(n, k, fn, check) for _ in range(nb)]
        med = lambda key: sorted(r[key] for r in rs)[len(rs) // 2]
        return {"calls": n * k, "bursts": len(rs), "value": med("value"), "p50_ms": med("p50_ms"),
                "p99_ms": med("p99_ms"), "unit": "GiB/s", "errors": sum(r["errors"] for r in rs),
                "device_batches": [r["device_batches"] for r in rs],
                "calls_per_device_batch": [round(n * k / max(r["device_batches"], 1), 1) for r in rs],
                "per_burst": [{"value": round(r["value"], 3), "p50_ms": round(r["p50_ms"], 2),
                               "p99_ms": round(r["p99_ms"], 2)} for r in rs]}

    nc = len(comp_blocks)
    n_lone = 11  # lone decodes per codec: the p50 of 11 (5 swung by a tenth of a ms between runs)
    kmax = max(rounds, n_lone)
    ddst = {}  # one output buffer per (thread, call): checked after the run

    def dec(t, r):
        d = ddst.setdefault((t, r), bytearray(U))
        return c.Decompress(d, comp_blocks[(t + r) % nc])[0]
    dchk = lambda t, r, n: n == U and ddst[(t, r)] == raw_blocks[(t + r) % nc]
    edst = {}

    def enc(t, r):
        d = edst.setdefault((t, r), bytearray(bound))
        return c.Compress(d, raw_blocks[(t + r) % nc])[0]
    echk = lambda t, r, n: n > 0 and c.Decompress(bytearray(U), bytes(edst[(t, r)][:n]))[0] == U
    # buffers allocated and touched before any timing (bytearray(n) is calloc:
    # untouched pages would fault inside the library's copy-out), like the
    # recycled page buffers pkg/chunk decodes into
    for t in range(n_dec):
        for r in range(kmax if t == 0 else rounds):
            ddst[(t, r)] = bytearray(b"\x01") * U
    for t in range(n_enc):
        for r in range(kmax if t == 0 else rounds):
            edst[(t, r)] = bytearray(b"\x01") * bound
    # warm the coalescer and its staging (pinned once, then reused; growing a
    # slot pins new memory at ~0.1 s per GiB): one full-size batch per lane at
    # once (both lanes' first slots), then bursts of the timed size
    wpairs = [[(bytearray(U), comp_blocks[i % nc]) for i in range(n_dec)] for _ in range(2)]
    wth = [threading.Thread(target=c.DecompressBatch, args=(wp,)) for wp in wpairs]
    [x.start() for x in wth]
    [x.join() for x in wth]
    del wpairs
    warm = [run(n_dec, rounds, dec, dchk)["device_batches"] for _ in range(2)]
    warm += [run(n_enc, rounds, enc, echk)["device_batches"]]
    def native(n, k, fname, srcs, dsts, cap, check):
        """run() with n pthreads of juicefs_amd/lib/libjfscallers.so calling
        jfs_<fname> k times each (no interpreter lock between calls, like
        goroutines); same sources, destinations and checks as run()."""
        import ctypes
        cl = ctypes.CDLL(os.path.join(ROOT, "juicefs_amd", "lib", "libjfscallers.so"))
        cl.jfs_native_callers.restype = ctypes.c_double
        fn = ctypes.cast(getattr(L.load(), fname), ctypes.c_void_p)
        ns = len(srcs)
        sp = (ctypes.c_void_p * ns)(*[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value for b in srcs])
        ln = (ctypes.c_int64 * ns)(*[len(b) for b in srcs])
        dbuf = [(ctypes.c_char * len(dsts[(t, r)])).from_buffer(dsts[(t, r)]) for t in range(n) for r in range(k)]
        dp = (ctypes.c_void_p * (n * k))(*[ctypes.addressof(x) for x in dbuf])
        lat, ret = (ctypes.c_double * (n * k))(), (ctypes.c_int64 * (n * k))()
        b0 = batches()
        wall = cl.jfs_native_callers(fn, ctypes.c_int(c.algo), n, k, sp, ln, ns, dp, ctypes.c_int64(cap), lat, ret)
        b1 = batches()
        del dbuf, dp
        assert wall > 0, "native callers failed to start"
        errs = sum(1 for t in range(n) for r in range(k) if not check(t, r, int(ret[t * k + r])))
        flat = list(lat)
        return {"calls": n * k, "p50_ms": pct(flat, 0.5), "p99_ms": pct(flat, 0.99),
                "value": n * k * U / wall / 2**30, "unit": "GiB/s", "errors": errs, "device_batches": b1 - b0}

    def native_bursts(n, k, fname, srcs, dsts, cap, check, nb=5):
        rs = [native(n, k, fname, srcs, dsts, cap, check) for _ in range(nb)]
        med = lambda key: sorted(r[key] for r in rs)[len(rs) // 2]
        return {"calls": n * k, "bursts": len(rs), "value": med("value"), "p50_ms": med("p50_ms"),
                "p99_ms": med("p99_ms"), "unit": "GiB/s", "errors": sum(r["errors"] for r in rs),
                "device_batches": [r["device_batches"] for r in rs],
                "per_burst": [{"value": round(r["value"], 3), "p50_ms": round(r["p50_ms"], 2),
                               "p99_ms": round(r["p99_ms"], 2)} for r in rs]}

    out = {"decompress_lone": run(1, n_lone, dec, dchk), "compress_lone": run(1, 3, enc, echk),
           f"decompress_{n_dec}_concurrent": bursts(n_dec, rounds, dec, dchk),
           f"compress_{n_enc}_concurrent": bursts(n_enc, rounds, enc, echk),
           "warmup_device_batches": warm,
           "path": "LZ4 one-call API (jfs_compress / jfs_decompress) from concurrent host threads, host buffers, "
                   "1 GPU; value = uncompressed GiB/s over the wall time of all calls"}
    # the same calls from native threads (libjfscallers.so): the library without the interpreter lock
    out[f"decompress_{n_dec}_concurrent_native"] = native_bursts(n_dec, rounds, "jfs_decompress", comp_blocks, ddst,
                                                                 U, dchk)
    out[f"compress_{n_enc}_concurrent_native"] = native_bursts(n_enc, rounds, "jfs_compress", raw_blocks, edst,
                                                               bound, echk)
    out["native_path"] = ("*_native: n pthreads (juicefs_amd/callers/callers.c) call jfs_decompress / jfs_compress "
                          "k times each after one barrier, like pkg/chunk's goroutines; same buffers and checks")
    # the same calls with --compress zstd (ZStandard.Compress / Decompress)
    z = C.ZStandard()
    zb = z.CompressBound(U)
    zdst = {(t, r): bytearray(b"\x01") * zb for t in range(n_enc) for r in range(kmax if t == 0 else rounds)}
    zframes = []
    for i in range(min(nc, 8)):
        d = bytearray(zb)
        m = z.Compress(d, raw_blocks[i])[0]
        zframes.append(bytes(d[:m]))

    def zenc(t, r):
        return z.Compress(zdst[(t, r)], raw_blocks[(t + r) % nc])[0]
    zechk = lambda t, r, n: n > 0 and z.Decompress(bytearray(U), bytes(zdst[(t, r)][:n]))[0] == U
    zout = {(t, r): bytearray(b"\x01") * U for t in range(n_enc) for r in range(kmax if t == 0 else rounds)}

    def zdec(t, r):
        return z.Decompress(zout[(t, r)], zframes[(t + r) % len(zframes)])[0]
    zdchk = lambda t, r, n: n == U and zout[(t, r)] == raw_blocks[(t + r) % len(zframes)]
    out["zstd"] = {"compress_lone": run(1, 3, zenc, zechk), "decompress_lone": run(1, n_lone, zdec, zdchk),
                   f"compress_{n_enc}_concurrent": bursts(n_enc, rounds, zenc, zechk),
                   f"decompress_{n_enc}_concurrent": bursts(n_enc, rounds, zdec, zdchk),
                   "path": "Zstd one-call API (compress.go ZStandard: GPU encoder, level-1 class; GPU decoder)"}
    return out


def configs0_roundtrip(dev, nblk, U, seed_base=90001):
    """BASELINE configs[0]: LZ4 round trip of nblk x 4 MiB synthetic host
    blocks through the pkg/compress-shaped C ABI (jfs_compress_batch then
    jfs_decompress_batch; the cgo drop-in's batch form).  Every decoded block
    is compared with its source; the compressed bytes of every block are
    compared with the device-resident encoder's output for the same block."""
    import torch
    from juicefs_amd import compress as C
    from juicefs_amd import device as D
    raw = np.empty(nblk * U, dtype=np.uint8)
    per = 256
    dbuf = torch.empty(per * U, dtype=torch.uint8, device=dev)
    for s in range(0, nblk, per):
        k = min(per, nblk - s)
        D.gen_blocks(dbuf, k, U, "T", seed_base + s)
        raw[s * U:(s + k) * U] = dbuf[:k * U].cpu().numpy()
    del dbuf
    c = C.LZ4()
    bound = c.CompressBound(U)
    comp = np.zeros(nblk * bound, dtype=np.uint8)
    pairs = [(comp[i * bound:(i + 1) * bound], raw[i * U:(i + 1) * U]) for i in range(nblk)]
    c.CompressBatch(pairs)  # warm: the library's pinned staging grows to its chunk size once per process
    t0 = time.perf_counter()
    res = c.CompressBatch(pairs)
    tc = time.perf_counter() - t0
    sizes = [n for n, e in res]
    if any(e is not None or n <= 0 for n, e in res):
        raise RuntimeError("configs[0] compress failed")
    out = np.zeros(nblk * U, dtype=np.uint8)
    dpairs = [(out[i * U:(i + 1) * U], comp[i * bound:i * bound + sizes[i]]) for i in range(nblk)]
    c.DecompressBatch(dpairs)  # warm, as for compress: the decode chunks' staging and scratch
    out[:] = 0
    t0 = time.perf_counter()
    res = c.DecompressBatch(dpairs)
    td = time.perf_counter() - t0
    if any(e is not None or n != U for n, e in res) or not np.array_equal(out, raw):
        raise RuntimeError("configs[0] round trip mismatch")
    # compressed bytes == the device-resident encoder's (a sample of 64 blocks)
    ns = min(64, nblk)
    b = D.Lz4Batch(ns, U, "T", seed_base=seed_base, device=dev)
    dcomp = b.comp.cpu().numpy()
    same = all(int(b.csize[i]) == sizes[i] and
               np.array_equal(dcomp[i * b.slot:i * b.slot + sizes[i]], comp[i * bound:i * bound + sizes[i]])
               for i in range(ns))
    if not same:
        raise RuntimeError("configs[0] host-path bytes differ from the device encoder")
    total = nblk * U
    return {"value": total / (tc + td) / 2**30, "unit": "GiB/s",
            "compress": {"value": total / tc / 2**30, "unit": "GiB/s", "s": tc},
            "decompress": {"value": total / td / 2**30, "unit": "GiB/s", "s": td},
            "blocks": nblk, "ratio": total / float(sum(sizes)),
            "verified": "every block decoded == source; compressed bytes == device encoder on 64 blocks",
            "path": "BASELINE configs[0] through the C ABI batch surface (host buffers, pinned staging, GPU kernels); "
                    "value = uncompressed bytes / (compress s + decompress s)"}


def mixed_host_path(raw_src, nblk=4096, seed=11, device_mask=0):
    """BASELINE configs[4] on one GPU: mixed LZ4/Zstd blocks of 64 KiB-4 MiB
    (log-uniform sizes, codec alternating), host buffers in and out through the
    C ABI batch entry points.  Every block is checked against its source."""
    from juicefs_amd import compress as C
    rng = np.random.default_rng(seed)
    lo, hi = 64 << 10, 4 << 20
    sizes = np.exp(rng.uniform(np.log(lo), np.log(hi), nblk)).astype(np.int64)
    raws = [raw_src[i % len(raw_src)][:int(n)] for i, n in enumerate(sizes)]
    codecs = {"lz4": C.LZ4(), "zstd": C.ZStandard()}
    idx = {"lz4": list(range(0, nblk, 2)), "zstd": list(range(1, nblk, 2))}
    total = int(sizes.sum())
    comp = [None] * nblk
    cds = [codecs["lz4"] if i % 2 == 0 else codecs["zstd"] for i in range(nblk)]
    # one mixed-codec batch call per direction: the LZ4 and Zstd blocks run at
    # once on the device's two lanes (jfs_{de,}compress_batch_mixed)
    ents = [(cds[i], bytearray(cds[i].CompressBound(len(raws[i]))), raws[i]) for i in range(nblk)]
    t0 = time.perf_counter()
    res = C.CompressBatchMixed(ents, device_mask=device_mask)
    tc = time.perf_counter() - t0
    for i, ((_, buf, _), (n, e)) in enumerate(zip(ents, res)):
        if e is not None or n <= 0:
            raise RuntimeError(f"mixed compress failed: block {i}: {e}")
        comp[i] = bytes(buf[:n])
    best = 0.0
    for _ in range(2):
        outs = [(cds[i], bytearray(len(raws[i])), comp[i]) for i in range(nblk)]
        t0 = time.perf_counter()
        res = C.DecompressBatchMixed(outs, device_mask=device_mask)
        td = time.perf_counter() - t0
        for i, ((_, buf, _), (n, e)) in enumerate(zip(outs, res)):
            if e is not None or n != len(raws[i]) or bytes(buf) != raws[i]:
                raise RuntimeError(f"mixed round trip mismatch: block {i}")
        best = max(best, total / td / 2**30)
    csz = sum(len(x) for x in comp)
    return {"decompress": {"value": best, "unit": "GiB/s"},
            "compress": {"value": total / tc / 2**30, "unit": "GiB/s"},
            "blocks": nblk, "bytes": total, "ratio": total / csz,
            "sizes": "log-uniform 64 KiB-4 MiB, LZ4 and Zstd alternating",
            "path": "BASELINE configs[4] on 1 GPU: jfs_{de,}compress_batch_mixed (both codecs' batches at once), "
                    "host buffers in and out, GPU encoders and decoders, every block verified"}


def check_spread(device_blocks, ndev, nblk):
    """The dealer must have put blocks on every one of the job's ndev devices
    (as many as there were blocks): a library that saw fewer devices, or a deal
    that skipped one, fails the leg instead of reporting a one-GPU figure."""
    used = sorted(d for d, n in device_blocks.items() if n > 0)
    want = min(ndev, nblk)
    if len(used) < want:
        raise RuntimeError(f"dealer: blocks ran on devices {used}, expected {want} of the job's {ndev} GPUs")
    return used


def dealer_legs(batch, U, a, world=1):
    """Rank 0 with device_mask = all GPUs: host_path (LZ4 decompress and
    compress of host buffers) and configs[4] (mixed LZ4/Zstd, 64 KiB-4 MiB),
    the batch ABI dealing blocks round-robin over every visible device; the
    per-device block counters must show all `world` GPUs used."""
    from juicefs_amd import _lib as L
    ns = min(32, batch.nblk)
    comp = [batch.comp[i * batch.slot:i * batch.slot + int(batch.csize[i])].cpu().numpy().tobytes() for i in range(ns)]
    raws = [batch.raw[i * U:(i + 1) * U].cpu().numpy().tobytes() for i in range(ns)]
    lib = L.load()
    nvis = lib.jfs_device_count()
    if nvis < world:
        raise RuntimeError(f"dealer: the library sees {nvis} gfx950 devices, the job has {world}")
    lib.jfs_stats_reset()
    out = {"host_path": host_path_rate(comp, raws, U, a.host_blocks, device_mask=0)}
    if not a.no_mixed:
        _mark("mixed_host_path")
        out["mixed_host_path"] = mixed_host_path(raws, a.mixed_blocks, device_mask=0)
    ds = (L.JfsDeviceStat * 64)()
    nd = lib.jfs_device_stats(ds, 64)
    out["device_blocks"] = {int(ds[i].device): int(ds[i].blocks) for i in range(nd)}
    out["devices_used"] = check_spread(out["device_blocks"], world, a.host_blocks)
    out["value"] = _pick(out, "host_path", "lz4_decompress", "value")
    out["path"] = ("rank 0 alone, jfs_{de,}compress_batch with device_mask 0 (every visible GPU), blocks dealt "
                   "round-robin, one host thread per device; host buffers in and out")
    return out


class GpuHostOps:
    """The batch ABI of libjfsgpu.so as ranked_host_path uses it (host
    buffers; the tests substitute a CPU stand-in with the same methods)."""

    def __init__(self, dev):
        from juicefs_amd import compress as C
        self.dev = dev
        self.c = C.LZ4()

    def gen(self, nblk, U, seed):
        import torch
        from juicefs_amd import device as D
        dbuf = torch.empty(nblk * U, dtype=torch.uint8, device=self.dev)
        D.gen_blocks(dbuf, nblk, U, "T", seed)
        return dbuf.cpu().numpy()

    def bound(self, U):
        return self.c.CompressBound(U)

    def compress(self, pairs, mask):
        return self.c.CompressBatch(pairs, device_mask=mask)

    def decompress(self, pairs, mask):
        return self.c.DecompressBatch(pairs, device_mask=mask)

    def reset_stats(self):
        from juicefs_amd import _lib as L
        L.load().jfs_stats_reset()

    def device_blocks(self):
        from juicefs_amd import _lib as L
        ds = (L.JfsDeviceStat * 64)()
        nd = L.load().jfs_device_stats(ds, 64)
        return {int(ds[i].device): int(ds[i].blocks) for i in range(nd) if ds[i].blocks}


def ranked_host_path(S, world, rank, local, dev, nblk, U, ops=None):
    """BASELINE configs[0] on every rank (N > 1): each process compresses and
    decompresses its own nblk host blocks through jfs_{de,}compress_batch
    with device_mask = its GPU only (the batch ABI's device selection,
    SURVEY.md 8e), timed between barriers, max over ranks; value = all ranks'
    uncompressed bytes / that time.  The library's per-device counters must
    show every rank's blocks on its own GPU only: anything else (a rank whose
    blocks ran elsewhere, a mismatch on any rank) fails every rank loudly."""
    ops = ops or GpuHostOps(dev)
    mask = 1 << local
    raw = np.empty(nblk * U, dtype=np.uint8)
    raw[:] = ops.gen(nblk, U, S.seed_base(rank, nblk) + 70001)
    bound = ops.bound(U)
    comp = np.zeros(nblk * bound, dtype=np.uint8)
    pairs = [(comp[i * bound:(i + 1) * bound], raw[i * U:(i + 1) * U]) for i in range(nblk)]
    ops.compress(pairs, mask)  # warm: staging pinned, scratch sized
    ops.reset_stats()
    holder = {}

    def comp_step():
        holder["c"] = ops.compress(pairs, mask)
    tc = S.max_over_ranks(S.timed_steps(comp_step, 1, 0, lambda: None, world), world, dev)
    res = holder["c"]
    sizes = [n for n, e in res]
    ok = all(e is None and n > 0 for n, e in res)
    out = np.zeros(nblk * U, dtype=np.uint8)
    dpairs = [(out[i * U:(i + 1) * U], comp[i * bound:i * bound + sizes[i]]) for i in range(nblk)]
    ops.decompress(dpairs, mask)  # warm

    def dec_step():
        holder["d"] = ops.decompress(dpairs, mask)
    td = S.max_over_ranks(S.timed_steps(dec_step, 1, 0, lambda: None, world), world, dev)
    ok = ok and all(e is None and n == U for n, e in holder["d"]) and np.array_equal(out, raw)
    if not S.all_ranks_ok(ok, world, dev):
        raise RuntimeError("ranked host path: round trip mismatch on some rank")
    mine = ops.device_blocks()
    # every rank's blocks ran on its own GPU only
    if not S.all_ranks_ok(set(mine) == {local}, world, dev):
        raise RuntimeError(f"ranked host path: rank {rank} (local {local}) blocks ran on devices {sorted(mine)}; "
                           "some rank's device_mask was not honoured")
    total = world * nblk * U
    return {"decompress": {"value": total / td / 2**30, "unit": "GiB/s", "s": td},
            "compress": {"value": total / tc / 2**30, "unit": "GiB/s", "s": tc},
            "value": total / td / 2**30,
            "blocks_per_gpu": nblk, "n_gpus": world, "scaling": "weak",
            "rank0_device_blocks": mine, "each_rank_used_only_its_gpu": True,
            "path": "configs[0] per rank: jfs_compress_batch / jfs_decompress_batch with device_mask = 1 << "
                    "local_rank, host buffers, barrier-bracketed, max over ranks; every block verified"}


# ---------------------------------------------------------------------------
# device-resident sub-records (every rank)
# ---------------------------------------------------------------------------
def timed_launches(fn, steps, warmup, S, world, dev):
    """warmup + exactly `steps` launches between barriers; (max wall over
    ranks, mean HIP-event ms per launch on the launch stream)."""
    import torch
    stream = torch.cuda.current_stream()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    k = [0]

    def step():
        if k[0] >= warmup:
            i = k[0] - warmup
            ev[i][0].record(stream)
            fn(stream)
            ev[i][1].record(stream)
        else:
            fn(stream)
        k[0] += 1

    el = S.timed_steps(step, steps, warmup, torch.cuda.synchronize, world)
    el = S.max_over_ranks(el, world, dev)
    return el, float(np.mean([s.elapsed_time(e) for s, e in ev]))


def configs3_zstd(a, S, world, rank, dev):
    """BASELINE configs[3]: Zstd level-3 decode of 4096 x 4 MiB frames in HBM."""
    from juicefs_amd import device as D
    zb = D.ZstdBatch(a.blocks, a.block_bytes, a.cls, level=a.level, distinct=256, seed_base=S.seed_base(rank, 256),
                     device=dev)
    el, kms = timed_launches(zb.decompress, a.zstd_steps, 1, S, world, dev)
    if not S.all_ranks_ok(zb.verify(), world, dev):
        raise RuntimeError("configs[3] decoded output mismatch")
    U = a.block_bytes
    global ZSTD_FRAMES
    ZSTD_FRAMES = [zb.comp[i * zb.slot:i * zb.slot + int(zb.csize[i])].cpu().numpy().tobytes()
                   for i in range(min(16, a.blocks))]
    traffic, traffic_src = measured_traffic(a.zstd_traffic_file, a.blocks, U, ZSTD_KERNEL_SOURCES)
    return {"config": f"Zstd level-{a.level} decode, {a.blocks}x4MiB frames in HBM per GPU (BASELINE configs[3])",
            "value": S.whole_job_gib_s(world, a.blocks, U, a.zstd_steps, el), "unit": "GiB/s",
            "ms_per_step": el / a.zstd_steps * 1e3, "steps": a.zstd_steps, "n_gpus": world,
            "kernel_ms": kms, "ratio": a.blocks * U / zb.comp_bytes,
            "roofline": {"bound": "hbm", "achieved": (zb.comp_bytes + a.blocks * U) / (kms / 1e3) / 1e9,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": (zb.comp_bytes + a.blocks * U) / (kms / 1e3) / 1e9 / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": traffic_src,
                         "algorithmic_bytes_per_launch": zb.comp_bytes + a.blocks * U},
            "data": "synthetic text-like, 256 distinct blocks compressed by the host libzstd, replicated",
            "verified": "every frame's output compared with its source"}


def configs2_roundtrip(a, S, world, rank, dev):
    """BASELINE configs[2]: LZ4 compress + decompress of 4 MiB blocks dealt
    round-robin over the GPUs (block i -> rank i % N); a step = one encode
    launch + one decode launch over the rank's share, device-resident."""
    from juicefs_amd import device as D
    nb = a.c2_blocks
    # global block i = rank + N*j: the rank's share of a round-robin deal
    b = D.Lz4Batch(nb, a.block_bytes, a.cls, seed_base=700001 + rank * nb, device=dev)

    def step(stream):
        b.compress(stream)
        b.decompress(stream)

    el, kms = timed_launches(step, 3, 1, S, world, dev)
    if not S.all_ranks_ok(b.verify(), world, dev):
        raise RuntimeError("configs[2] round trip mismatch")
    U = a.block_bytes
    return {"config": f"LZ4 compress + decompress, {nb} x 4 MiB blocks per GPU, round-robin over {world} GPU(s) "
                      f"(BASELINE configs[2])",
            "value": S.whole_job_gib_s(world, nb, U, 3, el), "unit": "GiB/s",
            "ms_per_step": el / 3 * 1e3, "n_gpus": world, "blocks_per_gpu": nb,
            "step_kernel_ms": kms,
            "note": "value = uncompressed bytes / (encode + decode time) over all ranks; every block's compressed "
                    "size and decoded bytes verified"}


def checksum_and_aead(batch, S, world, dev):
    """SURVEY.md 8(f)4 and 8(f)3 on the headline's own buffers: CRC-32C of the
    4096 decoded 4 MiB blocks (object checksum + the disk cache's per-32 KiB
    sums, pkg/object/checksum.go:30-45, pkg/chunk/disk_cache_file.go:139-152)
    and AES-256-GCM seal of the 4096 compressed blocks (what an encrypted
    volume PUTs after compression, pkg/object/encrypt.go:226-257)."""
    import torch
    from juicefs_amd import device as D
    n, U = batch.nblk, batch.U
    offs = np.arange(n, dtype=np.int64)
    words = (U - 1) // (32 << 10) + 1
    sums = torch.empty(n * 4 * words, dtype=torch.uint8, device=dev)
    desc = D.make_desc(batch.out, offs * U, [U] * n, sums, offs * 4 * words, [4 * words] * n)
    crc = torch.empty(n, dtype=torch.int32, device=dev)
    ret = torch.empty(n, dtype=torch.int32, device=dev)
    el, kms = timed_launches(lambda st: D.crc32c(desc, crc, ret, seg_bytes=32 << 10, stream=st), 3, 1, S, world, dev)
    out = {"crc32c": {"value": S.whole_job_gib_s(world, n, U, 3, el), "unit": "GiB/s", "kernel_ms": kms,
                      "roofline": {"bound": "hbm", "achieved": n * U / (kms / 1e3) / 1e9, "peak": HBM_PEAK_GBS,
                                   "unit": "GB/s", "frac": n * U / (kms / 1e3) / 1e9 / HBM_PEAK_GBS},
                      "workload": f"{n} x 4 MiB decoded blocks: whole-block CRC-32C + big-endian sums per 32 KiB"}}
    rng = np.random.default_rng(5)
    kn = torch.from_numpy(rng.integers(0, 256, 64 * n, dtype=np.uint8)).to(dev)
    slot = batch.slot + 16
    sealed = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    adesc = D.make_aead_desc(batch.comp, offs * batch.slot, batch.csize, sealed, offs * slot, batch.csize + 16, kn,
                             offs * 64, offs * 64 + 32)
    aret = torch.empty(n, dtype=torch.int32, device=dev)
    el, kms = timed_launches(lambda st: D.aes256gcm(adesc, aret, True, stream=st), 3, 1, S, world, dev)
    if not bool((aret.cpu().numpy().astype(np.int64) == batch.csize + 16).all()):
        raise RuntimeError("AES-GCM seal failed")
    C = int(batch.csize.sum())
    for name in ("chacha20", "sm4gcm"):
        r2 = torch.empty(n, dtype=torch.int32, device=dev)
        el2, kms2 = timed_launches(lambda st, nm=name: D.aead(nm, adesc, r2, True, stream=st), 3, 1, S, world, dev)
        if not bool((r2.cpu().numpy().astype(np.int64) == batch.csize + 16).all()):
            raise RuntimeError(f"{name} seal failed")
        out[f"{name}_seal"] = {"value": world * C * 3 / el2 / 2**30, "unit": "GiB/s", "kernel_ms": kms2,
                               "roofline": {"bound": "hbm", "achieved": 2 * C / (kms2 / 1e3) / 1e9,
                                            "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                            "frac": 2 * C / (kms2 / 1e3) / 1e9 / HBM_PEAK_GBS},
                               "workload": f"{n} compressed blocks, one key/nonce per block (encrypt.go "
                                           f"{'CHACHA20_RSA' if name == 'chacha20' else 'SM4GCM'}); GiB/s of plaintext"}
    out["aes256gcm_seal"] = {"value": world * C * 3 / el / 2**30, "unit": "GiB/s", "kernel_ms": kms,
                             "roofline": {"bound": "hbm", "achieved": 2 * C / (kms / 1e3) / 1e9, "peak": HBM_PEAK_GBS,
                                          "unit": "GB/s", "frac": 2 * C / (kms / 1e3) / 1e9 / HBM_PEAK_GBS},
                             "workload": f"{n} compressed blocks ({C / n / 2**20:.2f} MiB each), one key/nonce per "
                                         "block; GiB/s of plaintext"}
    return out


def other_classes(a, S, world, rank, dev, nblk=1024):
    """SURVEY.md 8d data classes besides text: Z (zeros: a few long matches per
    block, the copy engine's bandwidth) and R (random: stored literal runs,
    a sanity bound near a device memcpy).  LZ4 decode of nblk x 4 MiB blocks
    in HBM, every block verified."""
    from juicefs_amd import device as D
    out = {}
    for cls in ("Z", "R"):
        b = D.Lz4Batch(nblk, a.block_bytes, cls, seed_base=S.seed_base(rank, nblk) + 777, device=dev)
        el, kms = timed_launches(b.decompress, 3, 1, S, world, dev)
        if not S.all_ranks_ok(b.verify(), world, dev):
            raise RuntimeError(f"class {cls}: decoded output mismatch")
        C = int(b.csize.sum())
        ach = (C + nblk * a.block_bytes) / (kms / 1e3) / 1e9
        out[cls] = {"value": S.whole_job_gib_s(world, nblk, a.block_bytes, 3, el), "unit": "GiB/s", "kernel_ms": kms,
                    "ratio": nblk * a.block_bytes / C, "blocks": nblk,
                    "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                 "frac": ach / HBM_PEAK_GBS}}
        del b
    return out


def measured_traffic(path, nblk, U, sources=KERNEL_SOURCES):
    """HBM bytes per launch from profiles/traffic.json (traffic_zstd.json for
    the Zstd decoder), only if it was measured on these kernel sources at this
    workload."""
    try:
        tj = json.load(open(path))
    except Exception:
        return None, "no traffic file"
    if tj.get("blocks") != nblk or tj.get("block_bytes") != U:
        return None, "traffic file is for another workload"
    if tj.get("kernel_src_sha256") != kernel_src_sha256(sources):
        return None, "traffic file is stale (kernel sources changed since it was measured)"
    stamp = tj.get("git_head") or f"kernel sources sha256 {tj.get('kernel_src_sha256', '')[:12]}"
    return tj.get("hbm_bytes_per_launch"), f"rocprofv3 PMC FETCH_SIZE/WRITE_SIZE ({stamp})"


DUMP_SAMPLE = 8 << 20  # decoded bytes kept by --dump-outputs (32 MiB as float32)


def dump_outputs(batch, dirpath, seed=20240917):
    """--dump-outputs: what a caller of batch.decompress holds after the last
    timed step.  decoded.npy = the output buffer's bytes as float32, all of
    them up to DUMP_SAMPLE, else the bytes at DUMP_SAMPLE seeded random
    offsets (ascending; the same offsets for the same blocks x block_bytes);
    sizes.npy = the per-block return values as float64."""
    import torch
    if batch.out.is_cuda:
        torch.cuda.synchronize()
    os.makedirs(dirpath, exist_ok=True)
    n = batch.out.numel()
    sample = batch.out
    if n > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(seed).integers(0, n, DUMP_SAMPLE, dtype=np.int64))
        sample = batch.out[torch.from_numpy(idx).to(batch.out.device)]
    np.save(os.path.join(dirpath, "decoded.npy"), sample.to(torch.float32).cpu().numpy())
    np.save(os.path.join(dirpath, "sizes.npy"), batch.dec_ret.to(torch.float64).cpu().numpy())


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(_spawn_ranks(a.gpus))

    import torch
    import torch.distributed as dist

    from juicefs_amd import shard as S
    env = S.rank_env()
    world, rank, local = env.world, env.rank, env.local
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if world > 1 and torch.cuda.device_count() < world:
        raise SystemExit(f"--gpus {world}: only {torch.cuda.device_count()} GPUs visible to rank {rank}")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)

    from juicefs_amd import device as D

    U, nblk = a.block_bytes, a.blocks
    t_setup = time.perf_counter()
    if a.codec == "lz4":
        batch = D.Lz4Batch(nblk, U, a.cls, seed_base=S.seed_base(rank, nblk), device=dev)
    else:
        batch = D.ZstdBatch(nblk, U, a.cls, level=a.level, distinct=256, seed_base=S.seed_base(rank, 256), device=dev)
    C = batch.comp_bytes
    setup_s = time.perf_counter() - t_setup

    # barrier + synchronize on both sides of exactly a.steps steps; max over ranks
    elapsed, kms = timed_launches(batch.decompress, a.steps, a.warmup, S, world, dev)
    kern_s = kms / 1e3
    if a.dump_outputs and rank == 0:
        dump_outputs(batch, a.dump_outputs)
    if a.full and not S.all_ranks_ok(batch.verify(), world, dev):
        raise SystemExit("decoded output mismatch: benchmark invalid")

    ms_per_step = elapsed / a.steps * 1e3
    value = S.whole_job_gib_s(world, nblk, U, a.steps, elapsed)
    achieved = (C + nblk * U) / kern_s / 1e9
    traffic, traffic_src = (None, "not measured for zstd")
    if a.codec == "lz4":
        traffic, traffic_src = measured_traffic(a.traffic_file, nblk, U)
        workload = "LZ4 decompress, 4096x4MiB blocks already in HBM (BASELINE configs[1])"
        kernel = "jfs::lz4d::lz4_decode_kernel"
        data = "synthetic (text-like blocks generated on GPU, SURVEY.md 8d; LZ4-compressed on GPU)"
    else:
        workload = f"Zstd level-{a.level} decompress, {nblk}x4MiB frames already in HBM (BASELINE configs[3])"
        kernel = "zscan + zlit + zseq + zexec (whole jfs_zstd_decompress_device call)"
        data = (f"synthetic text-like blocks (SURVEY.md 8d), {batch.distinct} distinct, compressed on the host by "
                f"libzstd level {a.level}, replicated to {nblk} frames")
    out = {
        "metric": METRIC,
        "value": value,
        "unit": "GiB/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": data,
        "config": {
            "workload": workload,
            "blocks_per_gpu": nblk, "block_bytes": U, "class": a.cls,
            "compressed_bytes_per_gpu": C, "ratio": nblk * U / C,
            "parallelism": f"{world} process(es), one per GPU, blocks sharded, no collective",
        },
        "roofline": {
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_src,
            "kernel": kernel, "kernel_ms": kms,
            "algorithmic_bytes_per_launch": C + nblk * U,
            "u_only_TBps": nblk * U / kern_s / 1e12,
        },
        "setup_s": setup_s,
    }
    extras = a.full and not a.no_extras
    if extras and a.codec == "lz4":
        try:
            _mark("configs_3")
            out["configs_3"] = configs3_zstd(a, S, world, rank, dev)
        except Exception as e:  # report, never fake
            out["configs_3"] = {"error": repr(e)}
        try:
            _mark("configs_2")
            out["configs_2"] = configs2_roundtrip(a, S, world, rank, dev)
        except Exception as e:
            out["configs_2"] = {"error": repr(e)}
        try:
            _mark("checksum_aead")
            out["checksum_aead"] = checksum_and_aead(batch, S, world, dev)
        except Exception as e:
            out["checksum_aead"] = {"error": repr(e)}
        try:
            _mark("lz4_other_classes")
            out["lz4_other_classes"] = other_classes(a, S, world, rank, dev)
        except Exception as e:
            out["lz4_other_classes"] = {"error": repr(e)}
    if extras and a.codec == "lz4" and world > 1 and not a.no_host_path:
        try:
            _mark("host_path_ranked")
            out["host_path_ranked"] = ranked_host_path(S, world, rank, local, dev, a.c0_blocks // 4, U)
        except Exception as e:
            out["host_path_ranked"] = {"error": repr(e)}
        # the single-process dealer (north_star's form of configs[4]): rank 0
        # alone drives every visible GPU through the batch ABI (device_mask 0
        # = all), round-robin per block; the other ranks wait at the barrier
        if rank == 0:
            try:
                _mark("dealer_all_gpus")
                out["dealer_all_gpus"] = dealer_legs(batch, U, a, world)
            except Exception as e:
                out["dealer_all_gpus"] = {"error": repr(e)}
        S._barrier(world)
    if a.full and rank == 0 and world == 1:
        # bounded sample for the CPU legs: 32 distinct blocks of the headline batch
        ns = min(32, nblk)
        comp_blocks = [batch.comp[i * batch.slot:i * batch.slot + int(batch.csize[i])].cpu().numpy().tobytes()
                       for i in range(ns)]
        if not a.no_cpu_baseline:
            T = host_threads()
            if a.codec == "lz4":
                cb = liblz4_baseline(comp_blocks, U, a.cpu_seconds, T)
                if cb is not None:
                    one = liblz4_baseline(comp_blocks, U, a.cpu_seconds / 3, 1)
                    cb["one_core"] = {"value": one["value"], "unit": "GiB/s"} if one else None
                    out["cpu_baseline"] = cb
                out["cpu_oracle"] = oracle_baseline(comp_blocks, U, a.cpu_seconds / 3, a.codec)
            else:
                out["cpu_baseline"] = libzstd_baseline(comp_blocks, U, a.cpu_seconds)
                out["cpu_oracle"] = oracle_baseline(comp_blocks, U, a.cpu_seconds / 3, a.codec)
        if extras and a.codec == "lz4":
            ex = {"lz4_compress": {"value": nblk * U / (batch.enc_ms / 1e3) / 2**30, "unit": "GiB/s",
                                   "kernel_ms": batch.enc_ms, "blocks": nblk,
                                   "note": "one GPU LZ4 encode launch (byte-identical to LZ4_compress_default)"}}
            try:
                zr, zratio, zms = D.zstd_compress_rate(min(a.extra_blocks, nblk), U, a.cls, seed_base=7, device=dev)
                ex["zstd_compress"] = {"value": zr, "unit": "GiB/s", "ratio": zratio, "kernel_ms": zms,
                                       "blocks": min(a.extra_blocks, nblk),
                                       "note": "one GPU Zstd encode launch; frames verified by the GPU decoder"}
            except Exception as e:  # report, never fake
                ex["zstd_compress"] = {"error": repr(e)}
            _mark("compress")
            out["compress"] = ex
            if not a.no_cpu_baseline:
                try:
                    rb = [batch.raw[i * U:(i + 1) * U].cpu().numpy().tobytes() for i in range(ns)]
                    out["cpu_codecs"] = cpu_codec_legs(rb, comp_blocks, ZSTD_FRAMES, U, a.cpu_seconds / 2)
                except Exception as e:
                    out["cpu_codecs"] = {"error": repr(e)}
            if not a.no_host_path:
                raw_blocks = [batch.raw[i * U:(i + 1) * U].cpu().numpy().tobytes() for i in range(ns)]
                try:
                    _mark("configs_0")
                    out["configs_0"] = configs0_roundtrip(dev, a.c0_blocks, U)
                except Exception as e:
                    out["configs_0"] = {"error": repr(e)}
                try:
                    _mark("host_path")
                    out["host_path"] = host_path_rate(comp_blocks, raw_blocks, U, a.host_blocks)
                except Exception as e:
                    out["host_path"] = {"error": repr(e)}
                try:
                    _mark("oneshot_concurrency")
                    out["oneshot_concurrency"] = oneshot_concurrency(comp_blocks, raw_blocks, U)
                except Exception as e:
                    out["oneshot_concurrency"] = {"error": repr(e)}
                if not a.no_mixed:
                    try:
                        _mark("mixed_host_path")
                        out["mixed_host_path"] = mixed_host_path(raw_blocks, a.mixed_blocks)
                    except Exception as e:
                        out["mixed_host_path"] = {"error": repr(e)}
    if rank == 0:
        print(json.dumps(out), flush=True)
        if a.full:
            # the full line is ~45 KB and a driver may keep only the tail of stdout:
            # a compact record (the same top-level fields, so it is itself a valid
            # result line) carrying every leg's headline figures follows it
            print(json.dumps(summary_record(out)), flush=True)
    if world > 1:
        dist.destroy_process_group()


def _pick(d, *path):
    """d[path...] rounded, or None when any step is missing / an error record."""
    for k in path:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    if isinstance(d, float):
        return round(d, 4 if abs(d) < 1 else 2)
    return d


def summary_record(out):
    """The result line's top-level fields plus a 'summary' of every leg
    (value, ms, roofline frac, traffic), kept under ~2 KB."""
    top = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                               "higher_is_better", "scaling", "vs_baseline", "dtype", "data") if k in out}
    top["value"] = _pick(out, "value")
    top["ms_per_step"] = _pick(out, "ms_per_step")
    top["data"] = "synthetic"
    top["config"] = {"workload": _pick(out, "config", "workload")}
    rf = out.get("roofline", {})
    top["roofline"] = {k: _pick(rf, k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic")}
    cb = out.get("cpu_baseline")
    if isinstance(cb, dict):
        top["cpu_baseline"] = {k: _pick(cb, k) for k in ("value", "unit", "cores", "kind")}
        top["cpu_baseline"]["one_core"] = _pick(cb, "one_core", "value")
        top["cpu_baseline"]["sample"] = "32 distinct headline blocks, liblz4 LZ4_decompress_safe"
    s = {}
    c3 = out.get("configs_3", {})
    s["configs_3"] = {"GiBs": _pick(c3, "value"), "ms": _pick(c3, "ms_per_step"),
                      "frac": _pick(c3, "roofline", "frac"), "traffic": _pick(c3, "roofline", "traffic")}
    s["configs_2"] = {"GiBs": _pick(out, "configs_2", "value"), "ms": _pick(out, "configs_2", "ms_per_step")}
    s["configs_0"] = {"GiBs": _pick(out, "configs_0", "value"),
                      "dec": _pick(out, "configs_0", "decompress", "value"),
                      "enc": _pick(out, "configs_0", "compress", "value")}
    s["configs_4_mixed"] = {"dec": _pick(out, "mixed_host_path", "decompress", "value"),
                            "enc": _pick(out, "mixed_host_path", "compress", "value")}
    s["host_path"] = {"dec": _pick(out, "host_path", "lz4_decompress", "value"),
                      "enc": _pick(out, "host_path", "lz4_compress", "value")}
    s["compress"] = {"lz4": _pick(out, "compress", "lz4_compress", "value"),
                     "zstd": _pick(out, "compress", "zstd_compress", "value")}
    oc = out.get("oneshot_concurrency", {})
    s["oneshot_lz4"] = {"dec_lone_p50_ms": _pick(oc, "decompress_lone", "p50_ms"),
                        "enc_lone_p50_ms": _pick(oc, "compress_lone", "p50_ms"),
                        "dec200_GiBs": _pick(oc, "decompress_200_concurrent", "value"),
                        "dec200_p99_ms": _pick(oc, "decompress_200_concurrent", "p99_ms"),
                        "dec200_native_GiBs": _pick(oc, "decompress_200_concurrent_native", "value"),
                        "dec200_native_p99_ms": _pick(oc, "decompress_200_concurrent_native", "p99_ms"),
                        "enc20_GiBs": _pick(oc, "compress_20_concurrent", "value")}
    s["oneshot_zstd"] = {"dec_lone_p50_ms": _pick(oc, "zstd", "decompress_lone", "p50_ms"),
                         "enc_lone_p50_ms": _pick(oc, "zstd", "compress_lone", "p50_ms"),
                         "dec20_GiBs": _pick(oc, "zstd", "decompress_20_concurrent", "value"),
                         "enc20_GiBs": _pick(oc, "zstd", "compress_20_concurrent", "value")}
    s["checksum_aead_GiBs"] = {k: _pick(out, "checksum_aead", k, "value")
                               for k in ("crc32c", "chacha20_seal", "sm4gcm_seal", "aes256gcm_seal")}
    s["lz4_classes_GiBs"] = {k: _pick(out, "lz4_other_classes", k, "value") for k in ("Z", "R")}
    s["cpu_codecs_16t"] = {k: _pick(out, "cpu_codecs", k, "value")
                           for k in ("lz4_compress", "zstd1_compress", "zstd_decompress_configs3")}
    for k in ("host_path_ranked", "dealer_all_gpus"):
        if k in out:
            s[k] = _pick(out, k, "value")
    top["summary"] = s
    return top


if __name__ == "__main__":
    main()
