"""The fast Zstd encoder on the GPU: the two new kernels against their host
twin record for record, jfs_zstd_compress_fast_device's frames through three
decoders, capacity and determinism rules, and the host-buffer calls in fast
parse mode.

Sizes, fast / exact level 1 (oracle.zstd_compress_l1), measured on an MI355X:
see DESIGN.md 4f.  The guard on T-200003 is the measured ratio plus 0.05."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest
import torch

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests import zstd_fast_cases as K

pytestmark = pytest.mark.gpu
CANARY = 0xA5
T200003_RATIO = 1.1474  # fast 73,409 / exact 63,976 bytes on T-200003, measured


def run_fast(dev, srcs, caps, shift=0):
    """Encode srcs[i] into a dst of caps[i] bytes; src and dst sit at odd offsets
    (moved by `shift`) inside canary-filled tensors.  Returns (ret, frames,
    whole dst array, dst offsets)."""
    soffs, doffs, so, do = [], [], 1 + shift, 3 + shift
    for s, c in zip(srcs, caps):
        soffs.append(so)
        doffs.append(do)
        so += len(s) + (3 if len(s) % 2 else 2)  # keeps every offset's parity
        do += c + (3 if c % 2 else 2)
    hsrc = np.full(so + 16, CANARY, dtype=np.uint8)
    for s, o in zip(srcs, soffs):
        hsrc[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    dsrc = torch.from_numpy(hsrc).to(dev)
    ddst = torch.full((do + 16,), CANARY, dtype=torch.uint8, device=dev)
    desc = D.make_desc(dsrc, soffs, [len(s) for s in srcs], ddst, doffs, caps)
    ret = torch.full((len(srcs),), -7, dtype=torch.int32, device=dev)
    D.zstd_compress_fast(desc, ret)
    torch.cuda.synchronize()
    r = ret.cpu().tolist()
    got = ddst.cpu().numpy()
    return r, [got[o:o + max(x, 0)].tobytes() for o, x in zip(doffs, r)], got, doffs


def canaries_intact(got, doffs, frames):
    want = np.full(len(got), CANARY, dtype=np.uint8)
    for o, f in zip(doffs, frames):
        want[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return np.array_equal(got, want)


def _libzstd_decode(frame, n):
    z = D._libzstd()
    if z is None:
        return None
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    buf = ctypes.create_string_buffer(max(n, 1))
    m = z.ZSTD_decompress(buf, n, frame, len(frame))
    assert not z.ZSTD_isError(m), "libzstd refuses the frame"
    return buf.raw[:m]


@pytest.fixture(scope="module")
def batch(gpu):
    """The shared case list encoded once in one mixed batch: (cases, ret, frames, dst, offsets)"""
    cs = K.cases()
    srcs = [s for _, s in cs]
    r, frames, got, doffs = run_fast(gpu, srcs, [D.zstd_bound(len(s)) for s in srcs])
    return cs, r, frames, got, doffs


def test_kernels_equal_twin(gpu):
    """every case in one device buffer, each at its own (odd) address"""
    cs = K.cases()
    offs, o = [], 1
    for _, s in cs:
        offs.append(o)
        o += len(s) + (3 if len(s) % 2 else 2)
    h = np.full(o + 16, CANARY, dtype=np.uint8)
    for (_, s), a in zip(cs, offs):
        h[a:a + len(s)] = np.frombuffer(s, dtype=np.uint8)
    d = torch.from_numpy(h).to(gpu)
    bad = []
    for (name, s), a in zip(cs, offs):
        if C.zstd_fast_seqs(s, device_ptr=d.data_ptr() + a) != C.zstd_fast_seqs(s):
            bad.append(name)
    assert not bad, bad


def test_frames_decode_three_ways(gpu, oracle, batch):
    cs, r, frames, got, doffs = batch
    for (name, s), x, f in zip(cs, r, frames):
        assert 0 < x <= D.zstd_bound(len(s)), (name, x)
        n, out = oracle.zstd_decompress(f, len(s))
        assert n == len(s) and out == s, name
        back = _libzstd_decode(f, len(s))
        assert back is None or back == s, name
    assert canaries_intact(got, doffs, frames), "a byte outside dst[0, ret) was written"
    from tests.test_zstd_gpu import run_device
    r2, outs = run_device(frames, [len(s) for _, s in cs], gpu, src_mis=3, dst_mis=5)
    assert r2 == [len(s) for _, s in cs] and outs == [s for _, s in cs]
    # n == 0 behaves as the exact encoder
    assert frames[0].hex() == "28b52ffd2000010000"


def test_capacity_rule(gpu, batch):
    cs, r, frames, _, _ = batch
    pick = [i for i, (name, _) in enumerate(cs) if name in ("T-0", "T-13", "T-65537", "zeros-262144", "R-65537")]
    srcs = [cs[i][1] for i in pick]
    bounds = [D.zstd_bound(len(s)) for s in srcs]
    # one byte under the bound: -2 and not a byte written, however small the frame would be
    ret, fr, got, doffs = run_fast(gpu, srcs, [b - 1 for b in bounds])
    assert ret == [-2] * len(srcs)
    assert (got == CANARY).all()
    ret, fr, got, doffs = run_fast(gpu, srcs, bounds)
    assert fr == [frames[i] for i in pick]


def test_bytes_do_not_depend_on_batch_or_alignment(gpu, batch):
    cs, r, frames, _, _ = batch
    d = dict(cs)
    src = d["T-200003"]
    want = frames[[n for n, _ in cs].index("T-200003")]
    alone = run_fast(gpu, [src], [D.zstd_bound(len(src))], shift=2)[1][0]
    assert alone == want
    others = [s for _, s in cs if len(s) >= 65535][:8] * 4
    srcs = others[:17] + [src] + others[17:32]
    assert len(srcs) == 33
    fr = run_fast(gpu, srcs, [D.zstd_bound(len(s)) for s in srcs], shift=1)[1]
    assert fr[17] == want


def test_size_guard_and_lz4(gpu, oracle, batch):
    cs, r, frames, _, _ = batch
    src = dict(cs)["T-200003"]
    fast = len(frames[[n for n, _ in cs].index("T-200003")])
    exact = len(oracle.zstd_compress_l1(src))
    lz4 = oracle.lz4_compress(src)[0]
    print(f"T-200003: fast {fast} exact {exact} ratio {fast / exact:.4f} lz4 {lz4}")
    assert fast <= (T200003_RATIO + 0.05) * exact
    assert fast < lz4, "no smaller than the exact LZ4 block"


def test_full_size_text_frame(gpu, lib, oracle):
    """32 blocks, 64 chunks: seq_cap and the block lists at the workload's size"""
    buf = ctypes.create_string_buffer(4 << 20)
    lib.jfs_gen_block_host(ctypes.addressof(buf), 4 << 20, b"T", 1)
    src = buf.raw
    r, frames, got, doffs = run_fast(gpu, [src], [D.zstd_bound(len(src))])
    print(f"T 4 MiB seed 1: fast {r[0]} exact {len(oracle.zstd_compress_l1(src))}")
    assert 0 < r[0] <= D.zstd_bound(len(src)) and canaries_intact(got, doffs, frames)
    n, out = oracle.zstd_decompress(frames[0], len(src))
    assert n == len(src) and out == src
    from tests.test_zstd_gpu import run_device
    r2, outs = run_device(frames, [len(src)], gpu)
    assert r2 == [len(src)] and outs[0] == src


def _host_blocks():
    return [gen_block("T", 31, 200003), gen_block("Z", 32, 300000), gen_block("R", 33, 5000),
            gen_block("T", 34, 65536), gen_block("T", 35, 6), b""]


def _decodes(oracle, frame, src):
    n, out = oracle.zstd_decompress(frame, len(src))
    return n == len(src) and out == src


def test_fast_mode_host_calls(gpu, lib, oracle):
    z = C.ZStandard()
    blocks = _host_blocks()
    exact = [oracle.zstd_compress_l1(b) for b in blocks]
    with C.zstd_parse_mode("fast"):
        for b, e in zip(blocks, exact):
            d = bytearray(z.CompressBound(len(b)))
            n, err = z.Compress(d, b)
            assert err is None and _decodes(oracle, bytes(d[:n]), b)
            if len(b) > 65536:
                assert bytes(d[:n]) != e  # the fast parse ran, not the exact one
            out = bytearray(len(b))
            m, err = z.Decompress(out, bytes(d[:n]))
            assert err is None and m == len(b) and bytes(out) == b
        pairs = [(bytearray(z.CompressBound(len(b))), b) for b in blocks]
        for (d, b), (n, err, crc) in zip(pairs, z.CompressBatchChecksum(pairs)):
            assert err is None and _decodes(oracle, bytes(d[:n]), b) and crc == oracle.crc32c(bytes(d[:n]))
        # a dst below the bound keeps its meaning
        n, err = z.Compress(bytearray(z.CompressBound(len(blocks[0])) - 1), blocks[0])
        assert err is not None and "buffer too short" in str(err)
    assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT
    # back in exact mode, same process: libzstd's bytes again
    for b, e in zip(blocks[:3], exact):
        d = bytearray(z.CompressBound(len(b)))
        n, err = z.Compress(d, b)
        assert err is None and bytes(d[:n]) == e


def test_fast_mode_compress_seal_roundtrip(gpu, lib):
    rng = random.Random(5)
    blocks = _host_blocks()[:5]
    params = [(bytes(rng.randrange(256) for _ in range(32)), bytes(rng.randrange(256) for _ in range(12)),
               bytes(rng.randrange(256) for _ in range(256))) for _ in blocks]
    pairs = [(bytearray(E.envelope_bound(L.ALGO_ZSTD, len(b), 256)), b) for b in blocks]
    with C.zstd_parse_mode("fast"):
        res = E.compress_seal_batch(L.ALGO_ZSTD, E.AES256GCM_RSA, pairs, params)
    assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT
    envs = []
    for (d, b), (n, err) in zip(pairs, res):
        assert err is None
        envs.append(bytes(d[:n]))
    outs = [bytearray(len(b)) for b in blocks]
    back = E.open_decompress_batch(L.ALGO_ZSTD, E.AES256GCM_RSA, list(zip(outs, envs)), [p[0] for p in params])
    for o, b, (n, err) in zip(outs, blocks, back):
        assert err is None and n == len(b) and bytes(o) == b


def test_fast_mode_compact_batch(gpu, lib, oracle):
    z = C.ZStandard()
    S = 100 << 10
    raws = [gen_block("T", 41, S), gen_block("Z", 42, S), gen_block("T", 43, S)]
    objs = [oracle.zstd_compress_l1(r) for r in raws]
    seg = [(0, 0, 0, S), (-1, 0, S, 5000), (1, 100, S + 5000, 50000), (1, 50100, 0, S - 50100), (2, 0, S - 50100, S)]
    seg_first = [0, 3, 5]
    gathered = [raws[0] + bytes(5000) + raws[1][100:50100], raws[1][50100:] + raws[2]]
    outs = [bytearray(z.CompressBound(len(g))) for g in gathered]
    with C.zstd_parse_mode("fast"):
        sres, ores, crcs = z.CompactBatch([(o, S) for o in objs], outs, (seg_first, seg), with_crc=True)
    assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT
    assert [r for r, e in sres] == [S, S, S] and all(e is None for r, e in sres)
    for g, o, (n, err), crc in zip(gathered, outs, ores, crcs):
        assert err is None and _decodes(oracle, bytes(o[:n]), g) and crc == oracle.crc32c(bytes(o[:n]))
        assert bytes(o[:n]) != oracle.zstd_compress_l1(g)


def test_exact_mode_still_writes_the_golden_frame(gpu, lib):
    """one case of tests/golden/zstd_l1_golden.json, with the fast mode used just before"""
    from tests.zstd_l1_cases import make_case
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "zstd_l1_golden.json")))
    case = [c for c in g["cases"] if c["kind"] == "M" and c["size"] == 300000][0]
    src = make_case(case["kind"], case["seed"], case["size"])
    z = C.ZStandard()
    with C.zstd_parse_mode("fast"):
        d = bytearray(z.CompressBound(len(src)))
        n, err = z.Compress(d, src)
        assert err is None and hashlib.sha256(bytes(d[:n])).hexdigest() != case["comp_sha"]
    with C.zstd_parse_mode("exact"):
        d = bytearray(z.CompressBound(len(src)))
        n, err = z.Compress(d, src)
    assert err is None and n == case["csize"] and hashlib.sha256(bytes(d[:n])).hexdigest() == case["comp_sha"]
