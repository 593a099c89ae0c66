"""The fast LZ4 encoder on the GPU: jfs_lz4_compress_fast_device against its
host twin byte for byte, capacity and determinism rules, decode through the
project's GPU decoders, and the host-buffer calls in fast parse mode."""
import random

import numpy as np
import pytest
import torch

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests import lz4_fast_cases as K

pytestmark = pytest.mark.gpu
CANARY = 0xA5


@pytest.fixture(scope="module")
def twins():
    """[(name, src, twin bytes)] for the shared input list, computed once"""
    return [(name, src, C.lz4_fast_host(src)) for name, src in K.cases()]


def run_fast(dev, srcs, caps):
    """Encode srcs[i] into a dst of caps[i] bytes; src and dst sit at odd offsets
    inside canary-filled tensors.  Returns (ret, whole dst tensor, dst offsets)."""
    soffs, doffs, so, do = [], [], 1, 3
    for s, c in zip(srcs, caps):
        soffs.append(so)
        doffs.append(do)
        so += len(s) + (3 if len(s) % 2 else 2)  # keeps every offset odd
        do += c + (3 if c % 2 else 2)
    hsrc = np.full(so + 16, CANARY, dtype=np.uint8)
    for s, o in zip(srcs, soffs):
        hsrc[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    dsrc = torch.from_numpy(hsrc).to(dev)
    ddst = torch.full((do + 16,), CANARY, dtype=torch.uint8, device=dev)
    desc = D.make_desc(dsrc, soffs, [len(s) for s in srcs], ddst, doffs, caps)
    ret = torch.full((len(srcs),), -7, dtype=torch.int32, device=dev)
    D.lz4_compress_fast(desc, ret, [len(s) for s in srcs])
    torch.cuda.synchronize()
    return ret.cpu().tolist(), ddst.cpu().numpy(), doffs


def expect_dst(total, doffs, caps, outs):
    want = np.full(total, CANARY, dtype=np.uint8)
    for o, c, out in zip(doffs, caps, outs):
        assert len(out) <= c
        want[o:o + len(out)] = np.frombuffer(out, dtype=np.uint8)
    return want


def test_device_equals_twin_mixed_batch(gpu, oracle, twins):
    srcs = [s for _, s, _ in twins]
    caps = [oracle.lz4_bound(len(s)) for s in srcs]
    ret, got, doffs = run_fast(gpu, srcs, caps)
    bad = [name for (name, _, t), r in zip(twins, ret) if r != len(t)]
    assert not bad, bad[:10]
    want = expect_dst(len(got), doffs, caps, [t for _, _, t in twins])
    if not np.array_equal(got, want):
        first = int(np.flatnonzero(got != want)[0])
        blk = max(i for i, o in enumerate(doffs) if o <= first)
        pytest.fail(f"first difference at dst byte {first}: block {twins[blk][0]}, offset {first - doffs[blk]}")


def test_capacity_cases_in_one_batch(gpu, oracle, twins):
    pick = [t for t in twins if t[0] in ("T-200003", "zeros-131072", "R-65537", "period3-65548", "T-13",
                                         "lits-cross-chunk", "zeros-0")]
    assert len(pick) == 7
    srcs = [s for _, s, _ in pick]
    caps = [oracle.lz4_bound(len(s)) for s in srcs]
    outs = [t for _, _, t in pick]
    # block 0: one byte short; block 2: no room at all; block 4: exactly enough; block 6: empty input, no room
    caps[0], caps[2], caps[4], caps[6] = len(outs[0]) - 1, 0, len(outs[4]), 0
    outs[0] = outs[2] = outs[6] = b""
    ret, got, doffs = run_fast(gpu, srcs, caps)
    assert ret == [len(o) for o in outs]
    assert np.array_equal(got, expect_dst(len(got), doffs, caps, outs))


def test_bytes_do_not_depend_on_the_batch(gpu, oracle, twins):
    src = gen_block("T", 21, 200003)
    cap = oracle.lz4_bound(len(src))
    ret1, got1, d1 = run_fast(gpu, [src], [cap])
    others = [s for _, s, _ in twins if 60000 < len(s) < 140000][:32]
    assert len(others) == 32
    srcs = others[:17] + [src] + others[17:]
    assert len(srcs) == 33
    retn, gotn, dn = run_fast(gpu, srcs, [oracle.lz4_bound(len(s)) for s in srcs])
    assert ret1[0] > 0 and retn[17] == ret1[0]
    assert np.array_equal(got1[d1[0]:d1[0] + ret1[0]], gotn[dn[17]:dn[17] + ret1[0]])
    assert bytes(got1[d1[0]:d1[0] + ret1[0]]) == C.lz4_fast_host(src)


def _gpu_decode(dev, comps, sizes, small):
    offs, o = [], 0
    for c in comps:
        offs.append(o)
        o += (len(c) + 15) // 16 * 16
    h = np.zeros(max(o, 16), dtype=np.uint8)
    for c, off in zip(comps, offs):
        h[off:off + len(c)] = np.frombuffer(c, dtype=np.uint8)
    dcomp = torch.from_numpy(h).to(dev)
    ooffs = [int(x) for x in np.cumsum([0] + sizes[:-1])]
    dout = torch.zeros(max(sum(sizes), 16), dtype=torch.uint8, device=dev)
    desc = D.make_desc(dcomp, offs, [len(c) for c in comps], dout, ooffs, sizes)
    ret = torch.full((len(comps),), -7, dtype=torch.int32, device=dev)
    if small:
        D.lz4_decompress_small(desc, ret, [len(c) for c in comps], sizes)
    else:
        D.lz4_decompress(desc, ret)
    torch.cuda.synchronize()
    out = dout.cpu().numpy().tobytes()
    return ret.cpu().tolist(), [out[o:o + n] for o, n in zip(ooffs, sizes)]


@pytest.mark.parametrize("small", [False, True], ids=["decode", "decode_small"])
def test_outputs_decode_on_the_gpu(gpu, twins, small):
    use = [t for t in twins if len(t[1]) > 0]
    if small:
        use = use[::4]
    ret, back = _gpu_decode(gpu, [t for _, _, t in use], [len(s) for _, s, _ in use], small)
    assert ret == [len(s) for _, s, _ in use]
    assert back == [s for _, s, _ in use]


def _stats_blocks(lib):
    s = (L.JfsOpStats * L.STATS_N)()
    lib.jfs_stats(s, L.STATS_N)
    return int(s[L.ALGO_LZ4 * 2 + 0].blocks)


def _host_blocks():
    return [gen_block("T", 31, 200003), gen_block("Z", 32, 70000), gen_block("R", 33, 5000),
            gen_block("T", 34, 65536), gen_block("T", 35, 12)]


def test_fast_mode_host_calls(gpu, lib, oracle):
    c = C.LZ4()
    blocks = _host_blocks()
    want = [C.lz4_fast_host(b) for b in blocks]
    before = _stats_blocks(lib)
    with C.lz4_parse_mode("fast"):
        for b, w in zip(blocks, want):
            d = bytearray(c.CompressBound(len(b)))
            n, err = c.Compress(d, b)
            assert err is None and bytes(d[:n]) == w
        pairs = [(bytearray(c.CompressBound(len(b))), b) for b in blocks]
        for (d, b), w, (n, err) in zip(pairs, want, c.CompressBatch(pairs)):
            assert err is None and bytes(d[:n]) == w
        pairs = [(bytearray(c.CompressBound(len(b))), b) for b in blocks]
        for (d, b), w, (n, err, crc) in zip(pairs, want, c.CompressBatchChecksum(pairs)):
            assert err is None and bytes(d[:n]) == w and crc == oracle.crc32c(w)
        # a block that does not fit keeps its meaning
        n, err = c.Compress(bytearray(len(want[0]) - 1), blocks[0])
        assert n == 0 and err is not None and err.code == L.JFS_ERR_COMPRESS_FAIL
    assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_EXACT
    assert _stats_blocks(lib) - before == 3 * len(blocks) + 1
    # back in exact mode, same process: liblz4's bytes again
    for b in blocks[:3]:
        d = bytearray(c.CompressBound(len(b)))
        n, err = c.Compress(d, b)
        assert err is None and bytes(d[:n]) == oracle.lz4_compress(b)[1]


def test_fast_mode_compress_seal_roundtrip(gpu, lib):
    rng = random.Random(5)
    blocks = _host_blocks()
    params = [(bytes(rng.randrange(256) for _ in range(32)), bytes(rng.randrange(256) for _ in range(12)),
               bytes(rng.randrange(256) for _ in range(256))) for _ in blocks]
    pairs = [(bytearray(E.envelope_bound(L.ALGO_LZ4, len(b), 256)), b) for b in blocks]
    with C.lz4_parse_mode("fast"):
        res = E.compress_seal_batch(L.ALGO_LZ4, E.AES256GCM_RSA, pairs, params)
    assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_EXACT
    envs = []
    for (d, b), p, (n, err) in zip(pairs, params, res):
        assert err is None
        # the sealed payload is as long as the fast block
        assert n == 3 + 256 + 12 + len(C.lz4_fast_host(b)) + 16
        envs.append(bytes(d[:n]))
    outs = [bytearray(len(b)) for b in blocks]
    back = E.open_decompress_batch(L.ALGO_LZ4, E.AES256GCM_RSA, list(zip(outs, envs)), [p[0] for p in params])
    for o, b, (n, err) in zip(outs, blocks, back):
        assert err is None and n == len(b) and bytes(o) == b


def test_fast_mode_compact_batch(gpu, lib, oracle):
    c = C.LZ4()
    S = 100 << 10
    raws = [gen_block("T", 41, S), gen_block("Z", 42, S), gen_block("T", 43, S)]
    objs = [oracle.lz4_compress(r)[1] for r in raws]
    seg = [(0, 0, 0, S), (-1, 0, S, 5000), (1, 100, S + 5000, 50000), (1, 50100, 0, S - 50100), (2, 0, S - 50100, S)]
    seg_first = [0, 3, 5]
    gathered = [raws[0] + bytes(5000) + raws[1][100:50100], raws[1][50100:] + raws[2]]
    outs = [bytearray(c.CompressBound(len(g))) for g in gathered]
    before = _stats_blocks(lib)
    with C.lz4_parse_mode("fast"):
        sres, ores, crcs = c.CompactBatch([(o, S) for o in objs], outs, (seg_first, seg), with_crc=True)
    assert lib.jfs_lz4_parse_mode() == L.LZ4_PARSE_EXACT
    assert [r for r, e in sres] == [S, S, S] and all(e is None for r, e in sres)
    for g, o, (n, err), crc in zip(gathered, outs, ores, crcs):
        assert err is None and bytes(o[:n]) == C.lz4_fast_host(g) and crc == oracle.crc32c(bytes(o[:n]))
        dn, back = oracle.lz4_decompress(bytes(o[:n]), len(g))
        assert dn == len(g) and back == g
    assert _stats_blocks(lib) - before == 2


@pytest.mark.parametrize("cls", ["T", "Z", "R"])
def test_full_size_block(gpu, oracle, cls):
    src = gen_block(cls, 1, 4 << 20)
    want = C.lz4_fast_host(src)
    cap = oracle.lz4_bound(len(src))
    ret, got, doffs = run_fast(gpu, [src], [cap])
    assert ret == [len(want)]
    assert np.array_equal(got, expect_dst(len(got), doffs, [cap], [want]))
    r, back = _gpu_decode(gpu, [want], [len(src)], small=True)
    assert r == [len(src)] and back == [src]
