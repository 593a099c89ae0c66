"""GPU: checksummed seekable Zstd objects.
jfs_zstd_compress_seekable_csum_device writes the seekable call's frames, byte
for byte, and a table of 12-byte entries whose third word is the low half of
XXH64 of the frame's content (tests/xxh64_ref.py); every Zstd reader, the
existing range decoder included, still reads the object."""
import struct

import numpy as np
import pytest
import torch

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd.blockgen import gen_block
from tests import zstd_seek_cases as S
from tests import zstd_seek_csum_cases as X
from tests.test_zstd_fast_gpu import _libzstd_decode
from tests.test_zstd_seekable_gpu import CANARY, intact, run_range
from tests.xxh64_ref import xxh64

pytestmark = pytest.mark.gpu
B = S.FRAME
SIZES = [B, B + 1, 2 * B, 4 * B + 777, 69 * B + 5]  # one frame; 2, 2, 5 and 70 frames
_cache = {}


def encode(dev, srcs, caps, fn, shift=0):
    """tests.test_zstd_seekable_gpu.encode for either encoder"""
    soffs, doffs, so, do = [], [], 1 + shift, 3 + shift
    for s, c in zip(srcs, caps):
        soffs.append(so)
        doffs.append(do)
        so += len(s) + (3 if len(s) % 2 else 2)
        do += c + (3 if c % 2 else 2)
    hsrc = np.full(so + 16, CANARY, dtype=np.uint8)
    for s, o in zip(srcs, soffs):
        hsrc[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    dsrc = torch.from_numpy(hsrc).to(dev)
    ddst = torch.full((do + 16,), CANARY, dtype=torch.uint8, device=dev)
    desc = D.make_desc(dsrc, soffs, [len(s) for s in srcs], ddst, doffs, caps)
    ret = torch.full((len(srcs),), -7, dtype=torch.int32, device=dev)
    fn(desc, ret)
    torch.cuda.synchronize()
    r = ret.cpu().tolist()
    got = ddst.cpu().numpy()
    return r, [got[o:o + max(x, 0)].tobytes() for o, x in zip(doffs, r)], got, doffs


def objects(dev):
    """(class, n) -> (raw, checksummed object, seekable object), each encoder once"""
    if "objs" not in _cache:
        keys = [(cls, n) for cls in "TZR" for n in SIZES]
        raws = [gen_block(cls, 7500 + i, n) for i, (cls, n) in enumerate(keys)]
        caps = [D.zstd_bound(len(r)) for r in raws]
        r, objs, got, doffs = encode(dev, raws, caps, D.zstd_compress_seekable_csum)
        assert all(0 < x <= c for x, c in zip(r, caps)), r
        assert intact(got, doffs, objs), "a byte outside dst[0, ret) was written"
        r8, objs8, _, _ = encode(dev, raws, caps, D.zstd_compress_seekable)
        _cache["objs"] = {k: (raw, o, o8) for k, raw, o, o8 in zip(keys, raws, objs, objs8)}
        _cache["batch"] = objs
    return _cache["objs"]


def split(obj, n):
    """(frames' bytes, table) of a checksummed object of n content bytes"""
    nb = -(-n // B)
    return obj[:len(obj) - (12 * nb + 17)], obj[len(obj) - (12 * nb + 17):]


@pytest.mark.parametrize("cls", ["T", "Z", "R"])
def test_layout_and_checksums(gpu, oracle, cls):
    for n in SIZES:
        raw, obj, obj8 = objects(gpu)[(cls, n)]
        if n <= B:
            assert obj == obj8 and S.parse_table(obj) is None, (cls, n)  # one frame: no table
            continue
        nb = -(-n // B)
        ent8 = S.parse_table(obj8)
        assert ent8 is not None and len(ent8) == nb
        assert len(obj) == len(obj8) + 4 * nb, (cls, n)  # ret = seekable ret + 4 nb
        body, t = split(obj, n)
        assert body == obj8[:len(obj8) - (8 * nb + 17)], "the frames are the seekable call's, byte for byte"
        p = X.parse(t, len(obj))
        assert p is not None and p[1] is True, (cls, n)
        assert [(c, d) for c, d, _ in p[0]] == list(ent8)
        assert t == X.table(p[0]), "the 12-byte table, field by field"
        assert struct.unpack_from("<II", t, 0) == (S.SKIP_MAGIC, 12 * nb + 9) and t[-5] == 0x80
        for k, (_, d, x) in enumerate(p[0]):
            assert x == xxh64(raw[k * B:k * B + d]) & 0xFFFFFFFF, (cls, n, k)
        # ordinary Zstd objects to every reader
        m, out = oracle.zstd_decompress(obj, n)
        assert m == n and out == raw, (cls, n)
        back = _libzstd_decode(obj, n)
        assert back is None or back == raw, (cls, n)
        assert S.parse_table(obj) is None, "to the in-object parser a table with checksums is no table"


def test_range_decoder_reads_it_as_no_table(gpu):
    keys = [("T", 4 * B + 777), ("Z", 2 * B), ("R", B + 1)]
    objs = [objects(gpu)[k][1] for k in keys]
    raws = [objects(gpu)[k][0] for k in keys]
    his = [3 * B + 10, 2 * B, B + 1]
    rets, img, do = run_range(gpu, objs, [len(r) for r in raws], [3 * B + 9, 0, B], his)
    assert rets == his  # a prefix decode with want = hi
    for i, r in enumerate(raws):
        assert img[do[i]:do[i] + his[i]].tobytes() == r[:his[i]]


def test_deterministic_and_independent_of_the_batch(gpu):
    raw, want, _ = objects(gpu)[("T", 4 * B + 777)]
    assert encode(gpu, [raw], [D.zstd_bound(len(raw))], D.zstd_compress_seekable_csum, shift=2)[1][0] == want
    others = [objects(gpu)[("Z", n)][0] for n in (B + 1, 2 * B, B)]
    srcs = others + [raw] + others
    got = encode(gpu, srcs, [D.zstd_bound(len(s)) for s in srcs], D.zstd_compress_seekable_csum, shift=1)[1]
    assert got[3] == want and got[:3] == got[4:] == [objects(gpu)[("Z", n)][1] for n in (B + 1, 2 * B, B)]


def test_capacity_rule(gpu):
    srcs = [objects(gpu)[k][0] for k in (("T", 2 * B), ("R", B + 1), ("Z", 4 * B + 777), ("T", B))]
    bounds = [D.zstd_bound(len(s)) for s in srcs]
    ret, _, got, _ = encode(gpu, srcs, [b - 1 for b in bounds], D.zstd_compress_seekable_csum)
    assert ret == [-2] * len(srcs) and (got == CANARY).all()


def test_host_calls_with_the_switch_on(gpu, lib):
    z = C.ZStandard()
    keys = [("T", 4 * B + 777), ("Z", 2 * B), ("R", B + 1), ("T", B)]
    blocks = [objects(gpu)[k][0] for k in keys]
    prev = C.set_zstd_parse_mode("seekable")
    try:
        assert C.set_zstd_seek_csum_mode("on") == "off"
        pairs = [(bytearray(z.CompressBound(len(b))), b) for b in blocks]
        for (d, b), (n, err), k in zip(pairs, z.CompressBatch(pairs), keys):
            assert err is None and bytes(d[:n]) == objects(gpu)[k][1], k
        d = bytearray(z.CompressBound(len(blocks[0])))
        n, err = z.Compress(d, blocks[0])
        assert err is None and bytes(d[:n]) == objects(gpu)[keys[0]][1]
        out = bytearray(len(blocks[0]))
        m, err = z.Decompress(out, bytes(d[:n]))
        assert err is None and m == len(blocks[0]) and bytes(out) == blocks[0]
        # off again: the 8-byte table; and the switch alone (another parse mode) changes nothing
        assert C.set_zstd_seek_csum_mode("off") == "on"
        n, err = z.Compress(d, blocks[0])
        assert err is None and bytes(d[:n]) == objects(gpu)[keys[0]][2]
    finally:
        C.set_zstd_seek_csum_mode("off")
        assert C.set_zstd_parse_mode(prev) == "seekable"
    assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT
    C.set_zstd_seek_csum_mode("on")
    try:
        d = bytearray(z.CompressBound(len(blocks[1])))
        n, err = z.Compress(d, blocks[1])
        assert err is None and X.parse(bytes(d[n - 17 - 24:n]), n) is None and S.parse_table(bytes(d[:n])) is None
    finally:
        C.set_zstd_seek_csum_mode("off")
