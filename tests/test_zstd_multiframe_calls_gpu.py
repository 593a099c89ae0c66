"""GPU: every host call that decodes whole Zstd objects replays 5-frame
seekable objects block-parallel: the bytes are the input's, and
jfs_zstd_split_frame_counts moves by the number of multi-frame objects, which
proves the route and not just the result."""
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block

pytestmark = pytest.mark.gpu
B = 128 << 10
N = 5 * B - 3
_cache = {}


def objects(gpu):
    """seven (raw, 5-frame seekable object) and three (raw, single frame)"""
    if not _cache:
        z = C.ZStandard()
        raws = [gen_block("T", 7500 + i, N) for i in range(7)]
        small = [gen_block("T", 7600 + i, 30000 + 1000 * i) for i in range(3)]
        with C.zstd_parse_mode("seekable"):
            pairs = [(bytearray(z.CompressBound(len(r))), r) for r in raws + small]
            res = z.CompressBatch(pairs)
        assert all(e is None for _, e in res)
        objs = [bytes(d[:n]) for (d, _), (n, _) in zip(pairs, res)]
        _cache["multi"] = list(zip(raws, objs[:7]))
        _cache["single"] = list(zip(small, objs[7:]))
    return _cache["multi"], _cache["single"]


def moved(fn, multi):
    """run fn; the frame counters moved by `multi` objects of five frames and nothing was handed"""
    D.zstd_split_counts(reset=True)
    D.zstd_split_frame_counts(reset=True)
    out = fn()
    done, handed = D.zstd_split_counts()
    assert handed == 0 and done >= multi, (done, handed)
    assert D.zstd_split_frame_counts() == (multi, 5 * multi)
    return out


def test_decompress(gpu):
    (raw, obj), = objects(gpu)[0][:1]
    out = bytearray(N)
    n, err = moved(lambda: C.ZStandard().Decompress(out, obj), 1)
    assert err is None and n == N and bytes(out) == raw


def test_decompress_batch(gpu):
    multi, single = objects(gpu)
    mix = multi[:3] + single[:1] + multi[3:5] + single[1:] + multi[5:]
    pairs = [(bytearray(len(r)), o) for r, o in mix]
    res = moved(lambda: C.ZStandard().DecompressBatch(pairs), 7)
    for (dst, _), (raw, _), (n, err) in zip(pairs, mix, res):
        assert err is None and n == len(raw) and bytes(dst) == raw


# two sources, each range crossing a frame edge
PLAN = ([0, 2], [(0, B - 100, 0, 300), (1, 2 * B - 50, 300, 200)])


def expect(multi):
    return multi[0][0][B - 100:B + 200] + multi[1][0][2 * B - 50:2 * B + 150]


def test_compact_batch(gpu, oracle):
    multi, _ = objects(gpu)
    z = C.ZStandard()
    out = bytearray(z.CompressBound(500))
    src_res, out_res = moved(lambda: z.CompactBatch([(o, N) for _, o in multi[:2]], [out], PLAN), 2)
    assert src_res == [(N, None)] * 2 and out_res[0][1] is None
    n, back = oracle.zstd_decompress(bytes(out[:out_res[0][0]]), 500)
    assert n == 500 and back == expect(multi)


def test_read_batch(gpu):
    multi, _ = objects(gpu)
    assert C.read_decode_mode() == "full" and C.read_seek_mode() == "off"
    dst = bytearray(500)
    res = moved(lambda: C.ZStandard().ReadBatch([(o, N) for _, o in multi[:2]], [dst], PLAN), 2)
    assert res[0] == [(N, None)] * 2 and res[1] == [(500, None)]
    assert bytes(dst) == expect(multi)


def test_open_decompress_batch(gpu, oracle):
    (raw, obj), = objects(gpu)[0][:1]
    key, nonce, wrapped = bytes(range(32)), bytes(range(12)), bytes(256)
    env = oracle.envelope(wrapped, nonce, oracle.seal("aes256gcm", key, nonce, obj))
    out = bytearray(N)
    res = moved(lambda: E.open_decompress_batch(L.ALGO_ZSTD, E.AES256GCM_RSA, [(out, env)], [key]), 1)
    assert res == [(N, None)] and bytes(out) == raw
