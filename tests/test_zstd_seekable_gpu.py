"""GPU: seekable Zstd objects.  jfs_zstd_compress_seekable_device
writes one frame per 128 KiB block and a seek table, checked with the test's
own table parser and header reader (tests/zstd_seek_cases.py) and through four
decoders; jfs_zstd_decompress_range_device decodes only the frames a byte range
touches, checked on encoder output and on hand-built objects for results,
bytes and untouched canaries, against lying tables and damaged frames, and on
both decode paths.

Sizes, seekable / fast (measured on an MI355X): T-200003
73,577 / 73,535 bytes = 1.0006; the guard is that ratio plus 0.01."""
import ctypes

import numpy as np
import pytest
import torch

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd.blockgen import gen_block
from tests import zstd_seek_cases as S
from tests.test_zstd_fast_gpu import _libzstd_decode
from tests.test_zstd_prefix_gpu import run as run_prefix

pytestmark = pytest.mark.gpu
CANARY = 0xA5
B = S.FRAME
SIZES = [0, 1, 6, B, B + 1, 2 * B, 3 * B + 5, 200003, (1 << 20) + 7]
T200003_RATIO = 1.0006  # seekable 73,577 / fast 73,535 bytes on T-200003 (seed 7016), measured


def encode(dev, srcs, caps, seekable=True, shift=0):
    """srcs[i] into a dst of caps[i] bytes, both at odd offsets (moved by shift)
    inside canary-filled tensors -> (ret, objects, whole dst array, dst offsets)"""
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
    (D.zstd_compress_seekable if seekable else D.zstd_compress_fast)(desc, ret)
    torch.cuda.synchronize()
    r = ret.cpu().tolist()
    got = ddst.cpu().numpy()
    return r, [got[o:o + max(x, 0)].tobytes() for o, x in zip(doffs, r)], got, doffs


def intact(got, doffs, objs):
    want = np.full(len(got), CANARY, dtype=np.uint8)
    for o, f in zip(doffs, objs):
        want[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return np.array_equal(got, want)


def run_range(dev, objs, caps, los, his):
    """One jfs_zstd_decompress_range_device call; every dst at an odd offset in a
    canary-filled tensor -> (rets, the whole tensor, dst offsets)"""
    so, do, off, doff = [], [], 0, 0
    for i, s in enumerate(objs):
        so.append(off + (7 * i) % 16 + 1)
        off = (so[-1] + len(s) + 64 + 15) & ~15
        do.append(doff + 1 + 2 * ((5 * i) % 8))
        doff = (do[-1] + max(caps[i], 0) + 64 + 15) & ~15
    host = np.zeros(off + 64, dtype=np.uint8)
    for s, o in zip(objs, so):
        host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    src_t = torch.from_numpy(host).to(dev)
    dst_t = torch.full((doff + 64,), CANARY, dtype=torch.uint8, device=dev)
    desc = D.make_desc(src_t, so, [len(s) for s in objs], dst_t, do, caps)
    ret = torch.full((len(objs),), -12345, dtype=torch.int32, device=dev)
    D.zstd_decompress_range(desc, torch.tensor(los, dtype=torch.int32, device=dev),
                            torch.tensor(his, dtype=torch.int32, device=dev), ret)
    torch.cuda.synchronize()
    return ret.cpu().tolist(), dst_t.cpu().numpy(), do


def check_image(img, do, writes):
    """the whole tensor: writes = [(input, flo, bytes)], canaries everywhere else"""
    want = np.full(len(img), CANARY, dtype=np.uint8)
    for i, flo, data in writes:
        want[do[i] + flo:do[i] + flo + len(data)] = np.frombuffer(data, dtype=np.uint8)
    bad = np.nonzero(img != want)[0]
    assert bad.size == 0, f"first wrong byte at {bad[0]} of the dst tensor"


def expect_range(obj, raw, cap, lo, hi):
    """(ret, flo, fhi) of a well-formed object with a table"""
    sel = S.select(obj, cap, lo, hi)
    if min(hi, cap) <= max(lo, 0):
        return 0, 0, 0
    return min(len(raw), min(hi, cap)), sel["flo"], sel["fhi"]


_cache = {}


def objects(dev):
    """(class, n) -> (raw, seekable object, fast frame), encoded once in two batches"""
    if "objs" not in _cache:
        keys = [(cls, n) for cls in "TZR" for n in SIZES] + [("T", 4 * B + 777), ("Z", B + 4000)]
        raws = [gen_block(cls, 7000 + i, n) for i, (cls, n) in enumerate(keys)]
        caps = [D.zstd_bound(len(r)) for r in raws]
        r, objs, got, doffs = encode(dev, raws, caps)
        assert all(0 < x <= c for x, c in zip(r, caps)), r
        assert intact(got, doffs, objs), "a byte outside dst[0, ret) was written"
        r2, fast, _, _ = encode(dev, raws, caps, seekable=False)
        _cache["objs"] = {k: (raw, o, f) for k, raw, o, f in zip(keys, raws, objs, fast)}
    return _cache["objs"]


@pytest.mark.parametrize("cls", ["T", "Z", "R"])
def test_encoder_layout(gpu, oracle, cls):
    from tests.test_zstd_gpu import run_device
    for n in SIZES:
        raw, obj, fast = objects(gpu)[(cls, n)]
        if n <= B:
            assert obj == fast, (cls, n)
            assert S.parse_table(obj) is None
            continue
        ent = S.parse_table(obj)
        nb = -(-n // B)
        assert ent is not None and len(ent) == nb, (cls, n)
        assert [d for _, d in ent] == [min(B, n - k * B) for k in range(nb)]
        at, frames = 0, []
        for k, (c, d) in enumerate(ent):
            info = S.frame_info(obj, at)
            assert info["size"] == c and info["content"] == d and info["single"] == 1, (cls, n, k, info)
            assert info["checksum"] == 0 and info["did"] == 0
            assert len(info["blocks"]) == 1 and info["blocks"][0][1] == 1, (cls, n, k)
            assert info["blocks"][0][2] != 3, "a treeless literal section in a frame of its own"
            frames.append(obj[at:at + c])
            at += c
        assert at + 8 * nb + 17 == len(obj)
        # every frame alone, and the object whole
        for k, f in enumerate(frames):
            m, out = oracle.zstd_decompress(f, B)
            assert m == ent[k][1] and out == raw[k * B:k * B + m], (cls, n, k)
        m, out = oracle.zstd_decompress(obj, n)
        assert m == n and out == raw, (cls, n)
        back = _libzstd_decode(obj, n)
        assert back is None or back == raw, (cls, n)
    big = [(objects(gpu)[(cls, n)][1], objects(gpu)[(cls, n)][0]) for n in SIZES if n > B]
    r, outs = run_device([o for o, _ in big], [len(w) for _, w in big], gpu, src_mis=3, dst_mis=5)
    assert r == [len(w) for _, w in big] and outs == [w for _, w in big]
    z = C.ZStandard()
    for o, w in big:
        out = bytearray(len(w))
        m, err = z.Decompress(out, o)
        assert err is None and m == len(w) and bytes(out) == w


def test_bytes_do_not_depend_on_batch_or_alignment(gpu):
    raw, want, _ = objects(gpu)[("T", 200003)]
    assert encode(gpu, [raw], [D.zstd_bound(len(raw))], shift=2)[1][0] == want
    others = [objects(gpu)[("T", n)][0] for n in (B + 1, 2 * B, 3 * B + 5, 6)] * 8
    srcs = others[:17] + [raw] + others[17:32]
    assert len(srcs) == 33
    assert encode(gpu, srcs, [D.zstd_bound(len(s)) for s in srcs], shift=1)[1][17] == want


def test_capacity_rule(gpu):
    srcs = [objects(gpu)[k][0] for k in (("T", 2 * B), ("R", B + 1), ("Z", 3 * B + 5), ("T", 6))]
    bounds = [D.zstd_bound(len(s)) for s in srcs]
    ret, _, got, _ = encode(gpu, srcs, [b - 1 for b in bounds])
    assert ret == [-2] * len(srcs) and (got == CANARY).all()


def test_size_guard(gpu):
    raw, obj, fast = objects(gpu)[("T", 200003)]
    print(f"T-200003: seekable {len(obj)} fast {len(fast)} ratio {len(obj) / len(fast):.4f}")
    assert len(obj) <= (T200003_RATIO + 0.01) * len(fast)


def test_host_calls_in_seekable_mode(gpu, lib, oracle):
    z = C.ZStandard()
    blocks = [gen_block("T", 31, 200003), gen_block("Z", 32, 300000), gen_block("R", 33, 5000), b""]
    assert lib.jfs_set_zstd_parse_mode(2) == -1
    prev = C.set_zstd_parse_mode("seekable")
    try:
        objs = []
        for b in blocks:
            d = bytearray(z.CompressBound(len(b)))
            n, err = z.Compress(d, b)
            assert err is None
            objs.append(bytes(d[:n]))
            out = bytearray(len(b))
            m, err = z.Decompress(out, objs[-1])
            assert err is None and m == len(b) and bytes(out) == b
        assert [len(S.parse_table(o) or []) for o in objs] == [2, 3, 0, 0]
        pairs = [(bytearray(z.CompressBound(len(b))), b) for b in blocks]
        for (d, b), (n, err), o in zip(pairs, z.CompressBatch(pairs), objs):
            assert err is None and bytes(d[:n]) == o
        n, err = z.Compress(bytearray(z.CompressBound(len(blocks[0])) - 1), blocks[0])
        assert err is not None and "buffer too short" in str(err)
    finally:
        assert C.set_zstd_parse_mode(prev) == "seekable"
    assert lib.jfs_zstd_parse_mode() == L.ZSTD_PARSE_EXACT
    m, out = oracle.zstd_decompress(objs[0], len(blocks[0]))
    assert m == len(blocks[0]) and out == blocks[0]


def ranges_for(n):
    return [(0, 1), (B - 1, B + 1), (2 * B, 2 * B + 1), (n - 1, n), (0, n), (5, 5), (-9, 3), (n - 5, n + 1000),
            (n, n + 7), (n + 100, 1 << 30), (B, B)]


@pytest.mark.parametrize("key", [("T", 4 * B + 777), ("Z", B + 4000)])
def test_ranges(gpu, key):
    raw, obj, _ = objects(gpu)[key]
    n = len(raw)
    rs = [r for r in ranges_for(n) if r[0] < n + 2 * B]
    rets, img, do = run_range(gpu, [obj] * len(rs), [n] * len(rs), [lo for lo, _ in rs], [hi for _, hi in rs])
    writes = []
    for i, (lo, hi) in enumerate(rs):
        ret, flo, fhi = expect_range(obj, raw, n, lo, hi)
        assert rets[i] == ret, (lo, hi, rets[i], ret)
        writes.append((i, flo, raw[flo:fhi]))
    check_image(img, do, writes)
    # a capacity above the content: hi > D; a capacity below it: -2 and nothing written
    rets, img, do = run_range(gpu, [obj, obj, obj], [n + 100, n - 1, n + 100], [n - 1, 0, n], [n + 50, 10, n + 100])
    assert rets == [n, -2, n]
    last = S.select(obj, n + 100, n - 1, n + 50)
    check_image(img, do, [(0, last["flo"], raw[last["flo"]:])])


def test_mixed_batch_and_objects_without_a_table(gpu, oracle):
    raw5, obj5, fast5 = objects(gpu)[("T", 4 * B + 777)]
    raw2, obj2, _ = objects(gpu)[("Z", B + 4000)]
    exact = oracle.zstd_compress_l1(raw2)
    broken = bytearray(obj5)
    broken[-1] ^= 1  # footer magic: an ordinary object of five frames
    broken = bytes(broken)
    # more than 64 frames: the scan's second round
    many_raw = [gen_block("T", 7100 + k, 100 + k) for k in range(70)]
    many, _ = S.build(many_raw)
    mraw = b"".join(many_raw)
    objs = [obj5, fast5, exact, broken, obj2, many, fast5]
    raws = [raw5, raw5, raw2, raw5, raw2, mraw, raw5]
    caps = [len(r) for r in raws]
    los = [3 * B + 9, 3 * B + 9, 70000, 2 * B, 0, 100 + 101 + 50, 0]
    his = [3 * B + 10, 3 * B + 10, 70001, 2 * B + 5, 1, len(mraw) - 3, caps[6] + 99]
    rets, img, do = run_range(gpu, objs, caps, los, his)
    plain = [1, 2, 3, 6]
    pr, pimg = run_prefix([objs[i] for i in plain], [caps[i] for i in plain], [his[i] for i in plain], gpu)
    writes = []
    for k, i in enumerate(plain):
        assert rets[i] == pr[k] == min(his[i], caps[i]), (i, rets[i], pr[k])
        # (bytes of dst[ret, dst_cap) are unspecified for a prefix decode: compare the prefix, canaries elsewhere)
        assert (img[do[i]:do[i] + rets[i]] == pimg[k][:rets[i]]).all() and pimg[k][:rets[i]].tobytes() == raws[i][:rets[i]]
        writes.append((i, 0, img[do[i]:do[i] + caps[i]].tobytes()))
    for i in (0, 4, 5):
        ret, flo, fhi = expect_range(objs[i], raws[i], caps[i], los[i], his[i])
        assert rets[i] == ret, (i, rets[i], ret)
        writes.append((i, flo, raws[i][flo:fhi]))
    assert S.select(many, caps[5], los[5], his[5])["first"] == 2 and S.select(many, caps[5], los[5], his[5])["count"] == 68
    check_image(img, do, writes)


def test_lying_table_and_damaged_frame(gpu):
    raw, obj, _ = objects(gpu)[("T", 4 * B + 777)]
    n = len(raw)
    ent = S.parse_table(obj)
    body = obj[:sum(c for c, _ in ent)]
    # frames 3 and 4 swap their decompressed sizes: every sum still holds
    lie = list(ent)
    lie[3], lie[4] = (ent[3][0], ent[4][1]), (ent[4][0], ent[3][1])
    lying = body + S.table(lie)
    assert S.parse_table(lying) == lie
    # one byte inside frame 3 changed: its content size, which the end of the frame is checked against
    # (a byte of an entropy stream may decode to other bytes of the same length, which no Zstd decoder sees)
    dmg = bytearray(obj)
    dmg[sum(c for c, _ in ent[:3]) + 5] ^= 0x5A
    dmg = bytes(dmg)
    objs = [lying, lying, lying, dmg, dmg, dmg]
    los = [3 * B + 5, 3 * B + 800, B + 1, B + 1, 3 * B - 1, 0]
    his = [3 * B + 6, n, 2 * B + 1, B + 2, 3 * B + 1, n]
    rets, img, do = run_range(gpu, objs, [n] * 6, los, his)
    assert rets[0] == -1 and rets[1] == -1 and rets[2] == 2 * B + 1
    assert rets[3] == B + 2 and rets[4] == -1 and rets[5] == -1
    for i in (2, 3):
        assert img[do[i] + B:do[i] + (3 * B if i == 2 else 2 * B)].tobytes() == raw[B:(3 * B if i == 2 else 2 * B)]
    # whatever a failed frame wrote stayed inside the selected frames' output ranges
    spans = {0: (3 * B, 3 * B + 777), 1: (3 * B + 777, n), 2: (B, 3 * B), 3: (B, 2 * B), 4: (2 * B, 4 * B), 5: (0, n)}
    writes = [(i, a, img[do[i] + a:do[i] + b].tobytes()) for i, (a, b) in spans.items()]
    check_image(img, do, writes)


def test_both_decode_paths(gpu):
    raw, obj, _ = objects(gpu)[("Z", B + 4000)]
    n = len(raw)
    D.zstd_split_counts(reset=True)
    rets, img, do = run_range(gpu, [obj], [n], [B - 1], [B + 1])
    done, handed = D.zstd_split_counts()
    assert rets == [B + 1] and done + handed == 2, "two frames through the small-batch path"
    check_image(img, do, [(0, 0, raw)])
    # 200 two-frame objects of about 140 KiB, every second one read at its end only: 300 frames, the entropy / exec path
    raws = [gen_block("T", 7300 + i, B + 12000 + 7 * i) for i in range(8)]
    objs = encode(gpu, raws, [D.zstd_bound(len(r)) for r in raws])[1]
    objs, raws = (objs * 25)[:200], (raws * 25)[:200]
    los = [0 if i % 2 == 0 else B + 5 for i in range(200)]
    his = [len(r) for r in raws]
    D.zstd_split_counts(reset=True)
    rets, img, do = run_range(gpu, objs, his, los, his)
    assert D.zstd_split_counts() == (0, 0), "300 frames take the one-wave path"
    assert rets == his
    check_image(img, do, [(i, 0 if i % 2 == 0 else B, raws[i][0 if i % 2 == 0 else B:]) for i in range(200)])
