"""GPU: on-device read assembly -- the flat-grid gather (jfs_read_gather_device)
against numpy and against the 2-D gather on the same plans, and jfs_read_batch
/ jfs_read_open_batch (ReadBatch, read_open_batch) against the existing batch
decoders plus a numpy stitch, with the CRC-32C check in front.

Every output sits at an odd offset inside a larger canary-filled buffer and
the whole buffer is compared with its expected image, so a byte written
outside dst[0, total), or anything written for a failed read, fails the test."""
import random

import numpy as np
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests.test_compact_gpu import CANARY, INT32_MIN, _expected, _sources, _tile, check_exact

pytestmark = pytest.mark.gpu

K16 = 16 << 10


def run_both(gpu, sources, blocks, src_n=None):
    """test_compact_gpu.run_gather's placement (sources at mixed alignments,
    every dst at an odd offset of a canary-filled tensor), through
    jfs_read_gather_device and through jfs_gather_device: both images must be
    the same bytes.  Returns the flat grid's (ret, image, dst offsets)."""
    import torch
    from juicefs_amd import device as D
    soffs, o = [], 0
    for i, s in enumerate(sources):
        o = (o + 15) // 16 * 16 + (i * 5) % 16
        soffs.append(o)
        o += len(s)
    simg = np.zeros(o + 16, dtype=np.uint8)
    for s, so in zip(sources, soffs):
        simg[so:so + len(s)] = s
    sbuf = torch.from_numpy(simg).to(gpu)
    doffs, o = [], 64
    for j, (segs, cap) in enumerate(blocks):
        o = (o + 15) // 16 * 16 + (2 * j + 1) % 16
        doffs.append(o)
        o += max(cap, sum(s[3] for s in segs)) + 80
    lens = [len(s) for s in sources]
    sdesc = D.make_desc(sbuf, soffs, lens, sbuf, soffs, lens)
    n_t = torch.tensor(lens if src_n is None else src_n, dtype=torch.int32, device=gpu)
    seg_first, seg = [0], []
    for segs, _ in blocks:
        seg += segs
        seg_first.append(len(seg))
    caps = [c for _, c in blocks]
    got = []
    for flat in (True, False):
        dbuf = torch.full((o + 64,), CANARY, dtype=torch.uint8, device=gpu)
        odesc, sdev = D.make_compact_desc(dbuf, doffs, caps, seg_first, seg)
        ret = torch.full((len(blocks),), 12345, dtype=torch.int32, device=gpu)
        if flat:
            D.read_gather(sdesc, n_t, odesc, sdev, caps, ret)
        else:
            D.gather(sdesc, n_t, odesc, sdev, max(caps), ret)
        torch.cuda.synchronize()
        got.append((ret.cpu().tolist(), dbuf.cpu().numpy()))
    assert got[0][0] == got[1][0]
    assert np.array_equal(got[0][1], got[1][1]), "flat and 2-D grid wrote different bytes"
    return got[0][0], got[0][1], doffs


def _mixed(total, k=0):
    """a total made of a source run, a hole and another source run"""
    a, h = total // 3, total // 5
    return _tile([p for p in [(0, 9 + k, a), (-1, 0, h), (1, 1234 + 3 * k, total - a - h)] if p[2] > 0])


def test_read_gather_tile_prefix_totals(gpu):
    """totals around the 16-byte word and the 16 KiB tile, one batch: an
    off-by-one in the tile prefix moves a workgroup to the wrong output"""
    sources = _sources([70000, 70000], seed=31)
    totals = [0, 1, 15, 16, 17, K16 - 1, K16, K16 + 1]
    blocks = [(_mixed(t, k), t + (k % 2)) for k, t in enumerate(totals)]
    ret, img, doffs = run_both(gpu, sources, blocks)
    check_exact(sources, blocks, ret, img, doffs)
    assert ret == totals
    blocks.reverse()  # and with the large outputs first
    ret, img, doffs = run_both(gpu, sources, blocks)
    check_exact(sources, blocks, ret, img, doffs)


def test_read_gather_heterogeneous_batch(gpu):
    n = (1 << 20) + 3
    sources = _sources([n + 8, 70000], seed=32)
    blocks = [(_mixed(4096), 4096), ([(1, 77, 0, 1)], 1), ([(0, 5, 0, n)], n), (_mixed(4096, 5), 5000)]
    ret, img, doffs = run_both(gpu, sources, blocks)
    check_exact(sources, blocks, ret, img, doffs)


def test_read_gather_many_one_byte_segments(gpu):
    sources = _sources([9000, 9000], seed=33)
    parts = [((k % 3) - 1, (k * 7) % 9000, 1) for k in range(5000)]  # hole, source 0, source 1, ...
    blocks = [(_mixed(100), 100), (_tile(parts), 5000), ([], 0)]
    ret, img, doffs = run_both(gpu, sources, blocks)
    check_exact(sources, blocks, ret, img, doffs)


def test_read_gather_boundaries_inside_words_and_holes(gpu):
    sources = _sources([5000, 5000], seed=34)
    blocks = []
    for cut in range(1, 16):  # a segment boundary at every position of a 16-byte word, source/source and source/hole
        blocks.append((_tile([(0, cut, 32 + cut), (1, 3 * cut, 64 - cut), (-1, 0, cut), (0, 100, 48)]), 200))
    blocks.append((_tile([(-1, 0, 4097)]), 4097))           # a hole only
    blocks.append((_tile([(-1, 0, 1), (1, 0, 1), (-1, 0, 33)]), 64))
    blocks.append(([], 16))                                 # seg_count == 0
    ret, img, doffs = run_both(gpu, sources, blocks)
    check_exact(sources, blocks, ret, img, doffs)
    assert ret[-1] == 0


def test_read_gather_verdicts_per_read(gpu):
    sources = _sources([5000, 5000, 5000], seed=35)
    src_n = [5000, -7, 4000]  # source 1 failed; source 2 decoded 4000 bytes
    good = _tile([(0, 3, 700), (-1, 0, 50), (2, 100, 3900)])
    blocks = [
        (good, 4650),
        (_tile([(0, 0, 100), (1, 0, 100)]), 200),        # reads a failed source
        (_tile([(0, 0, 10), (2, 100, 3901)]), 3911),     # one byte past source 2's length
        (_tile([(0, 0, 10), (3, 0, 10)]), 20),           # src == nsrc
        ([(0, 0, 0, 10), (0, 10, 11, 10)], 64),          # broken tiling
        (_tile([(0, 0, 33), (-1, 0, 32)]), 64),          # total == dst_cap + 1
        (good, 4660),
    ]
    verdicts = [4650, INT32_MIN, INT32_MIN, -1, -1, -1, 4650]
    ret, img, doffs = run_both(gpu, sources, blocks, src_n=src_n)
    want = np.full(len(img), CANARY, dtype=np.uint8)  # nothing at all for a failed read or a bad plan
    for j in (0, 6):
        want[doffs[j]:doffs[j] + 4650] = _expected(sources, good)
    assert ret == verdicts
    assert np.array_equal(img, want)


def test_read_gather_scratch_regrows_behind_a_call_in_flight(gpu):
    """The tile prefix lives in a per-device scratch block shared by every caller, 1 MiB at first and ordered across
    calls by an event.  Three calls in a row on one stream, nothing waited for in between: 4 one-byte reads, 300,000
    (their prefix, (nout + 1) * 4 bytes, no longer fits, so the block is freed and regrown while the first call's event
    is outstanding), 4 again.  Every byte and every result against numpy."""
    import torch
    from juicefs_amd import device as D
    src = np.frombuffer(gen_block("R", 41, 4096), dtype=np.uint8)
    sbuf = torch.from_numpy(src.copy()).to(gpu)
    sdesc = D.make_desc(sbuf, [0], [4096], sbuf, [0], [4096])
    src_n = torch.tensor([4096], dtype=torch.int32, device=gpu)
    calls = []
    for k, n in enumerate((4, 300000, 4)):
        at = (np.arange(n, dtype=np.int64) * 7 + k) % 4096  # read j is source byte at[j]
        seg = np.stack([np.zeros(n, np.int64), at, np.zeros(n, np.int64), np.ones(n, np.int64)], axis=1)
        dbuf = torch.full((n + 64,), CANARY, dtype=torch.uint8, device=gpu)
        odesc, sdev = D.make_compact_desc(dbuf, np.arange(n) + 32, np.ones(n, np.int32), np.arange(n + 1), seg)
        ret = torch.full((n,), 12345, dtype=torch.int32, device=gpu)
        calls.append((n, at, dbuf, odesc, sdev, ret))
    assert (300000 + 1) * 4 > 1 << 20 >= (4 + 1) * 4
    for n, _, _, odesc, sdev, ret in calls:
        D.read_gather(sdesc, src_n, odesc, sdev, np.ones(n, np.int32), ret)
    torch.cuda.synchronize()
    for n, at, dbuf, _, _, ret in calls:
        want = np.full(n + 64, CANARY, dtype=np.uint8)
        want[32:32 + n] = src[at]
        assert np.array_equal(ret.cpu().numpy(), np.ones(n, np.int32)), n
        assert np.array_equal(dbuf.cpu().numpy(), want), n


# ---- jfs_read_batch -----------------------------------------------------------

SRC = [("T", 65539), ("T", 40000), ("R", 4097), ("Z", 1)]  # class, decoded length
BLOCK = 65539
READ_PARTS = [
    [(0, 5, 60000), (-1, 0, 15), (1, 40000 - 17, 17), (0, 65524, 15)],  # sources 0 and 1
    [(2, 1000, 17), (-1, 0, 4097), (3, 0, 1), (2, 4096, 1)],            # sources 2 and 3
    [(-1, 0, 17), (-1, 0, 4097)],                                       # holes only
    [],                                                                 # an empty read
    [(1, 3, 4096)],                                                     # source 1 only
    [(1, 39999, 1), (2, 0, 4097), (-1, 0, 1)],                          # sources 1 and 2
]
FED = {0: {0}, 1: {0, 4, 5}, 2: {1, 5}, 3: {1}}  # source -> reads


def _plan(parts=READ_PARTS):
    seg_first, seg = [0], []
    for p in parts:
        seg += _tile(p)
        seg_first.append(len(seg))
    return seg_first, seg


_cache = {}


def _raws():
    if "raws" not in _cache:
        _cache["raws"] = [gen_block(cls, 700 + i, n) for i, (cls, n) in enumerate(SRC)]
        _cache["want"] = C.read_expect(_cache["raws"], _plan())
    return _cache["raws"], _cache["want"]


def _stored(oracle, codec):
    """the stored objects, encoded by the CPU oracle"""
    if codec not in _cache:
        enc = {"none": lambda b: b, "lz4": lambda b: oracle.lz4_compress(b)[1], "zstd": oracle.zstd_compress_l1}[codec]
        _cache[codec] = [enc(r) for r in _raws()[0]]
    return list(_cache[codec])


class Dst:
    """Read buffers at odd offsets inside canary-filled arrays."""

    def __init__(self, caps):
        self.offs = [2 * j + 1 for j in range(len(caps))]
        self.arr = [np.full(o + c + 48, CANARY, dtype=np.uint8) for o, c in zip(self.offs, caps)]
        self.views = [a[o:o + c] for a, o, c in zip(self.arr, self.offs, caps)]

    def check(self, j, want: bytes):
        img = np.full(len(self.arr[j]), CANARY, dtype=np.uint8)
        img[self.offs[j]:self.offs[j] + len(want)] = np.frombuffer(want, dtype=np.uint8)
        bad = np.nonzero(img != self.arr[j])[0]
        assert bad.size == 0, f"read {j}: first wrong byte at {bad[0] - self.offs[j]} of dst ({bad.size} wrong)"


def _codes(res):
    return [(n, e.code if e else None) for n, e in res]


def _read(c, objs, caps=None, crcs=None, parts=READ_PARTS):
    caps = caps or [BLOCK] * len(objs)
    dst = Dst([sum(p[2] for p in ps) + (j % 2) for j, ps in enumerate(parts)])
    sres, rres, got = c.ReadBatch(list(zip(objs, caps)), dst.views, _plan(parts), crcs=crcs)
    return dst, sres, rres, got


def _check_reads(dst, rres, failed_sources, parts=READ_PARTS, want=None):
    """reads fed by a failed source: JFS_ERR_CORRUPT and an untouched dst; the others: the stitch"""
    want = _raws()[1] if want is None else want
    dead = set().union(*[FED.get(s, set()) for s in failed_sources]) if failed_sources else set()
    for j in range(len(parts)):
        if j in dead:
            assert _codes(rres)[j] == (0, L.JFS_ERR_CORRUPT), j
            dst.check(j, b"")
        else:
            assert rres[j] == (len(want[j]), None), (j, rres[j])
            dst.check(j, want[j])


def _stat(lib, algo, d):
    s = (L.JfsOpStats * L.STATS_N)()
    lib.jfs_stats(s, L.STATS_N)
    return s[algo * 2 + d]


@pytest.mark.parametrize("codec", ["none", "lz4", "zstd"])
def test_read_batch_matches_decompress_batch_and_stitch(gpu, lib, oracle, codec):
    import torch
    c = C.NewCompressor(codec)
    stored = _stored(oracle, codec)
    dev0 = torch.cuda.current_device()
    lib.jfs_stats_reset()
    dst, sres, rres, got = _read(c, stored)
    assert torch.cuda.current_device() == dev0
    dec = _stat(lib, c.algo, 1)
    assert (dec.calls, dec.blocks, dec.errors, dec.batches) == (1, 4, 0, 1)
    assert dec.bytes_in == sum(len(s) for s in stored) and dec.bytes_out == sum(n for _, n in SRC)
    for a in range(3):
        enc = _stat(lib, a, 0)
        assert (enc.calls, enc.blocks, enc.bytes_in, enc.bytes_out, enc.errors, enc.batches) == (0,) * 6
    back = c.DecompressBatch([(bytearray(BLOCK), s) for s in stored])
    assert _codes(sres) == _codes(back) == [(n, None) for _, n in SRC]
    assert got == [0] * 4
    _check_reads(dst, rres, set())


@pytest.mark.parametrize("codec", ["none", "lz4", "zstd"])
def test_read_batch_corrupt_and_empty_sources(gpu, oracle, codec):
    c = C.NewCompressor(codec)
    stored, caps = _stored(oracle, codec), [BLOCK] * 4
    if codec == "none":
        caps[1] = 39999  # noOp.Decompress: "buffer too short"
    else:
        stored[1] = stored[1][:len(stored[1]) - 10]
    # one corrupt source fails exactly the reads it feeds
    dst, sres, rres, got = _read(c, stored, caps)
    back = c.DecompressBatch([(bytearray(n), s) for n, s in zip(caps, stored)])
    assert _codes(sres) == _codes(back) and sres[1][1] is not None
    _check_reads(dst, rres, {1})
    # an empty stored object: the codec's own answer, and a read that needs a byte of it fails
    objs = stored + [b""]
    parts = READ_PARTS + [[(4, 0, 1)], [(-1, 0, 3)]]
    dst, sres, rres, got = _read(c, objs, caps + [BLOCK], parts=parts)
    back = c.DecompressBatch([(bytearray(n), s) for n, s in zip(caps + [BLOCK], objs)])
    assert _codes(sres) == _codes(back)
    assert _codes(sres)[4] == ((0, None) if codec == "none" else (0, L.JFS_ERR_EMPTY_INPUT))
    _check_reads(dst, rres[:6], {1})
    assert _codes(rres)[6] == (0, L.JFS_ERR_CORRUPT) and rres[7] == (3, None)
    dst.check(6, b"")
    dst.check(7, bytes(3))
    # every source bad: a read made only of holes (and the empty read) still succeeds
    if codec == "none":
        bad, bcaps = stored, [0, 0, 0, 0]
    else:
        bad, bcaps = [b"\xff" * (7 + i) for i in range(4)], caps  # a literal run past the end / no Zstd magic
    dst, sres, rres, got = _read(c, bad, bcaps)
    assert all(e is not None for _, e in sres)
    _check_reads(dst, rres, {0, 1, 2, 3})
    assert rres[2] == (4114, None) and rres[3] == (0, None)


@pytest.mark.parametrize("codec", ["none", "lz4", "zstd"])
def test_read_batch_checksums(gpu, oracle, codec):
    c = C.NewCompressor(codec)
    stored = _stored(oracle, codec)
    crcs = [oracle.crc32c(s) for s in stored]
    # correct checksums pass, and come back as computed
    dst, sres, rres, got = _read(c, stored, crcs=crcs)
    assert _codes(sres) == [(n, None) for _, n in SRC] and got == crcs
    _check_reads(dst, rres, set())
    # one flipped payload bit
    flipped = list(stored)
    b = bytearray(stored[1])
    b[len(b) // 2] ^= 0x04
    flipped[1] = bytes(b)
    dst, sres, rres, got = _read(c, flipped, crcs=crcs[:2] + [None, -1])
    assert _codes(sres)[1] == (0, L.JFS_ERR_CHECKSUM)
    assert str(sres[1][1]) == f"verify checksum failed: {oracle.crc32c(flipped[1])} != {crcs[1]}"
    assert got == [crcs[0], oracle.crc32c(flipped[1]), 0, 0]
    assert [_codes(sres)[i] for i in (0, 2, 3)] == [(SRC[i][1], None) for i in (0, 2, 3)]
    _check_reads(dst, rres, {1})
    # corrupt for the codec and mismatching: the checksum wins; without one, the codec's own error
    caps = [BLOCK] * 4
    if codec == "none":
        caps[1] = 39999
        trunc = list(stored)
    else:
        trunc = list(stored)
        trunc[1] = stored[1][:len(stored[1]) - 10]
    back = c.DecompressBatch([(bytearray(n), s) for n, s in zip(caps, trunc)])
    assert back[1][1] is not None
    bad_crc = list(crcs)
    bad_crc[1] ^= 0x80000000
    dst, sres, rres, got = _read(c, trunc, caps, crcs=bad_crc)
    assert _codes(sres)[1] == (0, L.JFS_ERR_CHECKSUM) and got[1] == oracle.crc32c(trunc[1])
    _check_reads(dst, rres, {1})
    for skip in ([-1] * 4, None):
        dst, sres, rres, got = _read(c, trunc, caps, crcs=skip)
        assert _codes(sres) == _codes(back) and got == [0] * 4
        _check_reads(dst, rres, {1})
    # an empty object's CRC is 0
    dst, sres, rres, got = _read(c, stored + [b"", b""], [BLOCK] * 6, crcs=crcs + [0, 5])
    assert _codes(sres)[4] == ((0, None) if codec == "none" else (0, L.JFS_ERR_EMPTY_INPUT))
    assert _codes(sres)[5] == (0, L.JFS_ERR_CHECKSUM) and got[4:] == [0, 0]
    _check_reads(dst, rres, set())


# ---- jfs_read_open_batch ------------------------------------------------------

CIPHERS = [E.AES256GCM_RSA, E.CHACHA20_RSA, E.SM4GCM]
CODECS = {"none": L.ALGO_NONE, "lz4": L.ALGO_LZ4, "zstd": L.ALGO_ZSTD}
SRC_WRAPPED = [256, 1, 0, 1]  # payloads start at odd offsets
OPEN_ROWS = [(a, "lz4") for a in CIPHERS] + [(E.AES256GCM_RSA, "none"), (E.AES256GCM_RSA, "zstd")]


def _envelopes(algo, codec):
    """the stored envelopes, written by compress_seal_batch"""
    key = (algo, codec)
    if key not in _cache:
        rng = random.Random(5)
        rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
        params = [(rb(E.key_size(algo)), rb(12), rb(w)) for w in SRC_WRAPPED]
        raws = _raws()[0]
        pairs = [(bytearray(E.envelope_bound(CODECS[codec], len(r), len(p[2]))), r) for r, p in zip(raws, params)]
        res = E.compress_seal_batch(CODECS[codec], algo, pairs, params)
        assert all(e is None for _, e in res)
        _cache[key] = ([bytes(d[:n]) for (d, _), (n, _) in zip(pairs, res)], [p[0] for p in params])
    envs, keys = _cache[key]
    return list(envs), list(keys)


def _read_open(algo, codec, envs, keys, crcs=None):
    dst = Dst([sum(p[2] for p in ps) + (j % 2) for j, ps in enumerate(READ_PARTS)])
    sres, rres, got = E.read_open_batch(CODECS[codec], algo, [(e, BLOCK) for e in envs], keys, dst.views, _plan(),
                                        crcs=crcs)
    back = E.open_decompress_batch(CODECS[codec], algo, [(bytearray(BLOCK), e) for e in envs], keys)
    return dst, sres, rres, got, back


@pytest.mark.parametrize("algo,codec", OPEN_ROWS)
def test_read_open_batch(gpu, lib, oracle, algo, codec):
    envs, keys = _envelopes(algo, codec)
    crcs = [oracle.crc32c(e) for e in envs]
    lib.jfs_stats_reset()
    dst, sres, rres, got, back = _read_open(algo, codec, envs, keys, crcs=crcs)
    dec = _stat(lib, CODECS[codec], 1)
    assert (dec.calls, dec.blocks, dec.errors) == (2, 8, 0)  # this call and open_decompress_batch
    assert all(_stat(lib, a, 0).calls == 0 and _stat(lib, a, 0).blocks == 0 for a in range(3))
    assert _codes(sres) == _codes(back) == [(n, None) for _, n in SRC] and got == crcs
    _check_reads(dst, rres, set())
    # a flipped tag byte, and a header jfs_envelope_parse rejects
    bad = list(envs)
    e = bytearray(envs[1])
    e[-7] ^= 0x10
    bad[1] = bytes(e)
    bad[3] = b"\x00\x01"
    dst, sres, rres, got, back = _read_open(algo, codec, bad, keys)
    assert _codes(sres) == _codes(back)
    assert _codes(sres)[1] == (0, L.JFS_ERR_AUTH) and _codes(sres)[3] == (0, L.JFS_ERR_CORRUPT) and got == [0] * 4
    _check_reads(dst, rres, {1, 3})
    # the checksum covers the whole envelope and wins over both
    dst, sres, rres, got, back = _read_open(algo, codec, bad, keys, crcs=crcs)
    assert _codes(sres) == [(SRC[0][1], None), (0, L.JFS_ERR_CHECKSUM), (SRC[2][1], None), (0, L.JFS_ERR_CHECKSUM)]
    assert got == [crcs[0], oracle.crc32c(bad[1]), crcs[2], oracle.crc32c(bad[3])]
    _check_reads(dst, rres, {1, 3})
    # ... and where it matches, the open's and the parser's verdicts stand
    dst, sres, rres, got, back = _read_open(algo, codec, bad, keys, crcs=[oracle.crc32c(x) for x in bad])
    assert _codes(sres) == _codes(back)
    _check_reads(dst, rres, {1, 3})
