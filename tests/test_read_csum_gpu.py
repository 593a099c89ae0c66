"""GPU: the disk-cache checksums of the read calls (jfs_read_batch_csum,
jfs_read_open_batch_csum) and of the sealed batch decode
(jfs_open_decompress_batch_csum).

Expected checksum bytes are the CPU oracle's crc32c_segments over the numpy
model's bytes (read_expect), never the library's own.  Every checksum buffer
sits at an odd offset inside a canary-filled array and the whole array is
compared with its expected image, so a byte written behind
((n-1)/32768+1)*4, or anything written for a failed read or a read that asked
for no checksum, fails the test."""
import ctypes
import random

import numpy as np
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests.test_compact_gpu import CANARY
from tests.test_read_gpu import CIPHERS, Dst, _codes, _plan

pytestmark = pytest.mark.gpu

PIECE = 32768
SRC = [("T", 131077), ("R", 70001), ("T", 65536)]  # class, decoded length: 64 KiB .. 256 KiB
BLOCK = 131077
EDGE_TOTALS = [0, 1, 15, 16, 17, 32767, 32768, 32769, 65536, 98309]


def _mixed(total, k=0):
    """a total made of a run of source 0, a hole and a run of source 1"""
    a, h = total // 3, total // 5
    return [p for p in [(0, 9 + k, a), (-1, 0, h), (1, 1234 + 3 * k, total - a - h)] if p[2] > 0]


EDGE_PARTS = [_mixed(t, k) for k, t in enumerate(EDGE_TOTALS)]
SEAM_PARTS = [
    [(0, 100, 20000), (-1, 0, 5000), (1, 7, 15000)],  # its first piece spans source 0, a hole and source 1
    [(2, 333, 65536 - 333)],                          # an odd source offset: the packed bytes are shifted against the source
    [(1, 1, PIECE), (0, 3, 5)],                       # a seam five bytes into the second piece
]

_cache = {}


def _raws():
    if "raws" not in _cache:
        _cache["raws"] = [gen_block(cls, 900 + i, n) for i, (cls, n) in enumerate(SRC)]
    return _cache["raws"]


def _stored(oracle, codec):
    """the stored objects, encoded by the CPU oracle"""
    if codec not in _cache:
        enc = {"none": lambda b: b, "lz4": lambda b: oracle.lz4_compress(b)[1], "zstd": oracle.zstd_compress_l1}[codec]
        _cache[codec] = [enc(r) for r in _raws()]
    return list(_cache[codec])


def _want(oracle, raws, parts):
    """per read: (the model's bytes, the oracle's checksum bytes of them)"""
    key = ("want", id(raws), repr(parts))  # (the source lists live in _cache)
    if key not in _cache:
        outs = C.read_expect(raws, _plan(parts))
        _cache[key] = [(o, oracle.crc32c_segments(o)) for o in outs]
    return _cache[key]


class Sums:
    """Checksum buffers at odd offsets inside canary-filled arrays; wanted[j]
    false: read j passes no buffer."""

    def __init__(self, totals, wanted=None):
        self.wanted = [True] * len(totals) if wanted is None else list(wanted)
        self.offs = [2 * j + 3 for j in range(len(totals))]
        need = [C.csum_bytes(t) for t in totals]
        self.arr = [np.full(o + n + 40, CANARY, dtype=np.uint8) for o, n in zip(self.offs, need)]
        self.views = [a[o:o + n] if w else None for a, o, n, w in zip(self.arr, self.offs, need, self.wanted)]

    def check(self, j, want: bytes):
        img = np.full(len(self.arr[j]), CANARY, dtype=np.uint8)
        img[self.offs[j]:self.offs[j] + len(want)] = np.frombuffer(want, dtype=np.uint8)
        bad = np.nonzero(img != self.arr[j])[0]
        assert bad.size == 0, f"read {j}: first wrong checksum byte at {bad[0] - self.offs[j]} ({bad.size} wrong)"


def _totals(parts):
    return [sum(p[2] for p in ps) for ps in parts]


def _run(codec, objs, parts, caps=None, crcs=None, wanted=None, sealed=None):
    """one _csum call; sealed = (cipher name, keys) for jfs_read_open_batch_csum"""
    caps = caps or [BLOCK] * len(objs)
    totals = _totals(parts)
    dst, sums = Dst([t + (j % 2) for j, t in enumerate(totals)]), Sums(totals, wanted)
    src = list(zip(objs, caps))
    if sealed is None:
        res = C.NewCompressor(codec).ReadBatch(src, dst.views, _plan(parts), crcs=crcs, with_csum=sums.views)
    else:
        res = E.read_open_batch({"none": 0, "lz4": 1, "zstd": 2}[codec], sealed[0], src, sealed[1], dst.views,
                                _plan(parts), crcs=crcs, with_csum=sums.views)
    return (dst, sums) + tuple(res)


def _check_good(oracle, raws, parts, dst, sums, rres, cs, skip=()):
    """every read outside `skip` is good: its bytes, its checksum (inside the canaries) and the returned copy"""
    want = _want(oracle, raws, parts)
    for j, (data, ck) in enumerate(want):
        if j in skip:
            continue
        assert rres[j] == (len(data), None), (j, rres[j])
        dst.check(j, data)
        assert len(ck) == ((len(data) - 1) // PIECE + 1 if data else 1) * 4
        if sums.wanted[j]:
            sums.check(j, ck)
            assert cs[j] == ck, j
        else:
            sums.check(j, b"")
            assert cs[j] is None


def _check_dead(dst, sums, rres, cs, dead):
    for j in dead:
        assert _codes(rres)[j] == (0, L.JFS_ERR_CORRUPT), (j, rres[j])
        dst.check(j, b"")
        sums.check(j, b"")
        assert cs[j] is None


@pytest.fixture
def decode_mode(request):
    prev = C.set_read_decode_mode(request.param)
    yield request.param
    C.set_read_decode_mode(prev)


@pytest.mark.parametrize("decode_mode", ["full", "prefix"], indirect=True)
def test_read_csum_piece_edges(gpu, oracle, decode_mode):
    """totals around the 16-byte word and the 32 KiB piece, in one LZ4 call, in
    both decode modes: the checksums do not depend on where a decode stops"""
    assert C.read_decode_mode() == decode_mode
    dst, sums, sres, rres, got, cs = _run("lz4", _stored(oracle, "lz4"), EDGE_PARTS)
    if decode_mode == "full":
        assert _codes(sres) == [(n, None) for _, n in SRC]
    else:  # sources 0 and 1 stop at the last byte a read needs; nothing reads source 2
        assert all(e is None for _, e in sres) and sres[0][0] < SRC[0][1] and sres[2][0] == 0
    assert [n for n, _ in rres] == EDGE_TOTALS
    _check_good(oracle, _raws(), EDGE_PARTS, dst, sums, rres, cs)
    assert cs[0] == bytes(4)  # checksum() of no bytes: one zero word
    assert [len(x) for x in cs] == [4, 4, 4, 4, 4, 4, 4, 8, 8, 16]


def test_read_csum_piece_across_a_seam(gpu, oracle):
    dst, sums, sres, rres, got, cs = _run("lz4", _stored(oracle, "lz4"), SEAM_PARTS)
    assert _codes(sres) == [(n, None) for _, n in SRC]
    _check_good(oracle, _raws(), SEAM_PARTS, dst, sums, rres, cs)
    assert [len(x) for x in cs] == [8, 8, 8]


@pytest.mark.parametrize("codec", ["lz4", "zstd", "none"])
def test_read_csum_whole_block_is_the_disk_cache_layout(gpu, oracle, codec):
    """a read that takes one whole block: exactly what jfs_decompress_batch_csum writes for that block"""
    stored, raws = _stored(oracle, codec), _raws()
    parts = [[(i, 0, n)] for i, (_, n) in enumerate(SRC)]
    dst, sums, sres, rres, got, cs = _run(codec, stored, parts)
    _check_good(oracle, raws, parts, dst, sums, rres, cs)
    back = C.NewCompressor(codec).DecompressBatchChecksum([(bytearray(BLOCK), s) for s in stored])
    assert [(n, e) for n, e, _ in back] == [(n, None) for _, n in SRC]
    assert cs == [ck for _, _, ck in back]


MANY_SRC = 6
MANY_LEN = 65536
MANY_BAD = 3  # the corrupted source; only reads 19 and 20 use it


def _many():
    if "many" not in _cache:
        raws = [gen_block("TR"[i % 2], 950 + i, MANY_LEN) for i in range(MANY_SRC)]
        pool = [i for i in range(MANY_SRC) if i != MANY_BAD]
        parts = []
        for j in range(40):
            total = 1000 + 2477 * j  # 1000 .. 97603: one to three pieces
            a = min(total, 60000)
            first = MANY_BAD if j in (19, 20) else pool[j % 5]
            ps = [(first, j, a)]
            if total > a:
                ps.append((pool[(j + 2) % 5], 3, total - a))
            parts.append(ps)
        _cache["many"] = (raws, parts)
    return _cache["many"]


def test_read_csum_selective_and_failed(gpu, oracle):
    """40 reads, every third without a checksum buffer, one corrupted source
    that fails two reads in the middle: those keep their canaries, every other
    checksum is right, and everything else is the plain ReadBatch's"""
    raws, parts = _many()
    stored = [oracle.lz4_compress(r)[1] for r in raws]
    stored[MANY_BAD] = stored[MANY_BAD][:len(stored[MANY_BAD]) - 10]
    caps = [MANY_LEN] * MANY_SRC
    wanted = [j % 3 != 0 for j in range(40)]
    dst, sums, sres, rres, got, cs = _run("lz4", stored, parts, caps=caps, wanted=wanted)
    assert sres[MANY_BAD][1] is not None and all(e is None for i, (_, e) in enumerate(sres) if i != MANY_BAD)
    _check_dead(dst, sums, rres, cs, (19, 20))
    _check_good(oracle, raws, parts, dst, sums, rres, cs, skip=(19, 20))
    assert sum(len(x) // 4 for x in cs if x is not None) > 40  # reads of two and three pieces among them
    # the same input through the call without checksums
    plain = Dst([t + (j % 2) for j, t in enumerate(_totals(parts))])
    sres0, rres0, got0 = C.NewCompressor("lz4").ReadBatch(list(zip(stored, caps)), plain.views, _plan(parts))
    assert _codes(sres) == _codes(sres0) and _codes(rres) == _codes(rres0) and got == got0
    for a, b in zip(dst.arr, plain.arr):
        assert np.array_equal(a, b)


def test_read_csum_checksum_gate(gpu, oracle):
    """a source whose expected CRC-32C is wrong (JFS_ERR_CHECKSUM): the reads it feeds get no checksum bytes"""
    stored = _stored(oracle, "lz4")
    crcs = [oracle.crc32c(s) for s in stored]
    crcs[2] ^= 0x00010000
    parts = SEAM_PARTS + [[(0, 0, 70000)]]
    dst, sums, sres, rres, got, cs = _run("lz4", stored, parts, crcs=crcs)
    assert _codes(sres) == [(SRC[0][1], None), (SRC[1][1], None), (0, L.JFS_ERR_CHECKSUM)]
    assert got == [oracle.crc32c(s) for s in stored]
    _check_dead(dst, sums, rres, cs, (1,))
    _check_good(oracle, _raws(), parts, dst, sums, rres, cs, skip=(1,))


def _envelopes(algo):
    """the LZ4 blocks of SRC, sealed by compress_seal_batch"""
    key = ("env", algo)
    if key not in _cache:
        rng = random.Random(7)
        rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
        params = [(rb(E.key_size(algo)), rb(12), rb(w)) for w in (256, 1, 0)]  # payloads start at odd offsets
        pairs = [(bytearray(E.envelope_bound(L.ALGO_LZ4, len(r), len(p[2]))), r) for r, p in zip(_raws(), params)]
        res = E.compress_seal_batch(L.ALGO_LZ4, algo, pairs, params)
        assert all(e is None for _, e in res)
        _cache[key] = ([bytes(d[:n]) for (d, _), (n, _) in zip(pairs, res)], [p[0] for p in params])
    envs, keys = _cache[key]
    return list(envs), list(keys)


SEALED_PARTS = [EDGE_PARTS[k] for k in (0, 4, 6, 7, 9)] + [SEAM_PARTS[0], [(2, 0, 65536)]]


@pytest.mark.parametrize("algo", CIPHERS)
def test_read_open_csum(gpu, oracle, algo):
    envs, keys = _envelopes(algo)
    dst, sums, sres, rres, got, cs = _run("lz4", envs, SEALED_PARTS, sealed=(algo, keys))
    assert _codes(sres) == [(n, None) for _, n in SRC]
    _check_good(oracle, _raws(), SEALED_PARTS, dst, sums, rres, cs)
    # a flipped tag byte on source 2 fails the whole-block read alone
    bad = list(envs)
    e = bytearray(envs[2])
    e[-3] ^= 0x40
    bad[2] = bytes(e)
    dst, sums, sres, rres, got, cs = _run("lz4", bad, SEALED_PARTS, sealed=(algo, keys))
    assert _codes(sres)[2] == (0, L.JFS_ERR_AUTH)
    _check_dead(dst, sums, rres, cs, (6,))
    _check_good(oracle, _raws(), SEALED_PARTS, dst, sums, rres, cs, skip=(6,))


@pytest.mark.parametrize("algo", CIPHERS)
def test_open_decompress_batch_csum(gpu, lib, oracle, algo):
    """the sealed batch decode with checksums against DecompressBatchChecksum of
    the same plaintext blocks; an envelope with a bad tag reports JFS_ERR_AUTH
    and leaves its checksum buffer alone"""
    envs, keys = _envelopes(algo)
    e = bytearray(envs[1])
    e[-1] ^= 0x01
    envs[1] = bytes(e)
    nb = len(envs)
    sums = Sums([BLOCK] * nb)  # csum[i] holds ((dst_cap-1)/32768+1)*4 bytes
    outs = [np.full(BLOCK + 32, CANARY, dtype=np.uint8) for _ in range(nb)]
    iov, kp, cp = (L.JfsIov * nb)(), (ctypes.c_void_p * nb)(), (ctypes.c_void_p * nb)()
    keep = []
    for i in range(nb):
        s, k = ctypes.create_string_buffer(envs[i], len(envs[i])), ctypes.create_string_buffer(keys[i], len(keys[i]))
        keep += [s, k]
        iov[i].src, iov[i].src_len = ctypes.addressof(s), len(envs[i])
        iov[i].dst, iov[i].dst_cap = outs[i].ctypes.data, BLOCK
        kp[i], cp[i] = ctypes.addressof(k), sums.views[i].ctypes.data
    out_n = (ctypes.c_int64 * nb)()
    assert lib.jfs_open_decompress_batch_csum(L.ALGO_LZ4, E.cipher_id(algo), nb, iov, kp, out_n, cp, 0) == 0
    plain = C.NewCompressor("lz4").DecompressBatchChecksum([(bytearray(BLOCK), s) for s in _stored(oracle, "lz4")])
    raws = _raws()
    assert list(out_n) == [SRC[0][1], L.JFS_ERR_AUTH, SRC[2][1]]
    for i in (0, 2):
        assert plain[i][:2] == (SRC[i][1], None)
        assert plain[i][2] == oracle.crc32c_segments(raws[i])
        sums.check(i, plain[i][2])
        assert outs[i][:SRC[i][1]].tobytes() == raws[i] and (outs[i][SRC[i][1]:] == CANARY).all()
    sums.check(1, b"")
    assert (outs[1] == CANARY).all()
    # the Python form of the same call
    res = E.open_decompress_batch_csum(L.ALGO_LZ4, algo, [(bytearray(BLOCK), x) for x in envs], keys)
    assert [(n, e.code if e else None) for n, e, _ in res] == [(SRC[0][1], None), (0, L.JFS_ERR_AUTH), (SRC[2][1], None)]
    assert [ck for _, _, ck in res] == [plain[0][2], None, plain[2][2]]


def test_read_csum_device(gpu, oracle):
    """jfs_read_csum_device alone over reads packed in HBM at 16-byte aligned
    and at odd offsets: a read without pieces and a read whose verdict is not
    its total leave the checksum area's canary alone"""
    import torch
    from juicefs_amd import device as D
    totals = [98309, 4096, 32768, 5, 70001, 65536]
    wanted = [True, True, False, True, True, True]
    verdict = [98309, 4096, 32768, 5, -(1 << 31), 65536]  # read 4's gather failed
    offs, o = [], 0
    for j, t in enumerate(totals):
        o = (o + 15) // 16 * 16 + (0 if j % 2 == 0 else 2 * j + 1)  # odd offsets: the byte-wise path
        offs.append(o)
        o += t
    host = np.frombuffer(gen_block("T", 990, o + 16), dtype=np.uint8).copy()
    gat = torch.from_numpy(host).to(gpu)
    odesc, _ = D.make_compact_desc(gat, offs, totals, list(range(len(totals) + 1)), [(-1, 0, 0, t) for t in totals])
    words = [((t - 1) // PIECE + 1) if w else 0 for t, w in zip(totals, wanted)]
    pf = np.concatenate([[0], np.cumsum(words)]).astype(np.int32)
    npiece = int(pf[-1])
    ret = torch.tensor(verdict, dtype=torch.int32, device=gpu)
    area = torch.full((4 * npiece + 32,), CANARY, dtype=torch.uint8, device=gpu)
    D.read_csum(odesc, ret, torch.from_numpy(pf).to(gpu), npiece, area[16:])
    torch.cuda.synchronize()
    got = area.cpu().numpy()
    want = np.full(len(got), CANARY, dtype=np.uint8)
    for j, t in enumerate(totals):
        if wanted[j] and verdict[j] == t:
            ck = oracle.crc32c_segments(host[offs[j]:offs[j] + t].tobytes())
            want[16 + 4 * pf[j]:16 + 4 * pf[j + 1]] = np.frombuffer(ck, dtype=np.uint8)
    assert np.array_equal(got, want)
