"""GPU: the read calls with JFS_READ_SEEK=sparse -- every Zstd
source decoded through jfs_zstd_decompress_ranges_device for the list of ranges
the reads ask of it -- against the same calls with the switch off, on the same
plans: out_n, every output image (canaries included, tests.test_read_gpu.Dst),
src_n, crc_got and the disk-cache checksums are equal.  Each source is read in
its first and its last frame only, and jfs_zstd_sparse_counts shows that 2 of
the 5 frames of each seekable source were decoded and that both decoded frames
of the 12-byte object were compared with their checksums: the proof that the
decode was sparse, without any timing.  A damaged middle frame goes unseen (the
reads succeed) where the full decode fails; a flipped table checksum of a
selected frame fails exactly the reads that use the source."""
import random

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests import zstd_seek_cases as S
from tests import zstd_seek_csum_cases as X
from tests.test_compact_gpu import _tile
from tests.test_read_gpu import Dst, _codes

pytestmark = pytest.mark.gpu
B = S.FRAME
SIZES = [4 * B + 4321, 5 * B, 300000]  # an 8-byte seekable object, a 12-byte one (5 frames each), an exact frame
N0, N1, N2 = SIZES
PARTS = [
    [(0, 100, 3000), (-1, 0, 33), (1, N1 - 2000, 2000)],  # source 0's first frame, a hole, source 1's last
    [(0, N0 - 500, 500), (1, 5, 60)],                     # source 0's last frame, source 1's first
    [(2, 10, 1000), (2, N2 - 100, 100)],                  # the exact frame: prefix-decoded to its end
    [(1, B - 50, 40)],                                    # source 1's first frame once more
]
USES = {0: {0, 1}, 1: {0, 1, 3}, 2: {2}}  # source -> reads
FLAGS = [True, False, True, False]       # the reads that ask for their disk-cache checksum
DEV0 = 1                                  # device mask: the counters are read on device 0

_cache = {}


def _plan():
    seg_first, seg = [0], []
    for p in PARTS:
        seg += _tile(p)
        seg_first.append(len(seg))
    return seg_first, seg


def _raws():
    if "raws" not in _cache:
        _cache["raws"] = [gen_block("TZT"[i], 9900 + i, n) for i, n in enumerate(SIZES)]
        _cache["want"] = C.read_expect(_cache["raws"], _plan())
    return _cache["raws"], _cache["want"]


class _modes:
    """the encoder's modes for source i: seekable, seekable with checksums, exact"""

    def __init__(self, i):
        self.i = i

    def __enter__(self):
        self.parse = C.set_zstd_parse_mode("exact" if self.i == 2 else "seekable")
        self.csum = C.set_zstd_seek_csum_mode("on" if self.i == 1 else "off")

    def __exit__(self, *a):
        C.set_zstd_seek_csum_mode(self.csum)
        C.set_zstd_parse_mode(self.parse)


def _stored():
    if "stored" not in _cache:
        z, objs = C.ZStandard(), []
        for i, r in enumerate(_raws()[0]):
            with _modes(i):
                d = bytearray(z.CompressBound(len(r)))
                n, err = z.Compress(d, r)
            assert err is None
            objs.append(bytes(d[:n]))
        assert len(S.parse_table(objs[0])) == 5 and S.parse_table(objs[1]) is None and S.parse_table(objs[2]) is None
        t = objs[1][len(objs[1]) - (12 * 5 + 17):]
        assert X.parse(t, len(objs[1]))[1] is True
        _cache["stored"] = objs
    return list(_cache["stored"])


def _with(seek, decode, fn):
    ps, pd = C.set_read_seek_mode(seek), C.set_read_decode_mode(decode)
    try:
        D.zstd_sparse_counts(reset=True)
        return fn(), D.zstd_sparse_counts()
    finally:
        C.set_read_decode_mode(pd)
        assert C.set_read_seek_mode(ps) == seek


def _read(stored, crcs, with_csum):
    dst = Dst([sum(p[2] for p in ps) + (j % 2) for j, ps in enumerate(PARTS)])
    r = C.ZStandard().ReadBatch(list(zip(stored, SIZES)), dst.views, _plan(), crcs=crcs, device_mask=DEV0,
                                with_csum=FLAGS if with_csum else False)
    return dst, _codes(r[0]), _codes(r[1]), r[2], (r[3] if with_csum else None)


def _agree(run, want, crcs=None):
    for decode in ("full", "prefix-all"):
        off, c_off = _with("off", decode, run)
        sp, c_sp = _with("sparse", decode, run)
        assert C.read_seek_mode() == "off"
        assert c_off == (0, 0, 0)
        assert c_sp == (2, 4, 2), "2 of 5 frames per seekable source, both 12-byte frames compared"
        assert sp[1] == [(n, None) for n in SIZES]  # need reaches every source's end: min(size, need) = size
        if decode == "full":
            assert off[1] == sp[1]
        assert sp[2] == off[2] == [(len(w), None) for w in want]
        assert sp[3] == off[3] and (crcs is None or sp[3] == crcs)
        assert sp[4] == off[4]
        if sp[4] is not None:
            assert [c is not None for c in sp[4]] == FLAGS
        for j, w in enumerate(want):
            off[0].check(j, w)
            sp[0].check(j, w)
    return sp


@pytest.mark.parametrize("with_csum", [False, True])
def test_read_sparse_plain(gpu, oracle, with_csum):
    stored, (raws, want) = _stored(), _raws()
    crcs = [oracle.crc32c(o) for o in stored]
    sp = _agree(lambda: _read(stored, crcs, with_csum), want, crcs)
    if with_csum:
        assert sp[4][0] == oracle.crc32c_segments(want[0])


@pytest.mark.parametrize("with_csum", [False, True])
def test_read_sparse_sealed(gpu, with_csum):
    algo, (raws, want) = E.AES256GCM_RSA, _raws()
    rng = random.Random(12)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    params = [(rb(E.key_size(algo)), rb(12), rb(w)) for w in (256, 1, 0)]
    envs = []
    for i, (r, p) in enumerate(zip(raws, params)):
        pair = (bytearray(E.envelope_bound(L.ALGO_ZSTD, len(r), len(p[2]))), r)
        with _modes(i):
            (n, err), = E.compress_seal_batch(L.ALGO_ZSTD, algo, [pair], [p])
        assert err is None
        envs.append(bytes(pair[0][:n]))
    keys = [p[0] for p in params]

    def run():
        dst = Dst([sum(p[2] for p in ps) + (j % 2) for j, ps in enumerate(PARTS)])
        r = E.read_open_batch(L.ALGO_ZSTD, algo, list(zip(envs, SIZES)), keys, dst.views, _plan(), device_mask=DEV0,
                              with_csum=FLAGS if with_csum else False)
        return dst, _codes(r[0]), _codes(r[1]), r[2], (r[3] if with_csum else None)
    _agree(run, want)


def _frame_at(obj, entry, k):
    """where frame k of a five-frame object starts"""
    t = len(obj) - (entry * 5 + 17)
    return sum(int.from_bytes(obj[t + 8 + entry * q:t + 12 + entry * q], "little") for q in range(k))


def _flip(obj, at, mask):
    b = bytearray(obj)
    b[at] ^= mask
    return bytes(b)


def test_a_damaged_middle_frame_goes_unseen(gpu, oracle):
    stored, (raws, want) = _stored(), _raws()
    # frame 2's content size, in both seekable objects; the expected object CRC is that of the damaged bytes
    stored[0] = _flip(stored[0], _frame_at(stored[0], 8, 2) + 5, 0x5A)
    stored[1] = _flip(stored[1], _frame_at(stored[1], 12, 2) + 5, 0x5A)
    crcs = [oracle.crc32c(o) for o in stored]
    sp, counts = _with("sparse", "full", lambda: _read(stored, crcs, True))
    assert counts == (2, 4, 2)
    assert sp[1] == [(n, None) for n in SIZES] and sp[2] == [(len(w), None) for w in want] and sp[3] == crcs
    for j, w in enumerate(want):
        sp[0].check(j, w)
    off, counts = _with("off", "full", lambda: _read(stored, crcs, True))
    assert counts == (0, 0, 0)
    assert off[1] == [(0, L.JFS_ERR_CORRUPT), (0, L.JFS_ERR_CORRUPT), (N2, None)]
    assert off[2] == [(0, L.JFS_ERR_CORRUPT), (0, L.JFS_ERR_CORRUPT), (len(want[2]), None), (0, L.JFS_ERR_CORRUPT)]
    for j in (0, 1, 3):
        off[0].check(j, b"")


def test_checksum_mismatches(gpu, oracle):
    stored, (raws, want) = _stored(), _raws()
    good = list(stored)
    # the table checksum of frame 4 of the 12-byte object, one bit: a selected frame
    t = len(stored[1]) - (12 * 5 + 17)
    stored[1] = _flip(stored[1], t + 8 + 12 * 4 + 8, 0x01)
    crcs = [oracle.crc32c(o) for o in stored]
    sp, counts = _with("sparse", "full", lambda: _read(stored, crcs, True))
    assert counts == (2, 4, 2)
    assert sp[1] == [(N0, None), (0, L.JFS_ERR_CHECKSUM), (N2, None)] and sp[3] == crcs
    assert sp[2] == [(0, L.JFS_ERR_CORRUPT), (0, L.JFS_ERR_CORRUPT), (len(want[2]), None), (0, L.JFS_ERR_CORRUPT)]
    for j in USES[1]:
        sp[0].check(j, b"")  # nothing written
    sp[0].check(2, want[2])
    # the same flip in frame 2, which no read touches: unseen
    stored[1] = _flip(good[1], t + 8 + 12 * 2 + 8, 0x01)
    crcs = [oracle.crc32c(o) for o in stored]
    sp, _ = _with("sparse", "full", lambda: _read(stored, crcs, False))
    assert sp[1] == [(n, None) for n in SIZES] and sp[2] == [(len(w), None) for w in want]
    # without an expected CRC-32C a selected frame that does not decode is a corrupt source; with one that does
    # not match, the object checksum's verdict comes first, as with the switch off
    stored = list(good)
    stored[0] = _flip(good[0], 5, 0x5A)  # frame 0's content size
    sp, _ = _with("sparse", "full", lambda: _read(stored, None, False))
    assert sp[1] == [(0, L.JFS_ERR_CORRUPT), (N1, None), (N2, None)]
    assert sp[2] == [(0, L.JFS_ERR_CORRUPT), (0, L.JFS_ERR_CORRUPT), (len(want[2]), None), (len(want[3]), None)]
    crcs = [oracle.crc32c(good[0]), oracle.crc32c(good[1]) ^ 1, -1]
    for mode in ("sparse", "off"):
        r, _ = _with(mode, "full", lambda: _read(stored, crcs, False))
        assert r[1] == [(0, L.JFS_ERR_CHECKSUM), (0, L.JFS_ERR_CHECKSUM), (N2, None)], mode
        assert r[2] == [(0, L.JFS_ERR_CORRUPT), (0, L.JFS_ERR_CORRUPT), (len(want[2]), None), (0, L.JFS_ERR_CORRUPT)]
        assert r[3][:2] == [oracle.crc32c(stored[0]), oracle.crc32c(good[1])]
