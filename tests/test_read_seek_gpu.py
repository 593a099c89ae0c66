"""GPU: the read calls with JFS_READ_SEEK on (every Zstd source decoded through
jfs_zstd_decompress_range_device for the byte range the reads ask of it)
against the same calls with the switch off, on the same plans: out_n, every
output image (canaries included, tests.test_read_gpu.Dst) and the disk-cache
checksums are equal, src_n is min(size, need), and the corrupt, short-source
and unauthenticated sources fail their reads as before."""
import random

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests import zstd_seek_cases as S
from tests.test_compact_gpu import _tile
from tests.test_read_gpu import Dst, _codes

pytestmark = pytest.mark.gpu
B = S.FRAME
SIZES = [5 * B + 4321, 3 * B, 100000, 2 * B + 1, 2 * B, 1000, 4 * B]  # 2 and 5 are one frame; 4 is fast; 6 corrupt
NSRC = len(SIZES)
CAPS = [2000 if i == 5 else n for i, n in enumerate(SIZES)]  # source 5's block size allows the segment it is too short for


def _parts():
    n0 = SIZES[0]
    return [
        [(0, 4 * B + 50, 3000), (-1, 0, 33), (1, B - 10, 20), (3, 2 * B - 5, 6)],  # fragmented, across frame edges
        [(0, n0 - 100, 100)],                                                     # the last 100 bytes of a source
        [(1, 0, 3 * B)],                                                          # a whole block, with its checksum
        [(2, 5, 60000), (-1, 0, 15), (4, B + 7, 1000)],                           # a plain frame and a fast frame
        [(0, 3 * B + 1, 10), (0, B + 5, 10)],                                     # one source twice: lo is the smaller
        [(5, 900, 200)],                                                          # a source too short for the segment
        [(6, 0, 500), (2, 0, 10)],                                                # a corrupt source
        [(-1, 0, 77)],                                                            # only a hole
        [(4, 0, 1)],
    ]


def _plan(parts):
    seg_first, seg = [0], []
    for p in parts:
        seg += _tile(p)
        seg_first.append(len(seg))
    return seg_first, seg


def _ranges(parts, nsrc):
    lo, need = [None] * nsrc, [0] * nsrc
    for p in parts:
        for s, off, n in p:
            if s >= 0:
                need[s] = max(need[s], off + n)
                lo[s] = off if lo[s] is None else min(lo[s], off)
    return [x or 0 for x in lo], need


_cache = {}


def _raws():
    if "raws" not in _cache:
        _cache["raws"] = [gen_block("T" if i % 2 == 0 else "Z", 9700 + i, n) for i, n in enumerate(SIZES)]
    return _cache["raws"]


def _want(plan):
    """the reads' bytes; read 5 fails, so what stands in for the bytes source 5 lacks does not matter"""
    raws = list(_raws())
    raws[5] = raws[5] + bytes(200)
    return C.read_expect(raws, plan)


def _stored():
    """seekable objects; source 4 a fast frame; source 6 a seekable object whose first frame has a wrong magic"""
    if "stored" not in _cache:
        z = C.ZStandard()

        def enc(mode, b):
            with C.zstd_parse_mode(mode):
                d = bytearray(z.CompressBound(len(b)))
                n, err = z.Compress(d, b)
            assert err is None
            return bytes(d[:n])
        objs = [enc("fast" if i == 4 else "seekable", r) for i, r in enumerate(_raws())]
        assert [len(S.parse_table(o) or []) for o in objs] == [6, 3, 0, 3, 0, 0, 4]
        bad = bytearray(objs[6])
        bad[0] ^= 0xFF
        objs[6] = bytes(bad)
        _cache["stored"] = objs
    return list(_cache["stored"])


def _seek(mode, fn):
    prev = C.set_read_seek_mode(mode)
    try:
        return fn()
    finally:
        assert C.set_read_seek_mode(prev) == mode


def _flags(parts):
    return [j == 2 for j in range(len(parts))]


def _expect_src(need, on):
    out = []
    for i, n in enumerate(SIZES):
        if i == 6:
            out.append((0, L.JFS_ERR_CORRUPT))
        else:
            out.append((min(n, need[i]) if on else n, None))
    return out


def _check(run, parts, want, need):
    off = _seek("off", run)
    on = _seek("on", run)
    assert C.read_seek_mode() == "off"
    assert off[1] == _expect_src(need, False), off[1]
    assert on[1] == _expect_src(need, True), on[1]
    exp = [(len(w), None) for w in want]
    exp[5] = exp[6] = (0, L.JFS_ERR_CORRUPT)
    assert on[2] == off[2] == exp
    assert on[3] == off[3] and on[3][2] is not None and [c for j, c in enumerate(on[3]) if j != 2] == [None] * (len(parts) - 1)
    for j, w in enumerate(want):
        for r in (off, on):
            r[0].check(j, b"" if j in (5, 6) else w)


def test_read_seek_plain(gpu, oracle):
    parts, stored = _parts(), _stored()
    plan = _plan(parts)
    want = _want(plan)
    lo, need = _ranges(parts, NSRC)
    assert lo[0] == B + 5 and need[0] == SIZES[0] and need[5] == 1100 and lo[1] == 0
    crcs = [oracle.crc32c(o) for o in stored]

    def run():
        dst = Dst([sum(p[2] for p in ps) + (j % 2) for j, ps in enumerate(parts)])
        sres, rres, got, cs = C.ZStandard().ReadBatch(list(zip(stored, CAPS)), dst.views, plan, crcs=crcs,
                                                     with_csum=_flags(parts))
        assert got == crcs
        return dst, _codes(sres), _codes(rres), cs
    _check(run, parts, want, need)
    # the whole-block read's checksum is the block's disk-cache checksum
    on = _seek("on", run)
    assert on[3][2] == oracle.crc32c_segments(_raws()[1])
    # the decode modes stay what they are beside the switch
    for mode in ("prefix", "prefix-all"):
        prev = C.set_read_decode_mode(mode)
        try:
            r = _seek("on", run)
        finally:
            C.set_read_decode_mode(prev)
        assert r[1] == _expect_src(need, True) and r[2][0] == (len(want[0]), None)
        r[0].check(0, want[0])


def test_read_seek_sealed(gpu, oracle):
    algo, parts, raws = E.AES256GCM_RSA, _parts(), _raws()
    plan = _plan(parts)
    want = _want(plan)
    lo, need = _ranges(parts, NSRC)
    rng = random.Random(11)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    params = [(rb(E.key_size(algo)), rb(12), rb(w)) for w in (256, 1, 0, 1, 7, 2, 3)]
    pairs = [(bytearray(E.envelope_bound(L.ALGO_ZSTD, len(r), len(p[2]))), r) for r, p in zip(raws, params)]
    with C.zstd_parse_mode("seekable"):
        res = E.compress_seal_batch(L.ALGO_ZSTD, algo, pairs, params)
    assert all(e is None for _, e in res)
    envs = [bytes(d[:n]) for (d, _), (n, _) in zip(pairs, res)]
    keys = [p[0] for p in params]
    keys[6] = rb(E.key_size(algo))  # source 6 does not authenticate

    def run():
        dst = Dst([sum(p[2] for p in ps) + (j % 2) for j, ps in enumerate(parts)])
        sres, rres, got, cs = E.read_open_batch(L.ALGO_ZSTD, algo, list(zip(envs, CAPS)), keys, dst.views, plan,
                                                with_csum=_flags(parts))
        return dst, _codes(sres), _codes(rres), cs
    off = _seek("off", run)
    on = _seek("on", run)
    for r, is_on in ((off, False), (on, True)):
        exp = _expect_src(need, is_on)
        exp[6] = (0, L.JFS_ERR_AUTH)
        assert r[1] == exp, r[1]
    exp = [(len(w), None) for w in want]
    exp[5] = exp[6] = (0, L.JFS_ERR_CORRUPT)
    assert on[2] == off[2] == exp and on[3] == off[3] and on[3][2] == oracle.crc32c_segments(raws[1])
    for j, w in enumerate(want):
        on[0].check(j, b"" if j in (5, 6) else w)
