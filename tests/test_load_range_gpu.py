"""GPU: jfs_zstd_load_range_batch / ZStandard.LoadRangeBatch --
the fragment decode from host buffers, as a loadRange adapter calls it after
jfs_zstd_seek_plan and the ranged GET: the bytes equal the slice of the source,
every error maps to its JFS_ERR_*, nothing is written to dst for a failed
read, jfs_stats moves under (Zstd, decompress), good and bad reads mix."""
import ctypes

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from tests import zstd_seek_cases as S
from tests.test_zstd_frames_gpu import fetch, hand_built, ranges_for
from tests.test_zstd_seek_csum_gpu import objects

pytestmark = pytest.mark.gpu
B = S.FRAME
GUARD = 0xC3


def load(reads):
    """reads = [(table, object_len, frag, frag_off, lo, hi, block_size, dst_cap)] ->
    [(n or error code, the bytes written)]; every dst lies inside guard bytes that must survive"""
    bufs = [bytearray([GUARD]) * (cap + 32) for *_, cap in reads]
    views = [memoryview(b)[16:16 + cap] for b, (*_, cap) in zip(bufs, reads)]
    res = C.ZStandard().LoadRangeBatch([(v, t, olen, f, foff, lo, hi, bs)
                                        for v, (t, olen, f, foff, lo, hi, bs, _) in zip(views, reads)])
    out = []
    for (n, err), b, (*_, cap) in zip(res, bufs, reads):
        assert b[:16] == bytes([GUARD]) * 16 and b[16 + cap:] == bytes([GUARD]) * 16
        assert b[16 + n:16 + cap] == bytes([GUARD]) * (cap - n), "bytes behind the answer were written"
        out.append((err.code if err else n, bytes(b[16:16 + n])))
    return out


def stats(lib):
    arr = (L.JfsOpStats * L.STATS_N)()
    lib.jfs_stats(arr, L.STATS_N)
    s = arr[L.ALGO_ZSTD * 2 + 1]
    return {k: getattr(s, k) for k in ("calls", "blocks", "bytes_in", "bytes_out", "errors", "batches")}


def test_planned_reads_from_host_buffers(gpu, lib):
    reads, want = [], []
    for key, col, tails in ((("T", 4 * B + 777), 1, (64, 4096)), (("T", 4 * B + 777), 2, (64,)), (("Z", 2 * B), 1, (4096,)),
                            (("R", 69 * B + 5), 1, (64,))):
        got = objects(gpu)[key]
        raw, obj = got[0], got[col]
        n = len(raw)
        for tail in tails:
            for lo, hi in ranges_for(n) + [(B + 3, 2 * B - 5)]:
                t, frag, foff, p = fetch(obj, tail, lo, hi)
                a, b = max(lo, 0), min(hi, n)
                reads.append((t, len(obj), frag, foff, lo, hi, n, max(b - a, 0)))
                want.append((max(b - a, 0), raw[a:b] if b > a else b""))
    before = stats(lib)
    assert load(reads) == want
    d = {k: v - before[k] for k, v in stats(lib).items()}
    assert d == dict(calls=1, blocks=len(reads), batches=1, errors=0, bytes_out=sum(n for n, _ in want),
                     bytes_in=sum(len(r[0]) + len(r[2]) for r in reads))
    # a capacity above the range, a block above the content, the same table object shared by reads
    raw, obj, _ = objects(gpu)[("Z", 2 * B)]
    t, frag, foff, _ = fetch(obj, 4096, B - 1, B + 1)
    assert load([(t, len(obj), frag, foff, B - 1, B + 1, 2 * B + 50, 100), (t, len(obj), frag, foff, B, 1 << 40, 2 * B + 50, B),
                 (t, len(obj), frag, foff, -7, 2, 2 * B, 2)]) == [(2, raw[B - 1:B + 1]), (B, raw[B:]), (2, raw[:2])]


def test_errors_and_mixed_batch(gpu, lib):
    contents, obj, t, ent = hand_built(True)
    _, obj8, t8, _ = hand_built(False)
    raw = b"".join(contents)
    n, olen, body = len(raw), len(obj), obj[:len(obj) - len(t)]
    c0 = [sum(e[0] for e in ent[:k]) for k in range(len(ent) + 1)]
    d0 = [sum(e[1] for e in ent[:k]) for k in range(len(ent) + 1)]
    badsum = bytearray(t)
    badsum[8 + 12 * 2 + 8] ^= 0x10
    badsum = bytes(badsum)
    flip = bytearray(body)
    flip[c0[3] + 12 + 2000] ^= 0x04  # inside frame 3's raw block: it still decodes to the right length
    flip = bytes(flip)
    broke = bytearray(body)
    broke[c0[3] + 5] ^= 0x5A  # frame 3's content size
    broke = bytes(broke)
    damaged = raw[:d0[3] + 2000] + bytes([raw[d0[3] + 2000] ^ 0x04]) + raw[d0[3] + 2001:]
    reads = [
        (t, olen, body, 0, 0, n, n, n),                                   # 0: good, all frames
        (badsum, olen, body, 0, d0[2], d0[2] + 1, n, 1),                  # 1: -4: a checksum with a flipped bit
        (badsum, olen, body, 0, d0[3], n, n, n),                          # 2: good: that frame is not selected
        (t, olen, flip, 0, d0[3] + 5, d0[3] + 6, n, 1),                   # 3: -4: damage that decodes
        (t8, len(obj8), flip, 0, d0[3] + 1999, d0[3] + 2002, n, 3),       # 4: an 8-byte table cannot see it
        (t, olen, broke, 0, 0, n, n, n),                                  # 5: -1: a frame fails to decode
        (badsum, olen, broke, 0, 0, n, n, n),                             # 6: -1 wins over -4
        (t, olen, body[c0[1]:c0[3] - 1], c0[1], d0[1], d0[3], n, n),      # 7: -3: the fragment is short
        (t, olen, body, 0, 0, 10, n - 1, 10),                             # 8: -2: D > block_size
        (t, olen, body, 0, 0, 10, n, 9),                                  # 9: dst_cap below the range
        (t, olen + 1, body, 0, 0, 10, n, 10),                             # 10: an invalid table
        (t, olen, body, 0, 7, 7, n, 4),                                   # 11: an empty range
        (t, olen, b"", 0, n + 5, n + 9, n + 100, 4),                      # 12: behind the content
        (t, olen, body[c0[1]:c0[3]], c0[1], d0[1], d0[2] + 9, n, 5009),      # 13: good, frames 1 and 2 only
    ]
    before = stats(lib)
    got = load(reads)
    codes = [g[0] for g in got]
    assert codes == [n, L.JFS_ERR_CHECKSUM, n - d0[3], L.JFS_ERR_CHECKSUM, 3, L.JFS_ERR_CORRUPT, L.JFS_ERR_CORRUPT,
                     L.JFS_ERR_CORRUPT, L.JFS_ERR_SHORT_BUFFER, L.JFS_ERR_SHORT_BUFFER, L.JFS_ERR_CORRUPT, 0, 0, 10]
    assert got[0][1] == raw and got[2][1] == raw[d0[3]:] and got[4][1] == damaged[d0[3] + 1999:d0[3] + 2002]
    assert got[13][1] == raw[d0[1]:d0[2] + 9]
    d = {k: v - before[k] for k, v in stats(lib).items()}
    assert (d["calls"], d["blocks"], d["errors"], d["batches"]) == (1, len(reads), 8, 1)
    assert d["bytes_out"] == sum(c for c in codes if c > 0)


def test_invalid_arguments(gpu, lib):
    _, obj, t, _ = hand_built(True)
    body = obj[:len(obj) - len(t)]
    dst = ctypes.create_string_buffer(64)
    out = (ctypes.c_int64 * 1)(77)
    tp, fp = ctypes.cast(ctypes.c_char_p(t), ctypes.c_void_p), ctypes.cast(ctypes.c_char_p(body), ctypes.c_void_p)
    dp = ctypes.cast(dst, ctypes.c_void_p)

    def call(**kw):
        f = dict(table=tp, table_len=len(t), object_len=len(obj), frag=fp, frag_off=0, frag_len=len(body), lo=0, hi=10,
                 block_size=1 << 20, dst=dp, dst_cap=64)
        f.update(kw)
        r = (L.JfsRangeRead * 1)(L.JfsRangeRead(**f))
        return lib.jfs_zstd_load_range_batch(1, r, out, 0)
    assert call() == 0 and out[0] == 10 and dst.raw[:10] == b"".join(hand_built(True)[0])[:10]
    out[0] = 77
    for kw in (dict(table=None), dict(frag=None), dict(dst=None), dict(table_len=-1), dict(object_len=-1), dict(frag_off=-1),
               dict(frag_len=-1), dict(block_size=-1), dict(dst_cap=-1), dict(object_len=1 << 31), dict(block_size=1 << 31),
               dict(frag_len=1 << 31), dict(frag_off=1 << 31), dict(table_len=1 << 31)):
        assert call(**kw) == L.JFS_ERR_INVALID and out[0] == 77, kw
    assert lib.jfs_zstd_load_range_batch(-1, None, out, 0) == L.JFS_ERR_INVALID
    assert lib.jfs_zstd_load_range_batch(1, None, out, 0) == L.JFS_ERR_INVALID
    assert lib.jfs_zstd_load_range_batch(0, None, None, 0) == 0
    assert lib.jfs_zstd_load_range_batch(1, (L.JfsRangeRead * 1)(), out, 1 << 31) == L.JFS_ERR_INVALID  # checks come first
    assert call(dst=None, dst_cap=0, lo=5, hi=5) == 0 and out[0] == 0
