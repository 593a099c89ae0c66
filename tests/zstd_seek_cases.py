"""Seekable Zstd objects for the tests, independent of the encoder: objects
assembled by hand from the layout in include/jfs_gpucodec.h (raw-block frames
from tests/zstd_frames.py and a seek table written field by field), a
pure-Python table parser that follows the validity list of
jfs_zstd_decompress_range_device, and a reader of the frames' own headers."""
from __future__ import annotations

import struct

from tests import zstd_frames as ZF

SKIP_MAGIC = 0x184D2A5E
SEEK_MAGIC = 0x8F92EAB1
FRAME = 128 << 10
MAX_FRAMES = 16384  # what the encoder writes for its largest input; a longer table is no table


def raw_frame(data: bytes) -> bytes:
    """one single-segment frame with a content size and one raw block"""
    n = len(data)
    return ZF.write([ZF.frame([ZF.raw(data)], single=True, fcs_size=1 if n < 256 else 2 if n < 65536 + 256 else 4)])


def table(entries, nf=None, descriptor=0, skip_magic=SKIP_MAGIC, seek_magic=SEEK_MAGIC, size=None) -> bytes:
    """the seek table of frames [(compressed size, decompressed size)]; every field can be overridden"""
    nf = len(entries) if nf is None else nf
    size = 8 * len(entries) + 9 if size is None else size
    return (struct.pack("<II", skip_magic, size) + b"".join(struct.pack("<II", c, d) for c, d in entries) +
            struct.pack("<IBI", nf, descriptor, seek_magic))


def build(contents) -> tuple[bytes, list]:
    """(object, entries) of raw-block frames holding `contents` and their table"""
    frames = [raw_frame(c) for c in contents]
    entries = [(len(f), len(c)) for f, c in zip(frames, contents)]
    return b"".join(frames) + table(entries), entries


def parse_table(obj: bytes):
    """the entries of a valid table, else None"""
    n = len(obj)
    if n < 17 + 8 or struct.unpack_from("<I", obj, n - 4)[0] != SEEK_MAGIC or obj[n - 5] != 0:
        return None
    nf = struct.unpack_from("<I", obj, n - 9)[0]
    if nf < 1 or nf > MAX_FRAMES or 8 * nf + 17 > n:
        return None
    t = n - (8 * nf + 17)
    if struct.unpack_from("<II", obj, t) != (SKIP_MAGIC, 8 * nf + 9):
        return None
    ent = [struct.unpack_from("<II", obj, t + 8 + 8 * k) for k in range(nf)]
    if any(c < 1 for c, _ in ent) or sum(c for c, _ in ent) != t or sum(d for _, d in ent) >= 1 << 32:
        return None
    return ent


def select(obj: bytes, cap: int, lo: int, hi: int):
    """None without a table, else dict(total, first, count, coff, doff, flo, fhi):
    the frames whose output range meets [max(lo, 0), min(hi, cap))"""
    ent = parse_table(obj)
    if ent is None:
        return None
    lo, hi = max(lo, 0), min(hi, cap)
    pos, cpos, sel = 0, 0, []
    for k, (c, d) in enumerate(ent):
        if d > 0 and pos < hi and pos + d > lo and hi > lo:
            sel.append((k, cpos, pos, pos + d))
        pos, cpos = pos + d, cpos + c
    r = dict(total=pos, first=0, count=0, coff=0, doff=0, flo=0, fhi=0)
    if sel:
        r.update(first=sel[0][0], count=sel[-1][0] - sel[0][0] + 1, coff=sel[0][1], doff=sel[0][2], flo=sel[0][2],
                 fhi=sel[-1][3])
    return r


def frame_info(obj: bytes, at: int):
    """The test's own header reader: the frame at obj[at:] as dict(size, content,
    blocks=[(type, last, literal type or None)]) -- content None without an FCS."""
    assert struct.unpack_from("<I", obj, at)[0] == ZF.MAGIC
    fhd = obj[at + 4]
    single, fcsf = (fhd >> 5) & 1, fhd >> 6
    p = at + 5 + (0 if single else 1) + [0, 1, 2, 4][fhd & 3]
    fsz = [1 if single else 0, 2, 4, 8][fcsf]
    content = int.from_bytes(obj[p:p + fsz], "little") + (256 if fsz == 2 else 0) if fsz else None
    p += fsz
    blocks = []
    while True:
        bh = int.from_bytes(obj[p:p + 3], "little")
        last, bt, bs = bh & 1, (bh >> 1) & 3, bh >> 3
        p += 3
        blocks.append((bt, last, obj[p] & 3 if bt == 2 else None))
        p += 1 if bt == 1 else bs
        if last:
            break
    if fhd & 4:
        p += 4
    return dict(size=p - at, content=content, blocks=blocks, single=single, checksum=(fhd >> 2) & 1, did=fhd & 3)
