"""Stand-alone seek tables for the tests, both layouts: a table
written field by field with 8-byte or 12-byte entries, a pure-Python parser that
follows the validity list of jfs_zstd_seek_plan, and the plan it implies."""
from __future__ import annotations

import struct

from tests.xxh64_ref import xxh64
from tests.zstd_seek_cases import MAX_FRAMES, SEEK_MAGIC, SKIP_MAGIC, raw_frame


def table(entries, descriptor=None, nf=None, size=None, skip_magic=SKIP_MAGIC, seek_magic=SEEK_MAGIC) -> bytes:
    """entries of (c, d) give the 8-byte layout, of (c, d, checksum) the 12-byte one; every field can be overridden"""
    wide = bool(entries) and len(entries[0]) == 3
    descriptor = (0x80 if wide else 0) if descriptor is None else descriptor
    nf = len(entries) if nf is None else nf
    body = b"".join(struct.pack("<III" if wide else "<II", *e) for e in entries)
    size = len(body) + 9 if size is None else size
    return struct.pack("<II", skip_magic, size) + body + struct.pack("<IBI", nf, descriptor, seek_magic)


def build(contents, checksums: bool):
    """(object, table, entries) of raw-block frames holding `contents`"""
    frames = [raw_frame(c) for c in contents]
    ent = [(len(f), len(c)) + ((xxh64(c) & 0xFFFFFFFF,) if checksums else ()) for f, c in zip(frames, contents)]
    t = table(ent)
    return b"".join(frames) + t, t, ent


def parse(t: bytes, object_len: int):
    """(entries, checksums) of a valid stand-alone table, else None"""
    n = len(t)
    if n < 25 or n > object_len or object_len > 0x7FFFFFFF:
        return None
    if struct.unpack_from("<I", t, n - 4)[0] != SEEK_MAGIC or t[n - 5] not in (0, 0x80):
        return None
    e = 12 if t[n - 5] else 8
    nf = struct.unpack_from("<I", t, n - 9)[0]
    if nf < 1 or nf > MAX_FRAMES or e * nf + 17 != n:
        return None
    if struct.unpack_from("<II", t, 0) != (SKIP_MAGIC, e * nf + 9):
        return None
    ent = [struct.unpack_from("<III" if e == 12 else "<II", t, 8 + e * k) for k in range(nf)]
    if any(x[0] < 1 for x in ent) or sum(x[0] for x in ent) != object_len - n or sum(x[1] for x in ent) >= 1 << 32:
        return None
    return ent, e == 12


def plan(t: bytes, object_len: int, lo: int, hi: int, cap=None):
    """None without a valid table, else what jfs_zstd_seek_plan answers with
    status OK (cap None: hi' = min(hi, D)), plus cend / flo / fhi"""
    p = parse(t, object_len)
    if p is None:
        return None
    ent, wide = p
    total = sum(x[1] for x in ent)
    lo, hi = max(lo, 0), min(hi, total if cap is None else cap)
    pos, cpos, sel = 0, 0, []
    for k, x in enumerate(ent):
        c, d = x[0], x[1]
        # seek_select's rule: not wholly in front of the range, and starting inside it
        if hi > lo and not pos + d <= lo and pos < hi:
            sel.append((k, cpos, cpos + c, pos, pos + d))
        pos, cpos = pos + d, cpos + c
    r = dict(checksums=int(wide), nf=len(ent), content=total, first=0, count=0, get_off=0, get_len=0, first_off=0,
             flo=0, fhi=0, table_off=object_len - len(t), table_len=len(t))
    if sel:
        r.update(first=sel[0][0], count=sel[-1][0] - sel[0][0] + 1, get_off=sel[0][1], get_len=sel[-1][2] - sel[0][1],
                 first_off=sel[0][3], flo=sel[0][3], fhi=sel[-1][4])
    return r
