"""GPU: jfs_zstd_seek_tables_device alone against a pure-Python
footer check written here.  Hand-built objects of 1, 2, 63, 64, 65 and 16,384
frames in both layouts, at payload offsets 0, 1, 3 and 15 from a 16-byte
boundary; d_len of -1, 0, 24 and 25; a NULL src; every footer and header field
damaged a byte at a time; a frame count past the cap and past the input; a slot
one byte too short.  All inputs go through one launch; every slot and the bytes
around the packed buffer start as a canary, and the whole buffer is compared with
its expected image, so a byte written outside a table's place fails the test."""
import struct

import numpy as np
import pytest
import torch

from juicefs_amd import device as D
from tests import zstd_seek_csum_cases as X
from tests.zstd_seek_cases import MAX_FRAMES, SEEK_MAGIC, SKIP_MAGIC

pytestmark = pytest.mark.gpu
CANARY = 0xA5
GUARD = 64


def ref_table_len(buf: bytes, n: int) -> int:
    """the issue's checks, nothing more: the footer at the end of buf[:n], the skippable header it points to"""
    if n < 25:
        return 0
    if struct.unpack_from("<I", buf, n - 4)[0] != SEEK_MAGIC or buf[n - 5] not in (0x00, 0x80):
        return 0
    e = 12 if buf[n - 5] else 8
    nf = struct.unpack_from("<I", buf, n - 9)[0]
    if nf < 1 or nf > MAX_FRAMES:
        return 0
    t = e * nf + 17
    if t > n or struct.unpack_from("<II", buf, n - t) != (SKIP_MAGIC, e * nf + 9):
        return 0
    return t


def entries(nf, wide):
    return [(1 + k % 3, 131072) + (((k * 2654435761 + 99) & 0xFFFFFFFF,) if wide else ()) for k in range(nf)]


def obj(count, wide, **over):
    """frames' bytes (never read) and the table of `count` entries, any field of which `over` replaces"""
    ent = entries(count, wide)
    return bytes((7 * k + 1) & 255 for k in range(sum(x[0] for x in ent))) + X.table(ent, **over)


def slot_of(t):
    return (t + 15) // 16 * 16


def cases():
    """[(bytes, offset from a 16-byte boundary, d_len or None for len(bytes), slot bytes, null src)]"""
    out = []
    for nf in (1, 2, 63, 64, 65):
        for wide in (False, True):
            for off in (0, 1, 3, 15):
                o = obj(nf, wide)
                out.append((o, off, None, slot_of((12 if wide else 8) * nf + 17), False))
    big = obj(MAX_FRAMES, True)
    out.append((big, 5, None, slot_of(12 * MAX_FRAMES + 17), False))
    out.append((obj(MAX_FRAMES + 1, False), 2, None, slot_of(8 * (MAX_FRAMES + 1) + 17), False))  # past the cap
    alone = X.table(entries(1, False))  # 25 bytes: a table and no frame in front of it
    assert len(alone) == 25
    for n in (-1, 0, 24, 25):
        out.append((alone, 3, n, 32, False))
    out.append((obj(2, True), 1, None, 48, True))  # NULL src
    good = obj(3, True)
    n, t = len(good), 12 * 3 + 17
    for at in list(range(n - 9, n)) + list(range(n - t, n - t + 8)):  # the footer's 9 bytes, the header's 8
        for bit in (0x01, 0x80):
            b = bytearray(good)
            b[at] ^= bit
            out.append((bytes(b), at % 16, None, 64, False))
    for desc in (0x01, 0x40, 0x7F, 0x81, 0xFF):
        out.append((obj(3, False, descriptor=desc), 1, None, 64, False))
    out.append((obj(3, False, nf=0), 1, None, 64, False))
    short = X.table(entries(4, True))[12:]  # a footer that says 4 entries at the end of too few bytes
    out.append((short, 7, None, 80, False))
    out.append((obj(2, False), 9, None, 32, False))   # T = 33: the slot is one byte too short
    out.append((obj(2, False), 9, None, 48, False))   # and beside it the same table in a slot it fits
    out.append((obj(1, True), 15, None, 16, False))   # T = 29 in a slot of 16
    out.append((obj(1, True), 15, None, 0, False))    # an empty slot
    return out


def test_tables_into_slots(gpu):
    cs = cases()
    n = len(cs)
    at, pos = [], 0
    for o, off, _, _, _ in cs:
        at.append(pos + off)
        pos += (off + len(o) + 15) // 16 * 16 + 16
    host = np.full(pos, 0x3C, dtype=np.uint8)
    for (o, _, _, _, _), a in zip(cs, at):
        host[a:a + len(o)] = np.frombuffer(o, dtype=np.uint8)
    src = torch.from_numpy(host).to(gpu)
    lens = [len(o) if ln is None else ln for o, _, ln, _, _ in cs]
    slot_first = np.concatenate([[0], np.cumsum([c[3] for c in cs])]).astype(np.int32)
    packed = torch.full((GUARD + int(slot_first[-1]) + GUARD,), CANARY, dtype=torch.uint8, device=gpu)
    desc = np.zeros(n, dtype=D.DESC_DTYPE)
    desc["src"] = [0 if null else src.data_ptr() + a for (_, _, _, _, null), a in zip(cs, at)]
    desc["dst"], desc["src_len"], desc["dst_cap"] = 0xDEAD0000, -7, -7  # ignored
    t_desc = torch.from_numpy(desc.view(np.uint8).copy()).to(gpu)
    t_len = torch.tensor(lens, dtype=torch.int32, device=gpu)
    t_sf = torch.from_numpy(slot_first).to(gpu)
    t_tl = torch.full((n + 2,), -99, dtype=torch.int32, device=gpu)
    D.zstd_seek_tables(t_desc, t_len, t_sf, packed[GUARD:], t_tl[1:n + 1])
    torch.cuda.synchronize()
    got_len = t_tl.cpu().tolist()
    assert got_len[0] == -99 and got_len[-1] == -99
    want_img = np.full(packed.numel(), CANARY, dtype=np.uint8)
    want_len, placed = [], 0
    for (o, _, ln, slot, null), m, s0 in zip(cs, lens, slot_first[:-1]):
        t = 0 if null else ref_table_len(o, m)
        if t > slot:
            t = 0
        want_len.append(t)
        if t:
            want_img[GUARD + s0:GUARD + s0 + t] = np.frombuffer(o[m - t:m], dtype=np.uint8)
            placed += 1
    assert got_len[1:-1] == want_len
    bad = np.nonzero(packed.cpu().numpy() != want_img)[0]
    assert bad.size == 0, f"first wrong byte at {bad[0] - GUARD} of the packed buffer ({bad.size} wrong)"
    # what the cases are for: 40 + 1 + 1 + 1 good ones, and the d_len of 25
    assert placed == 43 and want_len[41] == 0 and want_len[-4:] == [0, 33, 0, 0]
    assert want_len[42:46] == [0, 0, 0, 25]
    assert torch.equal(src.cpu(), torch.from_numpy(host))  # the inputs are only read
