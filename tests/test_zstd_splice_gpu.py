"""GPU: jfs_zstd_splice_device alone -- seekable objects
assembled from frames that already exist.  Frames are cut out of the seekable
encoder's objects of text and random data (outputs of 2, 5 and 70 frames: 70
crosses the scan's 64-frame round; all PASS, all FRESH, alternating; both table
layouts), and hand-made records over patterned bytes sweep compressed lengths
1, 15, 16, 17, 33 and 131,093 over all 16 x 16 source and destination
alignments.  Every call's whole guard-filled destination is compared against
objects assembled in Python; verdicts (one byte short, a failed unit, a bad
record) write nothing; batches of 1 and of 64 outputs."""
import struct

import numpy as np
import pytest
import torch

from juicefs_amd import device as D
from juicefs_amd.blockgen import gen_block
from tests import zstd_seek_cases as S
from tests import zstd_seek_csum_cases as X
from tests.test_zstd_fast_gpu import _libzstd_decode
from tests.test_zstd_seekable_gpu import encode

pytestmark = pytest.mark.gpu
GUARD = 0x5A
B = S.FRAME
CHAIN_FAILED = -(1 << 31)


def P(data, d=None, x=0):
    """a PASS frame: stored bytes, content size, checksum word"""
    return dict(data=data, d=len(data) if d is None else d, x=x, fresh=False)


def Fr(data, d=None, h=0, ret=None):
    """a FRESH frame: its unit's buffer, content size, the unit's XXH64 and encode result (default: len(data))"""
    return dict(data=data, d=len(data) if d is None else d, h=h, fresh=True, ret=len(data) if ret is None else ret)


def table(frames, wide):
    ent = []
    for f in frames:
        c = f["ret"] if f["fresh"] else len(f["data"])
        ent.append((c, f["d"]) + (((f["h"] if f["fresh"] else f["x"]) & 0xFFFFFFFF,) if wide else ()))
    return X.table(ent) if wide else S.table(ent)


def assembled(frames, wide):
    return b"".join(f["data"] for f in frames) + table(frames, wide)


def run(dev, outs, wide, caps=None, dst_align=None, src_align=None):
    """One call.  outs = [[frame, ...]]; caps[j] (default: the object's size);
    output j's dst at alignment dst_align[j] (default 3 j + 1), frame q's bytes
    at alignment src_align(q) (default 5 q + 2) -> (rets, the dst image, dst offsets)"""
    frames = [(j, f) for j, fs in enumerate(outs) for f in fs]
    soff, pos = [], 0
    for q, (_, f) in enumerate(frames):
        a = (src_align(q) if src_align else 5 * q + 2) % 16
        pos = ((pos + 15) & ~15) + a
        soff.append(pos)
        pos += len(f["data"]) + 1
    host = np.full(pos + 32, 0xEE, dtype=np.uint8)
    for o, (_, f) in zip(soff, frames):
        host[o:o + len(f["data"])] = np.frombuffer(f["data"], dtype=np.uint8)
    src_t = torch.from_numpy(host).to(dev)
    sizes = [sum(len(f["data"]) for f in fs) + (12 if wide else 8) * len(fs) + 17 for fs in outs]
    caps = sizes if caps is None else caps
    doff, pos = [], 0
    for j, c in enumerate(caps):
        a = (dst_align[j] if dst_align else 3 * j + 1) % 16
        pos = ((pos + 15) & ~15) + 16 + a
        doff.append(pos)
        pos += max(c, sizes[j]) + 16
    dst_t = torch.full((pos + 32,), GUARD, dtype=torch.uint8, device=dev)
    fr = np.zeros(len(frames), dtype=D.SPLICE_FRAME_DTYPE)
    ulen, uhash = [], []
    for q, (j, f) in enumerate(frames):
        fr[q] = (src_t.data_ptr() + soff[q], 0 if f["fresh"] else f.get("c", len(f["data"])), f["d"], 0 if f["fresh"] else f["x"],
                 len(ulen) if f["fresh"] else -1, f.get("out", j), 0)
        if f["fresh"]:
            ulen.append(f["ret"])
            uhash.append(f["h"])
    so = np.zeros(len(outs), dtype=D.SPLICE_OUT_DTYPE)
    first = 0
    for j, fs in enumerate(outs):
        so[j] = (dst_t.data_ptr() + doff[j], caps[j], first, len(fs), 0)
        first += len(fs)
    t_fr = torch.from_numpy(fr.view(np.uint8).copy()).to(dev)
    t_so = torch.from_numpy(so.view(np.uint8).copy()).to(dev)
    t_len = torch.tensor(ulen or [0], dtype=torch.int32, device=dev)
    t_hash = torch.from_numpy(np.array(uhash or [0], dtype=np.uint64).view(np.int64).copy()).to(dev) if wide else None
    ret = torch.full((len(outs),), -777, dtype=torch.int32, device=dev)
    D.zstd_splice(t_so, t_fr, t_len, t_hash, ret)
    torch.cuda.synchronize()
    return ret.cpu().tolist(), dst_t.cpu().numpy(), doff


def check_image(img, doff, objs):
    """objs[j] = the bytes output j must hold (b"" for a failed one); guards everywhere else"""
    want = np.full(len(img), GUARD, dtype=np.uint8)
    for o, b in zip(doff, objs):
        want[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    bad = np.nonzero(img != want)[0]
    assert bad.size == 0, f"first wrong byte at {bad[0]} of the dst tensor ({len(bad)} wrong)"


_cache = {}


def material(dev):
    """(class, frames) -> (raw, [(frame bytes, content bytes)]): the seekable encoder's objects, cut at their tables"""
    if not _cache:
        keys = [(cls, nf) for cls in "TR" for nf in (2, 5, 70)]
        raws = [gen_block(cls, 8100 + i, (nf - 1) * B + 777 + 4000 * i) for i, (cls, nf) in enumerate(keys)]
        r, objs, _, _ = encode(dev, raws, [D.zstd_bound(len(x)) for x in raws])
        for k, raw, obj in zip(keys, raws, objs):
            ent = S.parse_table(obj)
            assert ent is not None and len(ent) == k[1]
            fr, at = [], 0
            for c, d in ent:
                fr.append((obj[at:at + c], d))
                at += c
            _cache[k] = (raw, fr, obj)
    return _cache


def hashes(dev, pieces):
    """XXH64 of every piece, on the device (jfs_xxh64_device)"""
    host = np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()
    t = torch.from_numpy(host).to(dev)
    offs = np.cumsum([0] + [len(p) for p in pieces[:-1]]).tolist()
    desc = D.make_desc(t, offs, [len(p) for p in pieces], t, [0] * len(pieces), [0] * len(pieces))
    h = torch.zeros(len(pieces), dtype=torch.int64, device=dev)
    D.xxh64(desc, h)
    torch.cuda.synchronize()
    return [int(x) & 0xFFFFFFFFFFFFFFFF for x in h.cpu().tolist()]


@pytest.mark.parametrize("wide", [False, True])
def test_encoder_frames_in_every_mix(gpu, wide):
    mat = material(gpu)
    outs, raws = [], []
    for (cls, nf), (raw, fr, obj) in mat.items():
        hs = hashes(gpu, [raw[k * B:(k + 1) * B] for k in range(nf)]) if wide else [0] * nf
        if wide and nf == 2:
            assert [h & 0xFFFFFFFF for h in hs] == [X.xxh64(raw[k * B:(k + 1) * B]) & 0xFFFFFFFF for k in range(nf)]
        for mix in ("pass", "fresh", "alt"):
            fs = []
            for k, (data, d) in enumerate(fr):
                fresh = mix == "fresh" or (mix == "alt" and k % 2 == 1)
                fs.append(Fr(data, d, hs[k]) if fresh else P(data, d, hs[k] & 0xFFFFFFFF))
            outs.append(fs)
            raws.append(raw)
        if not wide:  # all PASS over 8-byte tables is the encoder's own object again
            assert assembled(outs[-3], False) == obj
    want = [assembled(fs, wide) for fs in outs]
    r, img, doff = run(gpu, outs, wide)
    assert r == [len(w) for w in want]
    check_image(img, doff, want)
    for j in (0, 8, 9, 17):  # what came off the device decodes to the source, for libzstd too
        got = img[doff[j]:doff[j] + r[j]].tobytes()
        dec = _libzstd_decode(got, len(raws[j]))
        assert dec is None or dec == raws[j]
        ent = X.parse(got[len(got) - (12 if wide else 8) * len(outs[j]) - 17:], len(got))
        assert ent is not None and ent[1] == wide and len(ent[0]) == len(outs[j])


def patterned(n, seed):
    return bytes((seed * 131 + 7 * i + (i >> 8)) & 0xFF for i in range(n))


@pytest.mark.parametrize("wide", [False, True])
def test_lengths_over_all_alignments(gpu, wide):
    """Per output, 16 groups of the six lengths: a group's bytes add up to 7 mod
    16, so inside one output every length meets every destination alignment,
    each with another source alignment; the 16 outputs start at the 16
    destination alignments, so all 256 pairs occur for every length."""
    lens = [1, 15, 16, 17, 131093, 33]
    assert sum(lens) % 16 == 7
    bodies = {n: patterned(n + 15, n) for n in lens}
    outs = []
    for j in range(16):
        fs = []
        for a in range(16):
            for n in lens:
                data = bodies[n][a:a + n]
                fresh = wide and (a + n) % 3 == 0
                fs.append(Fr(data, n + a, 0x1234567800000000 | (n * 16 + a)) if fresh else P(data, n + a, 0xC0000000 | (n * 16 + a)))
        outs.append(fs)
    want = [assembled(fs, wide) for fs in outs]
    r, img, doff = run(gpu, outs, wide, dst_align=list(range(16)), src_align=lambda q: q // len(lens))
    assert r == [len(w) for w in want]
    check_image(img, doff, want)


@pytest.mark.parametrize("wide", [False, True])
def test_verdicts_write_nothing(gpu, wide):
    a, b, c = patterned(5000, 1), patterned(70000, 2), patterned(333, 3)
    good = [P(a), Fr(b, h=77), P(c)]
    size = len(assembled(good, wide))
    outs = [good,
            good,                                       # dst_cap one byte short
            [P(a), Fr(b, h=77, ret=0), P(c)],            # the unit's encoder answered 0
            [P(a), Fr(b, ret=-2), Fr(c, ret=CHAIN_FAILED)],  # a failed gather wins over an encoder's refusal
            [Fr(a, ret=-2), P(b), Fr(c, ret=-1)],        # else the first failed unit's result
            [P(a), dict(P(b), c=0)],                     # a PASS frame without bytes
            [P(a), dict(P(b), out=0)],                   # a frame that says it is another output's
            good]
    caps = [size, size - 1] + [size + 64] * 5 + [size + 1]
    r, img, doff = run(gpu, outs, wide, caps=caps)
    assert r == [size, 0, 0, CHAIN_FAILED, -2, -1, -1, size]
    want = assembled(good, wide)
    check_image(img, doff, [want, b"", b"", b"", b"", b"", b"", want])


@pytest.mark.parametrize("nout", [1, 64])
def test_batch_sizes(gpu, nout):
    outs = [[P(patterned(100 + 37 * j, j), x=j), Fr(patterned(1 + 1000 * (j % 5), j + 1), h=j << 3)] for j in range(nout)]
    for wide in (False, True):
        want = [assembled(fs, wide) for fs in outs]
        r, img, doff = run(gpu, outs, wide)
        assert r == [len(w) for w in want]
        check_image(img, doff, want)


def test_table_fields(gpu):
    """the table as the format writes it, field by field"""
    fs = [P(b"abc", d=9, x=0xDEADBEEF), Fr(b"defgh", d=11, h=0x1122334455667788)]
    r, img, doff = run(gpu, [fs], True)
    got = img[doff[0]:doff[0] + r[0]].tobytes()
    assert got == b"abcdefgh" + struct.pack("<II", 0x184D2A5E, 12 * 2 + 9) + struct.pack("<III", 3, 9, 0xDEADBEEF) + \
        struct.pack("<III", 5, 11, 0x55667788) + struct.pack("<IB", 2, 0x80) + struct.pack("<I", 0x8F92EAB1)
