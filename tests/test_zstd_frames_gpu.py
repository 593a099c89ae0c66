"""GPU: jfs_zstd_decompress_frames_device -- the range decode from
a stand-alone table and a fragment of the object's frames, as a ranged GET
planned by jfs_zstd_seek_plan delivers them, every decoded frame verified
against its table checksum.  Only table + fragment are uploaded; the whole
destination tensor is compared: the full decode inside [flo, fhi), the pre-fill
everywhere else."""
import numpy as np
import pytest
import torch

from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd.blockgen import gen_block
from tests import zstd_seek_cases as S
from tests import zstd_seek_csum_cases as X
from tests.test_zstd_seek_csum_gpu import objects
from tests.test_zstd_seekable_gpu import CANARY, check_image

pytestmark = pytest.mark.gpu
B = S.FRAME


def run_frames(dev, items):
    """items = [(table, object_len, frag, frag_off, cap, lo, hi)]; table / frag of
    None give NULL pointers, cap None a NULL dst.  Everything at odd offsets;
    -> (rets, the whole dst tensor, dst offsets)"""
    toffs, foffs, doffs, off, doff = [], [], [], 0, 0
    for i, (t, _, f, _, cap, _, _) in enumerate(items):
        toffs.append(None if t is None else off + 1 + (3 * i) % 8)
        off += len(t or b"") + 24
        foffs.append(None if f is None else off + 1 + (5 * i) % 8)
        off += len(f or b"") + 24
        doffs.append(None if cap is None else doff + 1 + 2 * ((5 * i) % 8))
        doff = (doff + max(cap or 0, 0) + 64 + 15) & ~15
    host = np.full(off + 64, 0xEE, dtype=np.uint8)
    for (t, _, f, _, _, _, _), to, fo in zip(items, toffs, foffs):
        if t:
            host[to:to + len(t)] = np.frombuffer(t, dtype=np.uint8)
        if f:
            host[fo:fo + len(f)] = np.frombuffer(f, dtype=np.uint8)
    buf = torch.from_numpy(host).to(dev)
    dst = torch.full((doff + 64,), CANARY, dtype=torch.uint8, device=dev)
    desc = D.make_frag_desc(buf, toffs, [len(it[0] or b"") for it in items],
                            [it[1] for it in items], foffs, [it[3] for it in items], [len(it[2] or b"") for it in items],
                            dst, doffs, [it[4] or 0 for it in items])
    ret = torch.full((len(items),), -12345, dtype=torch.int32, device=dev)
    D.zstd_decompress_frames(desc, torch.tensor([it[5] for it in items], dtype=torch.int32, device=dev),
                             torch.tensor([it[6] for it in items], dtype=torch.int32, device=dev), ret)
    torch.cuda.synchronize()
    return ret.cpu().tolist(), dst.cpu().numpy(), [d or 0 for d in doffs]


def fetch(obj, tail_len, lo, hi):
    """the ranged GETs of one read: (table, fragment, its offset, the plan), planned from the last tail_len bytes"""
    p = C.seek_plan(obj[len(obj) - tail_len:], len(obj), lo, hi)
    if p["status"] == "more":
        assert p["table_len"] > tail_len
        tail_len = p["table_len"]
        p = C.seek_plan(obj[p["table_off"]:p["table_off"] + p["table_len"]], len(obj), lo, hi)
    assert p["status"] == "ok"
    t = obj[p["table_off"]:p["table_off"] + p["table_len"]]
    return t, obj[p["get_off"]:p["get_off"] + p["get_len"]], p["get_off"], p


def ranges_for(n):
    mid = (n // B // 2) * B
    return [(0, 1), (n - 1, n), (mid + 5, mid + 6), (B - 1, B + 1), (0, n), (5, 5), (n, n + 7), (-9, 3), (n - 5, n + 1000)]


def test_planned_reads_in_one_batch(gpu):
    """8-byte and 12-byte tables in one batch; more than JFS_ZSTD_SPLIT_MAX expanded entries (the one-wave path)"""
    items, expect = [], []
    for key, col, tails in ((("T", 4 * B + 777), 1, (64, 4096)), (("T", 4 * B + 777), 2, (64, 4096)),
                            (("Z", 2 * B), 1, (64, 4096)), (("R", 69 * B + 5), 1, (64,)), (("R", 69 * B + 5), 2, (4096,))):
        got = objects(gpu)[key]
        raw, obj = got[0], got[col]
        n = len(raw)
        for tail in tails:
            for lo, hi in ranges_for(n) if n < 8 * B or tail == 64 else ranges_for(n)[:4]:
                t, frag, foff, p = fetch(obj, tail, lo, hi)
                assert p["checksums"] == (1 if col == 1 else 0)
                assert len(frag) < len(obj) - len(t) or p["count"] == p["nf"], "only the selected frames' bytes"
                w = X.plan(t, len(obj), lo, hi)
                items.append((t, len(obj), frag, foff, n, lo, hi))
                expect.append((0 if min(hi, n) <= max(lo, 0) else min(n, hi), w["flo"], raw[w["flo"]:w["fhi"]]))
    assert sum(X.plan(it[0], it[1], it[5], it[6])["count"] for it in items) > 128
    D.zstd_split_counts(reset=True)
    rets, img, do = run_frames(gpu, items)
    assert D.zstd_split_counts() == (0, 0)
    assert rets == [e[0] for e in expect]
    check_image(img, do, [(i, e[1], e[2]) for i, e in enumerate(expect)])


def test_small_batch_path_and_resident_object(gpu):
    raw, obj, obj8 = objects(gpu)[("Z", 2 * B)]
    n = len(raw)
    t, frag, foff, _ = fetch(obj, 64, B - 1, B + 1)
    t8, frag8, foff8, _ = fetch(obj8, 64, B + 7, B + 9)
    D.zstd_split_counts(reset=True)
    # the third input: the whole object as the fragment (a resident object, verified)
    rets, img, do = run_frames(gpu, [(t, len(obj), frag, foff, n, B - 1, B + 1), (t8, len(obj8), frag8, foff8, n + 50, B + 7, B + 9),
                                     (t, len(obj), obj, 0, n, 0, n)])
    done, handed = D.zstd_split_counts()
    assert done + handed == 5, "five frames through the small-batch path"
    assert rets == [B + 1, B + 9, n]
    check_image(img, do, [(0, 0, raw), (1, B, raw[B:]), (2, 0, raw)])


def hand_built(checksums):
    contents = [gen_block("R", 7700 + k, m) for k, m in enumerate((3000, 1, 5000, 70000, 300))]
    obj, t, ent = X.build(contents, checksums)
    return contents, obj, t, ent


def test_verdicts(gpu):
    contents, obj, t, ent = hand_built(True)
    _, obj8, t8, ent8 = hand_built(False)
    raw = b"".join(contents)
    n, olen, body = len(raw), len(obj), obj[:len(obj) - len(t)]
    assert body == obj8[:len(obj8) - len(t8)]
    c0 = [sum(e[0] for e in ent[:k]) for k in range(len(ent) + 1)]
    d0 = [sum(e[1] for e in ent[:k]) for k in range(len(ent) + 1)]
    # a table checksum with one flipped bit (frame 2)
    badsum = bytearray(t)
    badsum[8 + 12 * 2 + 8] ^= 0x10
    badsum = bytes(badsum)
    # one flipped bit inside frame 3's literals: a raw block, so every Zstd decoder returns the right length
    assert ent[3][0] == 70000 + 12  # magic 4, descriptor 1, content size 4, block header 3
    flip = bytearray(body)
    flip[c0[3] + 12 + 2000] ^= 0x04
    flip = bytes(flip)
    # frame 3's content size damaged: it fails to decode
    broke = bytearray(body)
    broke[c0[3] + 5] ^= 0x5A
    broke = bytes(broke)
    items = [
        (badsum, olen, body, 0, n, d0[2], d0[2] + 1),          # 0: selects frame 2: -4
        (badsum, olen, body, 0, n, 0, n),                      # 1: all frames: -4
        (badsum, olen, body, 0, n, d0[3], n),                  # 2: frames 3, 4: the plain result
        (badsum, olen, body[:c0[2]], 0, n, 0, d0[2]),          # 3: frames 0, 1 from their own fragment
        (t, olen, flip, 0, n, d0[3] + 5, d0[3] + 6),           # 4: -4 -- the point of the feature:
        (t8, len(obj8), flip, 0, n, d0[3] + 5, d0[3] + 6),     # 5: the same damage under an 8-byte table goes unseen
        (t, olen, flip, 0, n, 0, d0[3]),                       # 6: a read that does not select the frame
        (t, olen, broke, 0, n, 0, n),                          # 7: -1
        (badsum, olen, broke, 0, n, 0, n),                     # 8: -1 wins over -4
        (t, olen, body[c0[1]:c0[3] - 1], c0[1], n, d0[1], d0[3]),      # 9: one byte short at the end: -3
        (t, olen, body[c0[1] + 1:c0[3]], c0[1] + 1, n, d0[1], d0[3]),  # 10: and at the start
        (t, olen, body[c0[1]:c0[3]], c0[1], n, d0[1], d0[3]),          # 11: exactly the frames
        (t, olen, body, 0, n - 1, 0, 10),                      # 12: D > dst_cap: -2
        (t, olen, body, 0, 0, 0, 10),                          # 13: dst_cap == 0
        (t, olen, body, 0, n, 7, 7),                           # 14: an empty range
        (t, olen + 1, body, 0, n, 0, 10),                      # 15: invalid tables: -1
        (t[1:], olen, body, 0, n, 0, 10),                      # 16
        (X.table(ent, descriptor=0x81), olen, body, 0, n, 0, 10),  # 17
        (t8, olen, body, 0, n, 0, 10),                         # 18: the 8-byte table of the shorter object
        (None, olen, body, 0, n, 0, 10),                       # 19: NULLs and negative sizes: -1
        (t, olen, None, 0, n, 0, 10),                          # 20
        (t, olen, body, 0, None, 0, 10),                       # 21
        (t, olen, body, -1, n, 0, 10),                         # 22
        (t, -5, body, 0, n, 0, 10),                            # 23
        (t, olen, body, 0, n + 100, n - 1, n + 50),            # 24: hi > D under a larger capacity
    ]
    rets, img, do = run_frames(gpu, items)
    assert rets[:4] == [-4, -4, n, d0[2]]
    assert rets[4] == -4 and rets[5] == d0[3] + 6, "verification is what tells a silently damaged frame"
    assert rets[6] == d0[3]
    assert rets[7:9] == [-1, -1]
    assert rets[9:12] == [-3, -3, d0[3]]
    assert rets[12:15] == [-2, 0, 0]
    assert rets[15:24] == [-1] * 9
    assert rets[24] == n
    damaged = raw[:d0[3] + 2000] + bytes([raw[d0[3] + 2000] ^ 0x04]) + raw[d0[3] + 2001:]
    writes = [(0, d0[2], contents[2]), (1, 0, raw), (2, d0[3], raw[d0[3]:]), (3, 0, raw[:d0[2]]),
              (4, d0[3], damaged[d0[3]:d0[4]]), (5, d0[3], damaged[d0[3]:d0[4]]), (6, 0, raw[:d0[3]]),
              (11, d0[1], raw[d0[1]:d0[3]]), (24, d0[4], contents[4])]
    # whatever a failed frame wrote stayed inside the selected frames' output range
    writes += [(i, 0, img[do[i]:do[i] + n].tobytes()) for i in (7, 8)]
    check_image(img, do, writes)
