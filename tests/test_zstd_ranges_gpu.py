"""GPU: jfs_zstd_decompress_ranges_device -- one input decoded
for a list of byte ranges, exactly the frames some range touches, through a
seek table of either layout, the decoded frames of a 12-byte table verified.
Every destination is pre-filled with a guard pattern and the whole tensor is
compared: the source's bytes inside the selected frames' spans, the guard
everywhere else -- the frames between two ranges included.  What must be
selected comes from the pure-Python rule of tests/test_zstd_seek_ranges.py, and
jfs_zstd_sparse_counts must report exactly that many frames."""
import numpy as np
import pytest
import torch

from juicefs_amd import device as D
from juicefs_amd.blockgen import gen_block
from tests import zstd_seek_cases as S
from tests import zstd_seek_csum_cases as X
from tests.test_zstd_frames_gpu import hand_built, run_frames
from tests.test_zstd_seek_csum_gpu import encode, objects
from tests.test_zstd_seek_ranges import parse_any, rule
from tests.test_zstd_seekable_gpu import CANARY, check_image
from tests.xxh64_ref import xxh64

pytestmark = pytest.mark.gpu
B = S.FRAME
SIZES = [B, B + 1, 4 * B + 777, 69 * B + 5]  # 1, 2, 5 and 70 frames


def _run(dev, items, call):
    """items = [(object, dst_cap, ...)]: object None gives a NULL src, b"" an
    empty one.  An object that several items hold is uploaded once; every dst
    lies at an odd offset in a guard-filled tensor.  call(desc, ret) ->
    (rets, the whole dst tensor, dst offsets)"""
    so, do, at, off, doff = [], [], {}, 0, 0
    for i, it in enumerate(items):
        obj, cap = it[0], it[1]
        if obj is not None and id(obj) not in at:
            at[id(obj)] = (off + (7 * i) % 16 + 1, obj)
            off = (at[id(obj)][0] + len(obj) + 64 + 15) & ~15
        so.append(None if obj is None else at[id(obj)][0])
        do.append(doff + 1 + 2 * ((5 * i) % 8))
        doff = (do[-1] + max(cap, 0) + 64 + 15) & ~15
    host = np.zeros(off + 64, dtype=np.uint8)
    for o, obj in at.values():
        host[o:o + len(obj)] = np.frombuffer(obj, dtype=np.uint8)
    src_t = torch.from_numpy(host).to(dev)
    dst_t = torch.full((doff + 64,), CANARY, dtype=torch.uint8, device=dev)
    a = np.zeros(len(items), dtype=D.DESC_DTYPE)
    a["src"] = [0 if o is None else src_t.data_ptr() + o for o in so]
    a["dst"] = [dst_t.data_ptr() + o for o in do]
    a["src_len"] = [0 if it[0] is None else len(it[0]) for it in items]
    a["dst_cap"] = [it[1] for it in items]
    desc = torch.from_numpy(a.view(np.uint8).copy()).to(dev)
    ret = torch.full((len(items),), -12345, dtype=torch.int32, device=dev)
    call(desc, ret)
    torch.cuda.synchronize()
    return ret.cpu().tolist(), dst_t.cpu().numpy(), do


def run_ranges(dev, items, first=None, flat=None):
    """items = [(object, dst_cap, [(lo, hi), ...])]; first / flat replace the running sums and the flat list"""
    if first is None:
        first, flat = [0], []
        for it in items:
            flat += it[2]
            first.append(len(flat))

    def call(desc, ret):
        pairs = torch.from_numpy(np.array(flat, dtype=np.int32).reshape(-1)).to(dev)  # lo, hi, lo, hi, ...
        D.zstd_decompress_ranges(desc, torch.tensor(first, dtype=torch.int32, device=dev), pairs, ret)
    D.zstd_sparse_counts(reset=True)
    rets, img, do = _run(dev, items, call)
    return rets, img, do, D.zstd_sparse_counts()


def run_one_range(dev, items):
    """the same inputs, one range each, through jfs_zstd_decompress_range_device"""
    def call(desc, ret):
        D.zstd_decompress_range(desc, torch.tensor([it[2][0][0] for it in items], dtype=torch.int32, device=dev),
                                torch.tensor([it[2][0][1] for it in items], dtype=torch.int32, device=dev), ret)
    return _run(dev, items, call)


def expect(obj, raw, cap, ranges):
    """(ret, [(flo, bytes)] or None for a prefix decode, (tabled, selected, compared)) of a well-formed object"""
    r = rule(obj, cap, ranges)
    if r["bad"]:
        return -1, [], (0, 0, 0)
    if r["live"] == 0:
        return 0, [], (0, 0, 0)
    if not r["table"]:
        return min(len(raw), r["top"]), None, (0, 0, 0)
    if r["total"] > cap:
        return -2, [], (0, 0, 0)
    return (min(r["total"], r["top"]), [(s[2], raw[s[2]:s[2] + s[4]]) for s in r["sel"]],
            (1, len(r["sel"]), len(r["sel"]) if r["checksums"] else 0))


def check(dev, items, raws):
    """one call over items; raws[i] = item i's content.  Results, the whole image and the counters."""
    rets, img, do, counts = run_ranges(dev, items)
    writes, total = [], [0, 0, 0]
    for i, (obj, cap, ranges) in enumerate(items):
        ret, w, cnt = expect(obj, raws[i], cap, ranges)
        assert rets[i] == ret, (i, ranges, rets[i], ret)
        total = [a + b for a, b in zip(total, cnt)]
        if w is None:  # a prefix decode: dst[0, ret) is the content, dst[ret, dst_cap) is unspecified
            assert img[do[i]:do[i] + ret].tobytes() == raws[i][:ret], i
            writes.append((i, 0, img[do[i]:do[i] + cap].tobytes()))
        else:
            writes += [(i, flo, data) for flo, data in w]
    check_image(img, do, writes)  # every byte outside the selected spans is still guard
    assert counts == tuple(total), (counts, total)
    return rets, img, do


def lists_for(n):
    """first and last frame only; the frame edges; every frame; all empty; clamped and negative ends"""
    return [[(0, 1), (n - 1, n)], [(B - 1, B)], [(B, B + 1)], [(B - 1, B + 1), (n - 1, n)], [(0, n)],
            [(5, 5), (B, B), (n, n)], [(-9, 3), (n - 5, n + 1000)], [(-20, -10), (3 * B, 3 * B + 1), (n + 5, n + 9)]]


_cache = {}


def tabled(dev):
    """130 frames, content sizes cycling 0, 1, 777, 4096, each piece encoded on its own; the table written here in
    both layouts -> (raw, 8-byte object, 12-byte object, content edges)"""
    if "tabled" not in _cache:
        pieces = [gen_block("T", 8100 + k, [0, 1, 777, 4096][k % 4]) for k in range(130)]
        r, frames, _, _ = encode(dev, pieces, [D.zstd_bound(len(p)) for p in pieces], D.zstd_compress_fast)
        assert all(x > 0 for x in r)
        body = b"".join(frames)
        ent8 = [(len(f), len(p)) for f, p in zip(frames, pieces)]
        ent12 = [(len(f), len(p), xxh64(p) & 0xFFFFFFFF) for f, p in zip(frames, pieces)]
        raw = b"".join(pieces)
        assert len(body) + 12 * 130 + 17 < 200 << 10
        ed = [sum(len(p) for p in pieces[:k]) for k in range(131)]
        _cache["tabled"] = (raw, body + X.table(ent8), body + X.table(ent12), ed)
    return _cache["tabled"]


@pytest.mark.parametrize("cls", ["T", "Z", "R"])
def test_lists_on_encoder_objects(gpu, cls):
    items, raws = [], []
    for n in SIZES:
        raw, obj12, obj8 = objects(gpu)[(cls, n)]
        assert (parse_any(obj8) is None) == (n <= B)
        for obj in (obj8, obj12):
            for ls in lists_for(n) if n < 8 * B else lists_for(n)[:4] + lists_for(n)[5:]:
                items.append((obj, n, ls))
                raws.append(raw)
    # every frame of a 70-frame object, once per layout, under a larger capacity
    raw, obj12, obj8 = objects(gpu)[(cls, 69 * B + 5)]
    items += [(obj12, len(raw) + 100, [(0, len(raw) + 50)]), (obj8, len(raw) + 100, [(-3, B), (B, 1 << 30)])]
    raws += [raw, raw]
    check(gpu, items, raws)
    # first and last frame only: 2 of 70 frames, 68 untouched
    r = rule(obj12, len(raw), [(0, 1), (len(raw) - 1, len(raw))])
    assert [s[0] for s in r["sel"]] == [0, 69]


def test_one_range_equals_the_range_call(gpu, oracle):
    raw5, obj12, obj8 = objects(gpu)[("T", 4 * B + 777)]
    raw1, one, _ = objects(gpu)[("Z", B)]  # one frame: no table
    exact = oracle.zstd_compress_l1(raw1)  # the exact encoder's frame, no table
    broken = obj8[:-1] + bytes([obj8[-1] ^ 1])  # the footer magic: an ordinary object of five frames
    n = len(raw5)
    items = []
    for lo, hi in [(0, 1), (B - 1, B + 1), (2 * B, 2 * B + 1), (n - 1, n), (0, n), (5, 5), (-9, 3), (n - 5, n + 1000), (n, n + 7)]:
        items += [(obj8, n, [(lo, hi)]), (broken, n, [(lo, hi)])]
        if hi <= B + 1:
            items += [(one, B, [(lo, hi)]), (exact, B, [(lo, hi)])]
    items += [(obj8, n - 1, [(0, 10)]), (obj8, n + 100, [(n - 1, n + 50)]), (None, 100, [(0, 10)]), (b"", 100, [(0, 10)]),
              (obj8, 0, [(0, 10)])]
    a, aimg, ado, _ = run_ranges(gpu, items)
    b, bimg, bdo = run_one_range(gpu, items)
    assert a == b and ado == bdo
    for i, (obj, cap, _) in enumerate(items):
        if obj is None or parse_any(obj) is not None or a[i] <= 0:
            assert (aimg[ado[i] - 1:ado[i] + cap + 1] == bimg[ado[i] - 1:ado[i] + cap + 1]).all(), i
        else:  # a prefix decode: the bytes behind ret are unspecified
            assert (aimg[ado[i]:ado[i] + a[i]] == bimg[ado[i]:ado[i] + a[i]]).all(), i
    # 12-byte tables: jfs_zstd_decompress_frames_device, given the whole object as fragment
    t = obj12[len(obj12) - (12 * 5 + 17):]
    rs = [(0, 1), (B - 1, B + 1), (n - 1, n), (0, n), (5, 5), (-9, 3), (n - 5, n + 1000)]
    a, aimg, ado, counts = run_ranges(gpu, [(obj12, n, [r]) for r in rs])
    b, bimg, bdo = run_frames(gpu, [(t, len(obj12), obj12, 0, n, lo, hi) for lo, hi in rs])
    assert a == b
    for i in range(len(rs)):  # the guard bytes on either side included
        assert (aimg[ado[i] - 1:ado[i] + n + 1] == bimg[bdo[i] - 1:bdo[i] + n + 1]).all(), rs[i]
    assert counts == (6, 1 + 2 + 1 + 5 + 1 + 1, 11)


@pytest.mark.parametrize("wide", [False, True])
def test_hand_tabled_object(gpu, wide):
    raw, o8, o12, ed = tabled(gpu)
    obj, n = (o12 if wide else o8), len(raw)
    assert parse_any(obj)[1] == (12 if wide else 8) and ed[-1] == n
    k = 63  # content 4096: [ed[63], ed[64]); frame 64 has none
    assert ed[64] == ed[65] and ed[63] + 4096 == ed[64]
    lists = [
        [(ed[62], ed[66])],                                # frames 62 to 65, across the two rounds; 64 has no content
        [(ed[k] - 1, ed[k])], [(ed[k], ed[k] + 1)],        # hi == D_k does not select k; lo == D_k - 1 selects k - 1
        [(ed[k + 1] - 1, ed[k + 1] + 1)],                  # 63 and 65: the frame without content between them is not selected
        [(0, 1), (n - 1, n)],                              # first and last frame with content
        [(0, n)],                                          # every frame
        [(ed[q], ed[q] + 1) for q in range(3, 130, 8)],   # sixteen single frames, seven left out between each two
        [(ed[q] - 1, ed[q] + 1) for q in range(2, 130, 4)],
        [(7, 7), (ed[64], ed[64]), (n, n)],                # all empty
        [(-50, -1), (ed[129], n + 1000)],                  # clamped and negative ends
    ]
    items = [(obj, n + (i % 2), ls) for i, ls in enumerate(lists)]
    sel = [[s[0] for s in rule(obj, cap, ls)["sel"]] for _, cap, ls in items]
    assert sel[0] == [62, 63, 65] and sel[1] == [62] and sel[2] == [63] and sel[3] == [63, 65]
    assert sel[4] == [1, 129] and len(sel[5]) == 97 and sel[6] == list(range(3, 130, 8)) and sel[8] == []
    check(gpu, items, [raw] * len(items))


def test_mixed_batch_equals_each_kind_alone(gpu, oracle):
    """all kinds in one call; with every frame of both hand-tabled objects selected the expanded list holds 194
    entries and more, past the 128 inputs of the small-batch decode path"""
    raw, o8, o12, ed = tabled(gpu)
    raw5, e12, e8 = objects(gpu)[("R", 4 * B + 777)]
    raw2, _, _ = objects(gpu)[("Z", B + 1)]
    exact = oracle.zstd_compress_l1(raw2)
    n, n5 = len(raw), len(raw5)
    kinds = [
        ((o8, n, [(0, n)]), raw), ((o12, n, [(0, n)]), raw),
        ((e12, n5, [(0, 1), (n5 - 1, n5)]), raw5), ((e8, n5, [(B, B + 1), (3 * B, 3 * B + 1)]), raw5),
        ((exact, len(raw2), [(5, 6), (B - 10, B)]), raw2),
        ((e12, n5, [(5, 5)]), raw5), ((e8, n5, [(9, 3)]), raw5), ((o12, n - 1, [(0, 1)]), raw),
        ((e12, n5, [(2 * B - 1, 2 * B + 1)]), raw5),
    ]
    D.zstd_split_counts(reset=True)
    rets, img, do = check(gpu, [k[0] for k in kinds], [k[1] for k in kinds])
    assert D.zstd_split_counts() == (0, 0), "more than 128 entries take the one-wave path"
    assert rets == [n, n, n5, 3 * B + 1, B, 0, -1, -2, 2 * B + 1]
    for i, (item, r) in enumerate(kinds):
        alone, aimg, ado, _ = run_ranges(gpu, [item])
        assert alone == [rets[i]], i
        cap = item[1]
        if item[0] is exact:
            assert aimg[ado[0]:ado[0] + alone[0]].tobytes() == img[do[i]:do[i] + rets[i]].tobytes()
        else:
            assert aimg[ado[0]:ado[0] + cap].tobytes() == img[do[i]:do[i] + cap].tobytes(), i


def test_verdicts(gpu):
    contents, obj, t, ent = hand_built(True)
    _, obj8, t8, _ = hand_built(False)
    raw = b"".join(contents)
    n, body = len(raw), obj[:len(obj) - len(t)]
    c0 = [sum(e[0] for e in ent[:k]) for k in range(len(ent) + 1)]
    d0 = [sum(e[1] for e in ent[:k]) for k in range(len(ent) + 1)]
    badsum = bytearray(t)
    badsum[8 + 12 * 2 + 8] ^= 0x10  # frame 2's checksum, one bit
    badsum = body + bytes(badsum)
    flip = bytearray(body)
    flip[c0[3] + 12 + 2000] ^= 0x04  # one bit of frame 3's literals: a raw block, so the frame still returns its size
    flip12, flip8 = bytes(flip) + t, bytes(flip) + t8
    broke = bytearray(badsum)
    broke[c0[3] + 5] ^= 0x5A  # frame 3's content size: it fails to decode; frame 2's checksum is still flipped
    broke = bytes(broke)
    ends = [(0, 1), (n - 1, n)]
    items = [
        (badsum, n, [(d0[2], d0[2] + 1)]),            # 0: the flipped checksum's frame is selected: -4
        (badsum, n, [(0, 1), (d0[2], d0[3]), (n - 1, n)]),  # 1: among others: -4
        (badsum, n, ends),                            # 2: the same flip in an unselected frame: success
        (flip12, n, [(d0[3] + 5, d0[3] + 6)]),        # 3: a flipped literal bit in a selected frame, 12-byte table
        (flip8, n, [(d0[3] + 5, d0[3] + 6)]),         # 4: the same under an 8-byte table goes unseen
        (flip12, n, ends),                            # 5: and in an unselected frame
        (broke, n, [(0, n)]),                         # 6: a truncated frame and a checksum flip elsewhere: -1
        (broke, n, [(d0[3], d0[3] + 1)]),             # 7: -1
        (broke, n, [(0, 1)]),                         # 8: neither selected
        (obj, n - 1, ends),                           # 9: D > dst_cap: -2
        (obj8, n - 1, ends),                          # 10
        (obj, n, [(5, 4)]),                           # 11: hi < lo
        (obj, n, [(10, 20), (0, 5)]),                 # 12: out of order
        (obj8, n, [(0, 10), (9, 20)]),                # 13: overlapping
        (obj8, n, [(0, 1), (3, 2), (4, 5)]),          # 14
        (obj, n + 100, [(d0[4], n + 50)]),            # 15: hi > D under a larger capacity
    ]
    rets, img, do, counts = run_ranges(gpu, items)
    assert rets[:3] == [-4, -4, n]
    assert rets[3] < 0 and rets[3] == -4 and rets[4] == d0[3] + 6 and rets[5] == n
    assert rets[6:9] == [-1, -1, 1]
    assert rets[9:11] == [-2, -2] and rets[11:15] == [-1] * 4 and rets[15] == n
    damaged = raw[:d0[3] + 2000] + bytes([raw[d0[3] + 2000] ^ 0x04]) + raw[d0[3] + 2001:]
    first_last = lambda i: [(i, 0, contents[0]), (i, d0[4], contents[4])]
    writes = ([(0, d0[2], contents[2]), (1, 0, contents[0]), (1, d0[2], contents[2]), (1, d0[4], contents[4])] + first_last(2) +
              [(3, d0[3], damaged[d0[3]:d0[4]]), (4, d0[3], damaged[d0[3]:d0[4]])] + first_last(5) +
              [(8, 0, contents[0]), (15, d0[4], contents[4])])
    # whatever a failed frame wrote stayed inside the selected frames' spans
    writes += [(6, 0, img[do[6]:do[6] + n].tobytes()), (7, d0[3], img[do[7] + d0[3]:do[7] + d0[4]].tobytes())]
    check_image(img, do, writes)  # the bad lists, -2 and every unselected frame: nothing written
    assert counts[0] == 10 and counts[1] == 1 + 3 + 2 + 1 + 1 + 2 + 5 + 1 + 1 + 1
    # the running sums: a negative start, an end in front of its start; their neighbours are not harmed
    rets, img, do, counts = run_ranges(gpu, [(obj, n, None), (obj, n, None), (obj, n, None), (obj8, n, None)],
                                       first=[0, 1, -1, 1, 2], flat=[0, 1, n - 1, n])
    assert rets == [1, -1, -1, n] and counts == (2, 2, 1)
    check_image(img, do, [(0, 0, contents[0]), (3, d0[4], contents[4])])
    # NULL and empty inputs answer before their lists are looked at: the full decoder's answers
    early = [(None, 100, [(0, 10)]), (b"", 100, [(0, 10)]), (obj, 0, [(0, 10)])]
    want, wimg, _ = run_one_range(gpu, early)
    rets, img, do, counts = run_ranges(gpu, early, first=[0, -5, -9, -20], flat=[5, 4])
    assert rets == want and counts == (0, 0, 0) and (img == wimg).all() and (img == CANARY).all()
