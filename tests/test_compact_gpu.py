"""GPU: on-device compaction -- the gather kernel against numpy, the fused LZ4
decode -> gather -> encode chain against the CPU oracle, and jfs_compact_batch
(CompactBatch) against DecompressBatch + a host gather + CompressBatch.

Every gathered block sits at an odd offset inside a larger tensor pre-filled
with a canary; the whole tensor is compared with its expected image, so a
single byte written outside dst[0, total) fails the test."""
import numpy as np
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd.blockgen import gen_block

pytestmark = pytest.mark.gpu

CANARY = 0xA5
INT32_MIN = -(1 << 31)
LENGTHS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4097]


def _sources(lens, seed=11):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]


def _expected(sources, segs):
    out = np.zeros(sum(s[3] for s in segs), dtype=np.uint8)
    for src, src_off, dst_off, n in segs:
        if src >= 0:
            out[dst_off:dst_off + n] = sources[src][src_off:src_off + n]
    return out


def _tile(parts):
    """[(src, src_off, len)] -> [(src, src_off, dst_off, len)]"""
    segs, at = [], 0
    for src, src_off, n in parts:
        segs.append((src, src_off, at, n))
        at += n
    return segs


def run_gather(gpu, sources, blocks, src_n=None):
    """blocks: [(segs, dst_cap)].  Places every source at its own alignment and
    every dst at an odd offset (cycling through 1, 3, .. 15 mod 16) of a
    canary-filled tensor; returns (ret list, tensor image, [dst offsets])."""
    import torch
    from juicefs_amd import device as D
    soffs, o = [], 0
    for i, s in enumerate(sources):
        o = (o + 15) // 16 * 16 + (i * 5) % 16  # sources at mixed alignments too
        soffs.append(o)
        o += len(s)
    simg = np.zeros(o + 16, dtype=np.uint8)
    for s, so in zip(sources, soffs):
        simg[so:so + len(s)] = s
    sbuf = torch.from_numpy(simg).to(gpu)
    doffs, o = [], 64
    for j, (segs, cap) in enumerate(blocks):
        o = (o + 15) // 16 * 16 + (2 * j + 1) % 16
        doffs.append(o)
        o += max(cap, sum(s[3] for s in segs)) + 80
    dbuf = torch.full((o + 64,), CANARY, dtype=torch.uint8, device=gpu)
    lens = [len(s) for s in sources]
    sdesc = D.make_desc(sbuf, soffs, lens, sbuf, soffs, lens)
    n_t = torch.tensor(lens if src_n is None else src_n, dtype=torch.int32, device=gpu)
    seg_first, seg = [0], []
    for segs, _ in blocks:
        seg += segs
        seg_first.append(len(seg))
    odesc, sdev = D.make_compact_desc(dbuf, doffs, [c for _, c in blocks], seg_first, seg)
    ret = torch.full((len(blocks),), 12345, dtype=torch.int32, device=gpu)
    D.gather(sdesc, n_t, odesc, sdev, max(c for _, c in blocks), ret)
    torch.cuda.synchronize()
    return ret.cpu().tolist(), dbuf.cpu().numpy(), doffs


def check_exact(sources, blocks, ret, img, doffs, verdicts=None):
    want = np.full(len(img), CANARY, dtype=np.uint8)
    for j, (segs, cap) in enumerate(blocks):
        total = sum(s[3] for s in segs)
        v = total if verdicts is None else verdicts[j]
        assert ret[j] == v, (j, ret[j], v)
        if v >= 0:
            want[doffs[j]:doffs[j] + total] = _expected(sources, segs)
        elif v == INT32_MIN:  # may hold anything inside dst[0, total), nothing outside
            want[doffs[j]:doffs[j] + total] = img[doffs[j]:doffs[j] + total]
    bad = np.nonzero(want != img)[0]
    assert bad.size == 0, f"first wrong byte at {bad[0]} (of {bad.size}); dst offsets {doffs[:4]}..."


def test_gather_every_length_and_alignment(gpu):
    """One launch: every length x src_off % 16 x dst_off % 16; fillers (holes
    and source bytes in turn) set the destination alignment, so segments meet
    holes and other segments at every boundary position."""
    sources = _sources([70000, 70000])
    blocks, seen = [], set()
    for so in range(16):
        parts, at, k = [], 0, 0
        for da in range(16):
            for q in range(len(LENGTHS)):
                n = LENGTHS[(q + da) % len(LENGTHS)]  # rotate the order per alignment
                f = (da - at) % 16
                if f:
                    parts.append((-1, 0, f) if k % 2 else (1, 16 * (k % 4000) + 3, f))
                    at += f
                parts.append((k % 2, 16 * ((k * 37) % 4000) + so, n))
                seen.add((n, so, at % 16))
                at += n
                k += 1
        segs = _tile(parts)
        blocks.append((segs, at + (so % 3)))  # capacity: exact or a little more
    assert len(seen) == len(LENGTHS) * 16 * 16
    ret, img, doffs = run_gather(gpu, sources, blocks)
    check_exact(sources, blocks, ret, img, doffs)


def test_gather_many_one_byte_segments(gpu):
    sources = _sources([9000, 9000], seed=12)
    parts = [((k % 3) - 1, (k * 7) % 9000, 1) for k in range(5000)]  # hole, source 0, source 1, ...
    blocks = [(_tile(parts), 5000)]
    ret, img, doffs = run_gather(gpu, sources, blocks)
    check_exact(sources, blocks, ret, img, doffs)


def test_gather_one_large_segment(gpu):
    n = (1 << 20) + 3
    sources = _sources([n + 8], seed=13)
    blocks = [([(0, 5, 0, n)], n)]
    ret, img, doffs = run_gather(gpu, sources, blocks)
    check_exact(sources, blocks, ret, img, doffs)


def test_gather_small_and_threshold_totals(gpu):
    sources = _sources([70000, 70000], seed=14)
    blocks = []
    for t in (0, 1, 12, 13, 65546, 65547):
        parts = []
        if t:
            a = t // 3
            parts = [p for p in [(0, 9, a), (-1, 0, t // 5), (1, 1234, t - a - t // 5)] if p[2] > 0]
        blocks.append((_tile(parts), t))
    ret, img, doffs = run_gather(gpu, sources, blocks)
    check_exact(sources, blocks, ret, img, doffs)
    assert ret == [0, 1, 12, 13, 65546, 65547]


def test_gather_verdicts_per_block(gpu):
    """One launch, one failure per block, good blocks in between."""
    sources = _sources([5000, 5000, 5000], seed=15)
    src_n = [5000, -7, 4000]  # source 1 failed; source 2 decoded 4000 bytes
    good = _tile([(0, 3, 700), (-1, 0, 50), (2, 100, 3900)])  # ends exactly at source 2's 4000 bytes
    blocks = [
        (good, 4650),
        (_tile([(0, 0, 100), (1, 0, 100)]), 200),               # reads a failed source
        (good, 4660),
        (_tile([(0, 0, 10), (2, 100, 3901)]), 3911),            # one byte past source 2's length
        (_tile([(0, 0, 10), (3, 0, 10)]), 20),                  # src == nsrc
        ([(0, 0, 0, 10), (0, 10, 11, 10)], 64),                 # broken tiling
        (_tile([(0, 0, 33), (-1, 0, 32)]), 64),                 # total == dst_cap + 1
        (good, 4650),
    ]
    verdicts = [4650, INT32_MIN, 4650, INT32_MIN, -1, -1, -1, 4650]
    ret, img, doffs = run_gather(gpu, sources, blocks, src_n=src_n)
    check_exact(sources, blocks, ret, img, doffs, verdicts)


# ---- fused chains -----------------------------------------------------------

SRC_LENS = [70000, 96001, 131072, 150003, 180000, 200000]
TOTALS = [50000, 65546, 150001, 300000]  # below and above LZ4's 65,547-byte table switch


def _plan(src_lens, totals, groups, seed):
    """Random segments (fixed seed): output j draws from the sources in
    groups[j] (the last ones first, as far as the total allows) and from holes."""
    rng = np.random.default_rng(seed)
    seg_first, seg = [0], []
    for total, grp in zip(totals, groups):
        at, must = 0, list(grp)
        while at < total:
            n = int(min(total - at, rng.integers(1, 40000)))
            src = must.pop() if must else int(rng.choice(list(grp) + [-1]))
            if src >= 0:
                n = min(n, src_lens[src])
                off = int(rng.integers(0, src_lens[src] - n + 1))
            else:
                off = 0
            seg.append((src, off, at, n))
            at += n
        seg_first.append(len(seg))
    return seg_first, seg


def _fed_by(seg_first, seg, src):
    """Outputs with a segment that reads source `src`."""
    return {j for j in range(len(seg_first) - 1) if any(s[0] == src for s in seg[seg_first[j]:seg_first[j + 1]])}


def _host_gather(raws, seg_first, seg):
    return [_expected(raws, seg[seg_first[j]:seg_first[j + 1]]).tobytes() for j in range(len(seg_first) - 1)]


@pytest.fixture(scope="module")
def raws():
    return [np.frombuffer(gen_block("T", 900 + i, n), dtype=np.uint8) for i, n in enumerate(SRC_LENS)]


def test_lz4_compact_device_matches_oracle(gpu, oracle, raws):
    import torch
    from juicefs_amd import device as D
    groups = [(0, 1, 2, 3, 4), (0, 1, 2, 3, 4), (0, 2, 5), (1, 3, 4, 5)]  # source 5 feeds outputs 2 and 3 only
    seg_first, seg = _plan(SRC_LENS, TOTALS, groups, seed=21)
    assert _fed_by(seg_first, seg, 5) == {2, 3}
    want = [oracle.lz4_compress(b)[1] for b in _host_gather(raws, seg_first, seg)]
    comps = [oracle.lz4_compress(r.tobytes())[1] for r in raws]
    a16 = lambda n: (n + 15) // 16 * 16
    coffs = np.cumsum([0] + [a16(len(c)) for c in comps])
    doffs = np.cumsum([0] + [a16(n) for n in SRC_LENS])
    goffs = np.cumsum([0] + [a16(t) for t in TOTALS])
    bounds = [oracle.lz4_bound(t) for t in TOTALS]
    eoffs = np.cumsum([0] + [a16(b) for b in bounds])
    cimg = np.zeros(coffs[-1], dtype=np.uint8)
    for c, o in zip(comps, coffs):
        cimg[o:o + len(c)] = np.frombuffer(c, dtype=np.uint8)
    for truncated in (False, True):
        clens = [len(c) for c in comps]
        if truncated:
            clens[5] -= 10  # source 5's stream ends inside its last literals
        comp = torch.from_numpy(cimg).to(gpu)
        dec = torch.zeros(int(doffs[-1]), dtype=torch.uint8, device=gpu)
        gat = torch.zeros(int(goffs[-1]), dtype=torch.uint8, device=gpu)
        enc = torch.zeros(int(eoffs[-1]), dtype=torch.uint8, device=gpu)
        sdesc = D.make_desc(comp, coffs[:-1], clens, dec, doffs[:-1], SRC_LENS)
        gdesc, sdev = D.make_compact_desc(gat, goffs[:-1], TOTALS, seg_first, seg)
        edesc = D.make_desc(gat, goffs[:-1], TOTALS, enc, eoffs[:-1], bounds)
        src_ret = torch.full((6,), 777, dtype=torch.int32, device=gpu)
        ret = torch.full((4,), 777, dtype=torch.int32, device=gpu)
        D.lz4_compact(sdesc, src_ret, gdesc, sdev, edesc, max(TOTALS), ret)
        torch.cuda.synchronize()
        sr, r, img = src_ret.cpu().tolist(), ret.cpu().tolist(), enc.cpu().numpy()
        assert sr[:5] == SRC_LENS[:5]
        assert (sr[5] < 0) if truncated else (sr[5] == SRC_LENS[5])
        for j in range(4):
            if truncated and j >= 2:
                assert r[j] == INT32_MIN, (j, r[j])
            else:
                assert r[j] == len(want[j]), (j, r[j], len(want[j]))
                assert img[eoffs[j]:eoffs[j] + r[j]].tobytes() == want[j], j


def _stat(lib, algo, d):
    s = (L.JfsOpStats * L.STATS_N)()
    lib.jfs_stats(s, L.STATS_N)
    return s[algo * 2 + d]


@pytest.mark.parametrize("name", ["lz4", "zstd", "none"])
def test_compact_batch_matches_parent_abi(gpu, lib, oracle, raws, name):
    """Two independent compactions in one plan (sources 0-2 -> outputs 0-1,
    sources 3-5 -> outputs 2-3) against DecompressBatch + host gather +
    CompressBatchChecksum."""
    import torch
    c = C.NewCompressor(name)
    groups = [(0, 1, 2), (0, 2), (3, 4, 5), (3, 5)]
    seg_first, seg = _plan(SRC_LENS, TOTALS, groups, seed=22)
    assert _fed_by(seg_first, seg, 4) == {2}
    blocks = _host_gather(raws, seg_first, seg)
    stored = []
    for r in raws:  # the stored objects, written by this library
        d = bytearray(c.CompressBound(len(r)))
        n, e = c.CompressBatch([(d, r)])[0]
        assert e is None
        stored.append(bytes(d[:n]))
    ref_dst = [bytearray(c.CompressBound(len(b))) for b in blocks]
    ref = c.CompressBatchChecksum(list(zip(ref_dst, blocks)))
    assert all(e is None for _, e, _ in ref)

    def compact(objs, caps, dst_caps):
        dst = [bytearray(n) for n in dst_caps]
        dev0 = torch.cuda.current_device()
        lib.jfs_stats_reset()
        sres, ores, crcs = c.CompactBatch(list(zip(objs, caps)), dst, (seg_first, seg), with_crc=True)
        assert torch.cuda.current_device() == dev0
        dec, enc = _stat(lib, c.algo, 1), _stat(lib, c.algo, 0)
        assert (dec.calls, dec.blocks, enc.calls, enc.blocks) == (1, 6, 1, 4)
        assert dec.errors == sum(e is not None for _, e in sres)
        assert enc.errors == sum(e is not None for _, e in ores)
        assert enc.bytes_out == sum(n for n, e in ores if e is None)
        return dst, sres, ores, crcs

    bound_caps = [c.CompressBound(len(b)) for b in blocks]
    # all good
    dst, sres, ores, crcs = compact(stored, SRC_LENS, bound_caps)
    back = c.DecompressBatch([(bytearray(n), s) for n, s in zip(SRC_LENS, stored)])
    assert [(n, e) for n, e in sres] == [(n, e) for n, e in back] == [(n, None) for n in SRC_LENS]
    for j in range(4):
        n, e, crc = ref[j]
        assert ores[j] == (n, None) and crcs[j] == crc, j
        assert bytes(dst[j][:n]) == bytes(ref_dst[j][:n]), j
        if name == "lz4":
            assert bytes(dst[j][:n]) == oracle.lz4_compress(blocks[j])[1]
        if name == "none":
            assert bytes(dst[j][:n]) == blocks[j]
    # a failed source fails only the blocks it feeds
    bad, caps = list(stored), list(SRC_LENS)
    if name == "none":
        caps[4] -= 1  # noOp.Decompress: "buffer too short"
    else:
        bad[4] = stored[4][:len(stored[4]) - 10]
    dst, sres, ores, crcs = compact(bad, caps, bound_caps)
    back = c.DecompressBatch([(bytearray(n), s) for n, s in zip(caps, bad)])
    assert [n for n, _ in sres] == [n for n, _ in back]
    assert [e.code if e else None for _, e in sres] == [e.code if e else None for _, e in back]
    assert sres[4][1] is not None
    for j in range(4):
        if j == 2:
            assert ores[j][1] is not None and ores[j][1].code == L.JFS_ERR_CORRUPT and crcs[j] == 0, j
        else:
            n, e, crc = ref[j]
            assert ores[j] == (n, None) and crcs[j] == crc and bytes(dst[j][:n]) == bytes(ref_dst[j][:n]), j
    # a dst one byte short: the block's own codec error, as CompressBatch reports it
    short = list(bound_caps)
    short[1] = (ref[1][0] if name == "lz4" else bound_caps[1]) - 1
    dst, sres, ores, crcs = compact(stored, SRC_LENS, short)
    alone = c.CompressBatch([(bytearray(short[1]), blocks[1])])[0]
    assert alone[1] is not None and ores[1][1] is not None and ores[1][1].code == alone[1].code
    for j in (0, 2, 3):
        n, e, crc = ref[j]
        assert ores[j] == (n, None) and crcs[j] == crc and bytes(dst[j][:n]) == bytes(ref_dst[j][:n]), j


def _codes(res):
    return [(n, e.code if e else None) for n, e in res]


@pytest.mark.parametrize("name", ["lz4", "zstd", "none"])
def test_degenerate_plans(gpu, lib, name):
    """Plans that leave one side of the chain, or all of it, without work."""
    c = C.NewCompressor(name)
    lens = [3000, 4097, 5001]
    small = [np.frombuffer(gen_block("T", 950 + i, n), dtype=np.uint8) for i, n in enumerate(lens)]
    stored = []
    for r in small:
        d = bytearray(c.CompressBound(len(r)))
        n, e = c.CompressBatch([(d, r)])[0]
        assert e is None
        stored.append(bytes(d[:n]))

    def reference(blocks):
        dst = [bytearray(c.CompressBound(len(b))) for b in blocks]
        res = c.CompressBatchChecksum(list(zip(dst, blocks)))
        assert all(e is None for _, e, _ in res)
        return [(bytes(d[:n]), crc) for d, (n, _, crc) in zip(dst, res)]

    def compact(objs, caps, plan, blocks):
        dst = [bytearray(c.CompressBound(len(b))) for b in blocks]
        back = c.DecompressBatch([(bytearray(n), s) for n, s in zip(caps, objs)]) if objs else []
        lib.jfs_stats_reset()
        sres, ores, crcs = c.CompactBatch(list(zip(objs, caps)), dst, plan, with_crc=True)
        assert _codes(sres) == _codes(back)
        return dst, sres, ores, crcs

    # sources and no outputs: the sources are still decoded
    _, sres, ores, crcs = compact(stored, lens, ([0], []), [])
    assert _codes(sres) == [(n, None) for n in lens] and ores == [] and crcs == []
    # no sources: an output made of holes, one without a segment, one of a single hole byte
    plan = ([0, 2, 2, 3], [(-1, 0, 0, 1000), (-1, 0, 1000, 37), (-1, 0, 0, 1)])
    blocks = [bytes(1037), b"", bytes(1)]
    ref = reference(blocks)
    dst, sres, ores, crcs = compact([], [], plan, blocks)
    assert sres == []
    for j, (want, crc) in enumerate(ref):
        assert ores[j] == (len(want), None) and crcs[j] == crc and bytes(dst[j][:len(want)]) == want, j
    # the same outputs beside sources that nothing reads, and one that reads them
    seg = plan[1] + [(2, 5000, 0, 1), (-1, 0, 1, 15), (0, 1, 16, 2999)]
    blocks.append(_expected(small, seg[3:]).tobytes())
    ref = reference(blocks)
    dst, sres, ores, crcs = compact(stored, lens, ([0, 2, 2, 3, 6], seg), blocks)
    assert _codes(sres) == [(n, None) for n in lens]
    for j, (want, crc) in enumerate(ref):
        assert ores[j] == (len(want), None) and crcs[j] == crc and bytes(dst[j][:len(want)]) == want, j
    # every source answered on the host: every output fails, and no device work is queued
    if name == "none":
        objs, caps = stored, [n - 1 for n in lens]  # noOp.Decompress: "buffer too short"
    else:
        objs, caps = [b""] * 3, lens  # "decompress an empty input"
    plan = ([0, 1, 3], [(0, 0, 0, 10), (1, 0, 0, 10), (2, 0, 10, 10)])
    dst, sres, ores, crcs = compact(objs, caps, plan, [bytes(10), bytes(20)])
    assert all(e is not None for _, e in sres)
    assert [e.code for _, e in ores] == [L.JFS_ERR_CORRUPT] * 2 and crcs == [0, 0]
    assert all(not any(d) for d in dst)
    dec, enc = _stat(lib, c.algo, 1), _stat(lib, c.algo, 0)
    assert (dec.calls, dec.blocks, dec.errors, dec.batches) == (1, 3, 3, 0)
    assert (enc.calls, enc.blocks, enc.errors, enc.batches) == (1, 2, 2, 0)
    # neither
    assert c.CompactBatch([], [], ([0], []), with_crc=True) == ([], [], [])
