"""GPU: the LZ4 ranges decode by origin chase (lz4_chase.hip, reached through
jfs_lz4_decompress_ranges_device and, with JFS_READ_LZ4_CHASE on, through the
read calls) against the CPU oracle's full decode.  dst is pre-filled with a
poison byte, so a byte written outside the live ranges of a chased block, or
anything written for a bad list, fails the test; the diagnostic counters say
which blocks the chase resolved itself and which it handed to the prefix path."""
import random

import numpy as np
import pytest
import torch

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests import lz4_chase_cases as K
from tests.split_streams import chain_stream
from tests.test_read_gpu import Dst, _codes, _plan

pytestmark = pytest.mark.gpu

POISON = 0xEE
GUARD = 64


def run_ranges(dev, comps, caps, lists, host_lens=None, host_caps=None):
    """jfs_lz4_decompress_ranges_device over one batch -> (rets, [dst image with
    GUARD bytes on either side]).  lists: per block [(lo, hi)]."""
    so, off = [], 0
    for c in comps:
        so.append(off)
        off = (off + len(c) + 64 + 15) & ~15
    host = np.zeros(off + 64, dtype=np.uint8)
    for c, o in zip(comps, so):
        host[o:o + len(c)] = np.frombuffer(c, dtype=np.uint8)
    do, doff = [], GUARD
    for i, c in enumerate(caps):
        do.append(doff + (i % 4))  # (some dst not 4-aligned: the byte stores)
        doff = (doff + (i % 4) + c + 2 * GUARD + 15) & ~15
    src_t = torch.from_numpy(host).to(dev)
    dst_t = torch.full((doff + GUARD,), POISON, dtype=torch.uint8, device=dev)
    desc = D.make_desc(src_t, so, [len(c) for c in comps], dst_t, do, caps)
    first, flat = [0], []
    for ls in lists:
        flat += [v for r in ls for v in r]
        first.append(len(flat) // 2)
    rf = torch.tensor(first, dtype=torch.int32, device=dev)
    rg = torch.tensor(flat if flat else [0, 0], dtype=torch.int32, device=dev)
    ret = torch.full((len(comps),), 12345, dtype=torch.int32, device=dev)
    D.lz4_decompress_ranges(desc, rf, rg, ret, host_lens or [len(c) for c in comps], host_caps or caps)
    torch.cuda.synchronize()
    dh = dst_t.cpu().numpy()
    return ret.cpu().tolist(), [dh[o - GUARD:o + c + GUARD] for o, c in zip(do, caps)]


def live(ls, cap):
    return [(max(lo, 0), min(hi, cap)) for lo, hi in ls if min(hi, cap) > max(lo, 0)]


def check_chased(img, cap, ls, full, total):
    """bytes of the live ranges below total equal the full decode's; everything else is still poison"""
    want = np.full(cap + 2 * GUARD, POISON, dtype=np.uint8)
    for lo, hi in live(ls, cap):
        hi = min(hi, total)
        if hi > lo:
            want[GUARD + lo:GUARD + hi] = np.frombuffer(full[lo:hi], dtype=np.uint8)
    bad = np.nonzero(want != img)[0]
    assert bad.size == 0, f"first wrong byte at {bad[0] - GUARD} ({bad.size} wrong)"


def overlap_start(comp):
    """an output position in the middle of the first overlapped match, or None"""
    op = 0
    for ll, _, ml, off in K.sequences(comp):
        op += ll
        if ml > off > 0:
            return op + ml // 2
        op += ml
    return None


def range_lists(comp, total):
    mid = overlap_start(comp)
    out = [[(0, 1)], [(total - 1, total)], [(0, total)], [(0, total + 100)], [(total - 3, total + 40)],
           [(total + 5, total + 9)]]
    if total > 65536:
        out.append([(65536 - 37, 65536 + 41)])
    if mid is not None:
        out.append([(mid, min(mid + 9, total))])
    if total >= 100:  # three disjoint ranges with empty ones between them
        a, b, c = total // 7, total // 2, total - total // 9
        out.append([(0, 0), (a, a + 5), (b, b), (b, min(b + 1031, c)), (c, c), (c, total), (total, total)])
    return out


@pytest.fixture(scope="module")
def blocks(oracle):
    """[(name, compressed, source)] from both encoders: sizes at the edges the
    issue names, text / zeros / incompressible"""
    out = []
    def add(name, src):
        out.append((f"exact-{name}", oracle.lz4_compress(src)[1], src))
        out.append((f"fast-{name}", C.lz4_fast_host(src), src))
    for cls in "TZR":
        for n in (1, 13, 65535, 65537):
            add(f"{cls}-{n}", gen_block(cls, 3100 + n, n))
    add("T-1M", gen_block("T", 3200, 1 << 20))
    add("Z-1M", gen_block("Z", 0, 1 << 20))
    add("R-256K", gen_block("R", 3201, 256 << 10))
    # compressed sizes 255, 256, 257: one segment, exactly one, one byte of a second
    text, tail = gen_block("T", 3300, 2000), gen_block("R", 5, 40)
    for want in (255, 256, 257):
        src = next(text[:n] + tail[:k] for n in range(200, 600) for k in range(0, 40)
                   if len(oracle.lz4_compress(text[:n] + tail[:k])[1]) == want)
        out.append((f"exact-seg-{want}", oracle.lz4_compress(src)[1], src))
    return out


def test_ranges_match_the_full_decode_and_write_nothing_else(gpu, blocks):
    sizes = {len(c) for _, c, _ in blocks}
    assert {255, 256, 257} & sizes, sorted(sizes)[:20]
    comps, caps, lists, meta = [], [], [], []
    for name, comp, src in blocks:
        for ls in range_lists(comp, len(src)):
            for cap in (len(src), len(src) + 77):
                comps.append(comp)
                caps.append(cap)
                lists.append(ls)
                meta.append((name, src))
    D.lz4_chase_counts(reset=True)
    rets, imgs = [], []
    for g in range(0, len(comps), 100):
        r, im = run_ranges(gpu, comps[g:g + 100], caps[g:g + 100], lists[g:g + 100])
        rets += r
        imgs += im
    answered = 0
    for (name, src), cap, ls, r, img in zip(meta, caps, lists, rets, imgs):
        lv = live(ls, cap)
        h = max((hi for _, hi in lv), default=0)
        assert r == (min(len(src), h) if lv else 0), (name, ls, cap, r)
        check_chased(img, cap, ls if lv else [], src, len(src))
        answered += not lv
    chased, nbytes, hops, handed = D.lz4_chase_counts()
    assert handed == 0 and chased == len(comps) - answered, (chased, handed, answered)
    assert nbytes > 0 and hops > 0


def test_bad_lists_answer_minus_one_and_write_nothing(gpu, oracle):
    src = gen_block("T", 3400, 5000)
    comp = oracle.lz4_compress(src)[1]
    lists = [[(10, 5)], [(100, 200), (150, 300)], [(100, 200), (50, 60)], [(0, 10), (10, 10), (5, 30)], [(0, 10), (10, 20)]]
    D.lz4_chase_counts(reset=True)
    rets, imgs = run_ranges(gpu, [comp] * 5, [5000] * 5, lists)
    assert rets == [-1, -1, -1, -1, 20]
    for img in imgs[:4]:
        assert (img == POISON).all()
    check_chased(imgs[4], 5000, lists[4], src, 5000)
    # broken running sums: a negative first, a descending pair
    so = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).to(gpu)
    dst = torch.full((3, 5000), POISON, dtype=torch.uint8, device=gpu)
    desc = D.make_desc(so, [0, 0, 0], [len(comp)] * 3, dst.view(-1), [0, 5000, 10000], [5000] * 3)
    rf = torch.tensor([-1, 1, 0, 1], dtype=torch.int32, device=gpu)
    rg = torch.tensor([0, 10], dtype=torch.int32, device=gpu)
    ret = torch.full((3,), 7, dtype=torch.int32, device=gpu)
    D.lz4_decompress_ranges(desc, rf, rg, ret, [len(comp)] * 3, [5000] * 3)
    torch.cuda.synchronize()
    assert ret.cpu().tolist() == [-1, -1, 10]
    assert (dst[:2].cpu().numpy() == POISON).all()
    assert D.lz4_chase_counts()[3] == 0


def test_early_answers_are_the_full_decoders(gpu, oracle):
    """src_len == 0 and dst_cap == 0 answer what jfs_lz4_decompress_device answers, in front of a bad list."""
    comp = oracle.lz4_compress(gen_block("T", 3401, 300))[1]
    so = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).to(gpu)
    dst = torch.full((2, 300), POISON, dtype=torch.uint8, device=gpu)
    desc = D.make_desc(so, [0, 0], [0, len(comp)], dst.view(-1), [0, 300], [300, 0])
    want = torch.full((2,), 7, dtype=torch.int32, device=gpu)
    D.lz4_decompress(desc, want)
    rf = torch.tensor([0, 1, 2], dtype=torch.int32, device=gpu)
    rg = torch.tensor([10, 5, 0, 10], dtype=torch.int32, device=gpu)
    ret = torch.full((2,), 7, dtype=torch.int32, device=gpu)
    D.lz4_decompress_ranges(desc, rf, rg, ret, [0, len(comp)], [300, 0])
    torch.cuda.synchronize()
    assert ret.cpu().tolist() == want.cpu().tolist()
    assert (dst.cpu().numpy() == POISON).all()


def test_deep_chain_is_handed_to_the_prefix_decode(gpu, oracle):
    comp = chain_stream(K.CHASE_HOPS + 200)
    total, full = oracle.lz4_decompress(comp, 1 << 20)
    assert total > 0
    lists = [[(total - 40, total - 20)], [(100, 200)], [(0, total)]]
    D.lz4_chase_counts(reset=True)
    rets, imgs = run_ranges(gpu, [comp] * 3, [total] * 3, lists)
    counts = D.lz4_chase_counts()
    # the middle block's chains are shallow: chased; the others meet a chain deeper than the cap
    assert counts[0] == 1 and counts[3] == 2, counts
    check_chased(imgs[1], total, lists[1], full, total)
    assert rets[1] == 200
    # the handed-over blocks: ret and bytes of the small-batch prefix call with want = H
    for i in (0, 2):
        h = lists[i][-1][1]
        so = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).to(gpu)
        dst = torch.full((total,), POISON, dtype=torch.uint8, device=gpu)
        desc = D.make_desc(so, [0], [len(comp)], dst, [0], [total])
        ret = torch.zeros(1, dtype=torch.int32, device=gpu)
        D.lz4_decompress_prefix_small(desc, torch.tensor([h], dtype=torch.int32, device=gpu), ret, [len(comp)], [total])
        torch.cuda.synchronize()
        r = int(ret[0].item())
        assert rets[i] == r == h
        assert imgs[i][GUARD:GUARD + r].tobytes() == dst[:r].cpu().numpy().tobytes() == full[:r]
        assert (imgs[i][:GUARD] == POISON).all() and (imgs[i][GUARD + total:] == POISON).all()


def test_acceptance_corpus_slice(gpu, golden, oracle):
    """300 cases of the liblz4 acceptance corpus, range [0, cap): the oracle's
    value, or -- where the oracle rejects -- a value within the documented
    latitude (the negative value, or min(total, H) <= cap); nothing outside
    dst[0, cap) changes."""
    cases = golden["lz4"]["decode_corpus"][::10][:300]
    assert len(cases) == 300
    comps = [bytes.fromhex(e["src"]) for e in cases]
    caps = [max(e["cap"], 0) for e in cases]
    keep = [i for i, c in enumerate(comps) if len(c) > 0]
    rets, imgs = run_ranges(gpu, [comps[i] for i in keep], [caps[i] for i in keep], [[(0, caps[i])] for i in keep])
    seen_reject = 0
    for i, r, img in zip(keep, rets, imgs):
        e, cap = cases[i], caps[i]
        assert (img[:GUARD] == POISON).all() and (img[GUARD + cap:] == POISON).all(), i
        if cap == 0 or e["ret"] >= 0:
            assert r == e["ret"], (i, r, e["ret"])
            if r > 0:
                n, full = oracle.lz4_decompress(comps[i], cap)
                assert img[GUARD:GUARD + r].tobytes() == full[:r]
        else:
            seen_reject += 1
            assert r == e["ret"] or 0 <= r <= cap, (i, r, e["ret"])
    assert seen_reject > 0


def test_batch_above_the_small_batch_limit(gpu, oracle):
    """200 blocks of 64 KiB in one call: more than JFS_LZ4_SPLIT_MAX (128), which the chase does not depend on."""
    srcs = [gen_block("T", 3500 + i, 65536) for i in range(200)]
    comps = [oracle.lz4_compress(s)[1] for s in srcs]
    lists = [[(i * 300, i * 300 + 1000 + i)] for i in range(200)]
    D.lz4_chase_counts(reset=True)
    rets, imgs = run_ranges(gpu, comps, [65536] * 200, lists)
    assert rets == [ls[0][1] for ls in lists]
    for img, ls, s in zip(imgs, lists, srcs):
        check_chased(img, 65536, ls, s, 65536)
    counts = D.lz4_chase_counts()
    assert counts[0] == 200 and counts[3] == 0, counts


def test_sizes_beyond_the_host_budget_are_handed_over(gpu, oracle):
    src = gen_block("T", 3600, 70000)
    comp = oracle.lz4_compress(src)[1]
    D.lz4_chase_counts(reset=True)
    rets, imgs = run_ranges(gpu, [comp], [70000], [[(500, 900)]], host_lens=[64], host_caps=[1000])
    assert rets == [900] and imgs[0][GUARD:GUARD + 900].tobytes() == src[:900]
    assert D.lz4_chase_counts()[3] == 1


# ------------------------------------------------------------------ the read calls
NSRC, BLOCK = 8, 256 << 10


@pytest.fixture(scope="module")
def read_case(oracle):
    raws = [gen_block("T", 3700 + i, BLOCK) for i in range(NSRC)]
    stored = [oracle.lz4_compress(r)[1] for r in raws]
    rng = random.Random(17)
    parts = []
    for j in range(12):  # fragmented reads: a few pieces of several sources and a hole each
        ps = []
        for _ in range(rng.randrange(1, 5)):
            s = rng.randrange(-1, NSRC - 1)  # (the last source is left to the large read)
            ln = rng.randrange(1, 3000)
            ps.append((s, rng.randrange(0, BLOCK - ln) if s >= 0 else 0, ln))
        parts.append(ps)
    parts.append([(NSRC - 1, 1000, 200000)])  # one source asked for more than the threshold
    return raws, stored, parts


def _modes(decode, chase, cmax):
    return C.set_read_decode_mode(decode), C.set_read_lz4_chase_mode(chase), C.set_lz4_chase_max(cmax)


def _read(stored, parts, sealed=None):
    totals = [sum(p[2] for p in ps) for ps in parts]
    dst = Dst([t + (j % 2) for j, t in enumerate(totals)])
    src = list(zip(stored, [BLOCK] * len(stored)))
    wanted = [j == 1 for j in range(len(parts))]  # with_csum on one read
    if sealed is None:
        res = C.NewCompressor("lz4").ReadBatch(src, dst.views, _plan(parts), with_csum=wanted)
    else:
        res = E.read_open_batch(L.ALGO_LZ4, sealed[0], src, sealed[1], dst.views, _plan(parts), with_csum=wanted)
    return dst, res


@pytest.mark.parametrize("sealed", [False, True], ids=["read_batch", "read_open_batch-chacha20"])
def test_read_calls_mode_on_equals_mode_off(gpu, oracle, read_case, sealed):
    raws, stored, parts = read_case
    key = None
    if sealed:
        rng = random.Random(5)
        rb = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
        algo = E.CHACHA20_RSA
        params = [(rb(E.key_size(algo)), rb(12), rb(7 + i)) for i in range(NSRC)]
        pairs = [(bytearray(E.envelope_bound(L.ALGO_LZ4, len(r), len(p[2]))), r) for r, p in zip(raws, params)]
        res = E.compress_seal_batch(L.ALGO_LZ4, algo, pairs, params)
        assert all(e is None for _, e in res)
        stored = [bytes(buf[:n]) for (buf, _), (n, _) in zip(pairs, res)]
        key = (algo, [p[0] for p in params])
    want = C.read_expect(raws, _plan(parts))
    prev = _modes("prefix", "off", 0)
    try:
        dst0, res0 = _read(stored, parts, key)
        D.lz4_chase_counts(reset=True)
        assert D.lz4_chase_counts()[:2] == (0, 0)
        _modes("prefix", "on", 64 << 10)
        dst1, res1 = _read(stored, parts, key)
        counts = D.lz4_chase_counts()
        _modes("full", "on", 64 << 10)
        dst2, res2 = _read(stored, parts, key)
        _modes("full", "off", 0)
        dst3, res3 = _read(stored, parts, key)
    finally:
        _modes(*prev)
    # prefix mode: everything identical -- source and read results, checksums of the sources and of the reads
    assert _codes(res1[0]) == _codes(res0[0]) and _codes(res1[1]) == _codes(res0[1])
    assert list(res1[2]) == list(res0[2]) and res1[3] == res0[3]
    # full mode: the reads, their checksums and statuses; a chased source reports min(size, need) like prefix mode
    # (a source that was not chased is decoded whole, as with the switch off)
    touched = {p[0] for ps in parts[:-1] for p in ps if p[0] >= 0}
    assert _codes(res2[1]) == _codes(res3[1]) and res2[3] == res3[3] and list(res2[2]) == list(res3[2])
    assert _codes(res2[0]) == [_codes(res1[0])[i] if i in touched else _codes(res3[0])[i] for i in range(NSRC)]
    for j, w in enumerate(want):
        assert res0[1][j] == (len(w), None)
        for d in (dst0, dst1, dst2, dst3):
            d.check(j, w)
    assert res1[3][1] == oracle.crc32c_segments(want[1])
    # the seven fragmented sources were chased (those any read touches), the large one was not
    touched = {p[0] for ps in parts[:-1] for p in ps if p[0] >= 0}
    assert counts[0] == len(touched) and counts[3] == 0, counts
    assert 0 < counts[1] <= sum(p[2] for ps in parts[:-1] for p in ps) and counts[2] > 0
