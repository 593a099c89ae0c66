"""GPU: the LZ4 window decode (lz4_split.hip's WINDOW form, reached through
jfs_lz4_decompress_window_device_small and, with JFS_READ_LZ4_WINDOW on, through
the read calls) against the CPU oracle's full decode and the prefix calls.  dst
is pre-filled with a poison byte, so a byte written outside [floor, ret) of a
block the path decodes itself fails the test; the diagnostic counters say which
blocks were decoded from a chunk floor, which the probe sent to floor 0 and
which were handed to the exact kernel.

Blocks of 200,000 bytes -- three full 64 KiB chunks and a ragged one -- from the
fast encoder's host twin and from the oracle's exact encoder.
tests/test_lz4_window.py shows that the reference rule alone gives the counters
asserted here: no sequence of a fast block reaches below a chunk floor, and the
exact encoder's text blocks have sequences that do."""
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
from tests.test_read_gpu import Dst, _codes, _plan

pytestmark = pytest.mark.gpu

POISON = 0xEE
GUARD = 64
CHUNK = 65536
N = 200000


def floor_of(lo):
    return (max(lo, 0) // CHUNK) * CHUNK


def make_batch(dev, items):
    """items: [(stream or None for a NULL src, src_len or None for len(stream), dst_cap)] -> (desc, dst tensor, dst
    offsets).  Equal stream objects are staged once; some dst are not 4-aligned (the byte stores)."""
    place, off = {}, 0
    for s, _, _ in items:
        if s is not None and id(s) not in place:
            place[id(s)] = off
            off = (off + len(s) + 64 + 15) & ~15
    host = np.zeros(off + 64, dtype=np.uint8)
    for s, _, _ in items:
        if s is not None:
            host[place[id(s)]:place[id(s)] + len(s)] = np.frombuffer(s, dtype=np.uint8)
    do, doff = [], GUARD
    for i, (_, _, cap) in enumerate(items):
        do.append(doff + (i % 4))
        doff = (doff + (i % 4) + cap + 2 * GUARD + 15) & ~15
    src_t = torch.from_numpy(host).to(dev)
    dst_t = torch.full((doff + GUARD,), POISON, dtype=torch.uint8, device=dev)
    a = np.zeros(len(items), dtype=D.DESC_DTYPE)
    for i, (s, n, cap) in enumerate(items):
        a["src"][i] = 0 if s is None else src_t.data_ptr() + place[id(s)]
        a["dst"][i] = dst_t.data_ptr() + do[i]
        a["src_len"][i] = len(s) if n is None else n
        a["dst_cap"][i] = cap
    desc = torch.from_numpy(a.view(np.uint8).copy()).to(dev)
    desc._keep = src_t
    return desc, dst_t, do


def images(dst_t, do, items):
    dh = dst_t.cpu().numpy()
    return [dh[o - GUARD:o + cap + GUARD] for o, (_, _, cap) in zip(do, items)]


def run_window(dev, items, wins, host_lens=None, host_caps=None):
    """jfs_lz4_decompress_window_device_small over one batch -> (rets, [dst image with GUARD bytes on either side])"""
    desc, dst_t, do = make_batch(dev, items)
    lo = torch.tensor([w[0] for w in wins], dtype=torch.int32, device=dev)
    hi = torch.tensor([w[1] for w in wins], dtype=torch.int32, device=dev)
    ret = torch.full((len(items),), 12345, dtype=torch.int32, device=dev)
    lens = host_lens or [a if a is not None else len(s) for s, a, _ in items]
    D.lz4_decompress_window(desc, lo, hi, ret, lens, host_caps or [c for _, _, c in items])
    torch.cuda.synchronize()
    return ret.cpu().tolist(), images(dst_t, do, items)


def run_prefix(dev, items, wants, small):
    desc, dst_t, do = make_batch(dev, items)
    want = torch.tensor(wants, dtype=torch.int32, device=dev)
    ret = torch.full((len(items),), 12345, dtype=torch.int32, device=dev)
    if small:
        D.lz4_decompress_prefix_small(desc, want, ret, [a if a is not None else len(s) for s, a, _ in items],
                                      [c for _, _, c in items])
    else:
        D.lz4_decompress_prefix(desc, want, ret)
    torch.cuda.synchronize()
    return ret.cpu().tolist(), images(dst_t, do, items)


def check_image(img, cap, first, ret, full, what):
    """dst[first, ret) equals the full decode's bytes; everything else is still poison"""
    want = np.full(cap + 2 * GUARD, POISON, dtype=np.uint8)
    if ret > first:
        want[GUARD + first:GUARD + ret] = np.frombuffer(full[first:ret], dtype=np.uint8)
    bad = np.nonzero(want != img)[0]
    assert bad.size == 0, f"{what}: first wrong byte at {bad[0] - GUARD} ({bad.size} wrong)"


def windows(total, cap):
    return [
        (CHUNK + 4464, CHUNK + 8560),          # inside chunk 1
        (2 * CHUNK - 2000, 2 * CHUNK + 2096),  # straddling chunks 1 | 2
        (2 * CHUNK, 2 * CHUNK + 4096),         # lo on a boundary
        (150001, total),                       # hi = total
        (3 * CHUNK + 392, total - 1000),       # lo in the ragged chunk
        (70000, 70000),                        # lo = hi
        (total + 100, total + 200),            # lo > total
        (-5, 3000),                            # negative lo
        (140000, cap + 1000),                  # hi > cap
    ]


@pytest.fixture(scope="module")
def sources():
    """{kind: 200,000 bytes}: text, zeros, an incompressible chunk and more followed by text (a literal run crosses
    the first chunk boundary)"""
    return {"text": gen_block("T", 4100, N), "zeros": bytes(N),
            "rand-text": gen_block("R", 4101, 70000) + gen_block("T", 4102, N - 70000)}


@pytest.fixture(scope="module")
def fast(sources):
    out = {k: C.lz4_fast_host(v) for k, v in sources.items()}
    # the literal run of rand-text really crosses the boundary
    ll, _, _, _ = K.sequences(out["rand-text"])[0]
    assert ll > CHUNK
    return out


@pytest.fixture(scope="module")
def exact(sources, oracle):
    return {k: oracle.lz4_compress(v)[1] for k, v in sources.items()}


def expected(lo, hi, cap, total):
    """(ret, floor tried) by the header's contract for a well-formed block"""
    lo1, hi1 = max(lo, 0), min(hi, cap)
    if hi1 <= lo1:
        return 0, 0
    return min(total, hi1), floor_of(lo1)


def test_windows_on_fast_blocks(gpu, sources, fast):
    items, wins, meta = [], [], []
    for kind, comp in fast.items():
        for cap in (N, N + 300):
            for w in windows(N, cap):
                items.append((comp, None, cap))
                wins.append(w)
                meta.append(kind)
    D.lz4_window_counts(reset=True)
    rets, imgs = run_window(gpu, items, wins)
    floored = entries = 0
    for kind, (_, _, cap), (lo, hi), r, img in zip(meta, items, wins, rets, imgs):
        ret, fc = expected(lo, hi, cap, N)
        assert r == ret, (kind, lo, hi, cap, r)
        check_image(img, cap, fc, ret, sources[kind], (kind, lo, hi, cap))
        floored += ret > 0 and fc > 0
        entries += max(ret - fc, 0)
    counts = D.lz4_window_counts()
    assert floored > 0 and counts == (floored, 0, 0, entries), (counts, floored, entries)


def test_thread_per_segment_emit_above_the_wave_limit(gpu, sources, fast):
    """more than 65,536 segments in one call: the thread-per-segment form of the emit, same contract"""
    rnd = gen_block("R", 4103, N)
    srcs = dict(sources, rand=rnd)
    comps = dict(fast, rand=C.lz4_fast_host(rnd))
    kinds = ["rand", "rand-text", "rand", "text", "rand", "zeros"]
    ws = windows(N, N)
    items, wins, meta, nseg = [], [], [], 0
    while nseg <= 65536 + 256:
        k = kinds[len(items) % len(kinds)]
        items.append((comps[k], None, N))
        wins.append(ws[len(items) % 5])
        meta.append(k)
        nseg += (len(comps[k]) + 255) // 256
    D.lz4_window_counts(reset=True)
    rets, imgs = run_window(gpu, items, wins)
    floored = 0
    for kind, (lo, hi), r, img in zip(meta, wins, rets, imgs):
        ret, fc = expected(lo, hi, N, N)
        assert r == ret, (kind, lo, hi, r)
        check_image(img, N, fc, ret, srcs[kind], (kind, lo, hi))
        floored += fc > 0
    counts = D.lz4_window_counts()
    assert counts[:3] == (floored, 0, 0) and floored == len(items), counts


def test_windows_on_exact_text_equal_the_prefix_call(gpu, sources, exact):
    comp, src = exact["text"], sources["text"]
    items, wins = [], []
    for cap in (N, N + 300):
        for w in windows(N, cap):
            items.append((comp, None, cap))
            wins.append(w)
    D.lz4_window_counts(reset=True)
    rets, imgs = run_window(gpu, items, wins)
    counts = D.lz4_window_counts()
    pre, pimgs = run_prefix(gpu, items, [w[1] for w in wins], small=True)
    for (_, _, cap), (lo, hi), r, img, p, pimg in zip(items, wins, rets, imgs, pre, pimgs):
        lo1, hi1 = max(lo, 0), min(hi, cap)
        if hi1 <= lo1:
            assert r == 0 and (img == POISON).all(), (lo, hi, cap, r)
            continue
        assert r == p == min(N, hi1), (lo, hi, cap, r, p)
        assert img[GUARD + lo1:GUARD + r].tobytes() == pimg[GUARD + lo1:GUARD + r].tobytes() == src[lo1:r]
        # whichever floor the probe chose, nothing in front of the chunk floor or behind ret is written twice over
        assert (img[:GUARD] == POISON).all() and (img[GUARD + r:] == POISON).all()
        body = img[GUARD:GUARD + floor_of(lo1)]
        assert (body == POISON).all() or body.tobytes() == src[:floor_of(lo1)]
    assert counts[1] > 0 and counts[2] == 0, counts


def _with_offset(comp, pick, value=0):
    """the stream with the offset of the first sequence pick(op, ll, ml) accepts set to value, and that sequence's
    output position"""
    op = 0
    for ll, lit, ml, off in K.sequences(comp):
        if ml and pick(op, ll, ml):
            b = bytearray(comp)
            b[lit + ll], b[lit + ll + 1] = value & 255, value >> 8
            return bytes(b), op
        op += ll + ml
    raise AssertionError("no such sequence")


def test_bad_offset_in_front_of_the_floor_is_unseen(gpu, sources, fast):
    bad, at = _with_offset(fast["text"], lambda op, ll, ml: op > 1000)
    assert at < CHUNK - 1000
    lo, hi = 2 * CHUNK + 100, 2 * CHUNK + 4000
    D.lz4_window_counts(reset=True)
    rets, imgs = run_window(gpu, [(bad, None, N)], [(lo, hi)])
    assert rets == [hi]
    check_image(imgs[0], N, 2 * CHUNK, hi, sources["text"], "unseen fault")
    assert D.lz4_window_counts()[:3] == (1, 0, 0)


def test_bad_offset_inside_the_window_hands_the_block_over(gpu, fast):
    """An offset beyond the bytes produced: the one offset fault the full decoder answers with an error, and with
    16-bit offsets it can only stand in the block's first 64 KiB -- so the window starts there too."""
    lo, hi = 1000, 5000
    bad, at = _with_offset(fast["text"], lambda op, ll, ml: op + ll > lo + 500, 0xFFFF)
    assert lo < at < hi
    desc, dst_t, _ = make_batch(gpu, [(bad, None, N)])
    full = torch.full((1,), 7, dtype=torch.int32, device=gpu)
    D.lz4_decompress(desc, full)
    torch.cuda.synchronize()
    D.lz4_window_counts(reset=True)
    rets, imgs = run_window(gpu, [(bad, None, N)], [(lo, hi)])
    assert rets == full.cpu().tolist() and rets[0] < 0
    assert (imgs[0][:GUARD] == POISON).all() and (imgs[0][GUARD + N:] == POISON).all()
    assert D.lz4_window_counts()[:3] == (0, 0, 1)


def test_eight_mixed_blocks_equal_the_prefix_call(gpu, sources, fast, exact):
    cut = fast["text"][:len(fast["text"]) // 2]
    items = [
        (fast["text"], None, N), (exact["text"], None, N + 5), (fast["text"], 0, N),  # (an empty src)
        (fast["zeros"], None, 0),                                                     # cap 0
        (None, 4096, N),                                                              # a NULL src
        (cut, None, N),                                                               # a truncated stream
        (fast["zeros"], None, N), (exact["rand-text"], None, N),
    ]
    wins = [(CHUNK + 5, CHUNK + 900), (3 * CHUNK + 1, N + 100), (CHUNK, CHUNK + 10), (CHUNK, CHUNK + 10),
            (CHUNK, CHUNK + 10), (CHUNK + 7, N + 100), (2 * CHUNK + 3, 2 * CHUNK + 3), (2 * CHUNK - 9, 3 * CHUNK + 9)]
    rets, imgs = run_window(gpu, items, wins)
    pre, pimgs = run_prefix(gpu, items, [w[1] for w in wins], small=False)
    for i, ((_, _, cap), (lo, hi), r, img, p, pimg) in enumerate(zip(items, wins, rets, imgs, pre, pimgs)):
        if i == 6:  # lo = hi on a well-formed block: 0, where the prefix call decodes to hi
            assert r == 0 and (img == POISON).all()
            continue
        assert r == p, (i, r, p)
        assert (img[:GUARD] == POISON).all() and (img[GUARD + cap:] == POISON).all(), i
        if r > lo:
            assert img[GUARD + lo:GUARD + r].tobytes() == pimg[GUARD + lo:GUARD + r].tobytes(), i
    assert rets[0] == CHUNK + 900 and rets[1] == N and rets[7] == 3 * CHUNK + 9
    assert rets[5] < 0  # the truncated stream: the full decoder's error, through the hand-over


def test_sizes_over_the_hosts_copies_are_handed_over(gpu, sources, fast):
    D.lz4_window_counts(reset=True)
    lo, hi = CHUNK + 500, CHUNK + 900
    rets, imgs = run_window(gpu, [(fast["text"], None, N)], [(lo, hi)], host_lens=[64], host_caps=[1000])
    assert rets == [hi] and imgs[0][GUARD:GUARD + hi].tobytes() == sources["text"][:hi]
    assert D.lz4_window_counts()[:3] == (0, 0, 1)


# ------------------------------------------------------------------ the read calls
NSRC = 4


@pytest.fixture(scope="module")
def read_case():
    raws = [gen_block("T", 4200 + i, N) for i in range(NSRC)]
    stored = [C.lz4_fast_host(r) for r in raws]
    parts = []
    for s in range(NSRC):  # two reads per source at different chunks
        parts.append([(s, CHUNK + 300 + 11 * s, 2000)])
        parts.append([(s, 2 * CHUNK + 5000 + 7 * s, 3000), (-1, 0, 100), ((s + 1) % NSRC, 3 * CHUNK + 10, 500)])
    return raws, stored, parts


def _modes(decode, window):
    return C.set_read_decode_mode(decode), C.set_read_lz4_window_mode(window)


def _read(stored, parts, sealed=None):
    totals = [sum(p[2] for p in ps) for ps in parts]
    dst = Dst([t + (j % 2) for j, t in enumerate(totals)])
    src = list(zip(stored, [N] * len(stored)))
    wanted = [j == 1 for j in range(len(parts))]  # one read with its disk-cache checksum
    if sealed is None:
        res = C.NewCompressor("lz4").ReadBatch(src, dst.views, _plan(parts), with_csum=wanted)
    else:
        res = E.read_open_batch(L.ALGO_LZ4, sealed[0], src, sealed[1], dst.views, _plan(parts), with_csum=wanted)
    return dst, res


@pytest.mark.parametrize("sealed", [False, True], ids=["read_batch", "read_open_batch-chacha20"])
def test_read_calls_switch_on_equals_switch_off(gpu, oracle, read_case, sealed):
    raws, stored, parts = read_case
    key = None
    if sealed:
        rng = random.Random(6)
        rb = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
        algo = E.CHACHA20_RSA
        params = [(rb(E.key_size(algo)), rb(12), rb(7 + i)) for i in range(NSRC)]
        pairs = [(bytearray(E.envelope_bound(L.ALGO_LZ4, len(r), len(p[2]))), r) for r, p in zip(raws, params)]
        with C.lz4_parse_mode("fast"):  # (chunked blocks: the sealed payloads come from the library's encoder)
            res = E.compress_seal_batch(L.ALGO_LZ4, algo, pairs, params)
        assert all(e is None for _, e in res)
        stored = [bytes(buf[:n]) for (buf, _), (n, _) in zip(pairs, res)]
        key = (algo, [p[0] for p in params])
    want = C.read_expect(raws, _plan(parts))
    need = [max(p[1] + p[2] for ps in parts for p in ps if p[0] == s) for s in range(NSRC)]
    head = [[(s, 100 + s, 1500), (s, CHUNK - 1, 3)] for s in range(NSRC)]  # every source read from chunk 0
    prev = _modes("prefix", "off")
    try:
        D.lz4_window_counts(reset=True)
        dst0, res0 = _read(stored, parts, key)
        assert D.lz4_window_counts() == (0, 0, 0, 0)
        _modes("prefix", "on")
        dst1, res1 = _read(stored, parts, key)
        counts = D.lz4_window_counts(reset=True)
        _modes("full", "on")
        dst2, res2 = _read(stored, parts, key)
        counts_full = D.lz4_window_counts(reset=True)
        dsth, resh = _read(stored, head, key)
        counts_head = D.lz4_window_counts(reset=True)
        _modes("full", "off")
        dst3, res3 = _read(stored, parts, key)
        dsth0, resh0 = _read(stored, head, key)
    finally:
        _modes(*prev)
    # prefix mode: everything identical -- source and read results, checksums of the sources and of the reads
    assert _codes(res1[0]) == _codes(res0[0]) and _codes(res1[1]) == _codes(res0[1])
    assert list(res1[2]) == list(res0[2]) and res1[3] == res0[3]
    assert [n for n, _ in _codes(res1[0])] == need  # src_n = min(size, need)
    # full mode: the reads, their checksums and statuses are the switch-off call's; src_n as in prefix mode
    assert _codes(res2[1]) == _codes(res3[1]) and res2[3] == res3[3] and list(res2[2]) == list(res3[2])
    assert _codes(res2[0]) == _codes(res1[0]) and [n for n, _ in _codes(res3[0])] == [N] * NSRC
    for j, w in enumerate(want):
        assert res0[1][j] == (len(w), None)
        for d in (dst0, dst1, dst2, dst3):
            d.check(j, w)
    assert res1[3][1] == oracle.crc32c_segments(want[1])
    # every source starts in chunk 1: decoded from that floor, none sent to floor 0 or handed over
    assert counts[:3] == (NSRC, 0, 0) and counts_full[:3] == (NSRC, 0, 0), (counts, counts_full)
    # reads that all start in chunk 0: the call is the switch-off call, no window counter moves
    assert counts_head == (0, 0, 0, 0), counts_head
    assert _codes(resh[0]) == _codes(resh0[0]) and _codes(resh[1]) == _codes(resh0[1])
    for j, w in enumerate(C.read_expect(raws, _plan(head))):
        dsth.check(j, w)
        dsth0.check(j, w)
