"""GPU: every hand-over of the small-batch decoders (lz4_split.hip,
zstd_split.inc) to the exact kernels, through the full and the prefix
launchers.  Streams from tests/split_streams.py put a block on a known side of
each hand-over (the host model of the fix-up, the proven bound of the jump
rounds), and the test hook jfs_test_set_split_jump_rounds forces the one the
data cannot reach: a gather that meets an unsettled entry after part of dst is
written.  Bar: the oracle's return values and bytes on every input, nothing
written past cap, and the diagnostic counters naming the reason that fired."""
import pytest

from juicefs_amd import device as D
from juicefs_amd.blockgen import gen_block
from tests import split_streams as S
from tests import zstd_frames as Z
from tests.test_lz4_prefix_gpu import run as run_lz4_prefix
from tests.test_lz4_split_gpu import run_small
from tests.test_zstd_prefix_gpu import run as run_zstd_prefix
from tests.test_zstd_split_gpu import run_device

pytestmark = pytest.mark.gpu


@pytest.fixture
def jump_rounds():
    """set(lz4=, zstd=) overrides the jump rounds; (0, 0) is restored afterwards"""
    try:
        yield D.set_split_jump_rounds
    finally:
        D.set_split_jump_rounds(0, 0)


@pytest.fixture(scope="module")
def text(oracle):
    """one 64 KiB + 333 text block: (compressed, raw)"""
    raw = gen_block("T", 4201, 65536 + 333)
    return oracle.lz4_compress(raw)[1], raw


def lz4_counts(comps, raws, dev, **kw):
    """Full decode of one batch into exactly-sized outputs: exact against raws;
    returns the six counters of that launch."""
    D.lz4_split_counts(reset=True)
    r, outs = run_small(comps, [len(x) for x in raws], dev, **kw)
    assert r == [len(x) for x in raws]
    assert all(o == x for o, x in zip(outs, raws))
    return D.lz4_split_counts()


def lz4_prefix_counts(comps, raws, wants, dev):
    """The same through the prefix launcher: ret = min(total, want) and the
    oracle's prefix (the bytes between want and cap are not part of the
    contract; the helper checks every byte outside [dst, dst + cap))."""
    D.lz4_split_counts(reset=True)
    r, imgs = run_lz4_prefix(dev, "small", comps, [len(x) for x in raws], wants)
    for x, img, raw, w in zip(r, imgs, raws, wants):
        assert x == min(len(raw), w), (x, w)
        assert img[:x].tobytes() == raw[:x]
    return D.lz4_split_counts()


def zstd_counts(frames, raws, dev, **kw):
    D.zstd_split_counts(reset=True)
    r, outs = run_device(frames, [len(x) for x in raws], dev, **kw)
    assert r == [len(x) for x in raws]
    assert all(o == x for o, x in zip(outs, raws))
    return D.zstd_split_counts()


def zstd_prefix_counts(frames, raws, wants, dev):
    D.zstd_split_counts(reset=True)
    r, imgs = run_zstd_prefix(frames, [len(x) for x in raws], wants, dev)
    for x, img, raw, w in zip(r, imgs, raws, wants):
        assert x == min(len(raw), w), (x, w)
        assert img[:x].tobytes() == raw[:x]
    return D.zstd_split_counts()


# ---------------------------------------------- a. the fix-up does not converge
@pytest.fixture(scope="module")
def fix_batch(oracle, text):
    """[above the model's edge, at the edge, text]: (streams, decoded bytes)"""
    over, n_over = S.nonmerging_stream(S.NWG_OVER, 301)
    edge, n_edge = S.nonmerging_stream(S.NWG_EDGE, 302)
    # the blocks' first segments are workgroup-aligned in this order, as the model assumes
    assert len(over) == S.NWG_OVER * S.SPAN
    r_over, r_edge = S.fix_rounds_needed(over), S.fix_rounds_needed(edge, seg0=S.NWG_OVER * S.T)
    print("fix rounds predicted:", r_over, r_edge)
    assert not S.converges(r_over) and S.converges(r_edge)
    raws = []
    for s, n in ((over, n_over), (edge, n_edge)):
        got, out = oracle.lz4_decompress(s, n)
        assert got == n
        raws.append(out)
    return [over, edge, text[0]], raws + [text[1]]


@pytest.mark.parametrize("mis", [0, 5])
def test_lz4_fixup_not_converged_goes_exact(gpu, fix_batch, mis):
    """Seven workgroup spans of token chains that never merge need more fix-up
    rounds than are launched: that block, and only it, is handed over for that
    reason; six spans (five rounds) and the text block stay on the split path."""
    comps, raws = fix_batch
    cnt = lz4_counts(comps, raws, gpu, mis=mis)
    print("counts", cnt)
    assert cnt == (2, 1, 1, 0, 0, 0), cnt


@pytest.mark.parametrize("which", ["one", "mid", "cap-1", "cap"])
def test_lz4_fixup_not_converged_prefix(gpu, fix_batch, which):
    """The prefix launcher on the same batch: the fix-up walks the compressed
    bytes whole whatever `want` is, so the same block is handed over, to the
    exact kernel's prefix instantiation."""
    comps, raws = fix_batch
    wants = [{"one": 1, "mid": len(x) // 2 + 1, "cap-1": len(x) - 1, "cap": len(x)}[which] for x in raws]
    cnt = lz4_prefix_counts(comps, raws, wants, gpu)
    print("counts", cnt)
    assert cnt == (2, 1, 1, 0, 0, 0), cnt


# ------------------------------------------------ b. the gather is not settled
@pytest.fixture(scope="module")
def deep_batch(oracle, text):
    comps = [S.chain_stream(20000), S.chain_stream(3, seed=9)]
    raws = [oracle.lz4_decompress(c, 1 << 20)[1] for c in comps]
    assert [len(x) for x in raws] == [S.chain_size(20000), S.chain_size(3)]
    return comps + [text[0]], raws + [text[1]]


def test_lz4_unsettled_gather_goes_exact(gpu, deep_batch, jump_rounds):
    """One jump round (the hook) instead of the seven the bound asks for.  A
    wave issues all its hop loads before its store, so an entry of the
    20,000-unit chain that lies more than HOPS units into its wave's 256-entry
    span ends round 0 on a match byte of that span: the gather finds it, and
    the block is handed over with reason [3] after part of dst is written.
    The 3-unit chain (depth 2 <= HOPS) settles in the one round.  The text
    block may fall either way."""
    comps, raws = deep_batch
    jump_rounds(lz4=1)
    cnt = lz4_counts(comps[:1], raws[:1], gpu)
    print("deep alone", cnt)
    assert cnt == (0, 1, 0, 1, 0, 0), cnt
    cnt = lz4_counts(comps[1:2], raws[1:2], gpu)
    print("shallow alone", cnt)
    assert cnt == (1, 0, 0, 0, 0, 0), cnt
    for mis in (0, 5):
        cnt = lz4_counts(comps, raws, gpu, mis=mis)
        print("batch", cnt)
        assert cnt[0] + cnt[1] == 3 and cnt[0] >= 1 and cnt[1] == cnt[3] >= 1 and cnt[2] == cnt[4] == cnt[5] == 0, cnt
    # the prefix launcher, want inside the deep block
    for w in (777, 110003, len(raws[0]) - 1):
        cnt = lz4_prefix_counts(comps, raws, [w, len(raws[1]), len(raws[2]) - 5], gpu)
        print("prefix", w, cnt)
        assert cnt[0] + cnt[1] == 3 and cnt[0] >= 1 and cnt[1] == cnt[3] >= 1 and cnt[2] == cnt[4] == cnt[5] == 0, cnt
    # the computed count again: everything stays on the split path
    jump_rounds(0, 0)
    assert lz4_counts(comps, raws, gpu, mis=5) == (3, 0, 0, 0, 0, 0)
    assert lz4_prefix_counts(comps, raws, [110003, len(raws[1]), len(raws[2]) - 5], gpu) == (3, 0, 0, 0, 0, 0)


# ------------------------------------------------------- c. the same for Zstd
@pytest.fixture(scope="module")
def zdeep_batch(golden, oracle):
    import os
    deep, tiny = S.zstd_chain_frame(20000), S.zstd_chain_frame(3, seed=9)
    f = next(f for f in golden["zstd"]["frames"] if f["cls"] == "T" and 100000 <= f["size"] <= 1 << 20)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", golden["zstd"]["bin"]), "rb") as h:
        h.seek(f["off"])
        src = h.read(f["csize"])
    n, raw = oracle.zstd_decompress(src, f["size"])
    assert n == f["size"]
    return [deep[0], src, tiny[0]], [deep[1], raw, tiny[1]]


def test_zstd_unsettled_gather_goes_exact(gpu, zdeep_batch, jump_rounds):
    """The Zstd twin (zsjump / zsgather / zsverd have lz4_split.hip's
    structure): with one jump round the 20,000-unit chain frame, two blocks
    long, is handed to the exact replay after part of dst is written; the
    3-unit frame settles."""
    frames, raws = zdeep_batch
    jump_rounds(zstd=1)
    assert zstd_counts(frames[:1], raws[:1], gpu, src_mis=3, dst_mis=1) == (0, 1)
    assert zstd_counts(frames[2:], raws[2:], gpu) == (1, 0)
    cnt = zstd_counts(frames, raws, gpu, src_mis=5, dst_mis=3)
    print("batch", cnt)
    assert cnt[0] + cnt[1] == 3 and cnt[1] >= 1 and cnt[0] >= 1, cnt
    # the prefix launcher: want in the first and in the second block of the deep frame
    for w in (50001, 150001):
        cnt = zstd_prefix_counts(frames[:1], raws[:1], [w], gpu)
        assert cnt == (0, 1), (w, cnt)
        cnt = zstd_prefix_counts(frames, raws, [w, len(raws[1]), len(raws[2])], gpu)
        print("prefix", w, cnt)
        assert cnt[0] + cnt[1] == 3 and cnt[1] >= 1 and cnt[0] >= 1, (w, cnt)
    jump_rounds(0, 0)
    assert zstd_counts(frames[:1], raws[:1], gpu) == (1, 0)
    assert zstd_counts(frames, raws, gpu, src_mis=5, dst_mis=3) == (3, 0)
    assert zstd_prefix_counts(frames, raws, [150001, len(raws[1]), len(raws[2])], gpu) == (3, 0)


# ---------------------------------------------------- d. the bound at its edges
@pytest.mark.parametrize("k", [4, 5, 6])
def test_lz4_jump_rounds_at_the_bound(gpu, oracle, k):
    """Chains one step per token, as deep as want / 4 + 1 allows, at the sizes
    where the round count steps from k to k + 1: the computed rounds settle
    each on the split path.  Each size is a launch of its own (the largest
    size of a launch sizes its rounds)."""
    sizes = S.bound_edge_sizes(k, 4)
    assert [S.jump_rounds(n, 4) for n in sizes] == [k, k, k + 1]
    for i, n in enumerate(sizes):
        s = S.flat_chain_stream(n)
        got, raw = oracle.lz4_decompress(s, n)
        assert got == n
        cnt = lz4_counts([s], [raw], gpu, mis=5 * (i & 1))
        assert cnt == (1, 0, 0, 0, 0, 0), (n, cnt)
    # the prefix launcher on one longer stream, want at those sizes
    long_n = 4 * S.HOPS ** k + 4444
    s = S.flat_chain_stream(long_n)
    got, raw = oracle.lz4_decompress(s, long_n)
    assert got == long_n
    for n in sizes:
        cnt = lz4_prefix_counts([s], [raw], [n], gpu)
        assert cnt == (1, 0, 0, 0, 0, 0), (n, cnt)


@pytest.mark.parametrize("k", [4, 5, 6])
def test_zstd_jump_rounds_at_the_bound(gpu, k):
    """The same for Zstd: one step per 3-byte sequence, bound cap / 3 + 1."""
    sizes = S.bound_edge_sizes(k, 3)
    assert [S.jump_rounds(n, 3) for n in sizes] == [k, k, k + 1]
    for i, n in enumerate(sizes):
        f, raw = S.zstd_flat_chain_frame(n)
        cnt = zstd_counts([f], [raw], gpu, src_mis=3 * (i & 1), dst_mis=i)
        assert cnt == (1, 0), (n, cnt)


# ------------------------------------------------- e. reasons, not just results
TAIL = bytes([0xF0, 1]) + b"sixteen literals"
LITS = b"abcdefgh"


def reason_of(stream, cap, dev, oracle, undefined=(0, 0)):
    """Decode one hand-written stream alone: the oracle's return value (and
    bytes on success, but for the range liblz4 leaves undefined); returns the
    counters."""
    want, out = oracle.lz4_decompress(stream, cap)
    D.lz4_split_counts(reset=True)
    r, outs = run_small([stream], [cap], dev)
    assert r == [want], (r, want)
    if want >= 0:
        a, b = undefined
        assert outs[0][:a] == out[:a] and outs[0][b:] == out[b:]
    return want, D.lz4_split_counts()


def test_lz4_handover_reasons(gpu, oracle):
    good = bytes([0x80]) + LITS + (8).to_bytes(2, "little") + TAIL  # 8 literals, match 4 at offset 8, 16 literals
    want, cnt = reason_of(good, 28, gpu, oracle)
    assert want == 28 and cnt == (1, 0, 0, 0, 0, 0), (want, cnt)
    # offset 0 (liblz4 1.9.3 accepts it and copies four bytes of dst onto
    # themselves: the exact kernel returns the same 28), and an offset one past
    # the bytes produced (an error): a token fails a check
    for off, ok in ((0, True), (9, False)):
        bad = bytes([0x80]) + LITS + off.to_bytes(2, "little") + TAIL
        want, cnt = reason_of(bad, 28, gpu, oracle, undefined=(8, 12))
        assert (want == 28) == ok and (want < 0) != ok and cnt == (0, 1, 0, 0, 1, 0), (off, want, cnt)
    # the last sequence is a match: no final literal run
    for stream in (bytes([0x80]) + LITS + (8).to_bytes(2, "little"),
                   bytes([0x80]) + LITS + (8).to_bytes(2, "little") + bytes([0x40]) + b"wxyz" + (4).to_bytes(2, "little")):
        want, cnt = reason_of(stream, 64, gpu, oracle)
        assert want < 0 and cnt == (0, 1, 0, 0, 0, 1), (len(stream), want, cnt)
    # control: a 200-byte block from the encoder
    raw = gen_block("T", 77, 200)
    want, cnt = reason_of(oracle.lz4_compress(raw)[1], 200, gpu, oracle)
    assert want == 200 and cnt == (1, 0, 0, 0, 0, 0), (want, cnt)


def test_zstd_late_offset_before_frame_start(gpu, oracle):
    """3,000 sequences in one block, number 2,900 with an offset far before the
    frame start: zsemit's `bad` exit, taken by one of its threads after the
    others wrote their entries.  The exact replay reports the oracle's error."""
    seqs = [(3, 3, 6)] + [(0, 3, 6)] * 2999
    seqs[2900] = (0, 3, 20000 + 3)
    frame = Z.write([Z.frame([Z.comp(Z.lit_raw(b"zst"), seqs)])])
    want, _ = oracle.zstd_decompress(frame, 10000)
    assert want < 0
    D.zstd_split_counts(reset=True)
    r, _ = run_device([frame], [10000], gpu, src_mis=1, dst_mis=1)
    assert r == [want], (r, want)
    assert D.zstd_split_counts() == (0, 1)
    # its valid twin stays on the split path
    seqs[2900] = (0, 3, 6)
    good = Z.write([Z.frame([Z.comp(Z.lit_raw(b"zst"), seqs)])])
    want, out = oracle.zstd_decompress(good, 10000)
    assert want == 9003
    D.zstd_split_counts(reset=True)
    r, outs = run_device([good], [10000], gpu, src_mis=1, dst_mis=1)
    assert r == [want] and outs[0] == out
    assert D.zstd_split_counts() == (1, 0)
