"""GPU: multi-frame Zstd inputs on the small-batch decode path
(juicefs_amd/csrc/zstd_split.inc): concatenated frames, seekable
objects and skippable frames are replayed block-parallel by the origin map, with
the repeat offsets, the entropy tables, the content size and the reach of a
match held per frame; everything else is handed to the exact one-wave replay.
Bar: the oracle's (oracle/zstd_oracle.c) return code and bytes [0, ret) on
every input, guard bytes around dst unchanged, and the counters
jfs_zstd_split_counts / jfs_zstd_split_frame_counts naming the route."""
import numpy as np
import pytest
import torch

from juicefs_amd import compress as C
from juicefs_amd import device as D
from juicefs_amd.blockgen import gen_block
from tests import split_streams as S
from tests import zstd_frames as Z
from tests import zstd_multiframe_cases as M
from tests import zstd_seek_cases as SK
from tests import zstd_seek_csum_cases as SC
from tests.test_zstd_prefix_gpu import clamp, run_path
from tests.zstd_conformance_cases import pat

pytestmark = pytest.mark.gpu
B = 128 << 10
DEFAULT = 16384


def run_device(srcs, caps, dev, src_mis=0, dst_mis=0):
    """Decode each src into its own dst (cap bytes) in ONE device call;
    returns (rets, outputs[:ret]) and checks nothing is written past cap
    (the harness of tests/test_zstd_split_gpu.py, with a guard in front too)."""
    n = len(srcs)
    so, do, off, doff = [], [], 0, 16
    for i, s in enumerate(srcs):
        m = (src_mis + 7 * i) % 16 if src_mis else 0
        so.append(off + m)
        off = (off + m + len(s) + 64 + 15) & ~15
        dm = (dst_mis + 5 * i) % 16 if dst_mis else 0
        do.append(doff + dm)
        doff = (doff + dm + caps[i] + 64 + 15) & ~15
    host = np.zeros(off + 64, dtype=np.uint8)
    for s, o in zip(srcs, so):
        host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    src_t = torch.from_numpy(host).to(dev)
    dst_t = torch.full((doff + 64,), 0xAB, dtype=torch.uint8, device=dev)
    desc = D.make_desc(src_t, so, [len(s) for s in srcs], dst_t, do, caps)
    ret = torch.zeros(n, dtype=torch.int32, device=dev)
    D.zstd_decompress_sync(desc, ret)
    r = ret.cpu().tolist()
    dh = dst_t.cpu().numpy()
    for o, c in zip(do, caps):
        assert (dh[o + c:o + c + 16] == 0xAB).all() and (dh[o - 1] == 0xAB)
    return r, [dh[o:o + max(x, 0)].tobytes() for o, x in zip(do, r)]


def counts(reset=False):
    return D.zstd_split_counts(reset=reset), D.zstd_split_frame_counts(reset=reset)


def decode(src, cap, dev, oracle):
    """src alone and five times in one call, misaligned: the oracle's code and
    bytes each time.  Returns (code, (done, handed), (multi-frame inputs,
    frames)) of the lone call; the batch must count five times that."""
    want, wo = oracle.zstd_decompress(src, cap)
    counts(reset=True)
    r, outs = run_device([src], [cap], dev, src_mis=5, dst_mis=3)
    assert r == [want] and (want < 0 or outs[0] == wo), (r, want)
    lone = counts(reset=True)
    r, outs = run_device([src] * 5, [cap] * 5, dev, src_mis=1, dst_mis=7)
    assert r == [want] * 5 and (want < 0 or outs == [wo] * 5), (r, want)
    batch = counts()
    assert batch == tuple(tuple(5 * x for x in c) for c in lone), (lone, batch)
    return (want,) + lone


@pytest.fixture
def split_frames():
    try:
        yield C.set_zstd_split_frames
    finally:
        C.set_zstd_split_frames(DEFAULT)


def test_two_frames_take_the_origin_map(gpu, oracle, split_frames):
    """fails without the feature: two frames are replayed block-parallel, and
    the limit 1 restores the hand-over"""
    src = Z.write([M.small(1), M.small(2)])
    assert C.zstd_split_frames() == DEFAULT
    want, split, frames = decode(src, 660, gpu, oracle)
    assert want == 660 and split == (1, 0) and frames == (1, 2), (want, split, frames)
    assert split_frames(1) == DEFAULT
    want, split, frames = decode(src, 660, gpu, oracle)
    assert want == 660 and split == (0, 1) and frames == (0, 0), (want, split, frames)


@pytest.mark.parametrize("history", [False, True])
def test_repeat_offsets_restart_per_frame(gpu, oracle, history):
    desc = M.rep_reset(history)
    src, exp = Z.write(desc), Z.expand(desc)
    want, split, frames = decode(src, len(exp) + 9, gpu, oracle)
    assert want == len(exp) and split == (1, 0) and frames == (1, 2), (want, split, frames)


def test_match_reaches_the_frame_start_and_no_further(gpu, oracle):
    desc = M.frame_base(0)
    src, exp = Z.write(desc), Z.expand(desc)
    want, split, frames = decode(src, len(exp), gpu, oracle)
    assert want == len(exp) == 370 and split == (1, 0) and frames == (1, 2), (want, split, frames)
    # one byte further lies in frame 1's output, which holds the byte a decoder that crossed the edge would want
    src = Z.write(M.frame_base(1))
    want, split, frames = decode(src, 370, gpu, oracle)
    assert want < 0 and split == (0, 1) and frames == (0, 0), (want, split, frames)


@pytest.mark.parametrize("which", ["treeless", "fse_repeat"])
def test_tables_do_not_cross_frames(gpu, oracle, which):
    src = Z.write(M.treeless_across() if which == "treeless" else M.fse_repeat_across())
    want, split, frames = decode(src, 2000, gpu, oracle)
    assert want < 0 and split == (0, 1), (want, split)


def test_content_sizes_per_frame(gpu, oracle):
    want, split, frames = decode(Z.write(M.sizes_swapped()), 201, gpu, oracle)
    assert want < 0 and split == (0, 1), (want, split)
    want, split, frames = decode(Z.write(M.sizes_mixed()), 990, gpu, oracle)
    assert want == 990 and split == (1, 0) and frames == (1, 3), (want, split, frames)


@pytest.mark.parametrize("table", ["8-byte", "12-byte", "lying"])
def test_skippable_frames_and_unread_tables(gpu, oracle, table):
    parts = [Z.skip(b"in front"), M.small(1, single=True, fcs_size=2), Z.skip(b""), M.small(2), Z.skip(b"x" * 300, nibble=7),
             Z.frame([Z.raw(pat(77, 4))], single=True, fcs_size=1)]
    pb = M.parts_bytes(parts)
    body = b"".join(b for b, _ in pb)
    content = b"".join(c for _, c in pb)
    if table == "12-byte":
        ent = [(len(b), len(c), Z.xxh64(c) & 0xFFFFFFFF) for b, c in pb]
        tab = SC.table(ent)
        assert SC.parse(tab, len(body) + len(tab)) is not None
    else:
        ent = [(len(b), len(c)) for b, c in pb]
        if table == "lying":  # the last two data frames swap their sizes: every sum still holds
            ent[3], ent[5] = (ent[3][0], ent[5][1]), (ent[5][0], ent[3][1])
        tab = SK.table(ent)
        assert SK.parse_table(body + tab) == ent
    want, split, frames = decode(body + tab, len(content), gpu, oracle)
    assert want == len(content) == 737 and split == (1, 0) and frames == (1, 3), (want, split, frames)


def test_empty_frames(gpu, oracle):
    src = Z.write([M.small(1), M.empty_frame(), M.small(2)])
    want, split, frames = decode(src, 660, gpu, oracle)
    assert want == 660 and split == (1, 0) and frames == (1, 3), (want, split, frames)
    want, split, frames = decode(Z.write([M.empty_frame()] * 3), 10, gpu, oracle)
    assert want == 0 and split == (1, 0) and frames == (1, 3), (want, split, frames)


@pytest.mark.parametrize("check", ["ok", "bad"])
def test_checksummed_frame_is_handed(gpu, oracle, check):
    src = Z.write([M.small(1), M.small(2, checksum=check), M.small(3)])
    want, split, frames = decode(src, 990, gpu, oracle)
    assert (want == 990) == (check == "ok") and split == (0, 1) and frames == (0, 0), (want, split, frames)


def test_capacity(gpu, oracle):
    src = Z.write([M.small(1), M.small(2, single=True, fcs_size=2), M.small(3)])
    total = 990
    for cap in (total, total - 1, total + 1000, 660, 330, 331):
        want, split, frames = decode(src, cap, gpu, oracle)
        assert (want == total) == (cap >= total), (cap, want)
        assert split == ((1, 0) if cap >= total else (0, 1)), (cap, split)


def test_damage(gpu, oracle):
    good = Z.write([M.small(1), M.small(2)])
    one = Z.write([M.small(1)])
    bad = []
    for tail in (b"\x00", b"\x01\x02\x03\x04", one[:7]):
        bad.append(good + tail)
    flip = bytearray(good)
    flip[len(one) + 6] ^= 0x08  # frame 2: 4 magic + descriptor + window, then the block header (size bit 0)
    bad.append(bytes(flip))
    for src in bad:
        want, split, frames = decode(src, 660, gpu, oracle)
        assert want < 0 and split == (0, 1) and frames == (0, 0), (len(src), want, split, frames)


def test_frame_limit(gpu, oracle, split_frames):
    src = Z.write([M.small(k) for k in range(5)])
    split_frames(4)
    want, split, frames = decode(src, 1650, gpu, oracle)
    assert want == 1650 and split == (0, 1) and frames == (0, 0), (want, split, frames)
    split_frames(5)
    want, split, frames = decode(src, 1650, gpu, oracle)
    assert want == 1650 and split == (1, 0) and frames == (1, 5), (want, split, frames)


_cache = {}


def encoded(dev, cls):
    """[(raw, object, frames)]: the seekable encoders' objects (8-byte and
    12-byte tables) of 2, 5 and 70 frames, encoded once per class"""
    if cls not in _cache:
        from tests.test_zstd_seekable_gpu import encode
        out = []
        for k, nf in enumerate((2, 5, 70)):
            n = {2: B + 1, 5: 5 * B - 3, 70: 70 * B - 1}[nf]
            raw = gen_block(cls, 7400 + k, n)
            r, objs, _, _ = encode(dev, [raw], [D.zstd_bound(n)])
            assert r[0] > 0
            out.append((raw, objs[0], nf))
            # the checksummed call, through the same harness
            so = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(dev)
            dd = torch.zeros(D.zstd_bound(n), dtype=torch.uint8, device=dev)
            ret = torch.zeros(1, dtype=torch.int32, device=dev)
            D.zstd_compress_seekable_csum(D.make_desc(so, [0], [n], dd, [0], [D.zstd_bound(n)]), ret)
            torch.cuda.synchronize()
            m = int(ret[0].item())
            assert m > 0
            out.append((raw, dd[:m].cpu().numpy().tobytes(), nf))
        _cache[cls] = out
    return _cache[cls]


@pytest.mark.parametrize("cls", ["T", "Z", "R"])
def test_encoder_objects(gpu, cls):
    objs = encoded(gpu, cls)
    for raw, obj, nf in objs:
        counts(reset=True)
        r, outs = run_device([obj], [len(raw)], gpu, src_mis=3, dst_mis=1)
        assert r == [len(raw)] and outs[0] == raw, (cls, nf, r)
        split, frames = counts()
        assert split == (1, 0) and frames == (1, nf), (cls, nf, split, frames)
    # the 5-frame objects in a batch of 130: the one-wave path, identical results
    five = [(raw, obj) for raw, obj, nf in objs if nf == 5]
    srcs = ([o for _, o in five] * 65)[:130]
    raws = ([r for r, _ in five] * 65)[:130]
    counts(reset=True)
    r, outs = run_device(srcs, [len(x) for x in raws], gpu)
    assert counts() == ((0, 0), (0, 0))
    assert r == [len(x) for x in raws] and all(o == x for o, x in zip(outs, raws))


@pytest.mark.parametrize("path", [1, 5])
def test_prefix_launcher(gpu, path):
    raw, obj, nf = encoded(gpu, "T")[2]
    assert nf == 5
    n, cap = len(raw), len(raw) + 100
    wants = [1, B - 1, B, B + 1, 2 * B + 777, 5 * B - 3, n + 50, cap + 7]
    D.zstd_split_frame_counts(reset=True)
    rets, imgs, (done, handed) = run_path(path, [obj] * len(wants), [cap] * len(wants), wants, gpu)
    assert done + handed == len(wants) and handed == 0, (done, handed)
    for w, r, im in zip(wants, rets, imgs):
        assert r == min(n, clamp(w, cap)), (w, r)
        assert im[:r].tobytes() == raw[:r], w
    # the stop rule fires in front of a block, so even want = 1 walks frame 1 to its end and enters frame 2
    multi, frames = D.zstd_split_frame_counts()
    assert multi == len(wants) and 2 * multi <= frames <= 5 * multi, (multi, frames)


def test_hand_over_after_a_partial_write(gpu, oracle):
    """one jump round instead of the computed count: the deep chain of frame 2
    is met unsettled by the gather after part of dst is written"""
    deep, draw = S.zstd_chain_frame(20000)
    first = [M.small(1)]
    src = Z.write(first) + deep
    exp = Z.expand(first) + draw
    want, wo = oracle.zstd_decompress(src, len(exp))
    assert want == len(exp) and wo == exp
    try:
        D.set_split_jump_rounds(zstd=1)
        counts(reset=True)
        r, outs = run_device([src], [len(exp)], gpu, src_mis=3, dst_mis=1)
        assert r == [want] and outs[0] == exp
        assert counts() == ((0, 1), (0, 0))
    finally:
        D.set_split_jump_rounds(0, 0)
    counts(reset=True)
    r, outs = run_device([src], [len(exp)], gpu, src_mis=3, dst_mis=1)
    assert r == [want] and outs[0] == exp
    assert counts() == ((1, 0), (1, 2))
