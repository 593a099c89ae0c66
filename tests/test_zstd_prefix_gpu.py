"""GPU: jfs_zstd_decompress_prefix_device (every stage of the Zstd decoder stops
at the block that reaches `want` output bytes) against the CPU
oracle (oracle/zstd_oracle.c), on the small-batch path (1 and 5 inputs per
call) and the one-wave path (130 inputs per call, above JFS_ZSTD_SPLIT_MAX's
default); jfs_zstd_split_counts tells which path ran.

For a well-formed input the contract gives ret = min(size, want clamped to
[0, dst_cap]) and dst[0, ret) = that prefix of the full decode.  Every
destination lies at an odd offset in one 0xAB-filled device buffer that is
compared whole: nothing outside dst[0, dst_cap) may change, and for the stop
tests nothing from a given offset on."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from juicefs_amd import _lib as L
from juicefs_amd import device as D
from juicefs_amd.blockgen import gen_block
from tests import zstd_frames as Z
from tests.zstd_conformance_cases import FSE3, HB, LV, SV, T1, TB, pat

pytestmark = pytest.mark.gpu

BLK = 128 << 10
ZNB = 16  # zseqb: blocks per workgroup half (zstd_decode.hip)
CANARY = 0xAB
SLACK = 100  # dst_cap = size + SLACK, so that size + 1 and dst_cap differ
_cache = {}


def _raw8():
    data = gen_block("R", 77, 8 * BLK)
    return [Z.raw(data[i * BLK:(i + 1) * BLK]) for i in range(8)], data


def frames(oracle):
    """name -> (frame bytes, decoded bytes)"""
    if "frames" not in _cache:
        f = {}
        for name, n in (("T1", 100 << 10), ("T3", 384 << 10), ("T16", 2 << 20), ("T20", 20 * BLK)):
            raw = gen_block("T", 4200 + n % 97, n)
            f[name] = (oracle.zstd_compress_l1(raw), raw)
        blocks, data = _raw8()
        f["RAW8"] = (Z.write([Z.frame(blocks)]), data)
        # treeless literals and repeat-mode sequence tables (the conformance cases' blocks), raw and RLE blocks between
        desc = [Z.frame([HB, TB, Z.raw(pat(300)), Z.comp(LV, SV, seq=FSE3),
                         Z.comp(LV, SV, seq=dict(ll="rep", of="rep", ml="rep")), Z.rle(3, 9), T1, TB])]
        want = Z.expand(desc)
        assert want is not None
        f["CONF"] = (Z.write(desc), want)
        zero = bytes(2 * BLK)
        f["ZERO"] = (oracle.zstd_compress_l1(zero), zero)
        for name, (src, raw) in f.items():
            n, out = oracle.zstd_decompress(src, len(raw) + SLACK)
            assert n == len(raw) and out == raw, name
        _cache["frames"] = f
    return _cache["frames"]


def wants_for(size):
    cap = size + SLACK
    return [0, 1, 4096, BLK - 1, BLK, BLK + 1, ZNB * BLK - 1, ZNB * BLK, ZNB * BLK + 1, size - 1, size, size + 1,
            cap, cap + 1, -7]


def clamp(want, cap):
    return max(0, min(want, cap))


def plan(lib, src, cap, want):
    """jfs_zstd_plan_host_prefix of one input: (blocks walked, the rule fired)"""
    lib.jfs_zstd_plan_host_prefix.restype = None
    buf = ctypes.create_string_buffer(src, len(src))
    srcs = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    info = ctypes.create_string_buffer(64)
    tot = (ctypes.c_uint64 * 6)()
    lib.jfs_zstd_plan_host_prefix(srcs, (ctypes.c_int32 * 1)(len(src)), (ctypes.c_int32 * 1)(cap),
                                  (ctypes.c_int32 * 1)(want), 1, info, tot)
    n_blk, cap_out, want_st = struct.unpack_from("<IiI", info.raw, 52)
    assert cap_out == cap and (want_st & 0x7FFFFFFF) == clamp(want, cap) and tot[5] == clamp(want, cap)
    return n_blk, want_st >> 31


def blocks_of(src):
    """[(content position, type, size)] of the blocks of a one-frame source"""
    fhd = src[4]
    p = 5 + (0 if fhd & 0x20 else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if fhd & 0x20 else 0), 2, 4, 8)[fhd >> 6]
    out = []
    while True:
        bh = int.from_bytes(src[p:p + 3], "little")
        t, size = (bh >> 1) & 3, bh >> 3
        out.append((p + 3, t, size))
        p += 3 + (1 if t == 1 else size)
        if bh & 1:
            return out


def run(srcs, caps, wants, dev):
    """One jfs_zstd_decompress_prefix_device call.  Returns (rets, images):
    images[i] = dst[0, cap) of input i; everything around the destinations is
    checked to be untouched."""
    n = len(srcs)
    so, do, off, doff = [], [], 0, 0
    for i, s in enumerate(srcs):
        so.append(off + (7 * i) % 16)
        off = (so[-1] + len(s) + 64 + 15) & ~15
        do.append(doff + 1 + (5 * i) % 16)
        doff = (do[-1] + max(caps[i], 0) + 64 + 15) & ~15
    host = np.zeros(off + 64, dtype=np.uint8)
    for s, o in zip(srcs, so):
        host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    src_t = torch.from_numpy(host).to(dev)
    dst_t = torch.full((doff + 64,), CANARY, dtype=torch.uint8, device=dev)
    desc = D.make_desc(src_t, so, [len(s) for s in srcs], dst_t, do, caps)
    ret = torch.full((n,), -12345, dtype=torch.int32, device=dev)
    want_t = torch.tensor(wants, dtype=torch.int32, device=dev)
    D.zstd_decompress_prefix(desc, want_t, ret)
    torch.cuda.synchronize()
    dh = dst_t.cpu().numpy()
    outside = np.ones(len(dh), dtype=bool)
    for o, c in zip(do, caps):
        outside[o:o + max(c, 0)] = False
    assert (dh[outside] == CANARY).all(), "a byte outside dst[0, dst_cap) changed"
    return ret.cpu().tolist(), [dh[o:o + max(c, 0)] for o, c in zip(do, caps)]


def run_path(path, srcs, caps, wants, dev):
    """path 1 / 5: the small-batch path in calls of that many inputs; 130: one
    call of 130 inputs on the one-wave path (the list repeated to fill it)."""
    D.zstd_split_counts(reset=True)
    n = len(srcs)
    if path == 130:
        k = -(-130 // n)
        rets, imgs = run((srcs * k)[:130], (caps * k)[:130], (wants * k)[:130], dev)
        assert D.zstd_split_counts() == (0, 0), "the one-wave path was expected"
        for i in range(n, 130):  # the repeats agree with the first copy
            assert rets[i] == rets[i % n] and (imgs[i][:max(rets[i], 0)] == imgs[i % n][:max(rets[i], 0)]).all()
        return rets[:n], imgs[:n], (0, 0)
    rets, imgs = [], []
    for i in range(0, n, path):
        r, im = run(srcs[i:i + path], caps[i:i + path], wants[i:i + path], dev)
        rets += r
        imgs += im
    done, handed = D.zstd_split_counts()
    assert done + handed == n, "the small-batch path was expected"
    return rets, imgs, (done, handed)


def check_prefix(name, want, cap, ret, img, raw):
    exp = min(len(raw), clamp(want, cap))
    assert ret == exp, (name, want, ret, exp)
    assert img[:ret].tobytes() == raw[:ret], (name, want, "bytes differ")


@pytest.mark.parametrize("path", [1, 5, 130])
def test_prefix_results_match_oracle(gpu, oracle, path):
    """ret and dst[0, ret) for every frame and every want, on each path"""
    fr = frames(oracle)
    names, srcs, caps, wants = [], [], [], []
    for name, (src, raw) in fr.items():
        ws = wants_for(len(raw))
        if path == 1:  # single inputs: the stop, the block edge and the whole frame
            ws = [4096, BLK, len(raw)]
        for w in ws:
            names.append(name)
            srcs.append(src)
            caps.append(len(raw) + SLACK)
            wants.append(w)
    # the encoder's frames and the raw blocks first: one frame, no checksum, no error item, so stopped or not
    # the small-batch path replays every one of them itself
    proven = [i for i, nm in enumerate(names) if nm[0] == "T" or nm == "RAW8"]
    rest = [i for i in range(len(names)) if i not in proven]
    for part in (proven, rest):
        sel = lambda xs: [xs[i] for i in part]
        rets, imgs, (done, handed) = run_path(path, sel(srcs), sel(caps), sel(wants), gpu)
        for name, w, c, r, im in zip(sel(names), sel(wants), sel(caps), rets, imgs):
            check_prefix(name, w, c, r, im, fr[name][1])
        if path != 130 and part is proven:
            assert handed == 0, (done, handed)


def test_prefix_zero_block_never_stops(gpu, oracle, lib):
    """A zero-filled block has a tiny lower bound: the rule never fires, the
    frame is walked to its end and only the result is cut."""
    src, raw = frames(oracle)["ZERO"]
    cap = len(raw) + SLACK
    nb_full, _ = plan(lib, src, cap, cap)
    for w in (4096, BLK + 1, len(raw) - 1):  # (a want below the first block's few literals stops behind it)
        assert plan(lib, src, cap, w) == (nb_full, 0)
    rets, imgs, _ = run_path(1, [src], [cap], [BLK + 1], gpu)
    check_prefix("ZERO", BLK + 1, cap, rets[0], imgs[0], raw)


@pytest.mark.parametrize("path", [5, 130])
def test_prefix_raw_blocks_stop_exactly(gpu, oracle, lib, path):
    """raw blocks make the lower bound exact: ceil(want / 128 KiB) blocks are
    walked and nothing behind them is written"""
    src, raw = frames(oracle)["RAW8"]
    cap = len(raw) + SLACK
    wants = [0, 1, BLK - 1, BLK, BLK + 1, 300000, 7 * BLK, 7 * BLK + 1, len(raw), -3]
    for w in wants:
        k = -(-clamp(w, cap) // BLK)
        assert plan(lib, src, cap, w) == (min(k, 8), 1 if k < 8 else 0), w
    rets, imgs, _ = run_path(path, [src] * len(wants), [cap] * len(wants), wants, gpu)
    for w, r, im in zip(wants, rets, imgs):
        check_prefix("RAW8", w, cap, r, im, raw)
        end = -(-clamp(w, cap) // BLK) * BLK
        assert (im[end:] == CANARY).all(), (w, "written at or above the last walked block's end")


@pytest.mark.parametrize("path", [1, 130])
def test_prefix_skips_blocks_behind_the_stop(gpu, oracle, lib, path):
    """2 MiB of text, want = 4096: the rule walks at most 4 of the 16 blocks,
    and nothing from 512 KiB on is written"""
    src, raw = frames(oracle)["T16"]
    cap = len(raw) + SLACK
    assert plan(lib, src, cap, cap)[0] == 16
    n_blk, stopped = plan(lib, src, cap, 4096)
    assert stopped == 1 and 1 <= n_blk <= 4, (n_blk, stopped)
    rets, imgs, _ = run_path(path, [src], [cap], [4096], gpu)
    check_prefix("T16", 4096, cap, rets[0], imgs[0], raw)
    assert (imgs[0][4 * BLK:] == CANARY).all()


@pytest.mark.parametrize("path", [5, 130])
def test_prefix_stop_around_the_zseqb_halves(gpu, oracle, lib, path):
    """20 blocks: zseqb's first workgroup of an input takes blocks [0, 16), its
    second the rest.  Stops inside the first half, exactly at 16 blocks (the
    second half has no blocks and must not wait) and inside the second half."""
    src, raw = frames(oracle)["T20"]
    cap = len(raw) + SLACK
    assert plan(lib, src, cap, cap) == (20, 0)
    pick = {}
    for w in range(BLK // 2, len(raw), BLK // 8):  # the lower bound grows block by block: find a want per count
        nb, st = plan(lib, src, cap, w)
        if st:
            pick.setdefault(nb, w)
    for nb in (15, 16, 17, 19):
        assert nb in pick, (nb, sorted(pick))
    wants = [pick[nb] for nb in (15, 16, 17, 19)]
    rets, imgs, _ = run_path(path, [src] * 4, [cap] * 4, wants, gpu)
    for nb, w, r, im in zip((15, 16, 17, 19), wants, rets, imgs):
        check_prefix("T20", w, cap, r, im, raw)
        assert (im[nb * BLK:] == CANARY).all(), (nb, w)


def _flip(src, block, oracle, cap):
    """src with one byte of `block`'s literal section flipped so that the full decode fails: (bytes, code)"""
    bpos, t, size = blocks_of(src)[block]
    assert t == 2
    for d in range(8, 64):
        bad = bytearray(src)
        bad[bpos + d] ^= 0x5A
        n, _ = oracle.zstd_decompress(bytes(bad), cap)
        if n < 0:
            return bytes(bad), n
    raise AssertionError("no flip of the literal section failed the decode")


@pytest.mark.parametrize("path", [5, 130])
def test_prefix_faults(gpu, oracle, path):
    src, raw = frames(oracle)["T16"]
    size, cap = len(raw), len(raw) + SLACK
    # block 10: unseen behind the stop, reported when the whole frame is wanted
    bad10, code10 = _flip(src, 10, oracle, cap)
    # block 0: reported for every want > 0
    bad0, code0 = _flip(src, 0, oracle, cap)
    # a wrong content size and a wrong XXH64 on raw blocks: frame-end checks, never run on a stopped frame
    blocks, data = _raw8()
    fcs = Z.write([Z.frame(blocks, fcs_size=4, fcs=len(data) + 1)])
    xxh = Z.write([Z.frame(blocks, checksum="bad")])
    assert oracle.zstd_decompress(fcs, len(data) + SLACK)[0] < 0 and oracle.zstd_decompress(xxh, len(data) + SLACK)[0] < 0
    cases = [(bad10, cap, 4096, 4096, raw), (bad10, cap, size, code10, None),
             (fcs, len(data) + SLACK, 4096, 4096, data), (xxh, len(data) + SLACK, 4096, 4096, data),
             (fcs, len(data) + SLACK, len(data), oracle.zstd_decompress(fcs, len(data) + SLACK)[0], None),
             (xxh, len(data) + SLACK, len(data), oracle.zstd_decompress(xxh, len(data) + SLACK)[0], None)]
    cases += [(bad0, cap, w, code0, None) for w in (1, 4096, BLK + 1, size)]
    cases.append((bad0, cap, 0, 0, None))
    rets, imgs, _ = run_path(path, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], gpu)
    for i, ((s, c, w, exp, data), r, im) in enumerate(zip(cases, rets, imgs)):
        assert r == exp, (i, w, r, exp)
        if data is not None:
            assert im[:r].tobytes() == data[:r], i


def test_prefix_invalid_arguments(gpu, lib):
    assert lib.jfs_zstd_decompress_prefix_device(None, None, 0, None, None) == 0
    ret = torch.zeros(1, dtype=torch.int32, device=gpu)
    assert lib.jfs_zstd_decompress_prefix_device(ret.data_ptr(), None, 1, ret.data_ptr(), None) == L.JFS_ERR_INVALID
