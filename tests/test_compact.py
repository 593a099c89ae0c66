"""CPU: the compaction plan (compact_plan, the restatement of
pkg/vfs/compact.go:54-108 + readSlice) against a flat numpy model, and
jfs_compact_batch's host-side validation, which runs before any device is
touched.  No GPU compute is called here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slice_bytes(slices, seed=7):
    """Distinct random contents per slice id (keyed by (id, size))."""
    rng = np.random.default_rng(seed)
    data = {}
    for sid, size, _, _ in slices:
        if sid and (sid, size) not in data:
            data[(sid, size)] = rng.integers(0, 256, size, dtype=np.uint8)
    return data


def flat_model(slices, data, block_size):
    """compact.go:68-104 without blocks: write every slice's bytes (zeros for a
    hole) at pos, then cut the stream at block_size."""
    flat = np.zeros(sum(s[3] for s in slices), dtype=np.uint8)
    pos = 0
    for sid, size, off, ln in slices:
        if sid:
            flat[pos:pos + ln] = data[(sid, size)][off:off + ln]
        pos += ln
    return [flat[o:o + block_size] for o in range(0, len(flat), block_size)]


def gathered(sources_bytes, seg_first, seg):
    """The bytes a plan implies, block by block (the gather on the host)."""
    outs = []
    for j in range(len(seg_first) - 1):
        segs = seg[seg_first[j]:seg_first[j + 1]]
        out = np.zeros(sum(s[3] for s in segs), dtype=np.uint8)
        at = 0
        for src, src_off, dst_off, n in segs:
            assert dst_off == at and n > 0  # the tiling rule of jfs_compact_seg
            if src >= 0:
                assert src_off >= 0 and src_off + n <= len(sources_bytes[src])
                out[dst_off:dst_off + n] = sources_bytes[src][src_off:src_off + n]
            at += n
        outs.append(out)
    return outs


PLAN_CASES = {
    # slices start and end in the middle of stored blocks and of new blocks
    "mid_block": ([(1, 1000, 130, 700), (2, 300, 7, 200), (3, 64, 0, 64)], 256, 256),
    "hole_between": ([(1, 500, 10, 300), (0, 0, 0, 333), (2, 400, 399, 1)], 256, 256),
    "hole_only": ([(0, 0, 0, 700)], 256, 256),
    "exact_multiple": ([(1, 2048, 256, 512), (2, 256, 0, 256)], 256, 256),
    "src_block_larger": ([(1, 5000, 1000, 3000), (0, 0, 0, 10), (2, 1024, 0, 1024)], 256, 1024),
    "src_block_smaller": ([(1, 5000, 1, 4999), (2, 100, 50, 50)], 1000, 96),
    "same_slice_twice": ([(1, 900, 0, 300), (1, 900, 200, 700)], 512, 256),
    "empty": ([], 256, 256),
    "zero_len_slice": ([(1, 100, 5, 0), (2, 100, 0, 100)], 64, 64),
}


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_compact_plan_matches_flat_model(name):
    slices, B, S = PLAN_CASES[name]
    data = _slice_bytes(slices)
    sources, seg_first, seg = C.compact_plan(slices, B, S)
    blocks = []
    for si, b, blen in sources:
        sid, size = slices[si][0], slices[si][1]
        assert sid != 0 and blen == min(S, size - b * S) and blen > 0
        blocks.append(data[(sid, size)][b * S:b * S + blen])
    assert len(set((slices[si][0], slices[si][1], b) for si, b, _ in sources)) == len(sources)  # each block once
    want = flat_model(slices, data, B)
    got = gathered(blocks, seg_first, seg)
    assert len(got) == len(want) == len(seg_first) - 1
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert all(len(w) == B for w in want[:-1])  # only the last block is ragged
    assert seg_first[0] == 0 and seg_first[-1] == len(seg)


def test_compact_plan_default_source_block_size_and_bad_slice():
    slices = [(1, 700, 100, 600)]
    assert C.compact_plan(slices, 256) == C.compact_plan(slices, 256, 256)
    with pytest.raises(ValueError):
        C.compact_plan([(1, 100, 50, 51)], 256)


def _call(lib, algo, srcs, outs, seg_first, seg, src_n=True, out_n=True, null=()):
    """jfs_compact_batch over host buffers; `null` names pointer arguments to pass as NULL."""
    ns, no = len(srcs), len(outs)
    siov, oiov = (L.JfsIov * max(ns, 1))(), (L.JfsIov * max(no, 1))()
    keep = []
    for i, (buf, n, cap) in enumerate(srcs):
        keep.append(buf)
        siov[i].src = ctypes.cast(buf, ctypes.c_void_p) if buf is not None else None
        siov[i].src_len, siov[i].dst_cap = n, cap
    for j, (buf, cap) in enumerate(outs):
        keep.append(buf)
        oiov[j].dst = ctypes.cast(buf, ctypes.c_void_p) if buf is not None else None
        oiov[j].dst_cap = cap
    first = (ctypes.c_int32 * max(len(seg_first), 1))(*seg_first)
    segs = (L.JfsCompactSeg * max(len(seg), 1))()
    for k, s in enumerate(seg):
        segs[k].src, segs[k].src_off, segs[k].dst_off, segs[k].len = s
    a_src_n, a_out_n = (ctypes.c_int64 * max(ns, 1))(), (ctypes.c_int64 * max(no, 1))()
    args = {"src": siov, "out": oiov, "seg_first": first, "seg": segs, "src_n": a_src_n, "out_n": a_out_n}
    for k in null:
        args[k] = None
    return lib.jfs_compact_batch(algo, ns, args["src"], no, args["out"], args["seg_first"], args["seg"], args["src_n"],
                                 args["out_n"], None, 0)


def _valid():
    src = ctypes.create_string_buffer(b"\x10" * 40, 40)
    dst = ctypes.create_string_buffer(128)
    return [(src, 40, 64), (src, 40, 64)], [(dst, 128), (dst, 128)], [0, 2, 3], [(0, 0, 0, 8), (-1, 0, 8, 4), (1, 3, 0, 5)]


INVALID_CASES = {
    "src_index_nsrc": lambda s, o, f, g: (s, o, f, [g[0], g[1], (2, 3, 0, 5)]),
    "src_index_below_hole": lambda s, o, f, g: (s, o, f, [(-2, 0, 0, 8), g[1], g[2]]),
    "negative_src_off": lambda s, o, f, g: (s, o, f, [(0, -1, 0, 8), g[1], g[2]]),
    "len_zero": lambda s, o, f, g: (s, o, f, [g[0], g[1], (1, 3, 0, 0)]),
    "len_negative": lambda s, o, f, g: (s, o, f, [(0, 0, 0, -8), g[1], g[2]]),
    "tiling_gap": lambda s, o, f, g: (s, o, f, [g[0], (-1, 0, 9, 4), g[2]]),
    "tiling_overlap": lambda s, o, f, g: (s, o, f, [g[0], (-1, 0, 7, 4), g[2]]),
    "first_not_zero": lambda s, o, f, g: (s, o, f, [g[0], g[1], (1, 3, 1, 5)]),
    "seg_first_not_monotone": lambda s, o, f, g: (s, o, [0, 3, 2], g),
    "seg_first_negative": lambda s, o, f, g: (s, o, [-1, 2, 3], g),
    "negative_src_len": lambda s, o, f, g: ([(s[0][0], -1, 64), s[1]], o, f, g),
    "negative_block_size": lambda s, o, f, g: ([s[0], (s[1][0], 40, -64)], o, f, g),
    "negative_dst_cap": lambda s, o, f, g: (s, [o[0], (o[1][0], -1)], f, g),
    "null_src_bytes": lambda s, o, f, g: ([(None, 40, 64), s[1]], o, f, g),
    "null_dst_bytes": lambda s, o, f, g: (s, [(None, 128), o[1]], f, g),
}


@pytest.mark.parametrize("algo", [L.ALGO_NONE, L.ALGO_LZ4, L.ALGO_ZSTD])
@pytest.mark.parametrize("name", sorted(INVALID_CASES))
def test_compact_batch_rejects_invalid_plan(lib, name, algo):
    s, o, f, g = INVALID_CASES[name](*_valid())
    assert _call(lib, algo, s, o, f, g) == L.JFS_ERR_INVALID


@pytest.mark.parametrize("null", ["src", "out", "seg_first", "seg", "src_n", "out_n"])
def test_compact_batch_rejects_null_arrays(lib, null):
    s, o, f, g = _valid()
    assert _call(lib, L.ALGO_LZ4, s, o, f, g, null=(null,)) == L.JFS_ERR_INVALID


def test_compact_batch_rejects_bad_counts_and_algo(lib):
    s, o, f, g = _valid()
    assert _call(lib, 3, s, o, f, g) == L.JFS_ERR_INVALID
    assert _call(lib, -1, s, o, f, g) == L.JFS_ERR_INVALID
    assert lib.jfs_compact_batch(L.ALGO_LZ4, -1, None, 0, None, None, None, None, None, None, 0) == L.JFS_ERR_INVALID
    assert lib.jfs_compact_batch(L.ALGO_LZ4, 0, None, -1, None, None, None, None, None, None, 0) == L.JFS_ERR_INVALID


def test_compact_batch_validates_then_reports_no_device():
    """With the engine switched off (JFS_GPU_CODEC=off: no device, as on a
    machine without a GPU) a valid plan returns JFS_ERR_NO_DEVICE and an
    invalid one still JFS_ERR_INVALID: validation comes first."""
    code = (
        "from tests.test_compact import _call, _valid, INVALID_CASES\n"
        "from juicefs_amd import _lib as L\n"
        "lib = L.load()\n"
        "print(lib.jfs_device_count())\n"
        "for a in (0, 1, 2): print(_call(lib, a, *_valid()))\n"
        "print(_call(lib, 1, *INVALID_CASES['tiling_gap'](*_valid())))\n"
        "print(_call(lib, 1, [], [], [0], []))\n")
    env = dict(os.environ, JFS_GPU_CODEC="off")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert got == [0, L.JFS_ERR_NO_DEVICE, L.JFS_ERR_NO_DEVICE, L.JFS_ERR_NO_DEVICE, L.JFS_ERR_INVALID,
                   L.JFS_ERR_NO_DEVICE]
