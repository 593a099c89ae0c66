"""CPU: the read plan (read_plan / read_expect, the restatement of
pkg/vfs/reader.go:813-879) against a flat numpy model of dataReader.Read, and
the host-side validation of jfs_read_batch / jfs_read_open_batch, which runs
before any device is touched.  No GPU compute is called here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from tests.test_compact import INVALID_CASES, _slice_bytes, _valid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flat_read(page_len, offset, slices, data):
    """dataReader.Read without blocks: the chunk is the concatenation of its
    slices (zeros for id 0); the page is chunk[offset : offset + page_len],
    zero-filled past the chunk's end."""
    chunk = np.zeros(sum(s[3] for s in slices), dtype=np.uint8)
    pos = 0
    for sid, size, off, ln in slices:
        if sid:
            chunk[pos:pos + ln] = data[(sid, size)][off:off + ln]
        pos += ln
    page = np.zeros(page_len, dtype=np.uint8)
    part = chunk[offset:offset + page_len]
    page[:len(part)] = part
    return page.tobytes()


CHUNK_A = [(1, 1000, 130, 700), (0, 0, 0, 333), (2, 300, 7, 200), (3, 64, 0, 64)]
CHUNK_B = [(4, 5000, 1, 4999), (1, 1000, 0, 300), (0, 0, 0, 17)]
READ_CASES = {
    # reads begin and end inside slices and stored blocks; the same stored blocks feed several reads
    "inside_slices": ([(512, 100, CHUNK_A), (128, 690, CHUNK_A), (4096, 0, CHUNK_B)], 256),
    "zero_tail": ([(2000, 1000, CHUNK_A), (64, 1296, CHUNK_A)], 256),
    "past_the_end": ([(100, 1297, CHUNK_A), (100, 5000, CHUNK_A)], 96),
    "hole_only": ([(700, 5, [(0, 0, 0, 900)])], 256),
    "empty_read_and_empty_chunk": ([(0, 10, CHUNK_A), (33, 0, [])], 256),
    "block_larger_than_slices": ([(1297, 0, CHUNK_A), (5316, 0, CHUNK_B)], 4096),
    "one_byte_reads": ([(1, o, CHUNK_A) for o in (0, 699, 700, 1032, 1033, 1296)], 64),
}


@pytest.mark.parametrize("name", sorted(READ_CASES))
def test_read_plan_matches_flat_model(name):
    reads, S = READ_CASES[name]
    data = _slice_bytes([s for _, _, sl in reads for s in sl])
    sources, seg_first, seg = C.read_plan(reads, S)
    blocks = []
    for ri, si, b, blen in sources:
        sid, size = reads[ri][2][si][0], reads[ri][2][si][1]
        assert sid != 0 and blen == min(S, size - b * S) and blen > 0
        blocks.append(data[(sid, size)][b * S:b * S + blen])
    keys = [(reads[ri][2][si][0], reads[ri][2][si][1], b) for ri, si, b, _ in sources]
    assert len(set(keys)) == len(keys)  # each stored block once, however many reads touch it
    got = C.read_expect(blocks, (seg_first, seg))
    assert len(got) == len(reads) == len(seg_first) - 1
    for (page_len, offset, slices), g in zip(reads, got):
        assert g == flat_read(page_len, offset, slices, data)
    assert seg_first[0] == 0 and seg_first[-1] == len(seg)
    assert all(s[3] > 0 for s in seg)


def test_read_plan_and_expect_reject_bad_input():
    with pytest.raises(ValueError):
        C.read_plan([(10, 0, [(1, 100, 50, 51)])], 256)
    with pytest.raises(ValueError):
        C.read_plan([(10, 0, CHUNK_A)], 0)
    with pytest.raises(ValueError):  # a source shorter than its segment
        C.read_expect([b"abc"], ([0, 1], [(0, 1, 0, 3)]))
    with pytest.raises(ValueError):  # broken tiling
        C.read_expect([b"abcdef"], ([0, 2], [(0, 0, 0, 3), (0, 0, 4, 2)]))


KEY = ctypes.create_string_buffer(b"\x07" * 32, 32)


def _call(lib, algo, srcs, outs, seg_first, seg, null=(), cipher=None, crcs=None, keys="all"):
    """jfs_read_batch (cipher None) or jfs_read_open_batch over host buffers;
    `null` names pointer arguments to pass as NULL."""
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
    want = (ctypes.c_int64 * max(ns, 1))(*crcs) if crcs is not None else None
    if cipher is None:
        return lib.jfs_read_batch(algo, ns, args["src"], want, no, args["out"], args["seg_first"], args["seg"],
                                  args["src_n"], args["out_n"], None, 0)
    kp = (ctypes.c_void_p * max(ns, 1))()
    for i in range(ns):
        kp[i] = ctypes.addressof(KEY) if keys in ("all", None) or i not in keys else None
    return lib.jfs_read_open_batch(algo, cipher, ns, args["src"], None if keys is None else kp, want, no, args["out"],
                                   args["seg_first"], args["seg"], args["src_n"], args["out_n"], None, 0)


BOTH = [None, L.CIPHER_AES256GCM]


@pytest.mark.parametrize("cipher", BOTH)
@pytest.mark.parametrize("algo", [L.ALGO_NONE, L.ALGO_LZ4, L.ALGO_ZSTD])
@pytest.mark.parametrize("name", sorted(INVALID_CASES))
def test_read_batch_rejects_invalid_plan(lib, name, algo, cipher):
    s, o, f, g = INVALID_CASES[name](*_valid())
    assert _call(lib, algo, s, o, f, g, cipher=cipher) == L.JFS_ERR_INVALID


@pytest.mark.parametrize("cipher", BOTH)
@pytest.mark.parametrize("null", ["src", "out", "seg_first", "seg", "src_n", "out_n"])
def test_read_batch_rejects_null_arrays(lib, null, cipher):
    s, o, f, g = _valid()
    assert _call(lib, L.ALGO_LZ4, s, o, f, g, null=(null,), cipher=cipher) == L.JFS_ERR_INVALID


@pytest.mark.parametrize("cipher", BOTH)
def test_read_batch_rejects_bad_counts_and_algo(lib, cipher):
    s, o, f, g = _valid()
    assert _call(lib, 3, s, o, f, g, cipher=cipher) == L.JFS_ERR_INVALID
    assert _call(lib, -1, s, o, f, g, cipher=cipher) == L.JFS_ERR_INVALID
    assert lib.jfs_read_batch(L.ALGO_LZ4, -1, None, None, 0, None, None, None, None, None, None, 0) == L.JFS_ERR_INVALID
    assert lib.jfs_read_batch(L.ALGO_LZ4, 0, None, None, -1, None, None, None, None, None, None, 0) == L.JFS_ERR_INVALID
    assert lib.jfs_read_open_batch(L.ALGO_LZ4, 0, -1, None, None, None, 0, None, None, None, None, None, None,
                                   0) == L.JFS_ERR_INVALID


@pytest.mark.parametrize("cipher", BOTH)
def test_read_batch_rejects_total_over_dst_cap_and_bad_crc(lib, cipher):
    s, o, f, g = _valid()
    assert _call(lib, L.ALGO_LZ4, s, [(o[0][0], 11), o[1]], f, g, cipher=cipher) == L.JFS_ERR_INVALID  # total 12
    assert _call(lib, L.ALGO_LZ4, s, [o[0], (o[1][0], 4)], f, g, cipher=cipher) == L.JFS_ERR_INVALID   # total 5
    for bad in (-2, 1 << 32, -(1 << 40)):
        assert _call(lib, L.ALGO_LZ4, s, o, f, g, cipher=cipher, crcs=[-1, bad]) == L.JFS_ERR_INVALID


def test_read_open_batch_rejects_bad_cipher_and_keys(lib):
    s, o, f, g = _valid()
    for cipher in (-1, 3, 99):
        assert _call(lib, L.ALGO_LZ4, s, o, f, g, cipher=cipher) == L.JFS_ERR_INVALID
    assert _call(lib, L.ALGO_LZ4, s, o, f, g, cipher=L.CIPHER_SM4GCM, keys=None) == L.JFS_ERR_INVALID
    assert _call(lib, L.ALGO_LZ4, s, o, f, g, cipher=L.CIPHER_CHACHA20POLY1305, keys={1}) == L.JFS_ERR_INVALID


def test_read_batch_validates_then_reports_no_device():
    """With the engine switched off (JFS_GPU_CODEC=off: no device, as on a
    machine without a GPU) a valid plan returns JFS_ERR_NO_DEVICE and an
    invalid one still JFS_ERR_INVALID: validation comes first."""
    code = (
        "from tests.test_read import _call, _valid, INVALID_CASES\n"
        "from juicefs_amd import _lib as L\n"
        "lib = L.load()\n"
        "print(lib.jfs_device_count())\n"
        "for c in (None, 0, 1, 2):\n"
        "    for a in (0, 1, 2): print(_call(lib, a, *_valid(), cipher=c, crcs=[-1, 0xFFFFFFFF]))\n"
        "    print(_call(lib, 1, *INVALID_CASES['tiling_gap'](*_valid()), cipher=c))\n"
        "    print(_call(lib, 1, *_valid(), cipher=c, crcs=[1 << 32, 0]))\n"
        "    print(_call(lib, 1, [], [], [0], [], cipher=c))\n")
    env = dict(os.environ, JFS_GPU_CODEC="off")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    nd = L.JFS_ERR_NO_DEVICE
    assert got == [0] + [nd, nd, nd, L.JFS_ERR_INVALID, L.JFS_ERR_INVALID, nd] * 4
