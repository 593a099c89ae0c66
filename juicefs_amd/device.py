"""Device-resident batch helpers (torch tensors in HBM -> libjfsgpu device API).

PyTorch is only plumbing here: it owns the HBM allocations and the stream; the
byte work is the HIP kernels behind ``jfs_lz4_decompress_device`` /
``jfs_lz4_compress_device`` / ``jfs_zstd_decompress_device``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib as L
# the counter readers of the device calls, built from the table in switches.py
from .switches import (lz4_chase_counts, lz4_eseg_counts, lz4_split_counts, lz4_window_counts,  # noqa: F401
                       zstd_sparse_counts, zstd_split_counts, zstd_split_frame_counts)

DESC_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("src_len", "<i4"), ("dst_cap", "<i4")])
assert DESC_DTYPE.itemsize == ctypes.sizeof(L.JfsDevBlock)


def make_desc(src: torch.Tensor, src_offs, src_lens, dst: torch.Tensor, dst_offs, dst_caps) -> torch.Tensor:
    """Build a device tensor of jfs_dev_block descriptors (24 bytes each)."""
    n = len(src_offs)
    a = np.zeros(n, dtype=DESC_DTYPE)
    a["src"] = src.data_ptr() + np.asarray(src_offs, dtype=np.uint64)
    a["dst"] = dst.data_ptr() + np.asarray(dst_offs, dtype=np.uint64)
    a["src_len"] = np.asarray(src_lens, dtype=np.int32)
    a["dst_cap"] = np.asarray(dst_caps, dtype=np.int32)
    t = torch.from_numpy(a.view(np.uint8).copy())
    return t.to(src.device)


def _stream_ptr(stream) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {rc}")


def lz4_decompress(desc: torch.Tensor, ret: torch.Tensor, stream=None):
    n = desc.numel() // DESC_DTYPE.itemsize
    _check(L.load().jfs_lz4_decompress_device(desc.data_ptr(), n, ret.data_ptr(), _stream_ptr(stream)),
           "jfs_lz4_decompress_device")


def lz4_compress(desc: torch.Tensor, ret: torch.Tensor, stream=None):
    n = desc.numel() // DESC_DTYPE.itemsize
    _check(L.load().jfs_lz4_compress_device(desc.data_ptr(), n, ret.data_ptr(), _stream_ptr(stream)),
           "jfs_lz4_compress_device")


def lz4_decompress_small(desc: torch.Tensor, ret: torch.Tensor, src_lens, dst_caps, stream=None):
    """jfs_lz4_decompress_device_small: few blocks, each spread over the GPU;
    src_lens / dst_caps are host copies of the descriptors' sizes."""
    n = desc.numel() // DESC_DTYPE.itemsize
    sl = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in src_lens])
    dc = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in dst_caps])
    _check(L.load().jfs_lz4_decompress_device_small(desc.data_ptr(), sl, dc, n, ret.data_ptr(), _stream_ptr(stream)),
           "jfs_lz4_decompress_device_small")


def lz4_decompress_prefix(desc: torch.Tensor, want: torch.Tensor, ret: torch.Tensor, stream=None):
    """jfs_lz4_decompress_prefix_device: block i is decoded as far as its first
    want[i] bytes (want: an int32 device tensor, one entry per descriptor)."""
    n = desc.numel() // DESC_DTYPE.itemsize
    assert want.dtype == torch.int32 and want.numel() >= n
    _check(L.load().jfs_lz4_decompress_prefix_device(desc.data_ptr(), want.data_ptr(), n, ret.data_ptr(),
                                                     _stream_ptr(stream)), "jfs_lz4_decompress_prefix_device")


def lz4_decompress_prefix_small(desc: torch.Tensor, want: torch.Tensor, ret: torch.Tensor, src_lens, dst_caps,
                                stream=None):
    """jfs_lz4_decompress_prefix_device_small: the same through the small-batch
    path; src_lens / dst_caps are host copies of the descriptors' sizes."""
    n = desc.numel() // DESC_DTYPE.itemsize
    assert want.dtype == torch.int32 and want.numel() >= n
    sl = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in src_lens])
    dc = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in dst_caps])
    _check(L.load().jfs_lz4_decompress_prefix_device_small(desc.data_ptr(), sl, dc, want.data_ptr(), n,
                                                           ret.data_ptr(), _stream_ptr(stream)),
           "jfs_lz4_decompress_prefix_device_small")


def zstd_decompress_prefix(desc: torch.Tensor, want: torch.Tensor, ret: torch.Tensor, stream=None):
    """jfs_zstd_decompress_prefix_device: input i is decoded as far as the Zstd
    block that reaches its first want[i] bytes (want: an int32 device tensor,
    one entry per descriptor); ret[i] = min(size, want[i]) for a well-formed
    input."""
    n = desc.numel() // DESC_DTYPE.itemsize
    assert want.dtype == torch.int32 and want.numel() >= n
    _check(L.load().jfs_zstd_decompress_prefix_device(desc.data_ptr(), want.data_ptr(), n, ret.data_ptr(),
                                                      _stream_ptr(stream)), "jfs_zstd_decompress_prefix_device")


def set_split_jump_rounds(lz4: int = 0, zstd: int = 0):
    """Test hook (jfs_test_set_split_jump_rounds): the pointer-jumping rounds
    the small-batch decoders launch, full and prefix; 0 = the computed count.
    Process-global: a test that sets it restores (0, 0)."""
    _check(L.load().jfs_test_set_split_jump_rounds(int(lz4), int(zstd)), "jfs_test_set_split_jump_rounds")


def lz4_compress_small(desc: torch.Tensor, ret: torch.Tensor, src_lens, stream=None):
    """jfs_lz4_compress_device_small: few blocks, each parsed as segments
    across the GPU (same bytes as lz4_compress); src_lens = host copies."""
    n = desc.numel() // DESC_DTYPE.itemsize
    sl = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in src_lens])
    _check(L.load().jfs_lz4_compress_device_small(desc.data_ptr(), sl, n, ret.data_ptr(), _stream_ptr(stream)),
           "jfs_lz4_compress_device_small")


def lz4_compress_fast(desc: torch.Tensor, ret: torch.Tensor, src_lens, stream=None):
    """jfs_lz4_compress_fast_device: the throughput encoder (independent 64 KiB
    chunks, 64 positions searched at once).  Valid LZ4 blocks, not liblz4's
    bytes; src_lens = host copies."""
    n = desc.numel() // DESC_DTYPE.itemsize
    sl = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in src_lens])
    _check(L.load().jfs_lz4_compress_fast_device(desc.data_ptr(), sl, n, ret.data_ptr(), _stream_ptr(stream)),
           "jfs_lz4_compress_fast_device")


LIFT_DTYPE = np.dtype([("src", "<i4"), ("src_chunk", "<i4")])  # jfs_lz4_lift


def lz4_compress_fast_lift(desc: torch.Tensor, ret: torch.Tensor, src_lens, lift: torch.Tensor, src_desc: torch.Tensor,
                           src_n: torch.Tensor, src_src_lens, src_caps, lifted: torch.Tensor | None = None, stream=None):
    """jfs_lz4_compress_fast_lift_device: lz4_compress_fast of gathered blocks
    whose chunks named in `lift` (LIFT_DTYPE records on the device, one per
    64 KiB chunk, flat) take their sequence records from the stored streams of
    the sources in src_desc (src_n: what each decoded to).  src_lens,
    src_src_lens and src_caps are host copies; `lifted` (int32, one per block)
    receives the chunks lifted."""
    n = desc.numel() // DESC_DTYPE.itemsize
    ns = src_desc.numel() // DESC_DTYPE.itemsize
    sl = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in src_lens])
    ssl = (ctypes.c_int32 * max(ns, 1))(*[int(x) for x in src_src_lens])
    scp = (ctypes.c_int32 * max(ns, 1))(*[int(x) for x in src_caps])
    _check(L.load().jfs_lz4_compress_fast_lift_device(
        desc.data_ptr(), sl, n, lift.data_ptr(), src_desc.data_ptr(), src_n.data_ptr(), ssl, scp, ns, ret.data_ptr(),
        lifted.data_ptr() if lifted is not None else None, _stream_ptr(stream)), "jfs_lz4_compress_fast_lift_device")


def zstd_decompress(desc: torch.Tensor, ret: torch.Tensor, stream=None):
    n = desc.numel() // DESC_DTYPE.itemsize
    _check(L.load().jfs_zstd_decompress_device(desc.data_ptr(), n, ret.data_ptr(), _stream_ptr(stream)),
           "jfs_zstd_decompress_device")


def zstd_decompress_sync(desc: torch.Tensor, ret: torch.Tensor, stream=None):
    """zstd_decompress, waited for.  The library sizes its scratch inside the
    call (include/jfs_gpucodec.h), so there is never anything to resubmit."""
    zstd_decompress(desc, ret, stream)
    torch.cuda.synchronize()


def zstd_compress(desc: torch.Tensor, ret: torch.Tensor, stream=None):
    n = desc.numel() // DESC_DTYPE.itemsize
    _check(L.load().jfs_zstd_compress_device(desc.data_ptr(), n, ret.data_ptr(), _stream_ptr(stream)),
           "jfs_zstd_compress_device")


def zstd_compress_fast(desc: torch.Tensor, ret: torch.Tensor, stream=None):
    """jfs_zstd_compress_fast_device: the throughput encoder (independent 64 KiB
    chunks, block-local repeat offsets).  Valid Zstd frames, not libzstd's
    bytes; host-synchronous like zstd_compress."""
    n = desc.numel() // DESC_DTYPE.itemsize
    _check(L.load().jfs_zstd_compress_fast_device(desc.data_ptr(), n, ret.data_ptr(), _stream_ptr(stream)),
           "jfs_zstd_compress_fast_device")


def zstd_compress_seekable(desc: torch.Tensor, ret: torch.Tensor, stream=None):
    """jfs_zstd_compress_seekable_device: the fast parse, one frame per 128 KiB
    block and a seek table behind them (inputs of one block at most: the fast
    call's frame).  Ordinary Zstd objects to every reader; host-synchronous."""
    n = desc.numel() // DESC_DTYPE.itemsize
    _check(L.load().jfs_zstd_compress_seekable_device(desc.data_ptr(), n, ret.data_ptr(), _stream_ptr(stream)),
           "jfs_zstd_compress_seekable_device")


def zstd_decompress_range(desc: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, ret: torch.Tensor, stream=None):
    """jfs_zstd_decompress_range_device: input i is decoded for its output bytes
    [lo[i], hi[i]) (int32 device tensors, one entry per descriptor) -- only the
    frames the range touches when the object has a seek table, a prefix decode
    with want = hi[i] when it has none."""
    n = desc.numel() // DESC_DTYPE.itemsize
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32 and lo.numel() >= n and hi.numel() >= n
    _check(L.load().jfs_zstd_decompress_range_device(desc.data_ptr(), lo.data_ptr(), hi.data_ptr(), n, ret.data_ptr(),
                                                     _stream_ptr(stream)), "jfs_zstd_decompress_range_device")


def zstd_decompress_ranges(desc: torch.Tensor, rng_first: torch.Tensor, rng: torch.Tensor, ret: torch.Tensor, stream=None):
    """jfs_zstd_decompress_ranges_device: input i is decoded for the output
    ranges rng[rng_first[i] .. rng_first[i + 1]) (int32 device tensors: n + 1
    running sums, and (lo, hi) pairs, flat or of shape (R, 2)) -- exactly the
    frames some range touches, through a seek table of either layout, decoded
    frames checked against a 12-byte table's checksums; a prefix decode to the
    largest hi when the object has no table."""
    n = desc.numel() // DESC_DTYPE.itemsize
    assert rng_first.dtype == torch.int32 and rng.dtype == torch.int32 and rng_first.numel() >= n + 1
    assert rng.is_contiguous() and rng.numel() % 2 == 0
    _check(L.load().jfs_zstd_decompress_ranges_device(desc.data_ptr(), rng_first.data_ptr(),
                                                      rng.data_ptr() if rng.numel() else None, n, ret.data_ptr(),
                                                      _stream_ptr(stream)), "jfs_zstd_decompress_ranges_device")


def lz4_decompress_ranges(desc: torch.Tensor, rng_first: torch.Tensor, rng: torch.Tensor, ret: torch.Tensor, src_lens,
                          dst_caps, stream=None):
    """jfs_lz4_decompress_ranges_device: block i is decoded for the output
    ranges rng[rng_first[i] .. rng_first[i + 1]) only (int32 device tensors, as
    for zstd_decompress_ranges), every requested byte by the origin chase;
    src_lens / dst_caps are host copies of the descriptors' sizes.  ret[i] =
    min(size, largest clamped hi) for a well-formed block."""
    n = desc.numel() // DESC_DTYPE.itemsize
    assert rng_first.dtype == torch.int32 and rng.dtype == torch.int32 and rng_first.numel() >= n + 1
    assert rng.is_contiguous() and rng.numel() % 2 == 0
    sl = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in src_lens])
    dc = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in dst_caps])
    _check(L.load().jfs_lz4_decompress_ranges_device(desc.data_ptr(), sl, dc, rng_first.data_ptr(),
                                                     rng.data_ptr() if rng.numel() else None, n, ret.data_ptr(),
                                                     _stream_ptr(stream)), "jfs_lz4_decompress_ranges_device")


def lz4_decompress_window(desc: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, ret: torch.Tensor, src_lens, dst_caps,
                          stream=None):
    """jfs_lz4_decompress_window_device_small: block i is decoded for its output
    bytes [lo[i], hi[i]) (int32 device tensors, one entry per descriptor) from
    the 64 KiB chunk boundary below lo[i] where the block's sequences allow it,
    else from byte 0; src_lens / dst_caps are host copies of the descriptors'
    sizes.  ret[i] = min(size, hi[i] clamped) for a well-formed block."""
    n = desc.numel() // DESC_DTYPE.itemsize
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32 and lo.numel() >= n and hi.numel() >= n
    sl = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in src_lens])
    dc = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in dst_caps])
    _check(L.load().jfs_lz4_decompress_window_device_small(desc.data_ptr(), sl, dc, lo.data_ptr(), hi.data_ptr(), n,
                                                           ret.data_ptr(), _stream_ptr(stream)),
           "jfs_lz4_decompress_window_device_small")


SPLICE_FRAME_DTYPE = np.dtype([("src", "<u8"), ("c", "<i4"), ("d", "<i4"), ("x", "<u4"), ("unit", "<i4"), ("out", "<i4"),
                               ("reserved", "<i4")])
SPLICE_OUT_DTYPE = np.dtype([("dst", "<u8"), ("dst_cap", "<i4"), ("frame_first", "<i4"), ("frame_count", "<i4"),
                             ("reserved", "<i4")])
assert SPLICE_FRAME_DTYPE.itemsize == ctypes.sizeof(L.JfsSpliceFrame)
assert SPLICE_OUT_DTYPE.itemsize == ctypes.sizeof(L.JfsSpliceOut)


def zstd_splice(outs: torch.Tensor, frames: torch.Tensor, unit_len: torch.Tensor | None,
                unit_hash: torch.Tensor | None, ret: torch.Tensor, stream=None):
    """jfs_zstd_splice_device: every output (a uint8 device tensor of
    SPLICE_OUT_DTYPE records) is assembled from its frames (SPLICE_FRAME_DTYPE
    records: PASS frames copied from stored bytes, FRESH ones from their encode
    unit's buffer with the length the encoder left in unit_len) and gets its
    seek table -- 12-byte entries with the low words of unit_hash (an int64
    tensor of XXH64 values) for the FRESH frames, 8-byte entries when unit_hash
    is None.  ret[j] = the object's size, 0 when it exceeds dst_cap, or a failed
    unit's verdict.  Asynchronous."""
    no = outs.numel() // SPLICE_OUT_DTYPE.itemsize
    nf = frames.numel() // SPLICE_FRAME_DTYPE.itemsize
    assert ret.dtype == torch.int32 and ret.numel() >= no
    assert unit_len is None or unit_len.dtype == torch.int32
    assert unit_hash is None or unit_hash.dtype == torch.int64
    _check(L.load().jfs_zstd_splice_device(outs.data_ptr(), no, frames.data_ptr() if nf else None, nf,
                                           unit_len.data_ptr() if unit_len is not None else None,
                                           unit_hash.data_ptr() if unit_hash is not None else None, ret.data_ptr(),
                                           _stream_ptr(stream)), "jfs_zstd_splice_device")


def zstd_seek_tables(desc: torch.Tensor, lens: torch.Tensor, slot_first: torch.Tensor, tables: torch.Tensor,
                     table_len: torch.Tensor, stream=None):
    """jfs_zstd_seek_tables_device: the seek table at the end of input i -- the
    lens[i] bytes at descriptor i's src (lens: an int32 device tensor, negative
    for "no input") -- goes to tables[slot_first[i] : slot_first[i + 1]] (int32
    device tensor of n + 1 multiples of 16; tables: uint8) and its bytes to
    table_len[i]; 0, and nothing written, without a table that fits.
    Asynchronous."""
    n = desc.numel() // DESC_DTYPE.itemsize
    assert lens.dtype == torch.int32 and slot_first.dtype == torch.int32 and table_len.dtype == torch.int32
    assert lens.numel() >= n and slot_first.numel() >= n + 1 and table_len.numel() >= n and tables.dtype == torch.uint8
    _check(L.load().jfs_zstd_seek_tables_device(desc.data_ptr(), lens.data_ptr(), n, slot_first.data_ptr(),
                                                tables.data_ptr(), table_len.data_ptr(), _stream_ptr(stream)),
           "jfs_zstd_seek_tables_device")


def xxh64(desc: torch.Tensor, hash: torch.Tensor, ret: torch.Tensor | None = None, stream=None):
    """jfs_xxh64_device: hash[i] (an int64 device tensor holding the uint64
    bits) = XXH64, seed 0, of descriptor i's src[0, src_len); ret[i] (int32,
    optional) = 0, or -1 for a bad descriptor."""
    n = desc.numel() // DESC_DTYPE.itemsize
    assert hash.dtype == torch.int64 and hash.numel() >= n
    _check(L.load().jfs_xxh64_device(desc.data_ptr(), n, hash.data_ptr(), ret.data_ptr() if ret is not None else None,
                                     _stream_ptr(stream)), "jfs_xxh64_device")


def zstd_compress_seekable_csum(desc: torch.Tensor, ret: torch.Tensor, stream=None):
    """jfs_zstd_compress_seekable_csum_device: zstd_compress_seekable's frames,
    then a table of 12-byte entries whose third word is the low half of XXH64
    of the frame's content.  Host-synchronous."""
    n = desc.numel() // DESC_DTYPE.itemsize
    _check(L.load().jfs_zstd_compress_seekable_csum_device(desc.data_ptr(), n, ret.data_ptr(), _stream_ptr(stream)),
           "jfs_zstd_compress_seekable_csum_device")


FRAG_DTYPE = np.dtype([("table", "<u8"), ("table_len", "<i4"), ("object_len", "<i4"),
                       ("frag", "<u8"), ("frag_off", "<i4"), ("frag_len", "<i4"),
                       ("dst", "<u8"), ("dst_cap", "<i4"), ("reserved", "<i4")])
assert FRAG_DTYPE.itemsize == ctypes.sizeof(L.JfsSeekFrag)


def make_frag_desc(buf: torch.Tensor, table_offs, table_lens, object_lens, frag_offs_in_buf, frag_offs, frag_lens,
                   dst: torch.Tensor, dst_offs, dst_caps) -> torch.Tensor:
    """Build a device tensor of jfs_seek_frag descriptors (48 bytes each): the
    tables and fragments lie in `buf` at table_offs / frag_offs_in_buf; frag_offs
    are the fragments' positions in their objects.  An offset of None gives a
    NULL pointer."""
    n = len(table_offs)
    a = np.zeros(n, dtype=FRAG_DTYPE)

    def ptrs(t, offs):
        return np.asarray([0 if o is None else t.data_ptr() + o for o in offs], dtype=np.uint64)
    a["table"] = ptrs(buf, table_offs)
    a["frag"] = ptrs(buf, frag_offs_in_buf)
    a["dst"] = ptrs(dst, dst_offs)
    a["table_len"] = np.asarray(table_lens, dtype=np.int32)
    a["object_len"] = np.asarray(object_lens, dtype=np.int32)
    a["frag_off"] = np.asarray(frag_offs, dtype=np.int32)
    a["frag_len"] = np.asarray(frag_lens, dtype=np.int32)
    a["dst_cap"] = np.asarray(dst_caps, dtype=np.int32)
    return torch.from_numpy(a.view(np.uint8).copy()).to(buf.device)


def zstd_decompress_frames(desc: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, ret: torch.Tensor, stream=None):
    """jfs_zstd_decompress_frames_device: input i (make_frag_desc) is decoded for
    its content bytes [lo[i], hi[i]) from its table and a fragment of its
    frames; with a checksummed table every decoded frame is verified (-4)."""
    n = desc.numel() // FRAG_DTYPE.itemsize
    assert lo.dtype == torch.int32 and hi.dtype == torch.int32 and lo.numel() >= n and hi.numel() >= n
    _check(L.load().jfs_zstd_decompress_frames_device(desc.data_ptr(), lo.data_ptr(), hi.data_ptr(), n, ret.data_ptr(),
                                                      _stream_ptr(stream)), "jfs_zstd_decompress_frames_device")


def crc32c(desc: torch.Tensor, crc: torch.Tensor | None = None, ret: torch.Tensor | None = None,
           seg_bytes: int = 0, stream=None):
    """CRC-32C per descriptor (jfs_crc32c_device): whole-block values into
    `crc` (uint32 as int32 tensor), per-segment big-endian sums into each dst."""
    n = desc.numel() // DESC_DTYPE.itemsize
    _check(L.load().jfs_crc32c_device(desc.data_ptr(), n, seg_bytes, crc.data_ptr() if crc is not None else None,
                                      ret.data_ptr() if ret is not None else None, _stream_ptr(stream)),
           "jfs_crc32c_device")


AEAD_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("src_len", "<i4"), ("dst_cap", "<i4"),
                       ("key", "<u8"), ("nonce", "<u8")])


def make_aead_desc(src: torch.Tensor, src_offs, src_lens, dst: torch.Tensor, dst_offs, dst_caps,
                   kn: torch.Tensor, key_offs, nonce_offs) -> torch.Tensor:
    """jfs_aead_block descriptors (40 bytes each); keys and nonces live in `kn`."""
    a = np.zeros(len(src_offs), dtype=AEAD_DTYPE)
    a["src"] = src.data_ptr() + np.asarray(src_offs, dtype=np.uint64)
    a["dst"] = dst.data_ptr() + np.asarray(dst_offs, dtype=np.uint64)
    a["src_len"] = np.asarray(src_lens, dtype=np.int32)
    a["dst_cap"] = np.asarray(dst_caps, dtype=np.int32)
    a["key"] = kn.data_ptr() + np.asarray(key_offs, dtype=np.uint64)
    a["nonce"] = kn.data_ptr() + np.asarray(nonce_offs, dtype=np.uint64)
    return torch.from_numpy(a.view(np.uint8).copy()).to(src.device)


def aes256gcm(desc: torch.Tensor, ret: torch.Tensor, seal: bool, stream=None):
    """AES-256-GCM seal (True) or open (False) per jfs_aead_block descriptor."""
    n = desc.numel() // AEAD_DTYPE.itemsize
    lib = L.load()
    fn = lib.jfs_aes256gcm_seal_device if seal else lib.jfs_aes256gcm_open_device
    _check(fn(desc.data_ptr(), n, ret.data_ptr(), _stream_ptr(stream)), "jfs_aes256gcm")


CIPHERS = {"aes256gcm": L.CIPHER_AES256GCM, "chacha20": L.CIPHER_CHACHA20POLY1305, "sm4gcm": L.CIPHER_SM4GCM}


def aead(cipher: str, desc: torch.Tensor, ret: torch.Tensor, seal: bool, stream=None):
    """Seal (True) or open (False) with aes256gcm / chacha20 / sm4gcm per descriptor
    (jfs_aead_{seal,open}_device)."""
    n = desc.numel() // AEAD_DTYPE.itemsize
    lib = L.load()
    fn = lib.jfs_aead_seal_device if seal else lib.jfs_aead_open_device
    _check(fn(CIPHERS[cipher], desc.data_ptr(), n, ret.data_ptr(), _stream_ptr(stream)), "jfs_aead")


JFS_CHAIN_FAILED = -(1 << 31)  # the first step of a fused chain failed for this block


def lz4_compress_seal(comp_desc: torch.Tensor, aead_desc: torch.Tensor, ret_comp: torch.Tensor, ret: torch.Tensor,
                      stream=None):
    """Fused LZ4 compress -> AES-256-GCM seal (jfs_lz4_compress_seal_device)."""
    n = comp_desc.numel() // DESC_DTYPE.itemsize
    _check(L.load().jfs_lz4_compress_seal_device(comp_desc.data_ptr(), aead_desc.data_ptr(), n, ret_comp.data_ptr(),
                                                 ret.data_ptr(), _stream_ptr(stream)), "jfs_lz4_compress_seal_device")


def open_lz4_decompress(aead_desc: torch.Tensor, dec_desc: torch.Tensor, ret_open: torch.Tensor, ret: torch.Tensor,
                        stream=None):
    """Fused AES-256-GCM open -> LZ4 decompress (jfs_open_lz4_decompress_device)."""
    n = dec_desc.numel() // DESC_DTYPE.itemsize
    _check(L.load().jfs_open_lz4_decompress_device(aead_desc.data_ptr(), dec_desc.data_ptr(), n, ret_open.data_ptr(),
                                                   ret.data_ptr(), _stream_ptr(stream)), "jfs_open_lz4_decompress_device")


SEG_DTYPE = np.dtype([("src", "<i4"), ("src_off", "<i4"), ("dst_off", "<i4"), ("len", "<i4")])
COMPACT_OUT_DTYPE = np.dtype([("dst", "<u8"), ("dst_cap", "<i4"), ("seg_first", "<i4"), ("seg_count", "<i4"),
                              ("reserved", "<i4")])
assert SEG_DTYPE.itemsize == ctypes.sizeof(L.JfsCompactSeg)
assert COMPACT_OUT_DTYPE.itemsize == ctypes.sizeof(L.JfsCompactOut)


def make_compact_desc(dst: torch.Tensor, dst_offs, dst_caps, seg_first, seg):
    """Device tensors for a gather plan: (jfs_compact_out descriptors, one per
    output block at dst[dst_offs[j] : +dst_caps[j]]; jfs_compact_seg records).
    seg_first has one entry per block plus one; seg = [(src, src_off, dst_off, len)]."""
    n = len(dst_offs)
    o = np.zeros(n, dtype=COMPACT_OUT_DTYPE)
    o["dst"] = dst.data_ptr() + np.asarray(dst_offs, dtype=np.uint64)
    o["dst_cap"] = np.asarray(dst_caps, dtype=np.int32)
    first = np.asarray(seg_first, dtype=np.int32)
    o["seg_first"] = first[:n]
    o["seg_count"] = first[1:n + 1] - first[:n]
    s = np.zeros(max(len(seg), 1), dtype=SEG_DTYPE)
    if len(seg):
        a = np.asarray(seg, dtype=np.int32).reshape(-1, 4)
        s["src"], s["src_off"], s["dst_off"], s["len"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return (torch.from_numpy(o.view(np.uint8).copy()).to(dst.device),
            torch.from_numpy(s.view(np.uint8).copy()).to(dst.device))


def gather(src_desc: torch.Tensor, src_n: torch.Tensor, out_desc: torch.Tensor, seg: torch.Tensor, max_dst_cap: int,
           ret: torch.Tensor, stream=None):
    """jfs_gather_device: src_desc = jfs_dev_block per decoded source (its dst /
    dst_cap), src_n = their decoded lengths (int32, negative = failed)."""
    ns = src_desc.numel() // DESC_DTYPE.itemsize
    no = out_desc.numel() // COMPACT_OUT_DTYPE.itemsize
    _check(L.load().jfs_gather_device(src_desc.data_ptr(), src_n.data_ptr(), ns, out_desc.data_ptr(), no,
                                      seg.data_ptr(), int(max_dst_cap), ret.data_ptr(), _stream_ptr(stream)),
           "jfs_gather_device")


def read_gather(src_desc: torch.Tensor, src_n: torch.Tensor, out_desc: torch.Tensor, seg: torch.Tensor, dst_caps,
                ret: torch.Tensor, stream=None):
    """jfs_read_gather_device: gather()'s contract on the flat grid, for
    outputs of very different sizes; dst_caps = the outputs' dst_cap on the host."""
    ns = src_desc.numel() // DESC_DTYPE.itemsize
    no = out_desc.numel() // COMPACT_OUT_DTYPE.itemsize
    caps = np.ascontiguousarray(dst_caps, dtype=np.int32)
    if caps.size != no:
        raise ValueError("one dst_cap per output")
    _check(L.load().jfs_read_gather_device(src_desc.data_ptr(), src_n.data_ptr(), ns, out_desc.data_ptr(),
                                           caps.ctypes.data, no, seg.data_ptr(), ret.data_ptr(),
                                           _stream_ptr(stream)), "jfs_read_gather_device")


def read_csum(out_desc: torch.Tensor, ret: torch.Tensor, piece_first: torch.Tensor, npiece: int, csum: torch.Tensor,
              stream=None):
    """jfs_read_csum_device: the big-endian CRC-32C of every 32 KiB piece of the
    gathered reads whose verdict in `ret` is their dst_cap; piece_first (int32,
    one entry per read plus one) and its last entry npiece size the flat grid,
    piece p goes to csum[4p:4p+4]."""
    no = out_desc.numel() // COMPACT_OUT_DTYPE.itemsize
    if piece_first.numel() != no + 1 or csum.numel() * csum.element_size() < 4 * npiece:
        raise ValueError("piece_first needs one entry per read plus one, csum 4 bytes per piece")
    _check(L.load().jfs_read_csum_device(out_desc.data_ptr(), ret.data_ptr(), no, piece_first.data_ptr(), int(npiece),
                                         csum.data_ptr(), _stream_ptr(stream)), "jfs_read_csum_device")


def lz4_compact(src_desc: torch.Tensor, src_ret: torch.Tensor, gather_desc: torch.Tensor, seg: torch.Tensor,
                enc_desc: torch.Tensor, max_dst_cap: int, ret: torch.Tensor, stream=None):
    """Fused LZ4 decode -> gather -> LZ4 encode (jfs_lz4_compact_device)."""
    ns = src_desc.numel() // DESC_DTYPE.itemsize
    no = gather_desc.numel() // COMPACT_OUT_DTYPE.itemsize
    _check(L.load().jfs_lz4_compact_device(src_desc.data_ptr(), ns, src_ret.data_ptr(), gather_desc.data_ptr(),
                                           seg.data_ptr(), enc_desc.data_ptr(), no, int(max_dst_cap), ret.data_ptr(),
                                           _stream_ptr(stream)), "jfs_lz4_compact_device")


def gen_blocks(out: torch.Tensor, nblk: int, block_bytes: int, cls: str, seed_base: int, stream=None):
    """Fill out[0 : nblk*block_bytes] with synthetic blocks."""
    assert out.numel() >= nblk * block_bytes
    _check(L.load().jfs_gen_blocks_device(out.data_ptr(), nblk, block_bytes, cls.encode(), seed_base,
                                          _stream_ptr(stream)), "jfs_gen_blocks_device")


def lz4_bound(n: int) -> int:
    return n + n // 255 + 16


class Lz4Batch:
    """A batch of equal-size blocks resident in HBM: raw, compressed, decoded.

    Compressed block i lives at comp[i*slot : i*slot + csize[i]] with
    slot = bound rounded up to 256 bytes (16-byte aligned slots).
    """

    def __init__(self, nblk: int, block_bytes: int, cls: str = "T", seed_base: int = 1, device="cuda"):
        self.nblk, self.U = nblk, block_bytes
        self.slot = (lz4_bound(block_bytes) + 255) // 256 * 256
        self.device = torch.device(device)
        self.raw = torch.empty(nblk * block_bytes, dtype=torch.uint8, device=self.device)
        gen_blocks(self.raw, nblk, block_bytes, cls, seed_base)
        self.comp = torch.empty(nblk * self.slot, dtype=torch.uint8, device=self.device)
        self.ret = torch.empty(nblk, dtype=torch.int32, device=self.device)
        offs = np.arange(nblk, dtype=np.int64)
        self.enc_desc = make_desc(self.raw, offs * block_bytes, [block_bytes] * nblk, self.comp, offs * self.slot,
                                  [self.slot] * nblk)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lz4_compress(self.enc_desc, self.ret)
        e1.record()
        torch.cuda.synchronize()
        self.enc_ms = e0.elapsed_time(e1)  # one GPU LZ4 encode launch over the whole batch
        self.csize = self.ret.cpu().numpy().astype(np.int64)
        if (self.csize <= 0).any():
            raise RuntimeError("device LZ4 compression failed")
        self.out = torch.empty(nblk * block_bytes, dtype=torch.uint8, device=self.device)
        self.dec_desc = make_desc(self.comp, offs * self.slot, self.csize, self.out, offs * block_bytes,
                                  [block_bytes] * nblk)
        self.dec_ret = torch.empty(nblk, dtype=torch.int32, device=self.device)

    def decompress(self, stream=None):
        lz4_decompress(self.dec_desc, self.dec_ret, stream)

    def compress(self, stream=None):
        """Re-encode raw -> comp (same bytes and sizes as the first encode)."""
        lz4_compress(self.enc_desc, self.ret, stream)

    @property
    def comp_bytes(self) -> int:
        return int(self.csize.sum())

    def verify(self) -> bool:
        torch.cuda.synchronize()
        ok = bool((self.dec_ret == self.U).all().item())
        ok = ok and bool((self.ret.cpu().numpy().astype(np.int64) == self.csize).all())
        return ok and bool(torch.equal(self.out, self.raw))


def zstd_bound(n: int) -> int:
    return n + (n >> 8) + (((128 << 10) - n) >> 11 if n < (128 << 10) else 0)


def zstd_compress_rate(nblk: int, block_bytes: int, cls: str = "T", seed_base: int = 1, device="cuda"):
    """Time one GPU Zstd encode launch over nblk synthetic blocks in HBM and
    check every frame with the GPU decoder.  Returns (GiB/s, ratio, ms)."""
    dev = torch.device(device)
    raw = torch.empty(nblk * block_bytes, dtype=torch.uint8, device=dev)
    gen_blocks(raw, nblk, block_bytes, cls, seed_base)
    slot = (zstd_bound(block_bytes) + 255) // 256 * 256
    comp = torch.empty(nblk * slot, dtype=torch.uint8, device=dev)
    offs = np.arange(nblk, dtype=np.int64)
    desc = make_desc(raw, offs * block_bytes, [block_bytes] * nblk, comp, offs * slot, [slot] * nblk)
    ret = torch.empty(nblk, dtype=torch.int32, device=dev)
    zstd_compress(desc, ret)  # warm-up (scratch allocation)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    zstd_compress(desc, ret)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    csize = ret.cpu().numpy().astype(np.int64)
    if (csize <= 0).any():
        raise RuntimeError("device Zstd compression failed")
    out = torch.empty(nblk * block_bytes, dtype=torch.uint8, device=dev)
    ddesc = make_desc(comp, offs * slot, csize, out, offs * block_bytes, [block_bytes] * nblk)
    dret = torch.empty(nblk, dtype=torch.int32, device=dev)
    zstd_decompress_sync(ddesc, dret)
    if not (bool((dret == block_bytes).all().item()) and torch.equal(out, raw)):
        raise RuntimeError("Zstd round trip mismatch")
    return nblk * block_bytes / (ms / 1e3) / 2**30, nblk * block_bytes / float(csize.sum()), ms


def _libzstd():
    """The system libzstd (data generator for benchmarks only: it produces the
    level-3 frames the GPU decodes; nothing on the product path uses it)."""
    for path in ("/opt/conda/lib/libzstd.so.1", "/usr/lib/x86_64-linux-gnu/libzstd.so.1"):
        try:
            z = ctypes.CDLL(path)
        except OSError:
            continue
        z.ZSTD_compress.restype = ctypes.c_size_t
        z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        z.ZSTD_compressBound.restype = ctypes.c_size_t
        z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
        z.ZSTD_isError.restype = ctypes.c_uint
        z.ZSTD_isError.argtypes = [ctypes.c_size_t]
        z.ZSTD_decompress.restype = ctypes.c_size_t
        z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        z.path = path
        return z
    return None


class ZstdBatch:
    """nblk Zstd frames (level `level`, block_bytes each) resident in HBM.

    `distinct` different blocks are generated (GPU generator) and compressed
    with the system libzstd on the host, then replicated over the nblk slots
    (the GPU sees nblk independent frames; the bench uses 256 distinct frames,
    ~300 MB of compressed input, beyond the 256 MB MALL).  Slot = max frame size rounded up to 256 B.
    """

    def __init__(self, nblk: int, block_bytes: int, cls: str = "T", level: int = 3, distinct: int = 16,
                 seed_base: int = 1, device="cuda", cache_dir: str | None = None):
        from .blockgen import gen_block
        self.nblk, self.U, self.level = nblk, block_bytes, level
        self.device = torch.device(device)
        distinct = min(distinct, nblk)
        raws, frames = [], []
        cache = None
        if cache_dir:
            cache = os.path.join(cache_dir, f"zstd_{cls}_{block_bytes}_{level}_{distinct}_{seed_base}.npz")
        # the raw blocks come from the GPU generator (the host one takes ~0.5 s
        # per 4 MiB text block); frames from host libzstd on a thread pool
        # (ctypes drops the GIL inside ZSTD_compress)
        raw_t = torch.empty(distinct * block_bytes, dtype=torch.uint8, device=self.device)
        gen_blocks(raw_t, distinct, block_bytes, cls, seed_base)
        raw_np = raw_t.cpu().numpy()
        raws = [raw_np[i * block_bytes:(i + 1) * block_bytes].tobytes() for i in range(distinct)]
        del raw_t
        if cache and os.path.exists(cache):
            with np.load(cache) as f:  # our own file (allow_pickle stays False)
                blob, lens = f["blob"], f["lens"]
            o = 0
            for n in lens:
                frames.append(blob[o:o + n].tobytes())
                o += n
        else:
            z = _libzstd()
            if z is None:
                raise RuntimeError("no libzstd on this host to generate frames")

            def one(src):
                cap = z.ZSTD_compressBound(len(src))
                dst = ctypes.create_string_buffer(cap)
                n = z.ZSTD_compress(dst, cap, src, len(src), level)
                if z.ZSTD_isError(n):
                    raise RuntimeError("ZSTD_compress failed")
                return dst.raw[:n]
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:
                frames = list(ex.map(one, raws))
            if cache:
                os.makedirs(cache_dir, exist_ok=True)
                np.savez(cache, blob=np.frombuffer(b"".join(frames), dtype=np.uint8),
                         lens=np.array([len(f) for f in frames], dtype=np.int64))
        self.frames = frames
        self.slot = (max(len(f) for f in frames) + 255) // 256 * 256
        host = np.zeros(nblk * self.slot, dtype=np.uint8)
        self.csize = np.zeros(nblk, dtype=np.int64)
        for i in range(nblk):
            f = frames[i % distinct]
            host[i * self.slot:i * self.slot + len(f)] = np.frombuffer(f, dtype=np.uint8)
            self.csize[i] = len(f)
        self.comp = torch.from_numpy(host).to(self.device)
        self.raw = torch.from_numpy(np.frombuffer(b"".join(raws), dtype=np.uint8).copy()).to(self.device)
        self.distinct = distinct
        self.out = torch.empty(nblk * block_bytes, dtype=torch.uint8, device=self.device)
        offs = np.arange(nblk, dtype=np.int64)
        self.dec_desc = make_desc(self.comp, offs * self.slot, self.csize, self.out, offs * block_bytes,
                                  [block_bytes] * nblk)
        self.dec_ret = torch.empty(nblk, dtype=torch.int32, device=self.device)
        zstd_decompress_sync(self.dec_desc, self.dec_ret)  # sizes the device scratch for this batch

    def decompress(self, stream=None):
        zstd_decompress(self.dec_desc, self.dec_ret, stream)

    @property
    def comp_bytes(self) -> int:
        return int(self.csize.sum())

    def verify(self) -> bool:
        torch.cuda.synchronize()
        if not bool((self.dec_ret == self.U).all().item()):
            return False
        U, d = self.U, self.distinct
        for i in range(self.nblk):
            j = i % d
            if not torch.equal(self.out[i * U:(i + 1) * U], self.raw[j * U:(j + 1) * U]):
                return False
        return True
