"""Python mirror of JuiceFS pkg/compress over libjfsgpu.so.

Same names, argument meaning and error behaviour as
/root/reference/pkg/compress/compress.go so the parity tests read like the
reference's own compress_test.go:

    ZSTD_LEVEL = 1                                   compress.go:28
    class Compressor (Name / CompressBound / Compress / Decompress)   :31-36
    NewCompressor(algr) -> Compressor | None        :39-49
    noOp / ZStandard / LZ4                           :51-125

Go's ``(int, error)`` results become ``(n, err)`` tuples with ``err`` either
``None`` or a :class:`CompressError`.  ``dst`` must be a writable buffer
(bytearray / memoryview / numpy array); ``src`` any bytes-like object.  For
Zstd the capacity is ``len(dst)`` (Go passes ``cap(dst)``).

Every LZ4 byte is produced by the HIP kernels in libjfsgpu.so; there is no CPU
fallback (the library returns ``JFS_ERR_NO_DEVICE`` without a gfx950 GPU).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
# the run-time switches (read_seek_mode, set_read_seek_mode, zstd_parse_mode, lz4_chase_max, ...: switches.__all__),
# built from the one table in switches.py, and the two counter readers that belong here
from .switches import *  # noqa: F401,F403
from .switches import compact_lz4_lift_counts, compact_splice_counts  # noqa: F401

ZSTD_LEVEL = 1


class CompressError(Exception):
    def __init__(self, msg: str, code: int):
        super().__init__(msg)
        self.code = code


def _addr(buf, writable: bool):
    """Return (c_void_p, length, keepalive) for a buffer."""
    if buf is None:
        return None, 0, None
    # fast paths for the common types (a batch of 4,096 blocks spends
    # milliseconds here): the bytearray's own buffer / the bytes' own buffer
    t = type(buf)
    if t is bytearray and len(buf):
        c = ctypes.c_char.from_buffer(buf)
        return ctypes.c_void_p(ctypes.addressof(c)), len(buf), c
    if t is bytes and len(buf) and not writable:
        c = ctypes.c_char_p(buf)
        return ctypes.cast(c, ctypes.c_void_p), len(buf), (c, buf)
    mv = memoryview(buf)
    if not mv.contiguous:
        raise ValueError("buffer must be contiguous")
    mv = mv.cast("B")
    n = mv.nbytes
    if n == 0:
        return None, 0, mv
    if writable and mv.readonly:
        raise ValueError("dst must be writable")
    # address the buffer in place (no copy); numpy's view is much cheaper than
    # a per-call ctypes array type, which matters with 200 concurrent callers
    a = np.frombuffer(mv, dtype=np.uint8)
    return ctypes.c_void_p(a.ctypes.data), n, (mv, a)


def _err(code: int, dst_len: int, src_len: int, op: str) -> CompressError:
    if code == L.JFS_ERR_SHORT_BUFFER:
        return CompressError(f"buffer too short: {dst_len} < {src_len}", code)
    if code == L.JFS_ERR_EMPTY_INPUT:
        return CompressError("decompress an empty input", code)
    if code == L.JFS_ERR_COMPRESS_FAIL:
        return CompressError("lz4: compression failed (destination too small)", code)
    if code == L.JFS_ERR_CORRUPT:
        return CompressError("zstd: corrupted frame", code)
    if code == L.JFS_ERR_UNSUPPORTED:
        return CompressError(f"{op}: not supported by the GPU engine", code)
    if code == L.JFS_ERR_NO_DEVICE:
        return CompressError("no usable gfx950 device", code)
    if code <= L.JFS_ERR_BASE:
        return CompressError(f"{op}: error {code}", code)
    return CompressError(f"lz4: decompress failed ({code})", code)


class Compressor:
    """compress.go:31-36"""

    algo: int = -1

    def Name(self) -> str:
        return L.load().jfs_codec_name(self.algo).decode()

    def CompressBound(self, n: int) -> int:
        return int(L.load().jfs_compress_bound(self.algo, n))

    def Compress(self, dst, src):
        d, dn, kd = _addr(dst, True)
        s, sn, ks = _addr(src, False)
        r = int(L.load().jfs_compress(self.algo, d, dn, s, sn))
        if r < 0:
            return 0, _err(r, dn, sn, "compress")
        return r, None

    def Decompress(self, dst, src):
        d, dn, kd = _addr(dst, True)
        s, sn, ks = _addr(src, False)
        r = int(L.load().jfs_decompress(self.algo, d, dn, s, sn))
        if r < 0:
            # LZ4 passes LZ4_decompress_safe's negative value through (compress.go:124);
            # the other adapters return 0 with the error (compress.go:57-100).
            n = r if (self.algo == L.ALGO_LZ4 and r > L.JFS_ERR_BASE) else 0
            return n, _err(r, dn, sn, "decompress")
        return r, None

    # batch helpers (host buffers) -------------------------------------------
    def CompressBatch(self, pairs, device_mask: int = 0):
        return _batch(self.algo, pairs, device_mask, compress=True)

    def DecompressBatch(self, pairs, device_mask: int = 0):
        return _batch(self.algo, pairs, device_mask, compress=False)

    def DecompressBatchChecksum(self, pairs, device_mask: int = 0):
        """DecompressBatch plus each decoded block's disk-cache checksum
        (checksum() of pkg/chunk/disk_cache_file.go:139-152, written beside the
        block by disk_cache.go:536-537), computed on the GPU: [(n, err, csum)]"""
        return _batch(self.algo, pairs, device_mask, compress=False, with_csum=True)

    def CompressBatchChecksum(self, pairs, device_mask: int = 0):
        """CompressBatch plus each payload's CRC-32C (generateChecksum,
        pkg/object/checksum.go:30-45): [(n, err, crc)]"""
        return _batch(self.algo, pairs, device_mask, compress=True, with_crc=True)

    def CompactBatch(self, sources, outputs, plan, device_mask: int = 0, with_crc: bool = False):
        """Slice compaction on one GPU (jfs_compact_batch): decode the stored
        source objects, gather the planned byte ranges into new blocks and
        compress those, without a decoded byte leaving HBM.

        sources: list of (stored_object, block_size); outputs: list of writable
        dst buffers, one per new block; plan: (seg_first, seg) as compact_plan
        returns them, seg entries (src, src_off, dst_off, len) with src = -1
        for a hole.  Returns (src_results, out_results[, crcs]): [(n, err)] as
        DecompressBatch would give for the sources and as CompressBatch would
        give for the gathered blocks (JFS_ERR_CORRUPT for a block fed by a
        failed or short source), plus each payload's CRC-32C with with_crc."""
        lib = L.load()
        seg_first, seg = plan
        ns, no = len(sources), len(outputs)
        if len(seg_first) != no + 1:
            raise ValueError("seg_first must have one entry per output plus one")
        siov, oiov = (L.JfsIov * max(ns, 1))(), (L.JfsIov * max(no, 1))()
        keep = []
        for i, (obj, block_size) in enumerate(sources):
            s, sn, ks = _addr(obj, False)
            keep.append(ks)
            siov[i].src, siov[i].src_len, siov[i].dst, siov[i].dst_cap = s, sn, None, int(block_size)
        for j, dst in enumerate(outputs):
            d, dn, kd = _addr(dst, True)
            keep.append(kd)
            oiov[j].src, oiov[j].src_len, oiov[j].dst, oiov[j].dst_cap = None, 0, d, dn
        first = (ctypes.c_int32 * (no + 1))(*[int(x) for x in seg_first])
        segs = (L.JfsCompactSeg * max(len(seg), 1))()
        for k, (src, src_off, dst_off, n) in enumerate(seg):
            segs[k].src, segs[k].src_off, segs[k].dst_off, segs[k].len = int(src), int(src_off), int(dst_off), int(n)
        src_n, out_n = (ctypes.c_int64 * max(ns, 1))(), (ctypes.c_int64 * max(no, 1))()
        crc = (ctypes.c_uint32 * max(no, 1))()
        rc = lib.jfs_compact_batch(self.algo, ns, siov, no, oiov, first, segs, src_n, out_n, crc if with_crc else None,
                                   device_mask)
        if rc != 0:
            raise _err(rc, 0, 0, "compact")
        src_res, out_res = [], []
        for i in range(ns):
            r = int(src_n[i])
            if r < 0:
                n = r if (self.algo == L.ALGO_LZ4 and r > L.JFS_ERR_BASE) else 0
                src_res.append((n, _err(r, siov[i].dst_cap, siov[i].src_len, "decompress")))
            else:
                src_res.append((r, None))
        for j in range(no):
            r = int(out_n[j])
            total = sum(s[3] for s in seg[seg_first[j]:seg_first[j + 1]])
            out_res.append((0, _err(r, oiov[j].dst_cap, total, "compress")) if r < 0 else (r, None))
        if with_crc:
            return src_res, out_res, [int(crc[j]) for j in range(no)]
        return src_res, out_res

    def ReadBatch(self, sources, reads, plan, crcs=None, device_mask: int = 0, with_csum=False):
        """Read assembly on one GPU (jfs_read_batch): check the stored source
        objects against their CRC-32C, decode them and gather the planned byte
        ranges, so that only the requested bytes come back over the host link.

        sources: list of (stored_object, block_size); reads: list of writable
        dst buffers, one per read; plan: (seg_first, seg) as read_plan returns
        them; crcs: None, or one expected CRC-32C per source (None or -1: no
        checksum, verifyChecksum with "").  Returns (src_results, read_results,
        crc_got): [(n, err)] as DecompressBatch would give for the sources
        ("verify checksum failed" where the CRC differs), [(n, err)] per read
        (JFS_ERR_CORRUPT for a read fed by a failed or short source; its dst is
        untouched) and the computed CRC of every source that had an expected
        one.  read_expect gives the bytes a good read holds.

        with_csum (jfs_read_batch_csum): True, or per read True, False / None
        or a writable buffer of csum_bytes(total) bytes that receives the
        checksum in place.  The result gains a fourth list: per read its
        disk-cache checksum bytes (the big-endian CRC-32C of every 32 KiB
        piece, csum_bytes(n) bytes), None for a failed read and for a read
        that asked for none."""
        return _read_call(self.algo, None, sources, None, reads, plan, crcs, device_mask, with_csum)


class noOp(Compressor):  # noqa: N801  (reference name, compress.go:51)
    algo = L.ALGO_NONE


class ZStandard(Compressor):
    """compress.go:70-103; level is fixed at ZSTD_LEVEL (1)."""

    algo = L.ALGO_ZSTD

    def __init__(self, level: int = ZSTD_LEVEL):
        self.level = level

    def LoadRangeBatch(self, reads, device_mask: int = 0):
        """jfs_zstd_load_range_batch: reads = [(dst, table, object_len, frag,
        frag_off, lo, hi, block_size)], the table and the fragment of a seekable
        object as seek_plan says to fetch them; dst receives the content bytes
        [max(lo, 0), min(D, hi, block_size)).  Returns [(n, err)] per read; only
        tables and fragments go to the GPU and only those bytes come back."""
        n = len(reads)
        arr = (L.JfsRangeRead * max(n, 1))()
        keep = []
        for i, (dst, table, object_len, frag, frag_off, lo, hi, block_size) in enumerate(reads):
            dp, dn, k0 = _addr(dst, True)
            tp, tn, k1 = _addr(table, False)
            fp, fn, k2 = _addr(frag, False)
            keep.append((k0, k1, k2))
            arr[i] = L.JfsRangeRead(tp, tn, object_len, fp, frag_off, fn, lo, hi, block_size, dp, dn)
        out = (ctypes.c_int64 * max(n, 1))()
        rc = L.load().jfs_zstd_load_range_batch(n, arr, out, device_mask)
        if rc != 0:
            raise _err(rc, 0, 0, "LoadRangeBatch")
        res = []
        for i in range(n):
            if out[i] >= 0:
                res.append((int(out[i]), None))
            elif out[i] == L.JFS_ERR_CHECKSUM:
                res.append((0, CompressError("zstd: a frame's content does not match its seek-table checksum", out[i])))
            else:
                res.append((0, _err(out[i], len(reads[i][0]), reads[i][6] - max(reads[i][5], 0), "LoadRangeBatch")))
        return res


class LZ4(Compressor):
    """compress.go:105-125"""

    algo = L.ALGO_LZ4


def NewCompressor(algr: str):
    """compress.go:39-49: case-insensitive "zstd" / "lz4" / "none" / ""; else None."""
    a = L.load().jfs_codec_from_name(algr.encode())
    if a == L.ALGO_ZSTD:
        return ZStandard(ZSTD_LEVEL)
    if a == L.ALGO_LZ4:
        return LZ4()
    if a == L.ALGO_NONE:
        return noOp()
    return None


def lz4_fast_host(src) -> bytes:
    """The fast encoder's host twin (jfs_test_lz4_fast_host, test
    infrastructure): the bytes jfs_lz4_compress_fast_device writes for src."""
    lib = L.load()
    src = bytes(src)
    cap = int(lib.jfs_compress_bound(L.ALGO_LZ4, len(src)))
    dst = ctypes.create_string_buffer(max(cap, 1))
    n = int(lib.jfs_test_lz4_fast_host(ctypes.addressof(dst), cap, src, len(src)))
    return dst.raw[:n]


def lz4_fast_lift_host(src, lift, streams, src_caps):
    """The host twin with chunks lifted (jfs_test_lz4_fast_lift_host, test
    infrastructure): the bytes jfs_lz4_compress_fast_lift_device writes for the
    gathered block src.  lift: one (source, source chunk) per 64 KiB chunk of
    src, source < 0 for none; streams: the sources' stored LZ4 blocks;
    src_caps: their decode capacities.  Returns (bytes, chunks lifted, per chunk
    a lifted chunk's record count or -1)."""
    import numpy as np
    lib = L.load()
    src = bytes(src)
    nch = (len(src) + 65535) // 65536
    if len(lift) != nch or len(src_caps) != len(streams):
        raise ValueError("lz4_fast_lift_host: one candidate per chunk, one capacity per stream")
    flat = np.array([x for pair in lift for x in pair], dtype=np.int32).reshape(-1)
    bufs = [bytes(s) for s in streams]
    ptrs = (ctypes.c_char_p * max(len(bufs), 1))(*bufs)
    lens = np.array([len(s) for s in bufs], dtype=np.int32)
    caps = np.array(list(src_caps), dtype=np.int32)
    nrec = np.full(max(nch, 1), -1, dtype=np.int32)
    lifted = ctypes.c_int32(0)
    cap = int(lib.jfs_compress_bound(L.ALGO_LZ4, len(src)))
    dst = ctypes.create_string_buffer(max(cap, 1))
    n = int(lib.jfs_test_lz4_fast_lift_host(ctypes.addressof(dst), cap, src, len(src), flat.ctypes.data, len(bufs),
                                            ctypes.addressof(ptrs), lens.ctypes.data, caps.ctypes.data,
                                            ctypes.addressof(lifted), nrec.ctypes.data))
    return dst.raw[:n], int(lifted.value), nrec[:nch].tolist()


_PLAN_STATUS = {L.SEEK_PLAN_OK: "ok", L.SEEK_PLAN_MORE: "more", L.SEEK_PLAN_NONE: "none"}


def seek_plan(tail: bytes, object_len: int, lo: int, hi: int) -> dict:
    """jfs_zstd_seek_plan: from the last len(tail) bytes of a stored object, what
    to fetch for its content bytes [lo, hi).  Returns the plan's fields, with
    status "ok" (fetch [get_off, get_off + get_len)), "more" (fetch the table at
    [table_off, table_off + table_len) and ask again) or "none" (no table: fetch
    the object).  Needs no device."""
    p = L.JfsSeekPlan()
    buf = (ctypes.c_char * max(1, len(tail))).from_buffer_copy(bytes(tail) or b"\0")
    rc = L.load().jfs_zstd_seek_plan(ctypes.cast(buf, ctypes.c_void_p), len(tail), object_len, lo, hi, ctypes.byref(p))
    if rc != 0:
        raise ValueError(f"jfs_zstd_seek_plan: {rc}")
    d = {n: getattr(p, n) for n, _ in L.JfsSeekPlan._fields_ if n != "reserved"}
    d["status"] = _PLAN_STATUS[p.status]
    return d


def zstd_fast_seqs(src, device_ptr: int | None = None):
    """The fast Zstd parse's sequence records (test infrastructure): per 128 KiB
    block of src a (records, nl) pair, records = [(ll, ml, Offset_Value)] and
    nl the block's literal count.  From the host twin
    (jfs_test_zstd_fast_host_seqs), or, with device_ptr = the address of src's
    copy in device memory, from the kernels (jfs_test_zstd_fast_seqs_device)."""
    import numpy as np
    lib = L.load()
    n = len(src)
    nb = (n + (128 << 10) - 1) // (128 << 10)
    out = np.zeros(n // 4 + 4 * nb + 4, dtype=np.uint64)
    ns = np.zeros(nb + 1, dtype=np.int32)
    nl = np.zeros(nb + 1, dtype=np.int32)
    if device_ptr is None:
        keep = np.frombuffer(src, dtype=np.uint8) if n else np.zeros(1, dtype=np.uint8)
        total = int(lib.jfs_test_zstd_fast_host_seqs(keep.ctypes.data, n, out.ctypes.data, len(out), ns.ctypes.data,
                                                     nl.ctypes.data))
    else:
        total = int(lib.jfs_test_zstd_fast_seqs_device(device_ptr, n, out.ctypes.data, len(out), ns.ctypes.data,
                                                       nl.ctypes.data))
    if total < 0:
        raise RuntimeError(f"fast Zstd parse hook failed ({total})")
    blocks, at = [], 0
    for k in range(nb):
        r = out[at:at + int(ns[k])]
        at += int(ns[k])
        blocks.append(([(int(x) & 0x1FFFF, ((int(x) >> 17) & 0x1FFFF) + 3, int(x) >> 34) for x in r], int(nl[k])))
    assert at == total
    return blocks


def compact_plan(slices, block_size: int, src_block_size: int | None = None):
    """The gather plan of pkg/vfs/compact.go:54-108 (Compact + readSlice).

    slices: [(id, size, off, len)] in write order -- bytes [off, off+len) of
    slice `id`, which is `size` bytes long and stored in blocks cut at
    src_block_size (default block_size); id == 0 is a hole of `len` zero bytes
    (compact.go:70-77).  The new slice is their concatenation, cut at
    block_size (the last block is ragged).

    Returns (sources, seg_first, seg): sources = [(slice_index, block_index,
    block_len)], the stored blocks to fetch, each once, in first-use order
    (slice_index: the first entry of `slices` that names the slice);
    seg = [(src, src_off, dst_off, len)] with src an index into sources or -1
    for a hole, and seg_first (one entry per new block, plus one) delimiting
    each new block's segments -- the arguments of jfs_compact_batch."""
    S = int(src_block_size or block_size)
    B = int(block_size)
    if B <= 0 or S <= 0:
        raise ValueError("block sizes must be positive")
    sources, index, seg, seg_first = [], {}, [], []
    pos = 0  # position in the new slice

    def put(src, src_off, n):
        nonlocal pos
        while n > 0:  # cut at the new block boundaries
            take = min(n, B - pos % B)
            while len(seg_first) <= pos // B:
                seg_first.append(len(seg))
            seg.append((src, src_off, pos % B, take))
            pos, src_off, n = pos + take, src_off + take, n - take

    for si, (sid, size, off, ln) in enumerate(slices):
        if ln < 0 or (sid != 0 and (off < 0 or off + ln > size)):
            raise ValueError(f"slice {si}: [{off}, {off + ln}) outside its {size} bytes")
        if sid == 0:
            put(-1, 0, ln)
            continue
        p, end = off, off + ln
        while p < end:  # cut at the stored blocks' boundaries
            b = p // S
            take = min(end, (b + 1) * S) - p
            key = (sid, size, b)
            if key not in index:
                index[key] = len(sources)
                sources.append((si, b, min(S, size - b * S)))
            put(index[key], p - b * S, take)
            p += take
    seg_first.append(len(seg))
    return sources, seg_first, seg


def read_plan(reads, src_block_size: int):
    """The gather plan of a batch of dataReader.Read calls (pkg/vfs/reader.go:
    840-879 + readSlice :813-838).

    reads: [(page_len, offset, slices)] -- one page of page_len bytes filled
    from position `offset` of a chunk whose slice list is slices =
    [(id, size, off, len)] (as compact_plan takes them; id == 0 reads as
    zeros); what the slices do not cover is the page's zero tail.  Stored
    blocks are cut at src_block_size.

    Returns (sources, seg_first, seg): sources = [(read_index, slice_index,
    block_index, block_len)], every stored block the batch touches, once, in
    first-use order (shared between reads); seg / seg_first as for
    jfs_read_batch, one run of segments per read, the zero tail a hole."""
    S = int(src_block_size)
    if S <= 0:
        raise ValueError("block size must be positive")
    sources, index, seg, seg_first = [], {}, [], []
    for ri, (page_len, offset, slices) in enumerate(reads):
        seg_first.append(len(seg))
        read, pos = 0, 0
        if page_len < 0 or offset < 0:
            raise ValueError(f"read {ri}: negative page length or offset")
        for si, (sid, size, off, ln) in enumerate(slices):
            if ln < 0 or (sid != 0 and (off < 0 or off + ln > size)):
                raise ValueError(f"read {ri} slice {si}: [{off}, {off + ln}) outside its {size} bytes")
            if read < page_len and offset < pos + ln:  # reader.go:851-852
                toread = min(page_len - read, pos + ln - offset)
                p, end = off + (offset - pos), off + (offset - pos) + toread
                if sid == 0:
                    if toread > 0:
                        seg.append((-1, 0, read, toread))
                    p = end
                while p < end:  # cut at the stored blocks' boundaries
                    b = p // S
                    take = min(end, (b + 1) * S) - p
                    key = (sid, size, b)
                    if key not in index:
                        index[key] = len(sources)
                        sources.append((ri, si, b, min(S, size - b * S)))
                    seg.append((index[key], p - b * S, read + (p - (end - toread)), take))
                    p += take
                read += toread
                offset += toread
            pos += ln
        if read < page_len:  # reader.go:862-865
            seg.append((-1, 0, read, page_len - read))
    seg_first.append(len(seg))
    return sources, seg_first, seg


def read_expect(decoded_sources, plan):
    """What jfs_read_batch delivers for good reads: the stitch of the decoded
    sources a plan names, one bytes object per read."""
    seg_first, seg = plan
    outs = []
    for j in range(len(seg_first) - 1):
        out = bytearray()
        for src, src_off, dst_off, n in seg[seg_first[j]:seg_first[j + 1]]:
            if dst_off != len(out) or n <= 0:
                raise ValueError(f"read {j}: segments must tile the read in order")
            if src < 0:
                out += bytes(n)
            else:
                piece = bytes(decoded_sources[src][src_off:src_off + n])
                if src_off < 0 or len(piece) != n:
                    raise ValueError(f"read {j}: source {src} is shorter than [{src_off}, {src_off + n})")
                out += piece
        outs.append(bytes(out))
    return outs


def _read_call(algo: int, cipher, sources, keys, reads, plan, crcs, device_mask: int, with_csum=False):
    """jfs_read_batch (cipher None) / jfs_read_open_batch over host buffers;
    with_csum (True, or one flag per read): their _csum forms"""
    lib = L.load()
    seg_first, seg = plan
    ns, no = len(sources), len(reads)
    if len(seg_first) != no + 1:
        raise ValueError("seg_first must have one entry per read plus one")
    if crcs is not None and len(crcs) != ns:
        raise ValueError("one expected checksum (or None) per source")
    siov, oiov = (L.JfsIov * max(ns, 1))(), (L.JfsIov * max(no, 1))()
    kp = (ctypes.c_void_p * max(ns, 1))()
    keep = []
    for i, (obj, block_size) in enumerate(sources):
        s, sn, ks = _addr(obj, False)
        keep.append(ks)
        siov[i].src, siov[i].src_len, siov[i].dst, siov[i].dst_cap = s, sn, None, int(block_size)
        if cipher is not None:
            kk, _, k1 = _addr(keys[i], False)
            keep.append(k1)
            kp[i] = kk.value if isinstance(kk, ctypes.c_void_p) else kk
    for j, dst in enumerate(reads):
        d, dn, kd = _addr(dst, True)
        keep.append(kd)
        oiov[j].src, oiov[j].src_len, oiov[j].dst, oiov[j].dst_cap = None, 0, d, dn
    first = (ctypes.c_int32 * (no + 1))(*[int(x) for x in seg_first])
    segs = (L.JfsCompactSeg * max(len(seg), 1))()
    for k, (src, src_off, dst_off, n) in enumerate(seg):
        segs[k].src, segs[k].src_off, segs[k].dst_off, segs[k].len = int(src), int(src_off), int(dst_off), int(n)
    want = None
    if crcs is not None:
        want = (ctypes.c_int64 * max(ns, 1))(*[-1 if c is None else int(c) for c in crcs])
    src_n, out_n = (ctypes.c_int64 * max(ns, 1))(), (ctypes.c_int64 * max(no, 1))()
    got = (ctypes.c_uint32 * max(ns, 1))()
    cs_bufs = None
    if with_csum is not False and with_csum is not None:
        flags = [True] * no if with_csum is True else list(with_csum)
        if len(flags) != no:
            raise ValueError("one checksum flag (or buffer) per read")
        cs_bufs, cs_ptrs = [], (ctypes.c_void_p * max(no, 1))()
        for j, f in enumerate(flags):
            need = csum_bytes(sum(s[3] for s in seg[seg_first[j]:seg_first[j + 1]]))
            if f is None or f is False:
                cs_bufs.append(None)
                continue
            if f is True:
                f = bytearray(need)
            p, pn, kp_ = _addr(f, True)
            if pn < need:
                raise ValueError(f"read {j}: its checksum needs {need} bytes, the buffer holds {pn}")
            keep.append(kp_)
            cs_bufs.append(f)
            cs_ptrs[j] = p.value if isinstance(p, ctypes.c_void_p) else p
    if cipher is None and cs_bufs is None:
        rc = lib.jfs_read_batch(algo, ns, siov, want, no, oiov, first, segs, src_n, out_n, got, device_mask)
    elif cipher is None:
        rc = lib.jfs_read_batch_csum(algo, ns, siov, want, no, oiov, first, segs, src_n, out_n, got, cs_ptrs,
                                     device_mask)
    elif cs_bufs is None:
        rc = lib.jfs_read_open_batch(algo, cipher, ns, siov, kp, want, no, oiov, first, segs, src_n, out_n, got,
                                     device_mask)
    else:
        rc = lib.jfs_read_open_batch_csum(algo, cipher, ns, siov, kp, want, no, oiov, first, segs, src_n, out_n, got,
                                          cs_ptrs, device_mask)
    if rc != 0:
        raise _err(rc, 0, 0, "read")

    def err_of(code, dst_len, src_len, op):
        if code == L.JFS_ERR_AUTH:
            return CompressError("cipher: message authentication failed", code)
        return _err(code, dst_len, src_len, op)

    src_res, out_res = [], []
    for i in range(ns):
        r = int(src_n[i])
        if r == L.JFS_ERR_CHECKSUM:  # checksum.go:68
            src_res.append((0, CompressError(f"verify checksum failed: {int(got[i])} != {int(want[i])}", r)))
        elif r < 0:
            n = r if (algo == L.ALGO_LZ4 and r > L.JFS_ERR_BASE) else 0
            src_res.append((n, err_of(r, siov[i].dst_cap, siov[i].src_len, "decompress")))
        else:
            src_res.append((r, None))
    for j in range(no):
        r = int(out_n[j])
        out_res.append((0, err_of(r, oiov[j].dst_cap, 0, "read")) if r < 0 else (r, None))
    crc_got = [int(got[i]) for i in range(ns)]
    if cs_bufs is None:
        return src_res, out_res, crc_got
    sums = [bytes(memoryview(cs_bufs[j]).cast("B")[:csum_bytes(n)]) if e is None and cs_bufs[j] is not None else None
            for j, (n, e) in enumerate(out_res)]
    return src_res, out_res, crc_got, sums


CSUM_BLOCK = 32 << 10  # disk_cache_file.go csBlock


def csum_bytes(n: int) -> int:
    """Length of checksum() for n data bytes: ((n-1)/32768+1)*4 (Go integer division)."""
    return (int((n - 1) / CSUM_BLOCK) + 1) * 4


def CompressBatchMixed(entries, device_mask: int = 0):
    """entries: list of (Compressor, dst, src) with any mix of codecs; the
    codecs' batches run at once on the GPU(s) (jfs_compress_batch_mixed).
    Returns [(n, err)] with each Compressor's own result semantics."""
    return _batch_mixed(entries, device_mask, compress=True)


def DecompressBatchMixed(entries, device_mask: int = 0):
    """DecompressBatch over blocks of several codecs (jfs_decompress_batch_mixed)."""
    return _batch_mixed(entries, device_mask, compress=False)


def _batch_mixed(entries, device_mask: int, compress: bool):
    lib = L.load()
    nb = len(entries)
    iov = (L.JfsIov * max(nb, 1))()
    algos = (ctypes.c_int32 * max(nb, 1))()
    keep = []
    for i, (cd, dst, src) in enumerate(entries):
        d, dn, kd = _addr(dst, True)
        s, sn, ks = _addr(src, False)
        keep.append((kd, ks))
        iov[i].src, iov[i].src_len, iov[i].dst, iov[i].dst_cap = s, sn, d, dn
        algos[i] = cd.algo
    out = (ctypes.c_int64 * max(nb, 1))()
    fn = lib.jfs_compress_batch_mixed if compress else lib.jfs_decompress_batch_mixed
    rc = fn(algos, nb, iov, out, device_mask)
    if rc != 0:
        raise _err(rc, 0, 0, "batch")
    res = []
    for i in range(nb):
        r, algo = int(out[i]), int(algos[i])
        if r < 0:
            n = r if (algo == L.ALGO_LZ4 and not compress and r > L.JFS_ERR_BASE) else 0
            res.append((n, _err(r, iov[i].dst_cap, iov[i].src_len, "compress" if compress else "decompress")))
        else:
            res.append((r, None))
    return res


def _batch(algo: int, pairs, device_mask: int, compress: bool, with_crc: bool = False, with_csum: bool = False):
    """pairs: list of (dst, src).  Returns list of (n, err)."""
    lib = L.load()
    nb = len(pairs)
    iov = (L.JfsIov * max(nb, 1))()
    keep = []
    for i, (dst, src) in enumerate(pairs):
        d, dn, kd = _addr(dst, True)
        s, sn, ks = _addr(src, False)
        keep.append((kd, ks))
        iov[i].src, iov[i].src_len, iov[i].dst, iov[i].dst_cap = s, sn, d, dn
    out = (ctypes.c_int64 * max(nb, 1))()
    crc = (ctypes.c_uint32 * max(nb, 1))()
    cs_bufs = []
    if with_csum:
        cs_bufs = [ctypes.create_string_buffer(csum_bytes(max(iov[i].dst_cap, 0))) for i in range(nb)]
        cs_ptrs = (ctypes.c_void_p * max(nb, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in cs_bufs])
    if with_crc:
        rc = lib.jfs_compress_batch_crc(algo, nb, iov, out, crc, device_mask)
    elif with_csum:
        rc = lib.jfs_decompress_batch_csum(algo, nb, iov, out, cs_ptrs, device_mask)
    else:
        fn = lib.jfs_compress_batch if compress else lib.jfs_decompress_batch
        rc = fn(algo, nb, iov, out, device_mask)
    if rc != 0:
        raise _err(rc, 0, 0, "batch")
    res = []
    for i in range(nb):
        r = int(out[i])
        if r < 0:
            n = r if (algo == L.ALGO_LZ4 and not compress and r > L.JFS_ERR_BASE) else 0
            res.append((n, _err(r, iov[i].dst_cap, iov[i].src_len, "compress" if compress else "decompress")))
        else:
            res.append((r, None))
    if with_crc:
        return [(n, e, int(crc[i])) for i, (n, e) in enumerate(res)]
    if with_csum:
        return [(n, e, cs_bufs[i].raw[:csum_bytes(n)] if e is None else None) for i, (n, e) in enumerate(res)]
    return res
