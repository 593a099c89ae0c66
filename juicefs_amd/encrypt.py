"""Python mirror of JuiceFS's object-encryption data path over libjfsgpu.so,
fused with the codec.

    AES256GCM_RSA / CHACHA20_RSA / SM4GCM          pkg/object/encrypt.go:172-176
    NewDataEncryptor(keyEncryptor, algo)           :178-203 (here: cipher id)
    dataEncryptor.Encrypt / Decrypt                :226-284

The PUT path of an encrypted volume compresses a block (cached_store.go:372)
and then Encrypt()s it into the object envelope; the GET path Decrypt()s and
decompresses (:814).  ``compress_seal_batch`` / ``open_decompress_batch`` do
both steps on the GPU for many blocks at once.  The random data key, the
nonce and the key wrap (RSA / SM2 keyEncryptor, encrypt.go:234) stay with the
caller: seal takes (key, nonce, wrapped_key) per block, open takes the data
key the caller unwrapped from the envelope header (``parse_envelope``).
Results are ``(n, err)`` pairs like compress.py's batch helpers.
"""
from __future__ import annotations

import ctypes

from . import _lib as L
from .compress import CompressError, _addr, _err, _read_call, csum_bytes

AES256GCM_RSA = "aes256gcm-rsa"
CHACHA20_RSA = "chacha20-rsa"
SM4GCM = "sm4gcm"


def cipher_id(algo: str) -> int:
    """NewDataEncryptor's names ("" = AES-256-GCM); raises for an unsupported one."""
    c = L.load().jfs_cipher_from_name(algo.encode())
    if c < 0:
        raise ValueError(f"unsupport cipher: {algo}")
    return c


def key_size(algo: str) -> int:
    return L.load().jfs_cipher_key_size(cipher_id(algo))


def envelope_bound(codec: int, n: int, wrapped_len: int) -> int:
    return int(L.load().jfs_envelope_bound(codec, n, wrapped_len))


def parse_envelope(env: bytes):
    """(wrapped key, nonce, payload offset); raises CompressError like Decrypt's header checks."""
    i64 = ctypes.c_int64
    wo, wl, no, nl = i64(), i64(), i64(), i64()
    a, n, keep = _addr(env, False)
    r = int(L.load().jfs_envelope_parse(a, n, ctypes.byref(wo), ctypes.byref(wl), ctypes.byref(no), ctypes.byref(nl)))
    if r < 0:
        raise CompressError("malformed ciphertext", r)
    return bytes(env[wo.value:wo.value + wl.value]), bytes(env[no.value:no.value + nl.value]), r


def _err_of(code: int, dst_len: int, src_len: int, op: str) -> CompressError:
    if code == L.JFS_ERR_AUTH:
        return CompressError("cipher: message authentication failed", code)
    return _err(code, dst_len, src_len, op)


NONCE_SIZE = 12  # encrypt.go:239: aead.NonceSize() of all three ciphers


def _check_keys(algo: str, keys, nonces) -> None:
    """The C ABI reads jfs_cipher_key_size() key bytes and 12 nonce bytes per
    block through plain pointers; a shorter buffer would be read past its end.
    dataEncryptor.aead (encrypt.go:182-202, used at :235, :276) refuses a wrong key size with an
    error, and so does this, before anything reaches the library."""
    ks = key_size(algo)
    for i, k in enumerate(keys):
        if len(k) != ks:
            raise ValueError(f"block {i}: {algo or 'aes256gcm-rsa'} needs a {ks}-byte key, got {len(k)}")
    for i, n in enumerate(nonces or ()):
        if len(n) != NONCE_SIZE:
            raise ValueError(f"block {i}: nonce must be {NONCE_SIZE} bytes, got {len(n)}")


def compress_seal_batch(codec: int, algo: str, pairs, params, device_mask: int = 0, crcs: list | None = None):
    """pairs: [(dst, raw block)], params: [(key, nonce, wrapped_key)] -> [(envelope bytes, err)];
    with crcs=[], it receives each envelope's CRC-32C (generateChecksum)."""
    lib = L.load()
    nb = len(pairs)
    _check_keys(algo, [p[0] for p in params], [p[1] for p in params])
    iov = (L.JfsIov * max(nb, 1))()
    sp = (L.JfsSealParam * max(nb, 1))()
    keep = []
    for i, ((dst, src), (key, nonce, wrapped)) in enumerate(zip(pairs, params)):
        d, dn, kd = _addr(dst, True)
        s, sn, ks = _addr(src, False)
        kk, _, k1 = _addr(key, False)
        nn, _, k2 = _addr(nonce, False)
        ww, wn, k3 = _addr(wrapped, False)
        keep.append((kd, ks, k1, k2, k3))
        iov[i].src, iov[i].src_len, iov[i].dst, iov[i].dst_cap = s, sn, d, dn
        sp[i].key, sp[i].nonce, sp[i].wrapped, sp[i].wrapped_len = kk, nn, ww, wn
    out = (ctypes.c_int64 * max(nb, 1))()
    crc = (ctypes.c_uint32 * max(nb, 1))() if crcs is not None else None
    rc = lib.jfs_compress_seal_batch(codec, cipher_id(algo), nb, iov, sp, out, crc, device_mask)
    if rc != 0:
        raise _err_of(rc, 0, 0, "seal batch")
    if crcs is not None:
        crcs[:] = [int(crc[i]) for i in range(nb)]
    return [(int(out[i]), None) if out[i] >= 0 else
            (0, _err_of(int(out[i]), iov[i].dst_cap, iov[i].src_len, "compress+seal")) for i in range(nb)]


def open_decompress_batch(codec: int, algo: str, pairs, keys, device_mask: int = 0, with_csum: bool = False):
    """pairs: [(dst, envelope)], keys: [data key] -> [(n, err)] (n as jfs_decompress returns it).
    with_csum (jfs_open_decompress_batch_csum): [(n, err, csum)] as
    Compressor.DecompressBatchChecksum gives, the disk-cache checksum bytes
    of every opened and decoded block (None for a block that fails)."""
    lib = L.load()
    nb = len(pairs)
    _check_keys(algo, keys, None)
    iov = (L.JfsIov * max(nb, 1))()
    kp = (ctypes.c_void_p * max(nb, 1))()
    keep = []
    for i, ((dst, src), key) in enumerate(zip(pairs, keys)):
        d, dn, kd = _addr(dst, True)
        s, sn, ks = _addr(src, False)
        kk, _, k1 = _addr(key, False)
        keep.append((kd, ks, k1))
        iov[i].src, iov[i].src_len, iov[i].dst, iov[i].dst_cap = s, sn, d, dn
        kp[i] = kk.value if isinstance(kk, ctypes.c_void_p) else kk
    out = (ctypes.c_int64 * max(nb, 1))()
    if with_csum:
        cs_bufs = [ctypes.create_string_buffer(csum_bytes(max(iov[i].dst_cap, 0))) for i in range(nb)]
        cs_ptrs = (ctypes.c_void_p * max(nb, 1))(*[ctypes.cast(b, ctypes.c_void_p) for b in cs_bufs])
        rc = lib.jfs_open_decompress_batch_csum(codec, cipher_id(algo), nb, iov, kp, out, cs_ptrs, device_mask)
    else:
        rc = lib.jfs_open_decompress_batch(codec, cipher_id(algo), nb, iov, kp, out, device_mask)
    if rc != 0:
        raise _err_of(rc, 0, 0, "open batch")
    res = []
    for i in range(nb):
        r = int(out[i])
        if r < 0:
            n = r if (codec == L.ALGO_LZ4 and r > L.JFS_ERR_BASE) else 0
            res.append((n, _err_of(r, iov[i].dst_cap, iov[i].src_len, "open+decompress")))
        else:
            res.append((r, None))
    if with_csum:
        return [(n, e, cs_bufs[i].raw[:csum_bytes(n)] if e is None else None) for i, (n, e) in enumerate(res)]
    return res


def open_decompress_batch_csum(codec: int, algo: str, pairs, keys, device_mask: int = 0):
    """The sealed DecompressBatchChecksum: open_decompress_batch(with_csum=True)."""
    return open_decompress_batch(codec, algo, pairs, keys, device_mask, with_csum=True)


def compact_seal_batch(codec: int, algo: str, sources, keys, outputs, params, plan, device_mask: int = 0,
                       with_crc: bool = False):
    """Slice compaction of an encrypted volume on one GPU (jfs_compact_seal_batch):
    open and decode the stored envelopes, gather the planned byte ranges into
    new blocks, compress and seal those -- Compressor.CompactBatch with
    open_decompress_batch in front and compress_seal_batch behind, without a
    decoded or a decrypted byte leaving HBM.

    sources: [(envelope, block_size)], keys: [data key] (one per source);
    outputs: [writable dst], params: [(key, nonce, wrapped_key)] (one per
    output; a fresh key / nonce pair for every output is the caller's duty);
    plan: (seg_first, seg) as compress.compact_plan returns them.  Returns
    (src_results, out_results[, crcs]): [(n, err)] as open_decompress_batch
    gives for the sources and as compress_seal_batch gives for the gathered
    blocks (JFS_ERR_CORRUPT for a block fed by a failed or short source), plus
    each envelope's CRC-32C with with_crc."""
    lib = L.load()
    seg_first, seg = plan
    ns, no = len(sources), len(outputs)
    if len(seg_first) != no + 1:
        raise ValueError("seg_first must have one entry per output plus one")
    if len(keys) != ns or len(params) != no:
        raise ValueError("one key per source and one (key, nonce, wrapped_key) per output")
    _check_keys(algo, list(keys) + [p[0] for p in params], [p[1] for p in params])
    siov, oiov = (L.JfsIov * max(ns, 1))(), (L.JfsIov * max(no, 1))()
    kp = (ctypes.c_void_p * max(ns, 1))()
    sp = (L.JfsSealParam * max(no, 1))()
    keep = []
    for i, ((obj, block_size), key) in enumerate(zip(sources, keys)):
        s, sn, ks = _addr(obj, False)
        kk, _, k1 = _addr(key, False)
        keep.append((ks, k1))
        siov[i].src, siov[i].src_len, siov[i].dst, siov[i].dst_cap = s, sn, None, int(block_size)
        kp[i] = kk.value if isinstance(kk, ctypes.c_void_p) else kk
    for j, (dst, (key, nonce, wrapped)) in enumerate(zip(outputs, params)):
        d, dn, kd = _addr(dst, True)
        kk, _, k1 = _addr(key, False)
        nn, _, k2 = _addr(nonce, False)
        ww, wn, k3 = _addr(wrapped, False)
        keep.append((kd, k1, k2, k3))
        oiov[j].src, oiov[j].src_len, oiov[j].dst, oiov[j].dst_cap = None, 0, d, dn
        sp[j].key, sp[j].nonce, sp[j].wrapped, sp[j].wrapped_len = kk, nn, ww, wn
    first = (ctypes.c_int32 * (no + 1))(*[int(x) for x in seg_first])
    segs = (L.JfsCompactSeg * max(len(seg), 1))()
    for k, (src, src_off, dst_off, n) in enumerate(seg):
        segs[k].src, segs[k].src_off, segs[k].dst_off, segs[k].len = int(src), int(src_off), int(dst_off), int(n)
    src_n, out_n = (ctypes.c_int64 * max(ns, 1))(), (ctypes.c_int64 * max(no, 1))()
    crc = (ctypes.c_uint32 * max(no, 1))()
    rc = lib.jfs_compact_seal_batch(codec, cipher_id(algo), ns, siov, kp, no, oiov, sp, first, segs, src_n, out_n,
                                    crc if with_crc else None, device_mask)
    if rc != 0:
        raise _err_of(rc, 0, 0, "compact+seal")
    src_res, out_res = [], []
    for i in range(ns):
        r = int(src_n[i])
        if r < 0:
            n = r if (codec == L.ALGO_LZ4 and r > L.JFS_ERR_BASE) else 0
            src_res.append((n, _err_of(r, siov[i].dst_cap, siov[i].src_len, "open+decompress")))
        else:
            src_res.append((r, None))
    for j in range(no):
        r = int(out_n[j])
        total = sum(s[3] for s in seg[seg_first[j]:seg_first[j + 1]])
        out_res.append((0, _err_of(r, oiov[j].dst_cap, total, "compress+seal")) if r < 0 else (r, None))
    if with_crc:
        return src_res, out_res, [int(crc[j]) for j in range(no)]
    return src_res, out_res


def read_open_batch(codec: int, algo: str, sources, keys, reads, plan, crcs=None, device_mask: int = 0,
                    with_csum=False):
    """Read assembly of an encrypted volume on one GPU (jfs_read_open_batch):
    Compressor.ReadBatch with open_decompress_batch in front.  sources:
    [(envelope, block_size)], keys: [data key] (one per source); reads, plan,
    crcs and the result as for ReadBatch -- the expected CRC-32C covers the
    whole envelope, and a source that does not authenticate is a failed
    source.  with_csum (jfs_read_open_batch_csum): as for ReadBatch."""
    if len(keys) != len(sources):
        raise ValueError("one key per source")
    _check_keys(algo, keys, None)
    return _read_call(codec, cipher_id(algo), sources, keys, reads, plan, crcs, device_mask, with_csum)
