"""GPU: compaction of an encrypted volume (jfs_compact_seal_batch,
encrypt.compact_seal_batch): open -> decode -> gather -> encode -> seal on the
device, against the existing sealed batch calls (open_decompress_batch, a
numpy stitch, compress_seal_batch) and, independently, the CPU AEAD and codec
oracles.

Every output dst is a slice of a larger array pre-filled with a canary; the
whole array is compared with its expected image, so one byte written outside
the envelope -- or anything written for a failed block -- fails the test."""
import random

import numpy as np
import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CIPHERS = {E.AES256GCM_RSA: "aes256gcm", E.CHACHA20_RSA: "chacha20", E.SM4GCM: "sm4gcm"}
CODECS = {"none": L.ALGO_NONE, "lz4": L.ALGO_LZ4, "zstd": L.ALGO_ZSTD}
BLOCK = 70000
SRC = [("T", 70000), ("T", 65537), ("R", 4097), ("Z", 1)]  # class, decoded length
SRC_WRAPPED = [256, 1, 0, 1]                                 # payloads start at odd offsets
OUT_WRAPPED = [0, 1, 256]
BAD = 0  # the source the failure cases break: it feeds output 0 only


def _tile(parts):
    """[(src, src_off, len)] -> [(src, src_off, dst_off, len)]"""
    segs, at = [], 0
    for src, src_off, n in parts:
        segs.append((src, src_off, at, n))
        at += n
    return segs


OUT_PARTS = [
    # every source, the 60000-byte run, holes between sources
    [(0, 5, 60000), (-1, 0, 15), (1, 65537 - 17, 17), (2, 0, 4097), (3, 0, 1), (-1, 0, 16), (1, 7, 16), (0, 69985, 15)],
    # sources 1-3 only
    [(2, 1000, 17), (-1, 0, 4097), (1, 100, 4097), (3, 0, 1), (2, 4096, 1), (1, 3, 15), (1, 60000, 16), (-1, 0, 1)],
    # holes only
    [(-1, 0, 17), (-1, 0, 4097)],
]


def _plan(parts=OUT_PARTS):
    seg_first, seg = [0], []
    for p in parts:
        seg += _tile(p)
        seg_first.append(len(seg))
    return seg_first, seg


def _stitch(raws, parts):
    out = np.zeros(sum(p[2] for p in parts), dtype=np.uint8)
    for src, src_off, dst_off, n in _tile(parts):
        if src >= 0:
            out[dst_off:dst_off + n] = np.frombuffer(raws[src], dtype=np.uint8)[src_off:src_off + n]
    return out.tobytes()


def _params(algo, wrapped_lens, seed):
    rng = random.Random(seed)
    klen = E.key_size(algo)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    return [(rb(klen), rb(12), rb(w)) for w in wrapped_lens]


_cache = {}


def _data():
    """(decoded sources, the stitched output blocks): the numpy model, made once"""
    if "data" not in _cache:
        raws = [gen_block(cls, 500 + i, n) for i, (cls, n) in enumerate(SRC)]
        _cache["data"] = (raws, [_stitch(raws, p) for p in OUT_PARTS])
    return _cache["data"]


def _setup(algo, codec, mode="exact"):
    """The stored source envelopes (written by compress_seal_batch), the
    output parameters, and compress_seal_batch's envelopes and CRCs of the
    stitched blocks -- computed once per (cipher, codec, parse mode)."""
    key = (algo, codec, mode)
    RAWS, BLOCKS = _data()
    if key not in _cache:
        sp = _params(algo, SRC_WRAPPED, 1)
        op = _params(algo, OUT_WRAPPED, 2)

        def seal(blocks, params):
            pairs = [(bytearray(E.envelope_bound(CODECS[codec], len(b), len(p[2]))), b) for b, p in zip(blocks, params)]
            crcs = []
            res = E.compress_seal_batch(CODECS[codec], algo, pairs, params, crcs=crcs)
            assert all(e is None for _, e in res)
            return [bytes(d[:n]) for (d, _), (n, _) in zip(pairs, res)], crcs
        envs, _ = seal(RAWS, sp)
        ref, ref_crc = seal(BLOCKS, op)
        _cache[key] = (envs, sp, op, ref, ref_crc)
    return _cache[key]


class Dst:
    """Output buffers at odd offsets inside canary-filled arrays."""

    def __init__(self, caps):
        self.caps = list(caps)
        self.offs = [2 * j + 1 for j in range(len(caps))]
        self.arr = [np.full(o + c + 48, CANARY, dtype=np.uint8) for o, c in zip(self.offs, caps)]
        self.views = [a[o:o + c] for a, o, c in zip(self.arr, self.offs, caps)]

    def check(self, j, want: bytes):
        """the whole array: `want` at dst[0, len(want)), canary everywhere else"""
        img = np.full(len(self.arr[j]), CANARY, dtype=np.uint8)
        img[self.offs[j]:self.offs[j] + len(want)] = np.frombuffer(want, dtype=np.uint8)
        bad = np.nonzero(img != self.arr[j])[0]
        assert bad.size == 0, f"output {j}: first wrong byte at {bad[0] - self.offs[j]} of dst ({bad.size} wrong)"


def _codes(res):
    return [(n, e.code if e else None) for n, e in res]


def _run(algo, codec, envs, keys, op, caps=None, plan=None, blocks=None, block_size=BLOCK):
    blocks = _data()[1] if blocks is None else blocks
    if caps is None:
        caps = [E.envelope_bound(CODECS[codec], len(b), len(p[2])) for b, p in zip(blocks, op)]
    dst = Dst(caps)
    sres, ores, crcs = E.compact_seal_batch(CODECS[codec], algo, [(e, block_size) for e in envs], keys, dst.views, op,
                                            plan or _plan(), with_crc=True)
    return dst, sres, ores, crcs


def _decode(oracle, codec, comp, n):
    if codec == "none":
        return comp
    return (oracle.lz4_decompress(comp, n) if codec == "lz4" else oracle.zstd_decompress(comp, n))[1]


@pytest.mark.parametrize("codec", list(CODECS))
@pytest.mark.parametrize("algo", list(CIPHERS))
def test_parity_with_sealed_batch_calls_and_oracles(gpu, oracle, algo, codec):
    envs, sp, op, ref, ref_crc = _setup(algo, codec)
    dst, sres, ores, crcs = _run(algo, codec, envs, [p[0] for p in sp], op)
    assert _codes(sres) == [(n, None) for _, n in SRC]
    for j, block in enumerate(_data()[1]):
        assert ores[j] == (len(ref[j]), None) and crcs[j] == ref_crc[j], j
        dst.check(j, ref[j])
        # independently of this library: header, AEAD, codec and checksum on the CPU
        key, nonce, wrapped = op[j]
        env = ref[j]
        hdr = 3 + len(wrapped) + 12
        assert env[:hdr] == bytes([len(wrapped) >> 8, len(wrapped) & 255, 12]) + wrapped + nonce
        comp = oracle.open(CIPHERS[algo], key, nonce, env[hdr:])
        assert comp is not None, j
        assert _decode(oracle, codec, comp, len(block)) == block, j
        assert crcs[j] == oracle.crc32c(env), j


BAD_TAG_ROWS = [(a, "none") for a in CIPHERS] + [(E.AES256GCM_RSA, "lz4"), (E.AES256GCM_RSA, "zstd")]


@pytest.mark.parametrize("algo,codec", BAD_TAG_ROWS)
@pytest.mark.parametrize("how", ["tag_bit", "wrong_key"])
def test_unauthenticated_source_fails_only_what_it_feeds(gpu, algo, codec, how):
    """A source that does not open must count as a failed source on the
    device: a failed open leaves zeros, and for "none" zeros are a block."""
    envs, sp, op, ref, ref_crc = _setup(algo, codec)
    envs, keys = list(envs), [p[0] for p in sp]
    if how == "tag_bit":
        e = bytearray(envs[BAD])
        e[-7] ^= 0x10
        envs[BAD] = bytes(e)
    else:
        keys[BAD] = bytes(b ^ 0x55 for b in keys[BAD])
    dst, sres, ores, crcs = _run(algo, codec, envs, keys, op)
    want = [(n, None) for _, n in SRC]
    want[BAD] = (0, L.JFS_ERR_AUTH)
    assert _codes(sres) == want
    assert _codes(ores)[0] == (0, L.JFS_ERR_CORRUPT) and crcs[0] == 0
    dst.check(0, b"")
    for j in (1, 2):
        assert ores[j] == (len(ref[j]), None) and crcs[j] == ref_crc[j], j
        dst.check(j, ref[j])


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_source_errors_equal_open_decompress_batch(gpu, oracle, codec):
    algo = E.AES256GCM_RSA
    envs, sp, op, ref, ref_crc = _setup(algo, codec)
    key, nonce, wrapped = sp[0]
    sealed = lambda pt: oracle.envelope(wrapped, nonce, oracle.seal(CIPHERS[algo], key, nonce, pt))
    srcs = [
        b"\x00\x01",                          # shorter than a header
        envs[0][:3 + len(wrapped) + 12],      # 3 + wrapped + nonce >= n
        sealed(b"\xff" * 100),                # authentic, but not a compressed block
        sealed(b""),                          # authentic and empty
        envs[1],
    ]
    keys = [key, key, key, key, sp[1][0]]
    back = E.open_decompress_batch(CODECS[codec], algo, [(bytearray(BLOCK), s) for s in srcs], keys)
    assert [e.code if e else None for _, e in back][:2] == [L.JFS_ERR_CORRUPT] * 2
    assert back[2][1] is not None and back[3][1].code == L.JFS_ERR_EMPTY_INPUT and back[4] == (SRC[1][1], None)
    parts = [[(i, 0, 1)] for i in range(4)] + [[(4, 11, 4097), (-1, 0, 16)]]
    good = _stitch([b""] * 4 + [_data()[0][1]], parts[4])
    blocks = [b"\0"] * 4 + [good]
    p5 = _params(algo, [0, 1, 256, 1, 0], 3)
    dst, sres, ores, crcs = _run(algo, codec, srcs, keys, p5, plan=_plan(parts), blocks=blocks)
    assert _codes(sres) == _codes(back)
    for j in range(4):
        assert _codes(ores)[j] == (0, L.JFS_ERR_CORRUPT) and crcs[j] == 0, j
        dst.check(j, b"")
    alone = bytearray(E.envelope_bound(CODECS[codec], len(good), 0))
    n, e = E.compress_seal_batch(CODECS[codec], algo, [(alone, good)], [p5[4]])[0]
    assert e is None and ores[4] == (n, None)
    dst.check(4, bytes(alone[:n]))


@pytest.mark.parametrize("codec", list(CODECS))
def test_output_errors_equal_compress_seal_batch(gpu, codec):
    algo = E.CHACHA20_RSA
    envs, sp, op, ref, ref_crc = _setup(algo, codec)
    BLOCKS = _data()[1]
    caps = [E.envelope_bound(CODECS[codec], len(b), len(p[2])) for b, p in zip(BLOCKS, op)]
    caps[0] -= 1
    caps[1] = 10
    alone = E.compress_seal_batch(CODECS[codec], algo, [(bytearray(caps[j]), BLOCKS[j]) for j in (0, 1)], op[:2])
    assert all(e is not None for _, e in alone)
    dst, sres, ores, crcs = _run(algo, codec, envs, [p[0] for p in sp], op, caps=caps)
    assert _codes(sres) == [(n, None) for _, n in SRC]
    assert _codes(ores)[:2] == _codes(alone) and crcs[:2] == [0, 0]
    dst.check(0, b"")
    dst.check(1, b"")
    assert ores[2] == (len(ref[2]), None) and crcs[2] == ref_crc[2]
    dst.check(2, ref[2])
    # a source that fails on the device still wins over the block's own error
    keys = [p[0] for p in sp]
    keys[BAD] = bytes(len(keys[BAD]))
    dst, sres, ores, crcs = _run(algo, codec, envs, keys, op, caps=caps)
    assert _codes(ores)[0] == (0, L.JFS_ERR_CORRUPT) and _codes(ores)[1] == _codes(alone)[1]
    dst.check(0, b"")


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_fast_parse_mode_is_followed(gpu, lib, codec):
    algo = E.SM4GCM
    envs, sp, op, exact, _ = _setup(algo, codec)
    lz4_mode, zstd_mode = lib.jfs_lz4_parse_mode(), lib.jfs_zstd_parse_mode()
    with C.lz4_parse_mode("fast"), C.zstd_parse_mode("fast"):
        _, _, _, ref, ref_crc = _setup(algo, codec, mode="fast")
        dst, sres, ores, crcs = _run(algo, codec, envs, [p[0] for p in sp], op)
    assert (lib.jfs_lz4_parse_mode(), lib.jfs_zstd_parse_mode()) == (lz4_mode, zstd_mode)
    assert ref[0] != exact[0]  # the 60000-byte text run: the two parses differ
    for j in range(3):
        assert ores[j] == (len(ref[j]), None) and crcs[j] == ref_crc[j], j
        dst.check(j, ref[j])


@pytest.mark.parametrize("codec", list(CODECS))
def test_degenerate_plans(gpu, oracle, codec):
    algo = E.AES256GCM_RSA
    envs, sp, op, ref, ref_crc = _setup(algo, codec)
    # no sources: outputs made of holes, and one without a segment
    parts = [OUT_PARTS[2], []]
    blocks = [_data()[1][2], b""]
    dst, sres, ores, crcs = _run(algo, codec, [], [], [op[2], op[1]], plan=_plan(parts), blocks=blocks)
    assert sres == [] and ores[0] == (len(ref[2]), None) and crcs[0] == ref_crc[2]
    dst.check(0, ref[2])
    key, nonce, wrapped = op[1]
    n, e = ores[1]
    env = bytes(dst.views[1][:n])
    hdr = 3 + len(wrapped) + 12
    assert e is None and env[:hdr] == bytes([0, len(wrapped), 12]) + wrapped + nonce
    comp = oracle.open(CIPHERS[algo], key, nonce, env[hdr:])
    assert comp is not None and _decode(oracle, codec, comp, 16) == b"" and crcs[1] == oracle.crc32c(env)
    if codec != "zstd":  # byte-exact on the CPU too: an empty LZ4 block is one zero token
        assert comp == (b"" if codec == "none" else oracle.lz4_compress(b"")[1])
    dst.check(1, env)
    # no outputs: the sources are still opened and decoded
    _, sres, ores, crcs = _run(algo, codec, envs, [p[0] for p in sp], [], plan=([0], []), blocks=[])
    assert _codes(sres) == [(n, None) for _, n in SRC] and ores == [] and crcs == []
    # neither
    assert E.compact_seal_batch(CODECS[codec], algo, [], [], [], [], ([0], [])) == ([], [])


def _stat(lib, algo, d):
    s = (L.JfsOpStats * L.STATS_N)()
    lib.jfs_stats(s, L.STATS_N)
    return s[algo * 2 + d]


@pytest.mark.parametrize("codec", list(CODECS))
def test_stats_and_current_device(gpu, lib, codec):
    import torch
    algo = E.AES256GCM_RSA
    envs, sp, op, ref, _ = _setup(algo, codec)
    keys = [p[0] for p in sp]
    keys[BAD] = bytes(len(keys[BAD]))
    dev0 = torch.cuda.current_device()
    lib.jfs_stats_reset()
    _, sres, ores, _ = _run(algo, codec, envs, keys, op)
    assert torch.cuda.current_device() == dev0
    dec, enc = _stat(lib, CODECS[codec], 1), _stat(lib, CODECS[codec], 0)
    assert (dec.calls, dec.blocks, dec.errors, enc.calls, enc.blocks, enc.errors) == (1, 4, 1, 1, 3, 1)
    assert dec.bytes_out == sum(n for _, n in SRC[1:]) and dec.bytes_in == sum(len(e) for e in envs[1:])
    BLOCKS = _data()[1]
    assert enc.bytes_in == len(BLOCKS[1]) + len(BLOCKS[2]) and enc.bytes_out == len(ref[1]) + len(ref[2])
