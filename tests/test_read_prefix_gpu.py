"""GPU: the read calls in JFS_READ_DECODE_PREFIX mode (every LZ4 decode stops at
the last byte a read needs) against the same calls in full mode: out_n and
every output image are equal, src_n is min(size, need) for LZ4 and full mode's
for Zstd and "none", and the checksum, the short-source and the failed-read
verdicts keep their meaning.  Read buffers sit at odd offsets inside
canary-filled arrays (tests.test_read_gpu.Dst)."""
import os
import random
import subprocess
import sys

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests.test_compact_gpu import _tile
from tests.test_read_gpu import Dst, _codes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 256 << 10
NSRC = 6


def _parts():
    """12 reads of two source runs around a hole.  Source 0 is referenced only
    in its first 100 bytes, source 1 up to its last byte, source 5 not at all;
    2, 3 and 4 somewhere inside."""
    parts = []
    for j in range(12):
        a, b = (0, 1) if j < 2 else (2 + j % 3, 2 + (j + 1) % 3)
        if j == 0:
            parts.append([(0, 3, 97), (-1, 0, 33), (1, SIZE - 4097, 4097)])
        elif j == 1:
            parts.append([(1, 5, 60000), (-1, 0, 15), (0, 0, 64)])
        else:
            parts.append([(a, 1000 * j + 7, 4096 + j), (-1, 0, 17 * j), (b, 50000 + 3001 * j, 10000 + j)])
    return parts


def _plan(parts):
    seg_first, seg = [0], []
    for p in parts:
        seg += _tile(p)
        seg_first.append(len(seg))
    return seg_first, seg


def _need(parts, nsrc):
    need = [0] * nsrc
    for p in parts:
        for s, off, n in p:
            if s >= 0:
                need[s] = max(need[s], off + n)
    return need


_cache = {}


def _raws():
    if "raws" not in _cache:
        _cache["raws"] = [gen_block("T", 9500 + i, SIZE) for i in range(NSRC)]
    return _cache["raws"]


def _stored(oracle, codec):
    if codec not in _cache:
        enc = {"none": lambda b: b, "lz4": lambda b: oracle.lz4_compress(b)[1], "zstd": oracle.zstd_compress_l1}[codec]
        _cache[codec] = [enc(r) for r in _raws()]
    return list(_cache[codec])


def _read(codec, objs, parts, caps=None, crcs=None):
    c = C.NewCompressor(codec)
    caps = caps or [SIZE] * len(objs)
    dst = Dst([sum(p[2] for p in ps) + (j % 2) for j, ps in enumerate(parts)])
    sres, rres, got = c.ReadBatch(list(zip(objs, caps)), dst.views, _plan(parts), crcs=crcs)
    return dst, _codes(sres), _codes(rres), got


def _in_mode(mode, fn):
    prev = C.set_read_decode_mode(mode)
    try:
        return fn()
    finally:
        C.set_read_decode_mode(prev)


def small_batch_case(oracle):
    """full mode, then prefix mode, on the 6-source plan; raises on a difference"""
    parts, stored = _parts(), _stored(oracle, "lz4")
    want = C.read_expect(_raws(), _plan(parts))
    full = _in_mode("full", lambda: _read("lz4", stored, parts))
    pre = _in_mode("prefix", lambda: _read("lz4", stored, parts))
    assert full[1] == [(SIZE, None)] * NSRC
    need = _need(parts, NSRC)
    assert need[0] == 100 and need[1] == SIZE and need[5] == 0
    assert pre[1] == [(min(SIZE, n), None) for n in need]
    assert pre[2] == full[2] == [(len(w), None) for w in want]
    for j, w in enumerate(want):
        full[0].check(j, w)
        pre[0].check(j, w)
    assert C.read_decode_mode() == "full"


def test_read_prefix_small_batch(gpu, oracle):
    small_batch_case(oracle)


def test_read_prefix_one_workgroup_path(gpu):
    """JFS_LZ4_SPLIT_MAX is read once: a fresh child with the small-batch path
    switched off runs the same case through the one-workgroup kernel"""
    code = ("import os\n"
            "from tests import oracle_ctypes\n"
            "from tests.test_read_prefix_gpu import small_batch_case\n"
            "small_batch_case(oracle_ctypes.Oracle(os.path.join('oracle', '_build', 'liboracle.so')))\n"
            "print('verdict: equal')\n")
    env = dict(os.environ, JFS_LZ4_SPLIT_MAX="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "verdict: equal" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_read_prefix_sealed_with_checksums(gpu, oracle):
    algo, parts, raws = E.AES256GCM_RSA, _parts(), _raws()
    rng = random.Random(6)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    params = [(rb(E.key_size(algo)), rb(12), rb(w)) for w in (256, 1, 0, 1, 7, 2)]
    pairs = [(bytearray(E.envelope_bound(L.ALGO_LZ4, len(r), len(p[2]))), r) for r, p in zip(raws, params)]
    res = E.compress_seal_batch(L.ALGO_LZ4, algo, pairs, params)
    assert all(e is None for _, e in res)
    envs = [bytes(d[:n]) for (d, _), (n, _) in zip(pairs, res)]
    keys = [p[0] for p in params]
    crcs = [oracle.crc32c(e) for e in envs]
    want = C.read_expect(raws, _plan(parts))
    need = _need(parts, NSRC)

    def call(crc):
        dst = Dst([sum(p[2] for p in ps) + (j % 2) for j, ps in enumerate(parts)])
        sres, rres, got = E.read_open_batch(L.ALGO_LZ4, algo, [(e, SIZE) for e in envs], keys, dst.views, _plan(parts),
                                            crcs=crc)
        return dst, _codes(sres), _codes(rres), got

    full = _in_mode("full", lambda: call(crcs))
    pre = _in_mode("prefix", lambda: call(crcs))
    assert full[1] == [(SIZE, None)] * NSRC and pre[1] == [(min(SIZE, n), None) for n in need]
    assert pre[2] == full[2] == [(len(w), None) for w in want] and pre[3] == full[3] == crcs
    for j, w in enumerate(want):
        pre[0].check(j, w)
    # one wrong expected CRC: that source fails its checksum, the reads it feeds fail untouched
    wrong = list(crcs)
    wrong[3] ^= 1
    dst, sres, rres, got = _in_mode("prefix", lambda: call(wrong))
    assert sres[3] == (0, L.JFS_ERR_CHECKSUM)
    assert [sres[i] for i in (0, 1, 2, 4, 5)] == [(min(SIZE, need[i]), None) for i in (0, 1, 2, 4, 5)]
    fed = {j for j, p in enumerate(parts) if any(s == 3 for s, _, _ in p)}
    assert fed
    for j, w in enumerate(want):
        if j in fed:
            assert rres[j] == (0, L.JFS_ERR_CORRUPT), j
            dst.check(j, b"")
        else:
            assert rres[j] == (len(w), None), j
            dst.check(j, w)


def test_read_prefix_short_source(gpu, oracle):
    """a source that decodes to fewer bytes than a segment needs fails that read only"""
    raws = [gen_block("T", 9600, 1000), _raws()[0]]
    stored = [oracle.lz4_compress(r)[1] for r in raws]
    parts = [[(0, 900, 200), (1, 0, 50)], [(0, 0, 1000), (-1, 0, 3)], [(1, 70000, 5000)]]
    for mode in ("full", "prefix"):
        dst, sres, rres, got = _in_mode(mode, lambda: _read("lz4", stored, parts))
        assert sres == [(1000, None), (SIZE if mode == "full" else 75000, None)], (mode, sres)
        assert rres == [(0, L.JFS_ERR_CORRUPT), (1003, None), (5000, None)], (mode, rres)
        dst.check(0, b"")
        dst.check(1, raws[0] + bytes(3))
        dst.check(2, raws[1][70000:75000])


@pytest.mark.parametrize("codec", ["zstd", "none"])
def test_read_prefix_other_codecs_decode_whole(gpu, oracle, codec):
    parts, stored = _parts(), _stored(oracle, codec)
    want = C.read_expect(_raws(), _plan(parts))
    full = _in_mode("full", lambda: _read(codec, stored, parts))
    pre = _in_mode("prefix", lambda: _read(codec, stored, parts))
    assert pre[1] == full[1] == [(SIZE, None)] * NSRC
    assert pre[2] == full[2] == [(len(w), None) for w in want]
    for j, w in enumerate(want):
        full[0].check(j, w)
        pre[0].check(j, w)
