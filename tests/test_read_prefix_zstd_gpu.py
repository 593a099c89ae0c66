"""GPU: the read calls on Zstd sources in the three decode modes.  Modes "full"
and "prefix" agree in every field (mode "prefix" stops LZ4 decodes only);
"prefix-all" stops each Zstd decode at the Zstd block a read ends in: the same
out_n and bytes, and src_n = min(size, need).  The plans are those of
tests/test_read_prefix_gpu.py; read buffers sit at odd offsets inside
canary-filled arrays (tests.test_read_gpu.Dst)."""
import random

import pytest

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests.test_read_csum_gpu import Sums
from tests.test_read_gpu import Dst, _codes
from tests.test_read_prefix_gpu import NSRC, SIZE, _in_mode, _need, _parts, _plan, _raws, _read, _stored

pytestmark = pytest.mark.gpu
MODES = ("full", "prefix", "prefix-all")


def _src_n(mode, need, sizes):
    return [(min(s, n) if mode == "prefix-all" else s, None) for s, n in zip(sizes, need)]


def test_mode_names_and_values(gpu, lib):
    assert L.READ_DECODE_PREFIX_ALL == 2
    prev = C.set_read_decode_mode("prefix-all")
    try:
        assert C.read_decode_mode() == "prefix-all" and lib.jfs_read_decode_mode() == 2
        assert lib.jfs_set_read_decode_mode_ext(3) == -1 and lib.jfs_read_decode_mode() == 2
        # the first setter keeps its two modes; from mode 2 it still reports 2 as the previous one
        assert lib.jfs_set_read_decode_mode(2) == -1 and lib.jfs_read_decode_mode() == 2
        assert lib.jfs_set_read_decode_mode(0) == 2 and lib.jfs_set_read_decode_mode_ext(2) == 0
    finally:
        C.set_read_decode_mode(prev)
    with pytest.raises(ValueError):
        C.set_read_decode_mode("prefix-some")


def test_read_zstd_three_modes(gpu, oracle):
    """source 0 is needed to byte 100, source 1 whole, source 5 not at all (need = 0, src_n = 0)"""
    parts, stored = _parts(), _stored(oracle, "zstd")
    want = C.read_expect(_raws(), _plan(parts))
    need = _need(parts, NSRC)
    assert need[0] == 100 and need[1] == SIZE and need[5] == 0
    res = {m: _in_mode(m, lambda: _read("zstd", stored, parts)) for m in MODES}
    for m in MODES:
        dst, sres, rres, got = res[m]
        assert sres == _src_n(m, need, [SIZE] * NSRC), (m, sres)
        assert rres == [(len(w), None) for w in want], m
        for j, w in enumerate(want):
            dst.check(j, w)
    assert res["full"][1:] == res["prefix"][1:]
    assert C.read_decode_mode() == "full"


def test_read_zstd_stats_count_src_n(gpu, oracle, lib):
    """jfs_stats' bytes_out counts src_n"""
    parts, stored = _parts(), _stored(oracle, "zstd")
    need = _need(parts, NSRC)
    lib.jfs_stats_reset()
    _in_mode("prefix-all", lambda: _read("zstd", stored, parts))
    out = (L.JfsOpStats * L.STATS_N)()
    lib.jfs_stats(out, L.STATS_N)
    assert out[L.ALGO_ZSTD * 2 + 1].bytes_out == sum(min(SIZE, n) for n in need), out[L.ALGO_ZSTD * 2 + 1].bytes_out


def test_read_zstd_sealed_with_checksums(gpu, oracle):
    algo, parts, raws = E.AES256GCM_RSA, _parts(), _raws()
    rng = random.Random(16)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    params = [(rb(E.key_size(algo)), rb(12), rb(w)) for w in (256, 1, 0, 1, 7, 2)]
    pairs = [(bytearray(E.envelope_bound(L.ALGO_ZSTD, len(r), len(p[2]))), r) for r, p in zip(raws, params)]
    res = E.compress_seal_batch(L.ALGO_ZSTD, algo, pairs, params)
    assert all(e is None for _, e in res)
    envs = [bytes(d[:n]) for (d, _), (n, _) in zip(pairs, res)]
    keys = [p[0] for p in params]
    crcs = [oracle.crc32c(e) for e in envs]
    want = C.read_expect(raws, _plan(parts))
    need = _need(parts, NSRC)

    def call(crc):
        dst = Dst([sum(p[2] for p in ps) + (j % 2) for j, ps in enumerate(parts)])
        sres, rres, got = E.read_open_batch(L.ALGO_ZSTD, algo, [(e, SIZE) for e in envs], keys, dst.views, _plan(parts),
                                            crcs=crc)
        return dst, _codes(sres), _codes(rres), got

    res = {m: _in_mode(m, lambda: call(crcs)) for m in MODES}
    for m in MODES:
        dst, sres, rres, got = res[m]
        assert sres == _src_n(m, need, [SIZE] * NSRC), (m, sres)
        assert rres == [(len(w), None) for w in want] and got == crcs, m
        for j, w in enumerate(want):
            dst.check(j, w)
    assert res["full"][1:] == res["prefix"][1:]
    # one wrong expected CRC: that source fails its checksum, the reads it feeds fail untouched
    wrong = list(crcs)
    wrong[3] ^= 1
    dst, sres, rres, got = _in_mode("prefix-all", lambda: call(wrong))
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


def test_read_zstd_csum_variant(gpu, oracle):
    """jfs_read_batch_csum: the disk-cache checksums do not depend on where a decode stops"""
    parts, stored = _parts(), _stored(oracle, "zstd")
    want = C.read_expect(_raws(), _plan(parts))
    sums_want = [oracle.crc32c_segments(w) for w in want]
    need = _need(parts, NSRC)
    totals = [sum(p[2] for p in ps) for ps in parts]
    out = {}
    for m in MODES:
        def call():
            dst, sums = Dst([t + (j % 2) for j, t in enumerate(totals)]), Sums(totals)
            res = C.NewCompressor("zstd").ReadBatch(list(zip(stored, [SIZE] * NSRC)), dst.views, _plan(parts),
                                                    with_csum=sums.views)
            return (dst, sums) + tuple(res)
        dst, sums, sres, rres, got, cs = _in_mode(m, call)
        assert _codes(sres) == _src_n(m, need, [SIZE] * NSRC), m
        assert _codes(rres) == [(len(w), None) for w in want], m
        for j, w in enumerate(want):
            dst.check(j, w)
            sums.check(j, sums_want[j])
            assert cs[j] == sums_want[j]
        out[m] = (_codes(sres), _codes(rres), got, cs)
    assert out["full"] == out["prefix"]


def test_read_zstd_short_source(gpu, oracle):
    """a source that decodes to fewer bytes than a segment needs fails that read only"""
    raws = [gen_block("T", 9600, 1000), _raws()[0]]
    stored = [oracle.zstd_compress_l1(r) for r in raws]
    parts = [[(0, 900, 200), (1, 0, 50)], [(0, 0, 1000), (-1, 0, 3)], [(1, 70000, 5000)]]
    for mode in MODES:
        dst, sres, rres, got = _in_mode(mode, lambda: _read("zstd", stored, parts))
        assert sres == [(1000, None), (75000 if mode == "prefix-all" else SIZE, None)], (mode, sres)
        assert rres == [(0, L.JFS_ERR_CORRUPT), (1003, None), (5000, None)], (mode, rres)
        dst.check(0, b"")
        dst.check(1, raws[0] + bytes(3))
        dst.check(2, raws[1][70000:75000])


def test_read_zstd_every_need_is_the_capacity(gpu, oracle):
    """every source needed to its capacity: the full launcher runs, src_n is the size in every mode"""
    stored = _stored(oracle, "zstd")[:3]
    parts = [[(i, SIZE - 5000, 5000), (-1, 0, 9), (i, 0, 77)] for i in range(3)]
    want = C.read_expect(_raws()[:3], _plan(parts))
    for mode in MODES:
        dst, sres, rres, got = _in_mode(mode, lambda: _read("zstd", stored, parts))
        assert sres == [(SIZE, None)] * 3 and rres == [(len(w), None) for w in want], mode
        for j, w in enumerate(want):
            dst.check(j, w)


def test_read_lz4_prefix_all_is_prefix(gpu, oracle):
    """for LZ4, mode 2 is mode 1"""
    parts, stored = _parts(), _stored(oracle, "lz4")
    want = C.read_expect(_raws(), _plan(parts))
    one = _in_mode("prefix", lambda: _read("lz4", stored, parts))
    two = _in_mode("prefix-all", lambda: _read("lz4", stored, parts))
    assert one[1:] == two[1:] and two[1] == [(min(SIZE, n), None) for n in _need(parts, NSRC)]
    for j, w in enumerate(want):
        two[0].check(j, w)
