"""GPU: prefix LZ4 decode (jfs_lz4_decompress_prefix_device, the one-workgroup
kernel's PREFIX instantiation, and jfs_lz4_decompress_prefix_device_small, the
small-batch path cut to min(total, want)) against the CPU oracle's full decode.

Contract (include/jfs_gpucodec.h): ret = min(size, want) and dst[0, ret) is
the full decode's prefix for a well-formed stream; the full decoder's negative
value for a stream rejected in front of want; either of the two behind it.
Every dst sits at an odd offset inside a canary-filled tensor and the whole
tensor is checked outside [dst, dst + dst_cap)."""
import numpy as np
import pytest
import torch

from juicefs_amd import device as D
from juicefs_amd.blockgen import gen_block

pytestmark = pytest.mark.gpu

CANARY = 0xEE
PATHS = ["one_workgroup", "small"]


def walk(c: bytes):
    """LZ4 sequences of a well-formed block: [(token position, output position
    at which the sequence begins, position of its offset field or None for the
    final literal run)]"""
    seqs, ip, op, n = [], 0, 0, len(c)
    while ip < n:
        t0, o0, tok = ip, op, c[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = c[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        ip += ll
        op += ll
        if ip >= n:
            seqs.append((t0, o0, None))
            break
        seqs.append((t0, o0, ip))
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = c[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        op += ml + 4
    return seqs, op


def bad_offset_at(c: bytes, q_min: int):
    """c with the offset of the first sequence that begins at output position
    >= q_min set to 0xFFFF (more than the bytes produced there: rejected);
    returns (stream, q)"""
    seqs, _ = walk(c)
    t0, q, offpos = next(s for s in seqs if s[1] >= q_min and s[2] is not None)
    assert q < 65535 - 300
    b = bytearray(c)
    b[offpos:offpos + 2] = b"\xff\xff"
    return bytes(b), q


def run(dev, path, comps, caps, wants):
    """Decode comps[i] into a caps[i]-byte dst with wants[i]; sources at mixed
    alignments, every dst at an odd offset of a canary-filled tensor.  Returns
    (rets, [dst[0, cap) as numpy]) after checking every byte outside the dsts."""
    so, do, off, doff = [], [], 0, 64
    for i, (s, c) in enumerate(zip(comps, caps)):
        off = (off + 15) // 16 * 16 + (5 * i) % 16
        so.append(off)
        off += len(s) + 64
        doff = (doff + 15) // 16 * 16 + (2 * i + 1) % 16
        do.append(doff)
        doff += c + 80
    host = np.zeros(off + 64, dtype=np.uint8)
    for s, o in zip(comps, so):
        host[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    src_t = torch.from_numpy(host).to(dev)
    dst_t = torch.full((doff + 64,), CANARY, dtype=torch.uint8, device=dev)
    lens = [len(s) for s in comps]
    desc = D.make_desc(src_t, so, lens, dst_t, do, caps)
    want_t = torch.tensor(wants, dtype=torch.int32, device=dev)
    ret = torch.full((len(comps),), 12345, dtype=torch.int32, device=dev)
    if path == "small":
        D.lz4_decompress_prefix_small(desc, want_t, ret, lens, caps)
    else:
        D.lz4_decompress_prefix(desc, want_t, ret)
    torch.cuda.synchronize()
    img = dst_t.cpu().numpy()
    outside = np.ones(len(img), dtype=bool)
    for o, c in zip(do, caps):
        outside[o:o + c] = False
    bad = np.nonzero(outside & (img != CANARY))[0]
    assert bad.size == 0, f"{path}: byte {bad[0]} outside every dst was written ({bad.size} in all)"
    return ret.cpu().tolist(), [img[o:o + c] for o, c in zip(do, caps)]


def check_prefix(path, rets, outs, raws, wants, tail_canary):
    for i, (r, o, raw, w) in enumerate(zip(rets, outs, raws, wants)):
        exp = min(len(raw), max(w, 0))
        assert r == exp, (path, i, w, r, exp)
        assert o[:r].tobytes() == raw[:r], (path, i, w)
        if tail_canary:
            assert (o[r:] == CANARY).all(), (path, i, w, "a byte at or above ret was written")


_cache = {}


def text(oracle, n, seed):
    if (n, seed) not in _cache:
        raw = gen_block("T", seed, n)
        comp = oracle.lz4_compress(raw)[1]
        assert oracle.lz4_decompress(comp, n) == (n, raw)
        _cache[(n, seed)] = (raw, comp)
    return _cache[(n, seed)]


@pytest.mark.parametrize("path", PATHS)
def test_prefix_text_wants(gpu, oracle, path):
    size = 256 << 10
    raw, comp = text(oracle, size, 9100)
    cap = size + 300
    wants = [-1, 0, 1, 15, 16, 17, 4095, 4096, 4097, 65537, size - 1, size, size + 1, cap, cap + 5]
    D.lz4_split_counts(reset=True)
    rets, outs = run(gpu, path, [comp] * len(wants), [cap] * len(wants), wants)
    # the small-batch path decodes all of them itself, and writes nothing at or above ret
    check_prefix(path, rets, outs, [raw] * len(wants), wants, tail_canary=path == "small")
    if path == "small":
        done, handed = D.lz4_split_counts()[:2]
        assert (done, handed) == (len(wants), 0)


@pytest.mark.parametrize("path", PATHS)
def test_prefix_long_tokens_straddle_want(gpu, oracle, path):
    """one overlapped match of offset 1, one of offset 3 (the modulo loop) and
    one literal run (the serial path of the one-workgroup kernel), each cut at
    every want"""
    n = 1 << 20
    rng = np.random.default_rng(77)
    raws = [bytes(n), (b"abc" * (n // 3 + 1))[:n], rng.integers(0, 256, n, dtype=np.uint8).tobytes()]
    comps = [oracle.lz4_compress(r)[1] for r in raws]
    assert len(comps[0]) < 5000 and len(comps[1]) < 5000 and len(comps[2]) > n
    wants = [1, 5, 70000, (1 << 19) + 1]
    cs = [c for c in comps for _ in wants]
    rs = [r for r in raws for _ in wants]
    ws = wants * len(raws)
    D.lz4_split_counts(reset=True)
    rets, outs = run(gpu, path, cs, [n + 7] * len(cs), ws)
    check_prefix(path, rets, outs, rs, ws, tail_canary=False)
    if path == "small":  # what it decoded itself: nothing at or above ret (the counters tell which blocks)
        done, handed = D.lz4_split_counts()[:2]
        assert done + handed == len(cs)
        if handed == 0:
            check_prefix(path, rets, outs, rs, ws, tail_canary=True)


def test_prefix_stop_really_stops(gpu, oracle):
    """one-workgroup kernel: a text window produces a few KiB of output, so a
    stop at 4 KiB leaves everything from 512 KiB on untouched"""
    n = 1 << 20
    raw, comp = text(oracle, n, 9200)
    rets, outs = run(gpu, "one_workgroup", [comp], [n], [4096])
    assert rets == [4096] and outs[0][:4096].tobytes() == raw[:4096]
    assert (outs[0][512 << 10:] == CANARY).all()


@pytest.mark.parametrize("path", PATHS)
def test_prefix_fault_in_front_of_want(gpu, oracle, path):
    size = 256 << 10
    raw, comp = text(oracle, size, 9100)
    bad, q = bad_offset_at(comp, 30000)
    assert 30000 <= q < 35000
    full, _ = oracle.lz4_decompress(bad, size)
    assert full < 0
    # the full GPU decoder gives the same value (the reference of the contract)
    so = torch.from_numpy(np.frombuffer(bad, dtype=np.uint8).copy()).to(gpu)
    dst = torch.zeros(size, dtype=torch.uint8, device=gpu)
    ret = torch.zeros(1, dtype=torch.int32, device=gpu)
    D.lz4_decompress(D.make_desc(so, [0], [len(bad)], dst, [0], [size]), ret)
    torch.cuda.synchronize()
    assert int(ret[0].item()) == full
    rets, _ = run(gpu, path, [bad], [size], [60000])
    assert rets == [full]


@pytest.mark.parametrize("path", PATHS)
def test_prefix_fault_behind_want(gpu, oracle, path):
    size = 256 << 10
    raw, comp = text(oracle, size, 9100)
    bad, q = bad_offset_at(comp, 50000)
    assert 50000 <= q < 55000
    full, _ = oracle.lz4_decompress(bad, size)
    assert full < 0
    rets, outs = run(gpu, path, [bad], [size], [20000])
    assert rets[0] in (full, 20000), rets
    if rets[0] == 20000:
        assert outs[0][:20000].tobytes() == raw[:20000]


def test_prefix_both_paths_agree(gpu, oracle):
    rng = np.random.default_rng(5)
    t64 = gen_block("T", 9300, 64)
    raws = [gen_block("T", 9301, 70000), bytes(70000), rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(), b"a",
            t64, t64, gen_block("T", 9302, 40000)]
    comps = [oracle.lz4_compress(r)[1] for r in raws] + [b""]
    caps = [70000, 70001, 5000, 1, 64, 63, 40000, 100]
    wants = [33333, 69999, 4999, 1, 64, 63, 12345, 10]
    got = {p: run(gpu, p, comps, caps, wants) for p in PATHS}
    ra, oa = got[PATHS[0]]
    rb, ob = got[PATHS[1]]
    assert ra == rb
    for i, r in enumerate(ra):
        full, dec = oracle.lz4_decompress(comps[i], caps[i]) if comps[i] else (-1, b"")
        if full >= 0:
            assert r == min(full, wants[i]), (i, r, full)
            assert oa[i][:r].tobytes() == ob[i][:r].tobytes() == dec[:r], i
        else:
            assert r == full, (i, r, full)
    assert ra[5] < 0 and ra[7] == -1  # dst_cap 63 cannot hold the 64 bytes; the empty source
