"""GPU: jfs_compact_seal_batch with JFS_COMPACT_SPLICE all, for
all three ciphers and both table layouts.  Sources of 300,000 text bytes: three
frames, the last one short -- the smallest object with a full and a partial
frame to pass.  Every returned envelope is opened with the CPU AEAD; its payload
must be what jfs_compact_batch writes with the switch on over the plaintext
sources, and decode (CPU oracle) to the gathered bytes; header, crc and the
counters are checked.  A shifted plan equals the switch off exactly; with on and
off the sealed call is what it was; a source whose tag fails, a source without a
table, a short dst and a damaged checksum word behave as the header says.

test_one_overwrite_in_the_middle_frame fails without the feature: the counters
stay 0 and the payloads are whole re-encodes."""
import pytest
import torch  # noqa: F401  (before the library is loaded below: both then share one HIP runtime)

from juicefs_amd import _lib as L
from juicefs_amd import compress as C
from juicefs_amd import encrypt as E
from juicefs_amd.blockgen import gen_block
from tests.test_compact_seal_gpu import CIPHERS, Dst, _codes, _params
from tests.test_splice_plan import parse_any

pytestmark = pytest.mark.gpu
B = 128 << 10
D0 = 300000
AT = B + 50000  # the overwrite: inside the middle frame
Z = C.NewCompressor("zstd")
ZSTD = L.ALGO_ZSTD


@pytest.fixture(params=["off", "on"], ids=["table8", "table12"])
def layout(request, gpu):
    """seekable parse mode and the table layout under test; every switch put back afterwards"""
    prev = (C.set_zstd_parse_mode("seekable"), C.set_zstd_seek_csum_mode(request.param), C.set_compact_splice_mode("off"))
    C.compact_splice_counts(reset=True)
    yield request.param == "on"
    C.set_zstd_parse_mode(prev[0])
    C.set_zstd_seek_csum_mode(prev[1])
    C.set_compact_splice_mode(prev[2])


_raws = {}


def raws():
    """two text sources, two overwrites, one more text source: made once"""
    if not _raws:
        _raws["v"] = ([gen_block("T", 9800 + i, D0) for i in range(2)] + [gen_block("R", 9810 + i, 4096) for i in range(2)] +
                      [gen_block("T", 9820, D0)])
    return _raws["v"]


def store(blocks):
    """the stored plaintext objects of `blocks` in the current modes (CompressBatch)"""
    dsts = [bytearray(Z.CompressBound(len(r))) for r in blocks]
    res = Z.CompressBatch([(d, r) for d, r in zip(dsts, blocks)])
    assert all(e is None for _, e in res), res
    return [bytes(d[:n]) for d, (n, _) in zip(dsts, res)]


def seal(oracle, algo, payloads, params):
    """dataEncryptor.Encrypt of every payload, on the CPU"""
    return [oracle.envelope(w, nonce, oracle.seal(CIPHERS[algo], key, nonce, p)) for p, (key, nonce, w) in zip(payloads, params)]


def opened(oracle, algo, env, param):
    """(header, payload) of an envelope this call returned, opened on the CPU; the payload is None if the tag fails"""
    key, nonce, w = param
    hdr = bytes([len(w) >> 8, len(w) & 255, 12]) + w + nonce
    assert env[:len(hdr)] == hdr
    return hdr, oracle.open(CIPHERS[algo], key, nonce, env[len(hdr):])


def totals(plan):
    seg_first, seg = plan
    return [sum(s[3] for s in seg[seg_first[j]:seg_first[j + 1]]) for j in range(len(seg_first) - 1)]


def sealed_call(algo, envs, caps_src, keys, op, plan, caps=None):
    if caps is None:
        caps = [E.envelope_bound(ZSTD, t, len(p[2])) for t, p in zip(totals(plan), op)]
    dst = Dst(caps)
    sres, ores, crcs = E.compact_seal_batch(ZSTD, algo, list(zip(envs, caps_src)), keys, dst.views, op, plan, with_crc=True)
    outs = [bytes(v[:n]) if e is None else None for v, (n, e) in zip(dst.views, ores)]
    return dst, sres, ores, crcs, outs


def plain_call(stored, caps_src, plan):
    """jfs_compact_batch over the plaintext objects"""
    outs = [bytearray(Z.CompressBound(t)) for t in totals(plan)]
    sres, ores, crcs = Z.CompactBatch(list(zip(stored, caps_src)), outs, plan, with_crc=True)
    return sres, ores, [bytes(o[:n]) if e is None else None for o, (n, e) in zip(outs, ores)]


def overwrite_plan(pairs):
    """[(object, overwrite)]: one output per pair, the object with 4 KiB of the overwrite at AT"""
    seg_first, seg = [0], []
    for i, w in pairs:
        seg += [(i, 0, 0, AT), (w, 0, AT, 4096), (i, AT + 4096, AT + 4096, D0 - AT - 4096)]
        seg_first.append(len(seg))
    return seg_first, seg


SRC_WRAPPED = [256, 1, 0, 1, 2]  # payloads at 15 + wrapped_len: 271, 16, 15, 16, 17 bytes into the envelope
CAPS = [D0, D0, 4096, 4096, D0]


def setup(oracle, algo):
    rs = raws()
    stored = store(rs)
    for s in (stored[0], stored[1], stored[4]):
        assert len(parse_any(s)[0]) == 3
    sp = _params(algo, SRC_WRAPPED, 11)
    return rs, stored, sp, [p[0] for p in sp], seal(oracle, algo, stored, sp)


@pytest.mark.parametrize("algo", list(CIPHERS))
def test_one_overwrite_in_the_middle_frame(gpu, layout, oracle, algo):
    rs, stored, sp, keys, envs = setup(oracle, algo)
    plan = overwrite_plan([(0, 2), (1, 3)])
    op = _params(algo, [0, 257], 12)
    C.set_compact_splice_mode("on")
    p_src, p_out, want = plain_call(stored[:4], CAPS[:4], plan)
    assert C.compact_splice_counts(reset=True)[:3] == (2, 4, 2)
    C.set_compact_splice_mode("all")
    dst, sres, ores, crcs, outs = sealed_call(algo, envs[:4], CAPS[:4], keys[:4], op, plan)
    counts = C.compact_splice_counts()
    print("counts", counts, "sources", _codes(sres), "outputs", _codes(ores))
    assert counts[:3] == (2, 4, 2)  # per object: 2 passed, 1 re-encoded
    assert counts[3] == sum(parse_any(stored[i])[0][k][0] for i in (0, 1) for k in (0, 2))
    assert _codes(sres) == [(D0, None), (D0, None), (4096, None), (4096, None)] == _codes(p_src)
    gathered = C.read_expect(rs[:4], plan)
    for j in range(2):
        hdr, pay = opened(oracle, algo, outs[j], op[j])
        assert pay == want[j], j                                    # jfs_compact_batch with the switch on
        assert oracle.zstd_decompress(pay, D0) == (D0, gathered[j])
        assert len(parse_any(pay)[0]) == 3 and (parse_any(pay)[1] == 12) == layout
        assert ores[j] == (len(hdr) + len(pay) + 16, None) and ores[j][0] <= E.envelope_bound(ZSTD, D0, len(op[j][2]))
        assert crcs[j] == oracle.crc32c(outs[j])
        dst.check(j, outs[j])


@pytest.mark.parametrize("algo", list(CIPHERS))
def test_shifted_plan_is_the_switch_off(gpu, layout, oracle, algo):
    rs, stored, sp, keys, envs = setup(oracle, algo)
    plan = ([0, 1, 2], [(0, 4096, 0, D0 - 4096), (1, 4096, 0, D0 - 4096)])
    op = _params(algo, [1, 0], 13)
    C.set_compact_splice_mode("all")
    _, s_all, o_all, c_all, outs_all = sealed_call(algo, envs[:2], CAPS[:2], keys[:2], op, plan)
    assert C.compact_splice_counts() == (0, 0, 0, 0)
    C.set_compact_splice_mode("off")
    _, s_off, o_off, c_off, outs_off = sealed_call(algo, envs[:2], CAPS[:2], keys[:2], op, plan)
    assert outs_all == outs_off and outs_all[0] is not None
    assert (_codes(s_all), _codes(o_all), c_all) == (_codes(s_off), _codes(o_off), c_off)
    assert _codes(s_off) == [(D0, None)] * 2


@pytest.mark.parametrize("algo", list(CIPHERS))
def test_on_and_off_leave_the_sealed_call_alone(gpu, layout, oracle, algo):
    rs, stored, sp, keys, envs = setup(oracle, algo)
    plan = overwrite_plan([(0, 2), (1, 3)])
    op = _params(algo, [0, 257], 14)
    got = {}
    for mode in ("off", "on"):
        C.set_compact_splice_mode(mode)
        _, sres, ores, crcs, outs = sealed_call(algo, envs[:4], CAPS[:4], keys[:4], op, plan)
        got[mode] = (_codes(sres), _codes(ores), crcs, outs)
        assert C.compact_splice_counts() == (0, 0, 0, 0)
    assert got["on"] == got["off"]
    # and that is the whole re-encode: compress_seal_batch of the gathered bytes
    gathered = C.read_expect(rs[:4], plan)
    pairs = [(bytearray(E.envelope_bound(ZSTD, D0, len(p[2]))), g) for g, p in zip(gathered, op)]
    ref = E.compress_seal_batch(ZSTD, algo, pairs, op)
    assert [bytes(d[:n]) for (d, _), (n, _) in zip(pairs, ref)] == got["off"][3]


@pytest.mark.parametrize("algo", list(CIPHERS))
def test_flipped_tag_bit_in_a_mixed_call(gpu, layout, oracle, algo):
    rs, stored, sp, keys, envs = setup(oracle, algo)
    bad = bytearray(envs[0])
    bad[-1] ^= 0x10
    plan = overwrite_plan([(0, 2), (1, 3)])
    plan[1].append((0, 0, 0, D0))  # a third output: source 0 whole
    plan[0].append(len(plan[1]))
    op = _params(algo, [0, 257, 3], 15)
    C.set_compact_splice_mode("on")
    _, _, want = plain_call(stored[:4], CAPS[:4], plan)
    C.compact_splice_counts(reset=True)
    C.set_compact_splice_mode("all")
    dst, sres, ores, crcs, outs = sealed_call(algo, [bytes(bad)] + envs[1:4], CAPS[:4], keys[:4], op, plan)
    assert _codes(sres) == [(0, L.JFS_ERR_AUTH), (D0, None), (4096, None), (4096, None)]
    assert [c for _, c in _codes(ores)] == [L.JFS_ERR_CORRUPT, None, L.JFS_ERR_CORRUPT]
    assert C.compact_splice_counts()[:3] == (1, 2, 1)
    dst.check(0, b"")  # nothing written for a failed output
    dst.check(2, b"")
    hdr, pay = opened(oracle, algo, outs[1], op[1])
    assert pay == want[1] and crcs == [0, oracle.crc32c(outs[1]), 0]
    assert oracle.zstd_decompress(pay, D0) == (D0, C.read_expect(rs[:4], plan)[1])
    dst.check(1, outs[1])


@pytest.mark.parametrize("algo", list(CIPHERS))
def test_source_without_a_table_beside_seekable_ones(gpu, layout, oracle, algo):
    rs, stored, sp, keys, envs = setup(oracle, algo)
    C.set_zstd_parse_mode("fast")
    flat = store([rs[4]])[0]  # one frame, no table
    C.set_zstd_parse_mode("seekable")
    assert parse_any(flat) is None
    stored = stored[:4] + [flat]
    envs = envs[:4] + seal(oracle, algo, [flat], sp[4:])
    # output 0: frame 0 of source 0, then source 4 from B on; output 1: source 1 with its overwrite
    plan = ([0, 2, 5], [(0, 0, 0, B), (4, B, B, D0 - B)] + overwrite_plan([(1, 3)])[1])
    op = _params(algo, [5, 0], 16)
    C.set_compact_splice_mode("on")
    p_src, _, want = plain_call(stored, CAPS, plan)
    C.compact_splice_counts(reset=True)
    C.set_compact_splice_mode("all")
    dst, sres, ores, crcs, outs = sealed_call(algo, envs, CAPS, keys, op, plan)
    assert C.compact_splice_counts()[:3] == (2, 3, 3)  # its pieces are FRESH
    assert _codes(sres) == _codes(p_src) and all(e is None for _, e in sres)
    gathered = C.read_expect(rs, plan)
    for j in range(2):
        hdr, pay = opened(oracle, algo, outs[j], op[j])
        assert pay == want[j] and oracle.zstd_decompress(pay, D0) == (D0, gathered[j])
        assert crcs[j] == oracle.crc32c(outs[j])
        dst.check(j, outs[j])


@pytest.mark.parametrize("algo", list(CIPHERS))
def test_short_buffer_as_before(gpu, layout, oracle, algo):
    rs, stored, sp, keys, envs = setup(oracle, algo)
    plan = overwrite_plan([(0, 2), (1, 3)])
    op = _params(algo, [0, 257], 17)
    bounds = [E.envelope_bound(ZSTD, D0, len(p[2])) for p in op]
    C.set_compact_splice_mode("all")
    dst, sres, ores, crcs, outs = sealed_call(algo, envs[:4], CAPS[:4], keys[:4], op, plan, caps=[bounds[0] - 1, bounds[1]])
    assert _codes(ores)[0] == (0, L.JFS_ERR_SHORT_BUFFER) and ores[1][1] is None
    assert C.compact_splice_counts()[:3] == (1, 2, 1)
    dst.check(0, b"")
    dst.check(1, outs[1])
    assert opened(oracle, algo, outs[1], op[1])[1] is not None


@pytest.mark.parametrize("algo", list(CIPHERS))
def test_damaged_checksum_word_in_a_decoded_frame(gpu, oracle, algo):
    prev = (C.set_zstd_parse_mode("seekable"), C.set_zstd_seek_csum_mode("on"), C.set_compact_splice_mode("all"))
    try:
        rs, stored, sp, keys, envs = setup(oracle, algo)
        b = bytearray(stored[0])
        b[len(b) - (12 * 3 + 17) + 8 + 12 * 1 + 8] ^= 0x40  # frame 1's checksum word: the frame the overwrite decodes
        envs = seal(oracle, algo, [bytes(b)], sp[:1]) + envs[1:4]
        plan = overwrite_plan([(0, 2), (1, 3)])
        op = _params(algo, [0, 257], 18)
        dst, sres, ores, crcs, outs = sealed_call(algo, envs, CAPS[:4], keys[:4], op, plan)
        assert _codes(sres) == [(0, L.JFS_ERR_CHECKSUM), (D0, None), (4096, None), (4096, None)]
        assert [c for _, c in _codes(ores)] == [L.JFS_ERR_CORRUPT, None]
        dst.check(0, b"")
        assert opened(oracle, algo, outs[1], op[1])[1] is not None
    finally:
        C.set_zstd_parse_mode(prev[0])
        C.set_zstd_seek_csum_mode(prev[1])
        C.set_compact_splice_mode(prev[2])
