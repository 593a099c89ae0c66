"""GPU parity of the one-workgroup LZ4 decode kernel (lz4_decode.hip, reached
directly through jfs_lz4_decompress_device / jfs_lz4_decompress_prefix_device)
on streams made for the parser's deferred match-length test
(lz4_walkstep.h): the walk goes on from a token before it knows whether the
token's first match-length extension byte is 255, and has to come back when it
is.  Blocks of 20..40 KiB compressed (an 8 KiB span: at least three spans, so
next-span walking, fix-up rounds and span boundaries occur) with matches of
>= 274 bytes ("slow" tokens) at: lane 0's segment, a segment's last token, a
span's last token (its exit is the span's), a span's first token, across a
window end, two in a row, behind a literal-length extension, next to literal
runs of >= 270 bytes, extension byte 254 (not slow), a 255 token byte where no
extension is read; and the same streams truncated inside a slow token's
fields.  Bar: the oracle's return value (negative ones included) and bytes."""
import random

import numpy as np
import pytest

from juicefs_amd.blockgen import gen_block
from tests.test_lz4_kernel_gpu import _check, _tok

pytestmark = pytest.mark.gpu

SEGB, SPANB, WINB = 128, 8192, 2048
MODES = ["lane0", "seglast", "spanlast", "spanfirst", "winend", "pair", "litext", "litrun", "e254", "tok255"]


def build(mode, seed, size=30000):
    """A valid LZ4 block of about `size` compressed bytes: short tokens, and the
    mode's token wherever the compressed position asks for it.  Returns the
    stream and the compressed positions of its slow tokens."""
    rng = random.Random(seed)
    out = bytearray()
    produced = 0
    base = 0          # start of the parser's current span (a chain position)
    slow_at = []
    follow = 0        # slow tokens still to emit right behind this one

    def emit(ll, ml, slow=False):
        nonlocal produced, base
        lits = bytes(rng.randrange(256) for _ in range(ll))
        if produced + ll == 0:
            lits, ll = lits + b"x", ll + 1
        off = rng.randrange(1, min(produced + ll, 65535) + 1)
        pos = len(out)
        if slow:
            slow_at.append(pos)
        out.extend(_tok(lits, off, ml))
        produced += ll + ml
        if len(out) >= base + SPANB:  # this was the span's last token
            base = len(out)

    def long_ml():
        # extension bytes 255 0 / 255 k / 255 255 k
        return rng.choice([19 + 255, 19 + 255 + rng.randrange(1, 255), 19 + 510 + rng.randrange(0, 255)])

    while len(out) < size:
        pos = len(out)
        rel = pos - base
        ll, ml = rng.randrange(0, 7), rng.randrange(4, 19)
        want = False
        if follow:
            follow -= 1
            want = True
        elif mode == "lane0":
            want = 20 <= rel < SEGB and rng.randrange(4) == 0
        elif mode == "seglast":
            want = rel % SEGB >= SEGB - 6
        elif mode == "spanlast":
            want = rel >= SPANB - 6
        elif mode == "spanfirst":
            want = rel == 0 and pos > 0
        elif mode == "winend":
            want = rel % WINB >= WINB - 24 or pos % WINB >= WINB - 24
        elif mode == "pair":
            want = rng.randrange(12) == 0
            follow = 1 if want else 0
        elif mode == "litext":  # a one-byte literal extension and a 255 match extension
            want = rng.randrange(10) == 0
            if want:
                ll = rng.randrange(15, 15 + 255)
        elif mode == "litrun":  # e1 == 255: the literal length takes the exact rule, the match may too
            if rng.randrange(40) == 0:
                emit(rng.choice([270, 271, 300, 525]), long_ml() if rng.randrange(2) else 9, slow=True)
                continue
            want = rng.randrange(15) == 0
        elif mode == "e254":  # 19 + 254: extension byte 254, not slow
            if rng.randrange(8) == 0:
                emit(ll, 19 + 254)
                continue
            want = rng.randrange(30) == 0
        elif mode == "tok255":  # the byte at q is the next token's 0xFF; this token reads no extension
            if rng.randrange(8) == 0:
                emit(ll, rng.randrange(4, 19))
                emit(rng.randrange(15, 40), long_ml() if rng.randrange(3) == 0 else 19 + rng.randrange(0, 200), slow=True)
                continue
        if want:
            emit(ll, long_ml(), slow=True)
        else:
            emit(ll, ml)
    out += bytes([0xF0, 5]) + bytes(rng.randrange(256) for _ in range(20))
    return bytes(out), slow_at


_blocks = {}


def blocks():
    if not _blocks:
        for i, m in enumerate(MODES):
            _blocks[m] = build(m, 100 + i, size=20000 + 2000 * i)
    return _blocks


def text_block(oracle, seed):
    return oracle.lz4_compress(gen_block("T", seed, 1 << 16))[1]


def full_size(oracle, c):
    n, _ = oracle.lz4_decompress(c, 64 << 20)
    assert n > 0
    return n


def test_builder_places_the_tokens():
    for m, (c, slow_at) in blocks().items():
        assert 20000 <= len(c) <= 40960, (m, len(c))
        assert len(slow_at) >= (2 if m.startswith("span") else 8), (m, len(slow_at))


@pytest.mark.parametrize("mode", MODES)
def test_single_block(gpu, oracle, mode):
    c, _ = blocks()[mode]
    _check(gpu, oracle, [c], [full_size(oracle, c)])


def test_batch_of_seven_with_text(gpu, oracle):
    b = blocks()
    comps = [b["seglast"][0], text_block(oracle, 1), b["spanlast"][0], b["pair"][0], text_block(oracle, 2), b["winend"][0],
             b["litrun"][0]]
    _check(gpu, oracle, comps, [full_size(oracle, c) for c in comps])


@pytest.mark.parametrize("mis_d", [1, 5, 8, 15])
def test_destination_alignments(gpu, oracle, mis_d):
    b = blocks()
    comps = [b["spanfirst"][0], b["lane0"][0], b["tok255"][0]]
    _check(gpu, oracle, comps, [full_size(oracle, c) for c in comps], mis_d=mis_d, mis_s=mis_d % 4)


def test_truncated_inside_slow_tokens(gpu, oracle):
    """Streams cut inside each field of a slow token (token byte, literals,
    offset, each extension byte) and in the 70 bytes behind it, where the
    parser's next positions meet the end-of-input rules."""
    comps = []
    for m in ("pair", "seglast", "litext", "litrun"):
        c, slow_at = blocks()[m]
        for at in (slow_at[len(slow_at) // 2], slow_at[-1]):
            for n in list(range(at + 1, at + 8)) + [at + 12, at + 17, at + 18, at + 19, at + 33, at + 64, at + 70]:
                if n < len(c):
                    comps.append(c[:n])
    caps = [1 << 20] * len(comps)
    _check(gpu, oracle, comps, caps)


@pytest.mark.parametrize("batch", ["one", "seven"])
def test_prefix(gpu, oracle, batch):
    import torch
    from juicefs_amd import device as D
    b = blocks()
    names = ["spanlast"] if batch == "one" else ["seglast", "spanlast", "spanfirst", "pair", "winend", "litext", "tok255"]
    comps = [b[m][0] for m in names]
    if batch == "seven":
        comps[3] = text_block(oracle, 3)
    raws = []
    for c in comps:
        n, raw = oracle.lz4_decompress(c, 64 << 20)
        raws.append(raw[:n])
    for pick in ("one", "mid", "cap"):
        caps = [len(r) for r in raws]
        wants = [1 if pick == "one" else (len(r) // 2 + 7 * i) if pick == "mid" else len(r) for i, r in enumerate(raws)]
        slot_s = [(len(c) + 64 + 15) // 16 * 16 for c in comps]
        offs_s = np.cumsum([0] + slot_s[:-1])
        host = np.zeros(int(sum(slot_s)) + 64, dtype=np.uint8)
        for i, c in enumerate(comps):
            host[offs_s[i]:offs_s[i] + len(c)] = np.frombuffer(c, dtype=np.uint8)
        src = torch.from_numpy(host).to(gpu)
        slot_d = [(cp + 64 + 15) // 16 * 16 for cp in caps]
        offs_d = np.cumsum([0] + slot_d[:-1])
        out = torch.full((int(sum(slot_d)) + 64,), 0xEE, dtype=torch.uint8, device=gpu)
        desc = D.make_desc(src, offs_s, [len(c) for c in comps], out, offs_d, caps)
        ret = torch.full((len(comps),), 12345, dtype=torch.int32, device=gpu)
        D.lz4_decompress_prefix(desc, torch.tensor(wants, dtype=torch.int32, device=gpu), ret)
        torch.cuda.synchronize()
        r, img = ret.cpu().tolist(), out.cpu().numpy()
        for i, raw in enumerate(raws):
            exp = min(len(raw), wants[i])
            assert r[i] == exp, (pick, i, wants[i], r[i], exp)
            assert img[offs_d[i]:offs_d[i] + exp].tobytes() == raw[:exp], (pick, i, wants[i])
