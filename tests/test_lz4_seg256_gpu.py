"""GPU parity of the one-workgroup LZ4 decode kernel (lz4_decode.hip, reached
through jfs_lz4_decompress_device as in test_lz4_walk_defer_gpu.py) on blocks
made for a segment walk of 256 bytes per lane (a span of 16 KiB): 40..48 KiB
compressed, so three spans -- the next span walked ahead, a span boundary, and
restarts where the copier takes tokens exactly.

(a) text-like data from blockgen; (b) a token that starts at each of the last
3 and first 3 bytes of a segment, and of a span; (c) a match of >= 274 bytes
and a run of >= 270 literals (both take the exact next-position rule) across a
segment end and across a span end; (d) runs of 3-byte tokens, more than a
window's table holds, across a span end; (e) a block with an offset that reaches
before the output's first byte in its second span, with liblz4's exact
negative return.  Bar: the oracle's return
value and bytes."""
import random

import pytest

from juicefs_amd.blockgen import gen_block
from tests.test_lz4_kernel_gpu import _check, _tok

pytestmark = pytest.mark.gpu

SEGB, SPANB = 256, 64 * 256
SIZE = 44000


def build(mode, seed, ks=(0,), size=SIZE):
    """A valid LZ4 block of about `size` compressed bytes of short tokens, with
    the mode's tokens where the compressed position asks for them.  Returns the
    stream, the (position, rel) of the placed tokens (rel: their offset from
    the start of their span) and the positions of all offset fields."""
    rng = random.Random(seed)
    out = bytearray()
    produced = 0
    base = 0      # start of the parser's current span (a chain position)
    nspan = 0
    placed, off_at = [], []

    def emit(ll, ml, mark=False, rel=None):
        nonlocal produced, base, nspan
        lits = bytes(rng.randrange(256) for _ in range(ll))
        if produced + ll == 0:
            lits, ll = lits + b"x", ll + 1
        off = rng.randrange(1, min(produced + ll, 65535) + 1)
        if mark:
            placed.append((len(out), len(out) - base if rel is None else rel))
        t = _tok(lits, off, ml)
        off_at.append(len(out) + 1 + (0 if ll < 15 else 1 + (ll - 15) // 255) + ll)
        out.extend(t)
        produced += ll + ml
        if len(out) >= base + SPANB:  # this was the span's last token
            base = len(out)
            nspan += 1

    def target(rel):
        """The next relative position at which the mode wants a token to start
        (None: nowhere ahead in this span), and what to put there."""
        if mode == "segedge":    # boundary j of the span: k cycles through -3 .. 2
            j = (rel - 3) // SEGB + 1
            return j * SEGB + (j % 6) - 3, "short"
        if mode == "spanedge":   # one k per span boundary
            return SPANB + ks[nspan % len(ks)], "short"
        if mode == "longseg":    # every fourth segment end: a long match / a literal run, alternating
            j = ((rel + 1) // SEGB // 4 + 1) * 4
            return (j * SEGB - 2, "match") if (j // 4) % 2 else (j * SEGB - 6, "lits")
        if mode == "longspan":
            return (SPANB - 2, "match") if nspan % 2 == 0 else (SPANB - 6, "lits")
        return None, None

    while len(out) < size:
        rel = len(out) - base
        if mode == "tcap" and len(out) > 0 and (rel >= SPANB - 3000 or rel < 3000 and nspan > 0):
            emit(0, rng.randrange(4, 19), mark=True)  # 3 bytes
            continue
        t, what = target(rel) if len(out) > 0 else (None, None)
        if t is not None and t == rel:
            if what == "short":
                emit(rng.randrange(0, 7), rng.randrange(4, 19), mark=True)
            elif what == "match":
                emit(rng.randrange(0, 3), rng.choice([19 + 255, 19 + 255 + rng.randrange(1, 255), 19 + 510 + 7]), mark=True)
            else:
                emit(rng.choice([270, 271, 300, 525]), rng.choice([9, 19 + 255 + 3]), mark=True)
        elif t is not None and 3 <= t - rel <= 17:
            emit(t - rel - 3, rng.randrange(4, 19))  # ends exactly at the target
            if t >= SPANB:  # the target is the next span's first token, t - SPANB bytes past the nominal end
                emit(rng.randrange(0, 7), rng.randrange(4, 19), mark=True, rel=t)
        elif t is not None and t - rel < 3:
            emit(rng.randrange(3, 7), rng.randrange(4, 19))  # out of reach: on to the next one
        else:
            emit(rng.randrange(0, 7), rng.randrange(4, 19))
    out += bytes([0xF0, 5]) + bytes(rng.randrange(256) for _ in range(20))
    return bytes(out), placed, off_at


def text_block(oracle, seed):
    for raw in (88 << 10, 80 << 10, 96 << 10, 72 << 10, 104 << 10):
        c = oracle.lz4_compress(gen_block("T", seed, raw))[1]
        if 40 << 10 <= len(c) <= 48 << 10:
            return c
    raise AssertionError(f"no text block of 40..48 KiB compressed (last {len(c)})")


_blocks = {}


def blocks(oracle):
    if not _blocks:
        b = {}
        b["text1"] = (text_block(oracle, 11), [], [])
        b["text2"] = (text_block(oracle, 12), [], [])
        b["segedge"] = build("segedge", 201)
        for i, ks in enumerate([(-3, 0), (-2, 1), (-1, 2)]):
            b[f"spanedge{i}"] = build("spanedge", 210 + i, ks=ks)
        b["longseg"] = build("longseg", 220)
        b["longspan"] = build("longspan", 221)
        b["tcap"] = build("tcap", 230)
        # (e): the offset of a token in the second span := 65535, more than the output so far
        c, placed, off_at = build("plain", 240)
        at = min(o for o in off_at if o >= SPANB + 5000)
        bad = bytearray(c)
        bad[at:at + 2] = b"\xff\xff"
        b["badoffset"] = (bytes(bad), [(at, at - SPANB)], off_at)
        _blocks.update(b)
    return _blocks


def test_builder_places_the_tokens(oracle):
    b = blocks(oracle)
    assert len(b) == 10
    for name, (c, placed, _) in b.items():
        assert 40 << 10 <= len(c) <= 48 << 10, (name, len(c))
    # (b) every k in -3 .. 2 occurs at a segment end and at a span end
    assert {(rel + 3) % SEGB - 3 for _, rel in b["segedge"][1]} == set(range(-3, 3))
    assert len(b["segedge"][1]) >= 100
    ks = set()
    for i in range(3):
        ks |= {rel - SPANB for _, rel in b[f"spanedge{i}"][1]}
    assert ks == set(range(-3, 3)), ks
    # (c) both kinds at segment ends and at span ends
    assert {rel % SEGB for _, rel in b["longseg"][1]} == {SEGB - 2, SEGB - 6} and len(b["longseg"][1]) >= 30
    assert {rel for _, rel in b["longspan"][1]} == {SPANB - 2, SPANB - 6}
    # (d) more 3-byte tokens in a row than a window's table holds (TCAP = 448), on both sides of a span end
    assert len(b["tcap"][1]) >= 2 * 2 * 900
    # (e) the stop lies in the second span and the oracle rejects the block
    at = b["badoffset"][1][0][0]
    assert SPANB < at < 2 * SPANB
    assert oracle.lz4_decompress(b["badoffset"][0], 1 << 20)[0] < 0


NAMES = ["text1", "text2", "segedge", "spanedge0", "spanedge1", "spanedge2", "longseg", "longspan", "tcap", "badoffset"]


@pytest.mark.parametrize("name", NAMES)
def test_single_block(gpu, oracle, name):
    c = blocks(oracle)[name][0]
    n = oracle.lz4_decompress(c, 64 << 20)[0]
    _check(gpu, oracle, [c], [n if n > 0 else 1 << 20])


def test_all_in_one_batch_misaligned(gpu, oracle):
    comps = [blocks(oracle)[n][0] for n in NAMES]
    caps = []
    for c in comps:
        n = oracle.lz4_decompress(c, 64 << 20)[0]
        caps.append(n if n > 0 else 1 << 20)
    _check(gpu, oracle, comps, caps, mis_d=5, mis_s=1)
