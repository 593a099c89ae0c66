"""Streams and a Python restatement of the LZ4 origin chase
(juicefs_amd/csrc/lz4_chase.h), shared by tests/test_lz4_chase.py (host),
tests/test_lz4_chase_gpu.py (kernels) and scripts/lz4_chase_hops.py (the
histogram CHASE_HOPS is derived from).  Plain Python and numpy, no GPU."""
from __future__ import annotations

import numpy as np

from juicefs_amd.blockgen import gen_block

SEG = 256         # lz4_chase.h SEG
CHASE_HOPS = 2048   # lz4_chase.h CHASE_HOPS (test_lz4_chase.py holds the two together)


# ------------------------------------------------------------------ the rule, restated
def sequences(comp: bytes):
    """[(literal length, literal input position, match length, offset)] of a
    well-formed block; the last entry has match length 0."""
    out, i, n = [], 0, len(comp)
    while True:
        tok = comp[i]
        i += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = comp[i]
                i += 1
                ll += b
                if b != 255:
                    break
        lit = i
        i += ll
        if i >= n:
            out.append((ll, lit, 0, 0))
            return out
        off = comp[i] | comp[i + 1] << 8
        i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = comp[i]
                i += 1
                ml += b
                if b != 255:
                    break
        out.append((ll, lit, ml + 4, off))


def hop_depths(comp: bytes) -> np.ndarray:
    """Per output byte, the steps the chase rule takes to its literal: 0 for a
    literal, else 1 + the depth of mstart - off + (x - mstart) % off.  Sequences
    in order, each match as one numpy gather: every step goes backwards, so the
    depths a match reads are final when it is reached."""
    seqs = sequences(comp)
    total = sum(ll + ml for ll, _, ml, _ in seqs)
    depth = np.zeros(total, dtype=np.int32)
    op = 0
    for ll, _, ml, off in seqs:
        op += ll
        if ml == 0:
            break
        assert 1 <= off <= op
        if off >= ml:
            depth[op:op + ml] = depth[op - off:op - off + ml] + 1
        else:
            depth[op:op + ml] = np.resize(depth[op - off:op] + 1, ml)
        op += ml
    return depth


def hop_histogram(comp: bytes):
    """{depth: bytes} of one block, and its largest depth."""
    d = hop_depths(comp)
    h = np.bincount(d) if d.size else np.zeros(1, dtype=np.int64)
    return {int(k): int(v) for k, v in enumerate(h) if v}, int(d.max()) if d.size else 0


def hops_cap(max_depth: int) -> int:
    """The smallest power of two that is at least twice the deepest chain seen."""
    c = 1
    while c < 2 * max_depth:
        c *= 2
    return c


def mixed_block(seed: int, n: int) -> bytes:
    """Text, zeros, incompressible bytes and repeats of earlier text, in pieces of 1 to 48 KiB."""
    rng = np.random.default_rng(seed)
    text = gen_block("T", seed, n)
    out = bytearray()
    while len(out) < n:
        k = int(rng.integers(1 << 10, 48 << 10))
        kind = int(rng.integers(0, 4))
        at = len(out)
        if kind == 0 or at == 0:
            out += text[at:at + k]
        elif kind == 1:
            out += bytes(k)
        elif kind == 2:
            out += gen_block("R", seed * 131 + at, k)
        else:
            back = int(rng.integers(0, at))
            out += bytes(out[back:back + k])
    return bytes(out[:n])


# ------------------------------------------------------------------ hand-built streams
def _len_bytes(v: int) -> bytes:
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return bytes(out)


def seq(lits: bytes, ml: int, off: int) -> bytes:
    """One sequence: the literals, then a match of ml >= 4 bytes at offset off."""
    ll, m = len(lits), ml - 4
    out = bytearray([(min(ll, 15) << 4) | min(m, 15)])
    if ll >= 15:
        out += _len_bytes(ll - 15)
    out += lits + bytes([off & 255, off >> 8])
    if m >= 15:
        out += _len_bytes(m - 15)
    return bytes(out)


def last(lits: bytes) -> bytes:
    """The final, literals-only sequence."""
    ll = len(lits)
    out = bytearray([min(ll, 15) << 4])
    if ll >= 15:
        out += _len_bytes(ll - 15)
    return bytes(out + lits)


def _bytes(seed: int, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def long_run_stream(off: int, run: int, seed: int = 3) -> bytes:
    """max(off, 20) literals, a match of `run` bytes at offset `off` (overlapped
    for run > off: the period rule), a short text piece with a second match into
    the run, and a 12-literal tail."""
    head = _bytes(seed, max(off, 20))
    return seq(head, run, off) + seq(b"between the runs", 40, 33) + last(b"tail-of-12-b")


def straddle_stream() -> bytes:
    """A token at position 253 whose three literal-length bytes (254, 255, 256)
    straddle the first 256-byte segment edge and whose 238 match-length bytes
    (789 .. 1026) straddle the one at 1024; segments 2 and 3 lie inside its
    literals and hold no token start."""
    first = seq(_bytes(5, 243), 8, 100)           # 1 + 1 + 243 + 2 = 247 bytes
    pad = seq(b"", 4, 7) * 2                      # two 3-byte tokens: the next token starts at 253
    assert len(first) + len(pad) == 253
    lits = _bytes(6, 15 + 255 + 255 + 5)          # length bytes 255, 255, 5
    big = seq(lits, 4 + 15 + 255 * 237 + 9, 300)  # offset at 787, 788; 238 match-length bytes
    out = first + pad + big
    assert len(out) == 1027
    return out + seq(b"x", 30, 2) + last(b"the last twelve.")


def tokenless_segment_stream() -> bytes:
    """A 700-literal sequence: the segments inside its literals hold no token start."""
    return seq(_bytes(7, 700), 60, 650) + last(b"twelve bytes")


def final_len_stream(k: int) -> bytes:
    """A block that is one literals-only sequence of k bytes (k = 0: the empty
    block's single zero token).  Behind a match the acceptance conditions ask
    for five literals at least, so this is the only place a final run of 0 or
    1 can stand in a stream the chase accepts."""
    return last(b"z" * k)


def short_final_after_match(k: int) -> bytes:
    """A match followed by a final run of k < 5 literals: the match token fails
    the end-of-input conditions, so every position the chase visits it for is BAD."""
    return seq(_bytes(8, 40), 12, 17) + last(b"z" * k)


BAD_STREAMS = {
    # offset 0
    "offset-zero": seq(b"0123456789abcdef", 8, 0) + last(b"tail-of-12-b"),
    # offset beyond the bytes produced
    "offset-beyond": seq(b"0123456789abcdef", 8, 17) + last(b"tail-of-12-b"),
    # the stream ends inside the match-length bytes of its second token
    "cut-in-header": seq(b"0123456789abcdef", 8, 4) + seq(b"abcdefgh", 4 + 15 + 255 + 3, 9)[:-1],
}
