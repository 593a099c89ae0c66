"""Inputs shared by tests/test_lz4_fast.py (host twin) and
tests/test_lz4_fast_gpu.py (kernels), and a walker over LZ4 block sequences."""
from __future__ import annotations

import functools

import numpy as np

from juicefs_amd.blockgen import gen_block

CHUNK = 65536
LENGTHS = [0, 1, 4, 5, 11, 12, 13, 14, 63, 64, 65, 65535, 65536, 65537, 65548, 131071, 131072, 200003]
PERIODS = [1, 2, 3, 4, 63, 64, 65]


def _pattern(period: int, n: int) -> bytes:
    base = bytes((37 * i + 11 * period) & 255 for i in range(period))
    return (base * (n // period + 1))[:n]


def _rand(seed: int, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, bytes)]: every length in every data class, then the special blocks."""
    out = []
    big = {"T": gen_block("T", 7, max(LENGTHS)), "R": gen_block("R", 8, max(LENGTHS))}
    for n in LENGTHS:
        out.append((f"zeros-{n}", bytes(n)))
        for cls in "TR":
            out.append((f"{cls}-{n}", big[cls][:n]))
        for p in PERIODS:
            out.append((f"period{p}-{n}", _pattern(p, n)))
    r = _rand(1, 1000)
    # the last 12 bytes repeat earlier bytes: the end rules must keep them literal
    out.append(("tail-repeats", r + r[100:112]))
    out.append(("tail-repeats-long", r + r[:500]))
    # a literal run of 600 bytes across the first chunk boundary (the carry and its length bytes)
    out.append(("lits-cross-chunk", bytes(CHUNK - 200) + _rand(2, 600) + bytes(1000)))
    # chunks without any match between chunks with matches
    out.append(("matchless-chunks", bytes(1000) + _rand(3, 2 * CHUNK + 5000) + bytes(1000)))
    # a match that would run across a chunk boundary
    seg = _rand(4, 300)
    out.append(("match-cross-chunk", _rand(5, CHUNK - 450) + seg + seg + seg + _rand(6, 77)))
    out.append(("text-then-zeros", gen_block("T", 9, CHUNK - 30) + bytes(CHUNK + 100)))
    return out


def walk(comp: bytes, n: int):
    """Decode the sequence structure of an LZ4 block of n decoded bytes:
    [(literals, match_pos, match_len, offset)] with the last entry
    (literals, None, 0, 0).  Raises AssertionError on a malformed stream."""
    seqs, i, pos = [], 0, 0
    while True:
        assert i < len(comp), "ran out of input before the last sequence"
        tok = comp[i]
        i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = comp[i]
                i += 1
                lit += b
                if b != 255:
                    break
        i += lit
        pos += lit
        assert i <= len(comp)
        if i == len(comp):
            assert tok & 15 == 0, "the last sequence has a match length"
            seqs.append((lit, None, 0, 0))
            break
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
        ml += 4
        assert 1 <= off <= pos, (off, pos)
        seqs.append((lit, pos, ml, off))
        pos += ml
    assert pos == n, (pos, n)
    return seqs


def check_end_rules(comp: bytes, n: int):
    """LZ4 block format end rules, plus the fast parse's own chunk rule."""
    seqs = walk(comp, n)
    matches = [s for s in seqs if s[1] is not None]
    if n < 13:
        assert not matches, "blocks under 13 bytes are all literals"
    if matches:
        assert seqs[-1][0] >= 5, "the last 5 bytes are literals"
    for lit, pos, ml, off in matches:
        assert pos <= n - 12, "a match starts within the last 12 bytes"
        assert pos + ml <= n - 5
        assert off <= 65535
        assert (pos - off) // CHUNK == pos // CHUNK == (pos + ml - 1) // CHUNK, "a match leaves its chunk"
    return seqs
