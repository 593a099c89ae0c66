"""Inputs shared by tests/test_zstd_fast.py (host twin) and
tests/test_zstd_fast_gpu.py (kernels), and a decoder-faithful replay of the
fast Zstd parse's sequence records (RFC 8878 3.1.1.5)."""
from __future__ import annotations

import functools

import numpy as np

from juicefs_amd.blockgen import gen_block

CHUNK = 65536
BLOCK = 131072


def _rand(seed: int, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _pattern(period: int, n: int) -> bytes:
    base = bytes((37 * i + 11 * period) & 255 for i in range(period))
    return (base * (n // period + 1))[:n]


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, bytes)]: the smallest shapes at which the two kernels take
    another path."""
    out = []
    text = gen_block("T", 7, 196621)
    # under 7 bytes: F_NOCOMP; the chunk edge; the block edge; two blocks, three chunks
    for n in (0, 1, 6, 7, 13, 65535, 65536, 65537, 131071, 131072, 131073, 196621):
        out.append((f"T-{n}", text[:n]))
    # RLE blocks with k > 0, and long matches cut at chunk ends
    out.append(("zeros-262144", bytes(262144)))
    out.append(("period3", _pattern(3, 70001)))
    out.append(("period7", _pattern(7, 140001)))
    out.append(("R-65537", _rand(8, 65537)))  # raw blocks
    out.append(("T-200003", gen_block("T", 21, 200003)))
    # a literal run of 600 bytes across the chunk boundary inside block 0
    out.append(("lits-cross-chunk", bytes(CHUNK - 200) + _rand(2, 600) + bytes(1000)))
    # a 300-byte match (more than a lane extends alone) that spans tiles
    seg = _rand(4, 300)
    out.append(("match-cross-tile", _rand(3, 100) + seg + _rand(5, 50) + seg + _rand(6, 30)))
    # a match that would run across the chunk boundary: it ends at the chunk's last byte
    out.append(("match-ends-chunk", _rand(5, CHUNK - 450) + seg + seg + seg + _rand(6, 77)))
    # the copy of u + m + v has m replaced by a copy of w: three matches without a
    # literal between them, the third at the first one's offset
    u, m, v, w = _rand(10, 40), _rand(11, 8), _rand(12, 40), _rand(13, 8)
    out.append(("rep-no-literals", u + m + v + _rand(14, 100) + w + _rand(15, 100) + u + w + v + _rand(16, 20)))
    # period 1000 over two blocks: the same offset is the last one of block 0
    # and the first one of block 1
    p = _rand(17, 1000)
    out.append(("rep-across-blocks", (p * 140)[:BLOCK + 5000]))
    return out


def block_sizes(n: int):
    return [min(BLOCK, n - bs) for bs in range(0, n, BLOCK)]


def replay(src: bytes, blocks):
    """Decode blocks = [([(ll, ml, Offset_Value)], nl)] of src as a Zstd decoder
    would if every block ended up compressed, and check the fast parse's rules:
    counts, chunk-local matches, and no repeat code before a sequence of the
    same block (or, in block 0, the frame's start values) determined the entry
    it names.  Returns [(block, ll, Offset_Value)] of the repeat codes used."""
    out = bytearray()
    used = []
    sizes = block_sizes(len(src))
    assert len(blocks) == len(sizes)
    for k, ((recs, nl), bsz) in enumerate(zip(blocks, sizes)):
        bs = k * BLOCK
        assert len(recs) <= bsz // 4, (k, len(recs))
        # None: what the decoder holds here depends on the blocks before
        rep = [1, 4, 8] if k == 0 else [None, None, None]
        pos, lits = bs, 0
        for ll, ml, ofv in recs:
            out += src[pos:pos + ll]
            pos += ll
            lits += ll
            assert ofv >= 1 and ml >= 4
            if ofv > 3:
                off = ofv - 3
                rep = [off, rep[0], rep[1]]
            else:
                used.append((k, ll, ofv))
                idx = ofv - 1 if ll else ofv
                base = rep[idx] if idx < 3 else rep[0]
                assert base is not None, f"block {k}: Offset_Value {ofv} (ll {ll}) names an undetermined entry"
                off = base if idx < 3 else base - 1
                assert off > 0
                if idx == 1:
                    rep = [rep[1], rep[0], rep[2]]
                elif idx >= 2:
                    rep = [off, rep[0], rep[1]]
            assert off <= 65535 and (pos - bs - off) // CHUNK == (pos - bs) // CHUNK == (pos - bs + ml - 1) // CHUNK, \
                "a match leaves its chunk"
            for _ in range(ml):
                out.append(out[-off])
            pos += ml
        tail = nl - lits
        assert tail >= 0 and pos + tail == bs + bsz, (k, pos, tail, bsz)
        out += src[pos:pos + tail]
    assert bytes(out) == src
    return used
