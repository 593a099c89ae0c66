"""Hand-made LZ4 streams for the lift's rule (juicefs_amd/csrc/lz4_lift.h), shared
by tests/test_lz4_lift.py (the serial restatement, lift_host, in the
sanitizer-built host driver) and tests/test_lz4_lift_foreign_gpu.py
(lift_kernel, stitch and emit on the device), and the generator of blocks whose
64 KiB chunks a real encoder leaves liftable.  Plain Python and numpy, no GPU.

Every directed stream decodes to 2 * CH + 100 bytes unless its name says
otherwise and stays under 4 * 64 KiB stored: the index's fix-up rounds count
workgroup-boundary cascades (lz4_split.hip), so such a stream cannot exhaust
them and the device's verdict has no excuse to differ from the host rule's.

Not covered on purpose: lift_kernel's refusal of a chunk whose tokens, from the
first that starts at or above the chunk's floor, span 384 segments or more.  No
valid LZ4 stream spends 1.5 stored bytes per output byte (literals cost one
stored byte each plus one length byte per 255, a match of four bytes three), so
well-formed input does not reach it.  (The literals of the sequence that reaches
the floor are another matter: they may begin chunks below it, and
"literals-begin-two-chunks-below-F" is that case.)"""
from __future__ import annotations

import numpy as np

from juicefs_amd.blockgen import gen_block
from tests import lz4_chase_cases as K
from tests import lz4_fast_cases as F

CH = F.CHUNK
MAX_REC = CH // 4
SEG = K.SEG


def _rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def interior(c, n):
    return c >= 0 and (c + 1) * CH + 12 <= n


def fill(seed, upto, at, ml=30, off=9):
    """one sequence from output position `at` whose match ends exactly at `upto`"""
    return K.seq(_rand(seed, upto - at - ml), ml, off)


def ends_at_253():
    """chunk 0 as one sequence whose match ends on CH and whose stored bytes end at 253 mod 256"""
    for ml in range(8, 8 + 2 * SEG):
        s = K.seq(_rand(30, CH - ml), ml, 40)
        if len(s) % SEG == 253:
            return s
    raise AssertionError("no match length puts the next token at 253 mod 256")


def directed():
    """[(name, stream, chunk, ok, expected fields or None)]"""
    out = []
    tail = K.last(_rand(99, 100))
    ends = K.seq(_rand(1, CH - 20), 20, 100) + K.seq(_rand(2, CH - 50), 50, 30) + tail
    out.append(("match-ends-on-E", ends, 1, 1, dict(nrec=1, tail=0, lit0=CH - 50, pos=CH - 50, mlen=50, off=30, lit=CH - 50)))
    out.append(("match-ends-on-E-chunk-0", ends, 0, 1, dict(nrec=1, tail=0, lit0=CH - 20, pos=CH - 20, mlen=20, off=100)))
    cross = K.seq(_rand(3, CH - 6), 20, 10) + fill(4, 2 * CH, CH + 14) + tail
    out.append(("match-straddles-F", cross, 1, 0, None))
    out.append(("match-straddles-E", cross, 0, 0, None))
    on = K.seq(_rand(5, CH), 300, 1) + fill(6, 2 * CH, CH + 300) + tail
    out.append(("overlap-off1-on-F", on, 1, 0, None))
    behind = K.seq(_rand(7, CH + 1), 300, 1) + fill(8, 2 * CH, CH + 301) + tail
    out.append(("overlap-off1-behind-one-literal", behind, 1, 1, dict(nrec=2, tail=0, lit0=1, pos=1, mlen=300, off=1, lit=1)))
    lits = K.seq(_rand(9, 65000), 8, 50) + K.seq(_rand(10, 1000), 10, 20) + fill(11, 2 * CH, 66018) + tail
    out.append(("literals-across-F", lits, 1, 1, dict(nrec=2, tail=0, lit0=472, pos=472, mlen=10, off=20, lit=472)))
    none = K.seq(_rand(12, 100), 8, 50) + K.seq(_rand(13, 2 * CH + 500), 12, 9) + tail
    out.append(("no-match", none, 1, 1, dict(nrec=0, tail=CH, lit0=0, body=0)))
    far = K.seq(_rand(14, CH + 100), 16, 300) + fill(15, 2 * CH, CH + 116) + tail
    out.append(("offset-reaches-below-F", far, 1, 0, None))
    # kMaxRec four-byte matches tile a chunk only with the first on F, which copies from below it: refused by the
    # offset rule (the count rule cannot be met with more, matches being four bytes at least); behind four literals
    # the chunk holds kMaxRec - 1 of them and is lifted
    head = K.seq(_rand(16, CH - 8), 8, 20)
    out.append(("kMaxRec-matches", head + K.seq(b"", 4, 4) * MAX_REC + tail, 1, 0, None))
    out.append(("kMaxRec-less-one", head + K.seq(_rand(17, 4), 4, 4) + K.seq(b"", 4, 4) * (MAX_REC - 2) + tail, 1, 1,
                dict(nrec=MAX_REC - 1, tail=0, lit0=4, pos=4, mlen=4, off=4, lit=4)))
    # the source's true length: the chunk must be interior in it
    short = K.seq(_rand(18, CH - 20), 20, 100) + K.last(_rand(19, 11))
    out.append(("eleven-bytes-follow", short, 0, 0, None))
    out.append(("twelve-bytes-follow", K.seq(_rand(18, CH - 20), 20, 100) + K.last(_rand(19, 12)), 0, 1, dict(nrec=1, tail=0)))
    out.append(("chunk-past-the-end", ends, 2, 0, None))
    out.append(("negative-chunk", ends, -1, 0, None))
    # ---- the record shapes the fast parse never leaves: what a foreign encoder may store
    # the longest match a record holds: 65,535 bytes, which only fit behind one literal; 257 match-length bytes
    longest = K.seq(_rand(20, CH + 1), 65535, 1) + tail
    out.append(("longest-match", longest, 1, 1, dict(nrec=1, tail=0, lit0=1, pos=1, mlen=65535, off=1, lit=1)))
    # the longest literal run a record holds: the four bytes behind it are the shortest match
    runs = K.seq(_rand(21, CH - 20), 20, 100) + K.seq(_rand(22, CH - 4), 4, 50) + tail
    out.append(("longest-literal-run", runs, 1, 1,
                dict(nrec=1, tail=0, lit0=CH - 4, pos=CH - 4, mlen=4, off=50, lit=CH - 4)))
    # 300 literals, 200 of them in the chunk in front: the record keeps the 100 above F, stitch adds the carry
    below = K.seq(_rand(23, CH - 230), 30, 9) + K.seq(_rand(24, 300), 20, 50) + fill(25, 2 * CH, CH + 120) + tail
    out.append(("literals-begin-below-F", below, 1, 1, dict(nrec=2, tail=0, lit0=100, pos=100, mlen=20, off=50, lit=100)))
    out.append(("tail-runs-into-the-next-chunk", below, 0, 1, dict(nrec=1, tail=200, lit0=CH - 230, mlen=30, off=9)))
    # 1,024 sequences of 64 output and 64 stored bytes from stored position 65,788: the chunk's tokens lie in 257
    # segments, so the fifth round of 64 holds its last records
    many = head + b"".join(K.seq(_rand(1000 + i, 60), 4, 30) for i in range(CH // 64)) + tail
    out.append(("records-in-the-fifth-round", many, 1, 1,
                dict(nrec=CH // 64, tail=0, lit0=60, pos=60, mlen=4, off=30, lit=60)))
    # K.straddle_stream's token, moved: the chunk's first token stands at 253 mod 256, its three literal-length bytes
    # lie on both sides of a segment edge, and its 238 match-length bytes cross another
    big = K.seq(_rand(26, 15 + 255 + 255 + 5), 4 + 15 + 255 * 237 + 9, 300)
    edge = ends_at_253() + big + fill(27, 2 * CH, CH + 530 + 60463) + tail
    out.append(("token-spans-a-segment-edge", edge, 1, 1,
                dict(nrec=2, tail=0, lit0=530, pos=530, mlen=60463, off=300, lit=530)))
    # (3 * CH + 100 bytes) the first sequence of chunk 2 begins in chunk 0: between its token and the next one lie
    # 2 * CH + 500 literals, 514 segments without a token, which are no part of the chunk's span
    deep = K.seq(_rand(28, 100), 8, 50) + K.seq(_rand(29, 2 * CH + 500), 12, 9) + fill(31, 3 * CH, 2 * CH + 620) + tail
    out.append(("literals-begin-two-chunks-below-F", deep, 2, 1, dict(nrec=2, tail=0, lit0=608, pos=608, mlen=12, off=9, lit=608)))
    return out


def token_starts(stream):
    """[(stored position of the token, output position of its literals)] per sequence"""
    out, pos, op = [], 0, 0
    for ll, lit, ml, _ in K.sequences(stream):
        out.append((pos, op))
        op += ll + ml
        pos = lit + ll + (2 + (0 if ml - 4 < 15 else 1 + (ml - 4 - 15) // 255) if ml else 0)
    return out


def candidates(chunk, n, src=0):
    """A directed case's gathered block is its stream's own decode, n bytes; its candidates: the case's chunk of
    source `src` at its own place (an out-of-range chunk where chunk 0 or chunk 1 stands), nothing else."""
    lift = [(-1, 0)] * ((n + CH - 1) // CH)
    lift[chunk if interior(chunk, n) else min(max(chunk, 0), 1)] = (src, chunk)
    return lift


# ---------------------------------------------------------------- a real encoder's liftable chunks
N = 300000  # four whole chunks and a ragged fifth
NCH = 5
# where an output's 4 KiB piece is replaced: at a chunk's start, at a chunk's end, across a boundary, in the ragged tail
CUTS = [CH, 2 * CH - 4096, 2 * CH - 2048, 4 * CH + 1000]
PLANNED = [3, 3, 2, 4]


def overwritten(raws, cuts=CUTS):
    """output k: raws[k] with 4 KiB at cuts[k] taken from the next block; and per output chunk its candidate
    (src, src_chunk), every interior chunk the piece does not touch"""
    outs, lift = [], []
    for k, cut in enumerate(cuts):
        other, n = raws[(k + 1) % len(raws)], len(raws[k])
        outs.append(raws[k][:cut] + other[cut:cut + 4096] + raws[k][cut + 4096:])
        touched = {cut // CH, (cut + 4095) // CH}
        lift.append([(k, j) if interior(j, n) and j not in touched else (-1, 0) for j in range((n + CH - 1) // CH)])
    return outs, lift


def unshared_block(seed, n=N):
    """Every 64 KiB chunk is a pattern of its own, 1 to 3 KiB of random bytes repeated with a byte changed every
    few hundred, and ends in 16 random bytes: no chunk holds four bytes of another but by chance, and the literals
    of the 16 bytes keep a match from running over the chunk's end."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        period = int(rng.integers(1024, 3072))
        pat = rng.integers(0, 256, period, dtype=np.uint8)
        c = np.resize(pat, CH).copy()
        hits = np.cumsum(rng.integers(200, 600, CH // 200))
        hits = hits[hits < CH - 16]
        c[hits] ^= rng.integers(1, 256, len(hits), dtype=np.uint8)
        c[CH - 16:] = rng.integers(0, 256, 16, dtype=np.uint8)
        out += c.tobytes()
    return bytes(out[:n])


def zero_record_block(seed, n=N):
    """text chunk | random chunk | random chunk | text chunk | ragged text: the fast parse finds no match in the
    random chunks, so their lifted results are nrec = 0 and tail = CH"""
    t = gen_block("T", seed, n)
    return t[:CH] + _rand(seed + 1, CH) + _rand(seed + 2, CH) + t[3 * CH:]
