"""Streams that steer the small-batch decoders (juicefs_amd/csrc/lz4_split.hip,
zstd_split.inc) into their hand-overs to the exact kernels, with a host model
of the LZ4 fix-up that says which side of the hand-over a stream falls on.
Plain Python, no GPU: tests/test_split_streams.py checks the builders against
the CPU oracle, tests/test_split_fallback_gpu.py runs them on the device."""
from __future__ import annotations

import random

from tests import zstd_frames as Z

SEG = 256        # JFS_LZ4_SPLIT_SEG (jfs_internal.h): compressed bytes per segment, one lane each
T = 256          # lz4_split.hip T: segments per fix-up workgroup
FIX_ROUNDS = 6   # lz4_split.hip FIX_ROUNDS: fix_kernel launches per decode
SPAN = SEG * T   # compressed bytes one fix-up workgroup covers (64 KiB)
HOPS = 6         # origin_map.h HOPS: pointer hops per entry per jump round
ZBLOCK = 128 << 10  # Zstd Block_Maximum_Size


# ------------------------------------------------------------------ LZ4
def chain_stream(units, seed=7):
    """An LZ4 stream of `units` 11-byte output units, each one literal byte and
    a 10-byte match at offset 11: every match byte copies the same byte of the
    unit before, so its origin chain runs back through every earlier unit."""
    rng = random.Random(seed)
    first = bytes(rng.randrange(256) for _ in range(11))
    out = bytearray([0xB6]) + first + (11).to_bytes(2, "little")  # ll 11, ml 10
    for _ in range(units - 1):
        out += bytes([0x16, rng.randrange(256)]) + (11).to_bytes(2, "little")  # ll 1, ml 10
    out += bytes([0xF0, 1]) + bytes(rng.randrange(256) for _ in range(16))  # last: 16 literals
    return bytes(out)


def chain_size(units):
    """Decoded size of chain_stream(units): 21 bytes, 11 per further unit, 16 literals."""
    return 11 * units + 26


def parse(s, n, x):
    """The token chain function, lz4_split.hip's parse(): the position of the
    token after the one at x (n once the stream ends inside or right after it)."""
    tok = s[x]
    ip = x + 1
    ll = tok >> 4
    if ll == 15:
        while True:
            if ip >= n:
                return n
            b = s[ip]
            ip += 1
            ll += b
            if b != 255:
                break
    q = ip + ll
    if q >= n or q + 2 > n:
        return n
    q += 2
    if tok & 15 == 15:
        while q < n:
            b = s[q]
            q += 1
            if b != 255:
                break
    return q


def nonmerging_stream(nwg, hdr, seed=1):
    """-> (stream, decoded size).  A valid LZ4 block of nwg 64 KiB fix-up
    workgroup spans whose speculative token chains never merge with the true one.

    Every byte of 0x00..0x0E read as a token is ll 0, ml < 15: a 3-byte token.
    The stream is made of such bytes, so it carries three token chains, one per
    position mod 3, that never meet.  A span is 65536 = 1 (mod 3) bytes, so the
    true chain would meet the boundary segments' speculative one at every third
    workgroup; one shifter per span -- three consecutive 0x1X bytes, each a
    4-byte token (ll 1) to the chain that reads it -- moves all three chains
    together and keeps the true chain's distance to the boundary chain.
    Layout: F0 FF xx + hdr literals (270 <= hdr < 525) + the first offset, the
    3-byte tokens (offset low byte 0..14, high byte 0..1, never zero, at most
    270 <= hdr), the tail F0 01 + 16 literals.  The true chain starts at
    hdr + 5: with hdr = 2 (mod 3) it is the boundary segments' chain and the
    fix-up has nothing to do, otherwise it takes one round per workgroup."""
    assert 270 <= hdr < 525 and nwg >= 1
    rng = random.Random(seed)
    a = lambda: rng.randrange(15)  # noqa: E731

    def offset():
        hi = rng.randrange(2)
        return bytes([rng.randrange(0 if hi else 1, 15), hi])
    out = bytearray([0xF0, 0xFF, hdr - 270]) + bytes(a() for _ in range(hdr)) + offset()
    size = hdr + 4
    end = nwg * SPAN - 18  # the tail's first byte at the latest
    shifted = 0            # spans that have their shifter
    while len(out) + 3 <= end:
        if len(out) >= shifted * SPAN + SPAN // 2 and len(out) + 4 <= end:
            # the true chain's token 0x1X (ll 1): its literal and its offset's
            # low byte are the other two chains' 0x1X tokens, whose own literal
            # and offset are the alphabet bytes that follow
            out += bytes([0x10 + a(), 0x10 + a(), 0x10 + a(), rng.randrange(2)])
            size += 1 + (out[-4] & 15) + 4
            shifted += 1
            continue
        t = a()
        out += bytes([t]) + offset()
        size += t + 4
    out += bytes([0xF0, 1]) + bytes(a() for _ in range(16))
    return bytes(out), size + 16


def fix_rounds_needed(stream, seg0=0):
    """Host model of spec_kernel / fix_kernel for one block whose first segment
    is global segment seg0: the number of fix-up rounds in which a workgroup's
    last exit changes the next workgroup's first entry.  The verdict hands the
    block to the exact kernel when round FIX_ROUNDS - 1 still changed one, i.e.
    when this count reaches FIX_ROUNDS (converges()).

    Per segment: the speculative chain from the segment's first byte, its mark
    set and its exit.  Per round, every workgroup that holds a changed entry
    takes its first entry as the round before left it and settles the rest in
    order -- the fixed point of fix_kernel's LDS iteration, entry[t + 1] =
    exit(entry[t]).  A workgroup never sees what another one writes in the same
    round (all of them read their entries as they start)."""
    s, n = stream, len(stream)
    nseg = (n + SEG - 1) // SEG
    nxt = {}

    def step(x):
        y = nxt.get(x)
        if y is None:
            y = nxt[x] = parse(s, n, x)
        return y
    mark = bytearray(n)
    spec_exit = [0] * nseg
    entry = [0] * nseg
    for k in range(nseg):
        s1 = min(k * SEG + SEG, n)
        x = k * SEG
        while x < s1:
            mark[x] = 1
            x = step(x)
        spec_exit[k] = min(x, n)
        if k + 1 < nseg:
            entry[k + 1] = spec_exit[k]

    def seg_exit(k, x):
        s1 = min(k * SEG + SEG, n)
        while x < s1:
            if mark[x]:
                return spec_exit[k]
            x = step(x)
        return min(x, n)
    # workgroup w holds the block's segments [lo, hi)
    groups = []
    g = seg0
    while g < seg0 + nseg:
        hi = min((g // T + 1) * T, seg0 + nseg)
        groups.append((g - seg0, hi - seg0))
        g = hi
    dirty = [True] * len(groups)  # round 0 runs every workgroup
    rounds = 0
    while any(dirty):
        writes, nd = [], [False] * len(groups)
        for w, (lo, hi) in enumerate(groups):
            if not dirty[w]:
                continue  # same entries as the round before: same exits, nothing changes
            ent = entry[lo:hi]
            for k in range(lo, hi):
                if k + 1 >= nseg:
                    break  # the block's last segment hands nothing on
                ex = seg_exit(k, ent[k - lo])
                if k + 1 < hi:
                    ent[k + 1 - lo] = ex
                elif entry[k + 1] != ex:  # the next workgroup's first entry
                    writes.append((k + 1, ex))
                    nd[w + 1] = True
            entry[lo + 1:hi] = ent[1:]
        for k, ex in writes:
            entry[k] = ex
        if not writes:
            break
        rounds += 1
        dirty = nd
        assert rounds <= 4 * len(groups) + 8
    return rounds


def converges(rounds):
    """The fix-up of a block with fix_rounds_needed() = rounds stays on the
    split path: round FIX_ROUNDS - 1 (the last one launched) changed nothing."""
    return rounds < FIX_ROUNDS


# The edge the model finds for nonmerging_stream (tests/test_split_streams.py
# searches for it): the largest nwg whose fix-up converges, and the next one.
NWG_EDGE, NWG_OVER = 6, 7


def jump_rounds(size, unit, max_rounds=12):
    """The launchers' round count for `size` output bytes, origin_map.h
    rounds(): the smallest jr with HOPS^jr > size / unit + 1 (unit 4: LZ4, a
    chain step per token; unit 3: Zstd, a step per sequence), at most
    MAX_ROUNDS = 12.  tests/test_origin_map.py holds this mirror to the header."""
    jr, reach = 1, HOPS
    while reach <= size / unit + 1 and jr < max_rounds:
        jr, reach = jr + 1, reach * HOPS
    return jr


def bound_edge_sizes(k, unit):
    """Output sizes around the step from k to k + 1 jump rounds: the largest
    whose bound size / unit + 1 is below HOPS^k, the one whose bound is
    HOPS^k - 1, and one unit more (bound HOPS^k: the first with k + 1 rounds)."""
    return [unit * HOPS ** k - unit - 1, unit * (HOPS ** k - 2), unit * (HOPS ** k - 1)]


def flat_chain_stream(nbytes):
    """An LZ4 block of exactly nbytes output: 4 literals, then tokens ll 0,
    ml 4, offset 4 (every match byte's origin is the same byte of the token
    before: the origin chain of the last match is one step per token, about
    nbytes / 4), then the shortest tail the format allows after a 4-byte match
    (8..11 literals: the last match starts 12 bytes before the end)."""
    assert nbytes >= 16
    m = (nbytes - 4 - 8) // 4
    tail = nbytes - 4 - 4 * m
    assert 8 <= tail <= 11 and m >= 1
    out = bytearray([0x40]) + b"flat" + (4).to_bytes(2, "little")  # ll 4, ml 4
    out += (bytes([0x00]) + (4).to_bytes(2, "little")) * (m - 1)
    out += bytes([tail << 4]) + bytes(0x61 + i for i in range(tail))
    return bytes(out)


def flat_chain_depth(nbytes):
    """Tokens with a match in flat_chain_stream(nbytes): the hops its last match bytes need."""
    return (nbytes - 4 - 8) // 4


# ------------------------------------------------------------------ Zstd
def _seq(ll, ml, off):
    """(literal length, match length, offset) as zstd_frames takes it: Offset_Value = offset + 3."""
    return (ll, ml, off + 3)


def _frame(blocks):
    src, want = Z._build([Z.frame(blocks)])  # write() and expand() in one pass
    assert want is not None
    return src, want


def zstd_flat_chain_frame(nbytes):
    """-> (frame, decoded bytes), nbytes of them: 3 literals, then sequences
    (ll 0, ml 3, offset 3) in compressed blocks of at most 128 KiB of output,
    then 0..2 literals.  Every match byte copies the same byte of the sequence
    before, so the chain depth of the last match equals the number of sequences."""
    assert nbytes >= 6
    nseq, rest = (nbytes - 3) // 3, (nbytes - 3) % 3
    per = (ZBLOCK - 8) // 3
    blocks, done = [], 0
    while done < nseq:
        k = min(per, nseq - done)
        first, last = done == 0, done + k == nseq
        lits = (b"zst" if first else b"") + (b"xy"[:rest] if last else b"")
        seqs = [_seq(3 if first else 0, 3, 3)] + [_seq(0, 3, 3)] * (k - 1)
        blocks.append(Z.comp(Z.lit_raw(lits), seqs))
        done += k
    return _frame(blocks)


def zstd_flat_chain_depth(nbytes):
    return (nbytes - 3) // 3


def zstd_chain_frame(units, seed=7, per_block=10000):
    """-> (frame, decoded bytes).  The Zstd twin of chain_stream: 11 literals,
    then per unit one literal and a 10-byte match at offset 11 (sequences
    ll 1, ml 10, offset 11), in compressed blocks of per_block units; with
    units > per_block the chains cross block boundaries."""
    rng = random.Random(seed)
    blocks, done = [], 0
    while done < units:
        k = min(per_block, units - done)
        first = done == 0
        lits = bytes(rng.randrange(256) for _ in range(k + (10 if first else 0)))
        seqs = [_seq(11 if first else 1, 10, 11)] + [_seq(1, 10, 11)] * (k - 1)
        blocks.append(Z.comp(Z.lit_raw(lits), seqs))
        done += k
    return _frame(blocks)
