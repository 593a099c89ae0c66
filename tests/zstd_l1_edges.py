"""Directed inputs of the Zstd level-1 encoder (test data only): one named,
deterministic input per format feature that tests/zstd_frame_census.py can
name, each found by search against libzstd 1.4.9's ZSTD_compress(.., 1) and
kept as small as the feature allows.  tests/golden/make_zstd_l1_edges.py
records libzstd's frame of each (sha256) and the features the census reads from
it in tests/golden/zstd_l1_edges.json.

CASES maps a name to (generator, the features the case is there for); a case
usually shows more features than those, all of them recorded in the fixture.
UNREACHABLE maps every feature that no level-1 frame made without a dictionary
can hold to the reason.
"""
from __future__ import annotations

import functools

from juicefs_amd.blockgen import gen_block

B = 128 << 10  # block size


def rnd(seed: int, n: int) -> bytes:
    return gen_block("R", seed, n)


def text(seed: int, n: int) -> bytes:
    return gen_block("T", seed, n)


def alphabet(seed: int, n: int, k: int) -> bytes:
    """uniform bytes over k symbols: Huffman gains, a repeat of four bytes is rare"""
    return bytes(x % k for x in rnd(seed, n))


@functools.lru_cache(maxsize=None)
def skew(seed: int, n: int) -> bytes:
    """48 symbols in 16 classes of 3; class s (the number of trailing one bits of 16
    random bits) has probability 2^-(s+1): Huffman codes of every length up to the limit"""
    r = rnd(seed, n * 2)
    out = bytearray(n)
    for i in range(n):
        x = r[2 * i] | (r[2 * i + 1] << 8)
        s = 0
        while x & 1 and s < 15:
            s += 1
            x >>= 1
        out[i] = s * 3 + (r[2 * i + 1] >> 6) % 3
    return bytes(out)


def zero_noise(period: int, count: int) -> bytes:
    """zeros with one non-zero byte every `period` bytes: every sequence has the same
    literal length (2), the same offset (repeat offset 1) and the same match length"""
    out = bytearray(period * (count + 1))
    for i in range(1, count + 1):
        out[period * i] = 1 + (37 * i) % 255
    return bytes(out)


def alternating(seed: int) -> bytes:
    """three blocks: two random ones that differ in every byte, and a third that takes
    64 bytes of the first, 64 of the second, then four bytes of each in turn: every match
    is four bytes long at the other of the two offsets, with no literal between them --
    about 32,700 sequences in one block"""
    a = rnd(seed, B)
    b = bytes(x ^ (1 + y % 255) for x, y in zip(a, rnd(seed + 1, B)))
    c = bytearray(a[:64] + b[64:128])
    for p in range(128, B, 4):
        c += (a if (p >> 2) & 1 == 0 else b)[p:p + 4]
    return a + b + bytes(c)


def separated(seed: int, pieces: int) -> bytes:
    """256 random bytes, then `pieces` 12-byte pieces of them, each behind three fresh
    random bytes: about one sequence per piece"""
    base = rnd(seed, 256)
    fresh = rnd(seed + 1, 3 * pieces)
    out = bytearray(base)
    for i in range(pieces):
        at = (29 * i) % 240
        out += fresh[3 * i:3 * i + 3] + base[at:at + 12]
    return bytes(out)


def rle_literals(seed: int, pieces: int) -> bytes:
    """a first block of 16 * pieces random bytes (none of them 'x') and zeros, then each
    16-byte piece of those bytes behind one 'x': the second block's literals are `pieces`
    times the byte 'x'.  (It takes an earlier block: where every literal is the same byte
    and matches copy only what the frame already holds, the whole frame is that byte.)"""
    base = bytes(x if x != 0x78 else 0x79 for x in rnd(seed, 16 * pieces + 8))
    out = bytearray(base + bytes(B - len(base)))
    for i in range(pieces):
        out += b"x" + base[1 + 16 * i:17 + 16 * i]
    return bytes(out)


def treeless(seed: int, fresh: int) -> bytes:
    """a block of skewed bytes (one Huffman table), then `fresh` more of them and zeros
    to the end of a second block: few literals, cheaper with the first block's table"""
    return skew(seed, B) + skew(seed + 1, fresh) + bytes(B - fresh)


def far_copy(seed: int, gap: int, tail: int = 0) -> bytes:
    """256 random bytes, zeros, the same 256 bytes `gap` bytes behind their first copy, a random tail"""
    n = rnd(seed, 256)
    return n + bytes(gap - 256) + n + rnd(seed + 1, tail)


def zero_run(k: int) -> bytes:
    """one byte, k zeros, 64 random bytes: one match of k - 1 bytes"""
    return b"\x01" + bytes(k) + rnd(70, 64)


CASES = {}


def _case(name, fn, *features):
    assert name not in CASES
    CASES[name] = (fn, features)


# frame header: the content-size field on each side of its steps; a frame larger than its window
_case("empty", lambda: b"", "fcs_1byte", "block_raw")
_case("size_255", lambda: text(1, 255), "fcs_1byte", "size_255", "single_segment")
_case("size_256", lambda: text(2, 256), "fcs_2byte", "size_256")
_case("size_65791", lambda: text(3, 65791), "fcs_2byte", "size_65791", "huf_weights_fse", "huf_depth_11", "nbseq_2byte",
      "ll_fse", "of_fse", "ml_fse", "rep_offset_1", "rep_ll0")
_case("size_65792", lambda: text(4, 65792), "fcs_4byte", "size_65792")
_case("window_edge", lambda: far_copy(51, (1 << 19) - 300, 600), "window_descriptor", "offset_near_window")
# blocks
_case("const_1000", lambda: bytes(1000), "const_first_block_compressed", "block_compressed", "lit_raw_h1",
      "ll_predefined", "of_predefined", "ml_predefined", "nbseq_1byte")
_case("zeros_3_blocks", lambda: bytes(3 * B), "const_first_block_compressed", "block_rle")
_case("random_5000", lambda: rnd(5, 5000), "block_raw")
_case("tail_1", lambda: bytes(B + 1), "last_block_1")
_case("tail_2", lambda: bytes(B + 2), "last_block_2")
_case("tail_3", lambda: bytes(B + 3), "last_block_3")
# literals: Huffman in every size format, with no sequence at all
_case("alphabet16_200", lambda: alphabet(6, 200, 16), "lit_huf_1s", "zero_sequences", "huf_weights_direct")
_case("alphabet16_600", lambda: alphabet(7, 600, 16), "lit_huf_4s_10", "zero_sequences")
_case("alphabet16_5000", lambda: alphabet(8, 5000, 16), "lit_huf_4s_14", "zero_sequences")
_case("alphabet16_20000", lambda: alphabet(9, 20000, 16), "lit_huf_4s_18", "zero_sequences")
# literals: raw with each header, RLE, treeless in every size format
_case("raw_literals_40", lambda: rnd(14, 40) * 4, "lit_raw_h2")
_case("random_then_zeros", lambda: rnd(15, 5000) + bytes(5000), "lit_raw_h3")
_case("rle_literals_64", lambda: rle_literals(31, 64), "lit_rle")
_case("treeless_200", lambda: treeless(40, 200), "lit_treeless_1s")
_case("treeless_600", lambda: treeless(40, 600), "lit_treeless_4s_10")
_case("treeless_5000", lambda: treeless(40, 5000), "lit_treeless_4s_14")
_case("treeless_30000", lambda: treeless(40, 30000), "lit_treeless_4s_18")
# sequence count
_case("pieces_127", lambda: separated(60, 125), "nbseq_127", "nbseq_1byte")
_case("pieces_128", lambda: separated(60, 126), "nbseq_128", "nbseq_2byte")
_case("alternating_4", lambda: alternating(20), "nbseq_3byte", "rep_ll0", "ll_rle")
# table modes
_case("zero_noise", lambda: zero_noise(50, 20), "ll_rle", "of_rle", "ml_rle")
# values
_case("literal_run_70000", lambda: rnd(16, 70000) + bytes(B - 70000), "ll_ge_65536", "lit_raw_h3")
_case("match_65538", lambda: zero_run(65539), "ml_65538")
_case("match_65539", lambda: zero_run(65540), "ml_65539", "ml_ge_65539")
_case("match_65540", lambda: zero_run(65541), "ml_65540", "ml_ge_65539")
_case("far_140000", lambda: far_copy(50, 140000), "offset_gt_128k")

_NO_REPEAT = ("ZSTD_selectEncodingType, strategy fast: set_repeat needs the previous table marked FSE_repeat_valid, "
              "which only a dictionary does; a block's own table is left at FSE_repeat_check (the oracle's "
              "select_type has no repeat branch), and no searched input produced it")
_NO_REP23 = ("ZSTD_compressBlock_fast stores offcode 0 (Offset_Value 1) at both of its repeat checks -- offset_1 "
             "behind at least one literal, offset_2 right behind a match, where literal length 0 shifts value 1 to "
             "the second offset -- and offset + 3 for every hash match, even one at a repeat offset (the oracle's "
             "fast_block: offcode = 0 or offset_1 + 2); no searched input produced it")
UNREACHABLE = {
    "ll_repeat": _NO_REPEAT, "of_repeat": _NO_REPEAT, "ml_repeat": _NO_REPEAT,
    "rep_offset_2": _NO_REP23, "rep_offset_3": _NO_REP23,
}


@functools.lru_cache(maxsize=None)
def make(name: str) -> bytes:
    return CASES[name][0]()
