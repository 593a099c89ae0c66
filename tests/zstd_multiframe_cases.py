"""Hand-built multi-frame Zstd inputs for the small-batch decode path
(juicefs_amd/csrc/zstd_split.inc), from the frame writer tests/zstd_frames.py.
Plain Python; tests/test_zstd_multiframe_gpu.py decodes them on the device
against the CPU oracle."""
from __future__ import annotations

from tests import zstd_frames as Z
from tests.zstd_conformance_cases import A4, FSE3, LV, W4, pat, sym


def small(k: int, **kw):
    """one frame of one compressed block, 330 bytes of content"""
    seqs = [(50, 40, 13 + 3), (50, 60, 33 + 3), (50, 30, 100 + 3)]
    return Z.frame([Z.comp(Z.lit_raw(pat(200, k)), seqs)], **kw)


def rep_reset(history: bool):
    """[frame 1, frame 2]: frame 2's first sequences use repeat codes 1 (with
    literals), 2 and 3, i.e. offsets 1, 4 and 8 of a fresh frame; with
    `history` frame 1 ends with repeat offsets (7, 9, 11)"""
    f1 = Z.frame([Z.comp(Z.lit_raw(pat(60, 5)), [(20, 5, 11 + 3), (20, 5, 9 + 3), (20, 5, 7 + 3)])]) if history else small(3)
    f2 = Z.frame([Z.comp(Z.lit_raw(pat(40, 6)), [(5, 10, 1), (4, 5, 2), (9, 6, 3)])])
    return [f1, f2]


def frame_base(over: int):
    """[frame 1, frame 2]: frame 2 is 50 literals and a match of offset 50 +
    over.  Frame 1 ends with the byte frame 2 starts with, so a decoder that
    reads across the frame edge produces plausible bytes."""
    lits = pat(50, 8)
    f1 = Z.frame([Z.raw(pat(299, 7) + lits[:1])])
    f2 = Z.frame([Z.comp(Z.lit_raw(lits), [(50, 20, 50 + over + 3)])])
    return [f1, f2]


def treeless_across():
    """frame 1 defines a Huffman table, frame 2's first block is treeless"""
    f1 = Z.frame([Z.comp(Z.lit_huf(sym(300, 9, A4), W4), [(10, 20, 7)])])
    f2 = Z.frame([Z.comp(Z.lit_treeless(sym(77, 5, A4), encode_as=W4), [(17, 6, 12)])])
    return [f1, f2]


def fse_repeat_across():
    """frame 1 defines the three FSE tables, frame 2's first block repeats them"""
    seqs = [(10, 5, 4 + 3), (3, 4, 1)]
    f1 = Z.frame([Z.comp(LV, seqs, seq=FSE3)])
    f2 = Z.frame([Z.comp(LV, seqs, seq=dict(ll="rep", of="rep", ml="rep"))])
    return [f1, f2]


def sizes_swapped():
    """declares 100 / produces 101, then declares 101 / produces 100"""
    return [Z.frame([Z.raw(pat(101, 1))], single=True, fcs_size=1, fcs=100),
            Z.frame([Z.raw(pat(100, 2))], single=True, fcs_size=1, fcs=101)]


def sizes_mixed():
    """a frame without a content size between two with one"""
    return [small(1, single=True, fcs_size=2), small(2), small(3, single=True, fcs_size=4)]


def empty_frame():
    """content size 0 and one empty raw last block"""
    return Z.frame([Z.raw(b"")], single=True, fcs_size=1)


def parts_bytes(parts):
    """[(bytes, content)] of each part alone (a skippable frame has no content)"""
    out = []
    for p in parts:
        c = Z.expand([p])
        assert c is not None
        out.append((Z.write([p]), c))
    return out

