"""Hand-assembled Zstandard frames for the decoder's conformance tests.

CASES is a list of dicts: name, group, desc (a tests/zstd_frames.py
description), intent ("accept", "reject", or "verdict" where only libzstd's
answer is compared), why (the decoder constant or rule next to the case), twin
(for a reject: the accepted case that differs only in the field under test),
size (exact dst cap: the output size; for a reject, room for all a decoder
that missed the fault would write, so that the verdict cannot come from the
cap) and big (output of several MiB: decoded once per path and so with the
exact cap only, never multiplied)."""
from __future__ import annotations

from tests import zstd_frames as Z
from tests.zstd_frames import comp, frame, lit_huf, lit_raw, lit_rle, lit_treeless, raw, rle, skip, stray

CASES = []
_BY = {}
# libzstd 1.4.9 ignores the reserved Symbol_Compression_Modes bits and never checks that a sequence bitstream ends
# exactly: it accepts these, zstd >= 1.5 (the pinned version) and this project reject them
LAX_149 = {"reserved_mode_bits", "one_spare_bit", "one_bit_short", "eight_bits_short"}


def pat(n: int, k: int = 1) -> bytes:
    """n patterned bytes without short periods."""
    return bytes(((i * 131 + k * 17 + (i >> 8) * 7 + (i >> 3)) & 255) for i in range(n))


def sym(n: int, k: int, alphabet) -> bytes:
    """n bytes over a small alphabet (Huffman literals)."""
    m = len(alphabet)
    return bytes(alphabet[((i * 7 + k + (i >> 2) * 3 + (i >> 5)) % (2 * m)) % m] for i in range(n))


def pre(n: int):
    """RLE blocks making n bytes of output, 128 KiB of output per 4 frame bytes."""
    out, i = [], 0
    while n > 0:
        m = min(n, Z.BLOCK_MAX)
        out.append(rle((i * 37 + 1) & 255, m))
        n -= m
        i += 1
    return out


def case(name, group, desc, intent="accept", why="", twin=None, size=None, big=False):
    assert name not in _BY, name
    c = dict(name=name, group=group, desc=desc, intent=intent, why=why, twin=twin, big=big)
    out = Z.expand(desc)
    if intent == "accept":
        assert out is not None, name
    if intent == "reject":
        assert out is None, name
    if size is None:
        size = len(out) if out is not None else _BY[twin]["size"] if twin else 1 << 12
    c["size"] = size
    CASES.append(c)
    _BY[name] = c


def pair(name, group, good, bad, why, **kw):
    """An accepted case and its rejected twin."""
    case(name, group, good, "accept", why, **kw)
    case(name + "_bad", group, bad, "reject", why, twin=name, **kw)


# ------------------------------------------------------ frame and block layer
G = "frame"
for fs, n in ((1, 255), (2, 256), (2, 65791), (4, 65791), (8, 255), (4, 0), (1, 0)):
    case("fcs%d_%d" % (fs, n), G, [frame([raw(pat(n, fs))], single=True, fcs_size=fs)], why="FCS size / 2-byte bias")
case("fcs2_window", G, [frame([raw(pat(300))], fcs_size=2, wlog=10)], why="FCS beside a window descriptor")
pair("fcs4_300", G, [frame([raw(pat(300))], single=True, fcs_size=4)],
     [frame([raw(pat(300))], single=True, fcs_size=4, fcs=301)], "declared FCS one more than produced")
case("fcs4_300_less", G, [frame([raw(pat(300))], single=True, fcs_size=4, fcs=299)], "reject",
     "declared FCS one less than produced", twin="fcs4_300")
case("window_mantissa", G, [frame([raw(pat(40))], wlog=12, wmant=5)], why="window descriptor mantissa")
pair("window_log31", G, [frame([raw(pat(40))], wlog=31, wmant=7)], [frame([raw(pat(40))], wlog=32, wmant=7)],
     "window log maximum 31")
for ds in (1, 2, 4):
    pair("dictid%d_zero" % ds, G, [frame([raw(pat(33))], did_size=ds, did=0)],
         [frame([raw(pat(33))], did_size=ds, did=1)], "dictionary-ID field holding 0 / 1")
pair("unused_bit", G, [frame([raw(pat(20))], unused=1)], [frame([raw(pat(20))], reserved=1)],
     "reserved descriptor bit (the unused bit beside it is ignored)")
pair("checksum_ok", G, [frame([raw(pat(100)), comp(lit_raw(b"abc"), [(3, 40, 5)])], checksum="ok")],
     [frame([raw(pat(100)), comp(lit_raw(b"abc"), [(3, 40, 5)])], checksum="bad")], "content checksum")
for k in (0, 1, 3):
    case("checksum_cut%d" % k, G, [frame([raw(pat(100))], checksum="cut", cut_to=k)], "reject", "checksum cut short",
         twin="checksum_ok", size=100)
F1 = frame([raw(pat(50, 1)), comp(lit_raw(b"12345"), [(5, 9, 23)])])
F2 = frame([rle(7, 30)], single=True, fcs_size=1, checksum="ok")
F3 = frame([comp(lit_raw(pat(20, 3)), [(20, 4, 4)])])
case("two_frames", G, [F1, F2], why="frames back to back")
case("three_frames", G, [F1, F2, F3], why="frames back to back")
case("skip0_between", G, [F1, skip(b""), F2], why="skippable frame of 0 bytes")
case("skip5_between_after", G, [F1, skip(b"hello", nibble=7), F2, skip(b"", nibble=15), F3, skip(b"12345", nibble=1)],
     why="skippable frames, magics 0x184D2A5x")
case("skip_only", G, [skip(b"abc", nibble=3)], why="no Zstandard frame at all")
for nib in range(16):
    case("skip_magic%x" % nib, G, [skip(b"z", nibble=nib), F2], why="each of the 16 skippable magics")
case("skip_size_long", G, [F2, skip(b"abc", size=4)], "reject", "skippable size past the input", twin="skip0_between",
     size=30)
for k in (1, 2, 3, 4):
    case("trailing%d" % k, G, [F2, stray(b"\x00" * k)], "reject", "trailing bytes", twin="two_frames", size=30)
case("raw_block_0", G, [frame([raw(b""), raw(b"ab"), raw(b"")])], why="raw block of 0 bytes")
case("rle_block_0", G, [frame([rle(9, 0), rle(5, 3), rle(9, 0)])], why="RLE block of 0 bytes")
case("raw_block_128k", G, [frame([raw(pat(Z.BLOCK_MAX))])], why="raw block of 128 KiB")
case("rle_block_128k", G, [frame([rle(0x5A, Z.BLOCK_MAX), rle(0x11, 1)])], why="RLE block of 128 KiB")
pair("comp_block_128k_less1", G, [frame([comp(lit_raw(pat(Z.BLOCK_MAX - 5, 2)))])],
     [frame([comp(lit_raw(pat(Z.BLOCK_MAX - 4, 2)))])], "compressed-block size field 128 KiB - 1 / 128 KiB")
assert len(Z.write(_BY["comp_block_128k_less1"]["desc"])) == 6 + 3 + Z.BLOCK_MAX - 1
pair("block_type_comp", G, [frame([comp(lit_raw(b"abcd"))])], [frame([comp(lit_raw(b"abcd"), type=3)])],
     "reserved block type 3")
pair("two_raw_blocks", G, [frame([raw(b"abc"), raw(b"def")])], [frame([raw(b"abc", last=True), raw(b"def")])],
     "last-block bit set early: the bytes after it read as a new frame")
pair("raw_block_6", G, [frame([raw(b"abcdef")])], [frame([raw(b"abcdef", size=7)])], "block size past the input")
pair("magic", G, [frame([raw(pat(20))])], [frame([raw(pat(20))], magic=Z.MAGIC + 1)], "frame magic")
case("comp_block_regen_200k", G, [frame([comp(lit_rle(0x41, 10), [(10, 100000, 4), (0, 100000, 1)])])], "verdict",
     "one compressed block regenerating more than 128 KiB: libzstd's verdict", size=200010)

# ------------------------------------------------------------------- literals
G = "literals"
pair("lit_raw_0", G, [frame([raw(b"ab"), comp(lit_raw(b""), [(0, 5, 4)])])], [frame([raw(b"ab"), comp(lit_raw(b""))])],
     "raw literals of 0 bytes; alone with nbSeq 0 the block is 2 bytes, below libzstd's minimum of 3")
for n in (0, 30, 31, 32, 4095, 4096):
    if n:
        case("lit_raw_%d" % n, G, [frame([comp(lit_raw(pat(n, 5)))])],
             why="raw literals, size-format edge (1-byte format: bits 00 for an even size, 10 for an odd one)")
    case("lit_rle_%d" % n, G, [frame([comp(lit_rle(0x30 + n % 7, n))])], why="RLE literals, size-format edge")
for sf in (1, 3):
    case("lit_raw_31_sf%d" % sf, G, [frame([comp(lit_raw(pat(31, 6), sf=sf), [(20, 5, 4)])])], why="size format %d" % sf)
    case("lit_rle_0_sf%d" % sf, G, [frame([raw(b"ab"), comp(lit_rle(1, 0, sf=sf), [(0, 5, 4)])])],
         why="size format %d at regen 0" % sf)
case("lit_rle_4096_sf3_seq", G, [frame([comp(lit_rle(0x77, 4096), [(4000, 8, 4)])])], why="3-byte RLE header")
pair("lit_rle_131072", G, [frame([comp(lit_rle(0x21, 131072))])], [frame([comp(lit_rle(0x21, 131073))])],
     "literals of 128 KiB / one more")
pair("lit_raw_too_long", G, [frame([comp(lit_raw(b"abcdef"))])],
     [frame([comp(dict(type="raw", data=b"abcdef", regen=7))])], "raw literals past the block")
W4 = Z.huf_weights({0x61: 1, 0x62: 2, 0x63: 3, 0x64: 3})
A4 = [0x61, 0x62, 0x63, 0x64]
for n in (1, 255, 256, 1023):
    case("huf1_%d" % n, G, [frame([comp(lit_huf(sym(n, n, A4), W4, wmode=("fse", 6)))])],
         why="one-stream Huffman literals, above 255 too")
for n, sf in ((1023, 1), (1023, 2), (1023, 3), (1024, 2), (16383, 2), (16384, 3), (16383, 3)):
    case("huf4_%d_sf%d" % (n, sf), G,
         [frame([comp(lit_huf(sym(n, n + sf, A4), W4, wmode=("fse", 5), streams=4, sf=sf), [(5, 7, 4)])])],
         why="four streams across the 3/4/5-byte headers")
case("huf4_131072", G, [frame([comp(lit_huf(sym(131072, 3, A4), W4, wmode=("fse", 6), streams=4, sf=3))])],
     why="largest literal section")
case("huf4_first_stream_1byte", G, [frame([comp(lit_huf(sym(8, 1, [0x61, 0x62]), W4, streams=4, sf=1))])],
     why="every stream one byte, the section at its minimum of 10 bytes")
pair("huf4_jump", G, [frame([comp(lit_huf(sym(400, 2, A4), W4, streams=4, sf=1))])],
     [frame([comp(lit_huf(sym(400, 2, A4), W4, streams=4, sf=1, jump=[60, 60, 200]))])], "jump table summing past csize")
pair("huf1_stream", G, [frame([comp(lit_huf(sym(100, 2, A4), W4))])],
     [frame([comp(lit_huf(sym(100, 2, A4), W4, stream_bytes=b"\x00" * 24))])], "stream without its padding bit")
case("huf_direct_1", G, [frame([comp(lit_huf(sym(50, 1, [0, 1]), [1]))])], why="direct weights: 1 weight (odd)")
case("huf_direct_2", G, [frame([comp(lit_huf(sym(50, 2, [0, 1, 2]), [1, 1]))])], why="direct weights: 2 (even)")
case("huf_direct_127", G, [frame([comp(lit_huf(bytes(range(128)) * 3, [1] * 127))])], why="direct weights: 127 (odd)")
case("huf_direct_128", G, [frame([comp(lit_huf(bytes(range(129)) * 3, [1] * 128))])], why="direct weights: 128 (max)")
case("huf_direct_0_128", G, [frame([comp(lit_huf(sym(90, 3, [0, 128]), [1] + [0] * 127))])],
     why="direct weights, only the lowest and the highest reachable symbol (128)")
case("huf_fse_0_255", G, [frame([comp(lit_huf(sym(90, 4, [0, 255]), [1] + [0] * 254, wmode=("fse", 5)))])],
     why="only symbols 0 and 255 (255 weights need the FSE form)")
WT = Z.huf_weights({0: 2, 1: 2, 2: 2, **{i: i for i in range(3, 11)}, 11: 11, 12: 11})
for al in (5, 6):
    case("huf_fse_al%d" % al, G, [frame([comp(lit_huf(sym(300, al, list(range(13))), WT, wmode=("fse", al)))])],
         why="FSE-compressed weights at accuracy log %d" % al)
W11 = Z.huf_weights({**{i: i + 1 for i in range(10)}, 10: 11, 11: 11})
W12 = Z.huf_weights({0: 2, 1: 2, 2: 2, **{i: i for i in range(3, 12)}, 12: 12, 13: 12})
W13 = Z.huf_weights({0: 2, 1: 2, 2: 2, 3: 3, 4: 3, **{i: i - 1 for i in range(5, 14)}, 14: 13, 15: 13})
case("huf_depth11", G, [frame([comp(lit_huf(sym(200, 1, list(range(12))), W11))])], why="longest code 11 bits")
case("huf_depth12", G, [frame([comp(lit_huf(sym(200, 1, list(range(14))), W12))])], "verdict",
     "longest code 12 bits: beyond RFC 8878, libzstd's HUF_TABLELOG_MAX is 12")
case("huf_depth13", G, [frame([comp(lit_huf(sym(200, 1, list(range(12))), W13, encode_as=W11))])], "reject",
     "longest code 13 bits", twin="huf_depth11")
pair("huf_weights_sum", G, [frame([comp(lit_huf(sym(60, 1, [0, 1, 2, 3]), [3, 1, 1]))])],
     [frame([comp(lit_huf(sym(60, 1, [0, 1, 2]), [3, 1], encode_as=[3, 1, 1]))])], "weights not summing to a power of two")
HB = comp(lit_huf(sym(300, 9, A4), W4), [(10, 20, 7)])
TB = comp(lit_treeless(sym(500, 4, A4), streams=4, sf=1), [(30, 6, 1)])
T1 = comp(lit_treeless(sym(77, 5, A4)), [(17, 6, 12)])
case("treeless_after_huf", G, [frame([HB, TB, T1])], why="treeless literals reuse the previous table")
case("treeless_across_raw_literals", G, [frame([HB, comp(lit_raw(b"plain literals"), [(4, 9, 33)]), raw(b"rawblock"), TB])],
     why="the table survives blocks without Huffman literals")
case("treeless_first_block", G, [frame([comp(lit_treeless(sym(77, 5, A4), encode_as=W4), [(17, 6, 12)])])], "reject",
     "treeless literals with no table", twin="treeless_after_huf", size=400)
pair("treeless_second_frame", G, [frame([HB]), frame([comp(lit_huf(sym(77, 5, A4), W4), [(17, 6, 12)])])],
     [frame([HB]), frame([comp(lit_treeless(sym(77, 5, A4), encode_as=W4), [(17, 6, 12)])])],
     "the table is not carried into the next frame")

# ------------------------------------------------- sequence headers and tables
G = "seq_tables"
P16 = raw(pat(16, 9))
pair("nbseq0", G, [frame([comp(lit_raw(b"only literals"))])],
     [frame([comp(lit_raw(b"only literals"), seq=dict(tail=b"\x00"))])], "nbSeq 0 followed by bytes")
for n, form in ((1, 1), (127, 1), (127, 2), (128, 2), (0x7EFF, 2), (0x7F00, 3), (0x7F01, 3)):
    case("nbseq_%d_form%d" % (n, form), G, [frame([P16, comp(lit_raw(b""), [(0, 3, 4)] * n, seq=dict(nbseq_form=form))])],
         why="nbSeq in its %d-byte form" % form)
LLN = [8, 4, 4, 4, 2, 2, 2, 2, 1, 1, 1, 1]  # LL codes 0..11, accuracy log 5
OFN = [4, 2, 8, 8, 4, 2, 1, 1, 1, 1]        # OF codes 0..9
MLN = [6, 6, 4, 4, 2, 2, 2, 2, 1, 1, 1, 1]  # ML codes 0..11
FSE3 = dict(ll=("fse", 5, LLN), of=("fse", 5, OFN), ml=("fse", 5, MLN))
RLE3 = dict(ll=("rle", 2), of=("rle", 3), ml=("rle", 4))
SQ = [(2, 7, 9), (2, 7, 12), (2, 7, 8), (2, 7, 15)]          # LL code 2, OF code 3, ML code 4 throughout
SV = [(0, 3, 9), (5, 6, 2), (11, 14, 40), (1, 3, 1), (0, 9, 3), (3, 4, 300)]
LV = lit_raw(pat(40, 2))
for f in ("ll", "of", "ml"):
    case("mode_%s_rle" % f, G, [frame([P16, comp(LV, SQ, seq={f: RLE3[f]})])], why="RLE mode for %s alone" % f)
    case("mode_%s_fse" % f, G, [frame([raw(pat(300)), comp(LV, SV, seq={f: FSE3[f]})])], why="FSE mode for %s alone" % f)
    case("mode_%s_repeat" % f, G, [frame([raw(pat(300)), comp(LV, SV, seq={f: FSE3[f]}), comp(LV, SV[::-1], seq={f: "rep"})])],
         why="Repeat mode for %s alone" % f)
case("mode_all_predefined", G, [frame([raw(pat(300)), comp(LV, SV)])], why="Predefined mode for all")
case("reserved_mode_bits", G, [frame([raw(pat(300)), comp(LV, SV, seq=dict(reserved_modes=1))])], "reject",
     "reserved bits of the Symbol_Compression_Modes byte", twin="mode_all_predefined")
case("repeat_after_predefined", G, [frame([raw(pat(300)), comp(LV, SV), comp(LV, SV, seq=dict(ll="rep", of="rep", ml="rep"))])],
     why="Repeat after Predefined")
case("repeat_after_rle", G, [frame([P16, comp(LV, SQ, seq=RLE3), comp(LV, SQ[::-1], seq=dict(ll="rep", of="rep", ml="rep"))])],
     why="Repeat after RLE")
case("repeat_after_fse_twice", G, [frame([raw(pat(300)), comp(LV, SV, seq=FSE3), comp(LV, SV, seq=dict(ll="rep", of="rep", ml="rep")),
                                          rle(3, 9), comp(LV, SV[::-1], seq=dict(ll="rep", of="rep", ml="rep"))])],
     why="Repeat after FSE, and again across an RLE block")
for f in ("ll", "of", "ml"):
    case("repeat_first_block_%s" % f, G, [frame([raw(pat(300)), comp(LV, SV, seq={f: "rep"})])], "reject",
         "Repeat mode with no previous table", twin="mode_all_predefined")
    pair("repeat_second_frame_%s" % f, G, [frame([raw(pat(300)), comp(LV, SV, seq=FSE3)]), frame([raw(pat(300)), comp(LV, SV)])],
         [frame([raw(pat(300)), comp(LV, SV, seq=FSE3)]), frame([raw(pat(300)), comp(LV, SV, seq={f: "rep"})])],
         "tables are not carried into the next frame")


def wide(al, used, nsym):
    """Counts at accuracy log al: one cell for each used symbol, the rest on symbol 0 (in `used`)."""
    n = [0] * nsym
    for s in used:
        n[s] = 1
    n[0] = (1 << al) - (len(set(used)) - 1)
    return n


for f, mx, sq in (("ll", 9, (2, 7, 9)), ("of", 8, (2, 7, 9)), ("ml", 9, (2, 7, 9))):
    c = Z.seq_codes(sq)[{"ll": 0, "of": 6, "ml": 3}[f]]
    sq0 = {"ll": (0, 7, 9), "of": (2, 7, 1), "ml": (2, 3, 9)}[f]
    pair("fse_%s_al_max" % f, G, [frame([P16, comp(LV, [sq, sq0, sq], seq={f: ("fse", mx, wide(mx, [0, c], c + 1))})])],
         [frame([P16, comp(LV, [sq, sq0, sq], seq={f: ("fse", mx + 1, wide(mx + 1, [0, c], c + 1))})])],
         "accuracy log maximum for %s is %d" % (f, mx))
    top = Z.FIELD[f][2]
    pair("fse_%s_top_symbol" % f, G, [frame([P16, comp(LV, [sq, sq0, sq], seq={f: ("fse", 6, wide(6, [0, c, top], top + 1))})])],
         [frame([P16, comp(LV, [sq, sq0, sq], seq={f: ("fse", 6, wide(6, [0, c, top + 1], top + 2))})])],
         "highest symbol of %s is %d" % (f, top))
case("fse_less_than_one", G, [frame([raw(pat(300)), comp(LV, SV, seq=dict(
    ll=("fse", 6, [20, 10, 8, 8, 4, 4, 2, 2, -1, -1, -1, 2, -1]), of=("fse", 5, [8, 8, 4, 4, -1, 2, 2, -1, 1, 1]),
    ml=("fse", 6, [30, 10, 5, 5, 5, 2, 2, -1, -1, -1, -1, 1])))])], why="counts of -1 (less than 1)")
case("fse_zero_runs", G, [frame([raw(pat(300)), comp(lit_raw(pat(60, 2)), [(0, 3, 9), (24, 35, 9), (13, 3, 9), (0, 10, 9)], seq=dict(
    ll=("fse", 5, [16] + [0] * 12 + [8] + [0] * 6 + [8]), ml=("fse", 5, [20, 0, 0, 0, 0, 0, 0, 10] + [0] * 24 + [2])))])],
     why="zero-run repeat flags: runs of 12, 6, 5 and 24")
pair("rle_ll_35", G, [frame([comp(lit_rle(0x42, 131072), [(65536, 3, 4), (65536, 5, 1)], seq=dict(ll=("rle", 35)))])],
     [frame([comp(lit_rle(0x42, 70000), [dict(llc=36, ml=3, ofv=4)], seq=dict(ll=("rle", 36)))])], "RLE-mode LL symbol maximum 35")
pair("rle_ml_52", G, [frame([P16, comp(lit_raw(b""), [(0, 65539, 4)], seq=dict(ml=("rle", 52)))])],
     [frame([P16, comp(lit_raw(b""), [dict(ll=0, mlc=53, ofv=4)], seq=dict(ml=("rle", 53)))])], "RLE-mode ML symbol maximum 52")
case("rle_of_32", G, [frame([P16, comp(lit_raw(b""), [dict(ll=0, ml=3, ofc=32)], seq=dict(of=("rle", 32)))])], "reject",
     "RLE-mode OF symbol above 31", twin="mode_of_rle")

# ------------------------------------------------------------ sequence values
G = "seq_values"
for which in ("min", "max"):
    ext = (lambda b: 0) if which == "min" else (lambda b: (1 << b) - 1)
    lo = [dict(llc=c, llx=ext(Z.LL_BITS[c]), mlc=c, mlx=ext(Z.ML_BITS[c]), ofv=4 + c) for c in range(34)]
    hi = [dict(llc=34, llx=ext(15), mlc=52, mlx=ext(16), ofv=1)]
    h2 = [dict(llc=35, llx=ext(16) >> (1 if which == "max" else 0), mlc=51, mlx=ext(15), ofv=2)]
    ml = [dict(ll=0, mlc=c, mlx=ext(Z.ML_BITS[c]), ofv=4 + c) for c in range(34, 53)]
    blocks = [raw(pat(64, 4))]
    for s in (lo, hi, h2, ml):
        need = sum(Z.seq_codes(q)[8] for q in s)
        blocks.append(comp(lit_rle(0x30 + len(blocks), need + 2) if need > 70000 else lit_raw(pat(need + 2, len(blocks))), s))
    case("ll_ml_codes_%s" % which, G, [frame(blocks)], why="every LL code 0-35 and ML code 0-52 at %s extra bits" % which)
case("ll_code35_max", G, [frame([P16, comp(lit_rle(0x55, 131071), [dict(llc=35, llx=65535, ml=3, ofv=4)])])],
     why="literal-length code 35 at maximum extra bits (131071 literals)")
for c in range(2, 25):
    off = (1 << c) - 3
    big = off >= (1 << 20)
    pair("of_code%d_min" % c, G, [frame(pre(off - 1) + [comp(lit_raw(b"x"), [(1, 5, off + 3)])], wlog=max(10, c + 1))],
         [frame(pre(off - 1) + [comp(lit_raw(b"x"), [(0, 5, off + 3)])], wlog=max(10, c + 1))],
         "offset code %d: offset equal to the bytes produced / one more" % c, big=big)
    if c < 24:
        off = (1 << (c + 1)) - 4
        case("of_code%d_max" % c, G, [frame(pre(off + 9) + [comp(lit_raw(b"x"), [(1, 5, off + 3)])], wlog=max(10, c + 2))],
             why="offset code %d at maximum extra bits" % c, big=big)
case("of_code0_1", G, [frame([P16, comp(lit_raw(b"ab"), [(1, 4, 1), (1, 4, 2), (0, 5, 3)])])], why="offset codes 0 and 1")
PRE16M = pre((1 << 24) + 64)
for c in range(25, 32):
    case("of_code%d_twin" % c, G, [frame([P16, comp(lit_raw(b"ab"), [(1, 4, 4), dict(ll=1, ml=4, ofc=2, ofx=1)],
                                                    seq=dict(of=("fse", 5, wide(5, [0, 2, c], c + 1))))])],
         why="the table of of_code%d with its last sequence on code 2" % c)
    case("of_code%d" % c, G, [frame([P16, comp(lit_raw(b"ab"), [(1, 4, 4), dict(ll=1, ml=4, ofc=c, ofx=0)],
                                           seq=dict(of=("fse", 5, wide(5, [0, 2, c], c + 1))))])], "reject",
         "offset code %d reaches past any output" % c, twin="of_code%d_twin" % c)
case("of_code25_after_16m", G, [frame(PRE16M + [comp(lit_raw(b"ab"), [(1, 4, 4), dict(ll=1, ml=4, ofc=25, ofx=0)])], wlog=26)],
     "reject", "offset code 25 after 16 MiB of output", twin="of_code24_min", size=(1 << 24) + 64 + 10, big=True)
case("of_code31_alias_twin", G,
     [frame([raw(pat(32, 8)), comp(lit_raw(b"abcd"), [(1, 4, 10), (1, 4, 14), (1, 4, 20), dict(ll=1, ml=4, ofc=4, ofx=3)],
                                   seq=dict(of=("fse", 5, wide(5, [0, 3, 4, 31], 32))))])],
     why="the table and sequences of of_code31_alias_* with the last sequence on code 4")
for tag, x in (("rep0", 3), ("rep1", 3 + (1 << 29)), ("rep2_5", 3 + (2 << 29) + 5)):
    case("of_code31_alias_" + tag, G,
         [frame([raw(pat(32, 8)), comp(lit_raw(b"abcd"), [(1, 4, 10), (1, 4, 14), (1, 4, 20), dict(ll=1, ml=4, ofc=31, ofx=x)],
                                        seq=dict(of=("fse", 5, wide(5, [0, 3, 4, 31], 32))))])],
         "reject", "offset 2^31 + %d - 3 reads as a symbolic repeat offset when bit 31 flags one" % x, twin="of_code31_alias_twin")

# ------------------------------------------------------------- repeat offsets
G = "repeat_offsets"
SETUP = [(2, 4, 5 + 3), (2, 4, 9 + 3), (2, 4, 14 + 3)]  # rep = 14, 9, 5
PERMS = [(1, 2, 3), (1, 3, 2), (2, 1, 3), (2, 3, 1), (3, 1, 2), (3, 2, 1)]
for tag, lls in (("ll_pos", (1, 2, 1)), ("ll_zero", (0, 0, 0)), ("ll_mixed", (0, 1, 0)), ("ll_mixed2", (1, 0, 1))):
    s = list(SETUP)
    for p in PERMS:
        s += [(lls[i], 3 + i, p[i]) for i in range(3)]
    case("rep_orders_" + tag, G, [frame([raw(pat(40, 3)), comp(lit_raw(pat(sum(q[0] for q in s), 5)), s)])],
         why="Offset_Value 1/2/3 in every order")
for n in (7, 8, 9, 17, 64, 65):
    s = list(SETUP) + [((i * 5 + n) % 3 % 2 * (1 + i % 2), 3 + i % 4, 1 + (i * 7 + i // 3 + n) % 3) for i in range(n - 3)]
    assert len(s) == n
    case("rep_chain_%d" % n, G, [frame([raw(pat(40, n)), comp(lit_raw(pat(sum(q[0] for q in s), n)), s)])],
         why="repeat-offset chain across the 8-record period / 64-lane wave")
case("rep_walk_down", G, [frame([raw(pat(64, 2)), comp(lit_raw(b"q"), [(1, 4, 43)] + [(0, 3, 3)] * 70)])],
     why="70 x (Offset_Value 3, ll 0) from rep0 = 40: walks down through 1")
for nl, ov, good in ((1, 1, True), (4, 2, True), (8, 3, True), (3, 2, False), (7, 3, False), (7, 2, True), (4, 3, False)):
    case("rep_initial_%dbytes_ov%d" % (nl, ov), G, [frame([comp(lit_raw(pat(nl + 1, 1)), [(nl, 4, ov)])])],
         "accept" if good else "reject", "initial repeat offsets 1/4/8 used by the first sequence",
         twin=None if good else "rep_initial_%dbytes_ov%d" % ({2: 4, 3: 8}[ov], ov), size=nl + 5)
for tag, mid in (("direct", []), ("raw", [raw(pat(9, 2))]), ("rle", [rle(0x66, 9)]), ("mixed", [rle(1, 0), raw(b"k"), comp(lit_raw(b"xyz"))])):
    case("rep_carry_" + tag, G, [frame([raw(pat(40, 3)), comp(lit_raw(b"abcdef"), SETUP)] + mid +
                                       [comp(lit_raw(b"123456"), [(1, 4, 2), (2, 5, 3), (0, 3, 1), (1, 3, 1)])])],
         why="repeat offsets carried into the next compressed block")
case("rep_not_across_frames", G, [frame([raw(pat(40, 3)), comp(lit_raw(b"abcdef"), SETUP)]),
                                  frame([comp(lit_raw(pat(30, 7)), [(25, 6, 1), (1, 4, 2), (1, 4, 3)])])],
     why="repeat offsets restart at 1/4/8 in every frame")

# ------------------------------------------------------------------ bit budget
G = "bit_budget"
BB = dict(ll=("fse", 9, wide(9, [0, 25], 26)), of=("fse", 8, wide(8, [0, 24], 25)), ml=("fse", 9, wide(9, [0, 52], 53)))
case("bits72_x40", G, [frame(PRE16M + [comp(lit_raw(pat(127 * 40, 6)), [dict(llc=25, llx=63, mlc=52, mlx=65535, ofc=24, ofx=i) for i in range(40)],
                                          seq=BB)], wlog=25)],
     why="40 sequences of 9+8+9 state bits and 24+16+6 extra bits: 72 bits each (ring budget)", big=True)
case("bits89_x40", G, [frame([P16, comp(lit_rle(1, 131072), [dict(llc=35, llx=65535, mlc=52, mlx=65535, ofc=31, ofx=(1 << 31) - 1)] * 40, seq=dict(
    ll=("fse", 9, wide(9, [0, 35], 36)), of=("fse", 8, wide(8, [0, 31], 32)), ml=("fse", 9, wide(9, [0, 52], 53))))])],
     "reject", "the 89-bit form (OF 31, LL 35, ML 52): comparable by verdict only", twin="bits72_x40", size=1 << 20)
P1K = raw(pat(1100, 4))
for c in range(2, 10):
    pos = (17 + c) % 8
    case("pad_pos%d" % pos, G, [frame([P1K, comp(lit_raw(b"a"), [(1, 3, 1 << c)], seq=dict(want_pad_pos=pos))])],
         why="padding bit at position %d of the final byte" % pos)
pair("pad_pos_ref", G, [frame([P1K, comp(lit_raw(b"a"), [(1, 3, 512)])])],
     [frame([P1K, comp(lit_raw(b"a"), [(1, 3, 512)], seq=dict(last_byte=0))])], "final byte 0: no padding bit")
case("one_spare_bit", G, [frame([P1K, comp(lit_raw(b"a"), [(1, 3, 512)], seq=dict(spare_bits=1))])], "reject",
     "one unread bit left over", twin="pad_pos_ref")
case("one_bit_short", G, [frame([P1K, comp(lit_raw(b"a"), [(1, 3, 512), (0, 4, 700)], seq=dict(drop_bits=1))])], "reject",
     "one bit too few: the last read runs past the start of the stream", twin="pad_pos_ref", size=1100 + 8)
case("eight_bits_short", G, [frame([P1K, comp(lit_raw(b"a"), [(1, 3, 512), (0, 4, 700), (0, 3, 600)], seq=dict(drop_bits=30))])], "reject",
     "30 bits too few: a sequence starts with the stream already over-read", twin="pad_pos_ref", size=1100 + 11)
ALLR = dict(ll=("rle", 0), ml=("rle", 0))
case("seq_stream_1byte", G, [frame([P1K, comp(lit_raw(b""), [(0, 3, 4)], seq=dict(of=("rle", 2), want_stream_len=1, **ALLR))])],
     why="sequence bitstream of 1 byte")
for nb in (2, 15, 16, 17, 32, 33):
    case("seq_stream_%dbytes" % nb, G, [frame([P1K, comp(lit_raw(b""), [(0, 3, 256 + 7 * i) for i in range(nb - 1)],
                                                     seq=dict(of=("rle", 8), want_stream_len=nb, **ALLR))])],
         why="sequence bitstream of %d bytes" % nb)

# ---------------------------------------------------------------- replay edges
G = "replay"
OFFS = list(range(1, 17)) + [63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193]
P8K = raw(pat(8200, 11))
for ml in (3, 64, 65, 200):
    s = [(i % 3, ml, o + 3) for i, o in enumerate(OFFS)]
    case("offsets_ml%d" % ml, G, [frame([P8K, comp(lit_raw(pat(sum(q[0] for q in s), ml)), s)], wlog=14)],
         why="offsets around 16 / 64 / 2048 / 8192 with match length %d" % ml)
case("match_70000", G, [frame([P8K, comp(lit_raw(b"uvw"), [(1, 70000, 1 + 3), (1, 70000, 64 + 3), (1, 70000, 8193 + 3)])], wlog=18)],
     why="match length 70000 at offsets 1, 64, 8193")
for o in (8191, 8192, 8193):
    case("offset_%d_alone" % o, G, [frame([P8K, comp(lit_raw(b"uvw"), [(3, 300, o + 3)])], wlog=14)], why="offset beside R = 8192")
case("literal_runs", G, [frame([P16, comp(lit_raw(pat(63 + 64 + 65 + 2047 + 2048 + 2049 + 5, 3)),
                                         [(63, 4, 9), (64, 4, 70), (65, 3, 1), (2047, 5, 2000), (2048, 4, 2), (2049, 3, 4100)])])],
     why="literal runs of 63/64/65 and 2047/2048/2049")
case("match_into_raw_block", G, [frame([raw(pat(100, 5)), comp(lit_raw(b"abcdefgh"), [(8, 40, 20 + 3), (0, 30, 108 + 40 + 3)])])],
     why="match source spanning the boundary into a preceding raw block")
case("match_into_rle_block", G, [frame([raw(pat(10)), rle(0xEE, 100), comp(lit_raw(b"abcdefgh"), [(8, 40, 20 + 3), (0, 30, 108 + 40 + 10 + 3)])])],
     why="match source spanning the boundary into a preceding RLE block")
pair("offset_within_frame", G, [frame([raw(pat(50, 1))]), frame([raw(pat(20, 2)), comp(lit_raw(b"ab"), [(2, 5, 22 + 3)])])],
     [frame([raw(pat(50, 1))]), frame([raw(pat(20, 2)), comp(lit_raw(b"ab"), [(2, 5, 23 + 3)])])],
     "an offset in the second frame reaching into the first frame's output")
for n in (0, 1, 3000):
    case("literals_left_%d" % n, G, [frame([P16, comp(lit_raw(pat(5 + n, n)), [(2, 4, 5), (3, 3, 1)])])],
         why="%d literals after the last sequence" % n)
case("literals_one_short", G, [frame([P16, comp(lit_raw(pat(5, 0)), [(2, 4, 5), (4, 3, 1)])])], "reject",
     "sequences asking for one literal more than the section holds", twin="literals_left_0", size=29)

GROUPS = ["frame", "literals", "seq_tables", "seq_values", "repeat_offsets", "bit_budget", "replay"]
assert {c["group"] for c in CASES} == set(GROUPS)
for _c in CASES:
    if _c["intent"] == "reject" and _c["twin"]:
        assert _BY[_c["twin"]]["intent"] == "accept", _c["name"]
BY_NAME = _BY


def caps(c):
    """The dst caps a case is decoded with: exact and one short (big cases: exact only)."""
    if c["big"]:
        return [c["size"]]
    out = [c["size"]] + ([c["size"] - 1] if c["size"] > 0 else [])
    if c["intent"] == "accept" and c["name"] in CAP0:
        out.append(0)
    return out


CAP0 = {"fcs1_255", "two_frames", "lit_rle_4096", "huf4_1024_sf2", "mode_all_predefined", "rep_chain_9", "offsets_ml3",
        "raw_block_0", "fcs4_0"}

_CACHE = {}


def built(c):
    """(frame bytes, expected output or None) of a case, built once."""
    if c["name"] not in _CACHE:
        _CACHE[c["name"]] = Z._build(c["desc"])
    return _CACHE[c["name"]]


def fixture():
    """tests/golden/zstd_conformance.json as {(name, cap): entry}."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_conformance.json")) as f:
        return {(e["name"], int(cap)): dict(name=e["name"], frame_sha=e["frame_sha"], cap=int(cap), ret=v[0], err=v[1], out_sha=v[2])
                for e in json.load(f)["cases"] for cap, v in e["caps"].items()}


def expected(c, e, oracle):
    """(result, output sha256) this project owes for a fixture entry: libzstd
    1.4.9's, except for LAX_149, where it is the CPU oracle's in its default
    mode (the pinned version's rules): a rejection."""
    if c["name"] in LAX_149:
        r, _ = oracle.zstd_decompress(built(c)[0], e["cap"])
        assert r < 0, c["name"]
        return r, None
    return e["ret"], e["out_sha"]
