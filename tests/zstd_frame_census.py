"""Test-only Zstandard frame reader, written from RFC 8878: it decodes a whole
frame (header, raw / RLE / compressed blocks, every literals format, every
sequence-table mode, the backward bitstreams, the repeat-offset rules) and
names the format features the frame uses.

    census(frame) -> (decoded bytes, set of feature names)

FEATURES lists every name it can give.  The reader is a decoder of its own:
a census counts only when the decoded bytes equal the encoder's input, which
the callers check.  It shares the FSE table builder and the code / baseline
tables with the frame writer tests/zstd_frames.py.
"""
from __future__ import annotations

from tests.zstd_frames import (BLOCK_MAX, FIELD, LL_BASE, LL_BITS, MAGIC, ML_BASE, ML_BITS, fse_table, huf_codes,
                               huf_full, rle_table, xxh64)

NEAR_WINDOW = 1024  # "near the window": an offset within this many bytes of the frame's window size

FEATURES = (
    # frame header
    "fcs_1byte", "fcs_2byte", "fcs_4byte",  # width of the frame-content-size field
    "size_255", "size_256", "size_65791", "size_65792",  # content sizes on each side of the width steps
    "single_segment", "window_descriptor",
    # blocks
    "block_raw", "block_rle", "block_compressed",
    "const_first_block_compressed",  # a first block of one repeated byte, sent compressed (not RLE)
    "last_block_1", "last_block_2", "last_block_3",  # a last block of 1 / 2 / 3 bytes behind other blocks
    "zero_sequences",  # a compressed block with literals only
    # literals section
    "lit_raw_h1", "lit_raw_h2", "lit_raw_h3",  # raw literals, 1- / 2- / 3-byte header
    "lit_rle",
    "lit_huf_1s", "lit_huf_4s_10", "lit_huf_4s_14", "lit_huf_4s_18",  # Huffman: 1 stream; 4 streams, 10/14/18-bit sizes
    "lit_treeless_1s", "lit_treeless_4s_10", "lit_treeless_4s_14", "lit_treeless_4s_18",
    "huf_weights_direct", "huf_weights_fse",
    "huf_depth_11",  # longest Huffman code = 11 bits
    # sequence count
    "nbseq_1byte", "nbseq_2byte", "nbseq_3byte", "nbseq_127", "nbseq_128",
    # table mode per field
    "ll_predefined", "ll_rle", "ll_fse", "ll_repeat",
    "of_predefined", "of_rle", "of_fse", "of_repeat",
    "ml_predefined", "ml_rle", "ml_fse", "ml_repeat",
    # values
    "ll_ge_65536",  # literal length code 35
    "ml_65538", "ml_65539", "ml_65540",  # the last length of match-length code 51, the first two of code 52
    "ml_ge_65539",
    "rep_offset_1", "rep_offset_2", "rep_offset_3",  # Offset_Value 1 / 2 / 3
    "rep_ll0",  # a repeat offset with literal length 0 (the shifted rule)
    "offset_gt_128k",  # a match that starts in an earlier block
    "offset_near_window",  # window descriptor present, an offset within NEAR_WINDOW of the window size
)


class Corrupt(Exception):
    pass


def _need(ok, what):
    if not ok:
        raise Corrupt(what)


class _Fwd:
    """LSB-first forward bit reader over b[at:]."""

    def __init__(self, b: bytes, at: int, end: int):
        self.v, self.pos, self.at, self.nbits = int.from_bytes(b[at:end], "little"), 0, at, 8 * (end - at)

    def peek(self, n):
        return (self.v >> self.pos) & ((1 << n) - 1)

    def skip(self, n):
        self.pos += n

    def read(self, n):
        x = self.peek(n)
        self.pos += n
        return x

    def end(self):
        _need(self.pos <= self.nbits, "FSE table description runs past its section")
        return self.at + (self.pos + 7) // 8


class _Back:
    """Backward bitstream: the last byte holds the padding 1-bit; reads come from the top down."""

    PAD = 64

    def __init__(self, b: bytes):
        _need(len(b) > 0 and b[-1] != 0, "backward bitstream without its end mark")
        v = int.from_bytes(b, "little")
        self.left = v.bit_length() - 1
        self.v = (v & ((1 << self.left) - 1)) << self.PAD

    def read(self, n):
        """n bits; bits past the start of the stream read as zero and left goes negative"""
        self.left -= n
        _need(self.left >= -self.PAD, "backward bitstream overrun")
        return (self.v >> (self.left + self.PAD)) & ((1 << n) - 1)

    def peek_msb(self, n):
        """the next n bits without consuming them (zero-filled past the start)"""
        return (self.v >> (self.left - n + self.PAD)) & ((1 << n) - 1) if self.left - n >= -self.PAD else 0


def read_ncount(b: bytes, at: int, end: int, max_al: int, max_sym: int):
    """FSE table description -> (accuracy log, counts, offset behind it)"""
    r = _Fwd(b, at, end)
    al = r.read(4) + 5
    _need(al <= max_al, "FSE accuracy log too high")
    remaining, threshold, nb, norm = (1 << al) + 1, 1 << al, al + 1, []
    while remaining > 1 and len(norm) <= max_sym:
        mx = 2 * threshold - 1 - remaining
        low = r.peek(nb - 1)
        if low < mx:
            v = low
            r.skip(nb - 1)
        else:
            v = r.peek(nb)
            if v >= threshold:
                v -= mx
            r.skip(nb)
        c = v - 1
        remaining -= abs(c)
        _need(remaining >= 1, "FSE counts exceed the table")
        norm.append(c)
        if c == 0:
            while True:
                z = r.read(2)
                norm += [0] * z
                if z != 3:
                    break
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    _need(remaining == 1 and len(norm) <= max_sym + 1, "FSE counts do not fill the table")
    return al, norm, r.end()


def _huf_tree(b: bytes, at: int, end: int, feats: set):
    """Huffman tree description -> ({symbol: (code, length)}, depth, offset behind it)"""
    _need(at < end, "no Huffman tree description")
    h = b[at]
    at += 1
    if h >= 128:
        n = h - 127
        nbytes = (n + 1) // 2
        _need(at + nbytes <= end, "direct weights cut short")
        w = []
        for i in range(n):
            x = b[at + i // 2]
            w.append(x >> 4 if i % 2 == 0 else x & 15)
        at += nbytes
        feats.add("huf_weights_direct")
    else:
        _need(at + h <= end and h >= 2, "FSE-coded weights cut short")
        al, norm, p = read_ncount(b, at, at + h, 6, 12)
        tab = fse_table(al, norm)
        _need(tab is not None, "weight table does not build")
        bs = _Back(b[p:at + h])
        s1, s2, w = bs.read(al), bs.read(al), []
        _need(bs.left >= 0, "weight stream shorter than its two states")
        while True:
            w.append(tab["sym"][s1])
            s1 = tab["base"][s1] + bs.read(tab["nb"][s1])
            if bs.left < 0:
                w.append(tab["sym"][s2])
                break
            w.append(tab["sym"][s2])
            s2 = tab["base"][s2] + bs.read(tab["nb"][s2])
            if bs.left < 0:
                w.append(tab["sym"][s1])
                break
        _need(len(w) <= 255, "too many Huffman weights")
        at += h
        feats.add("huf_weights_fse")
    hf = huf_full(w)
    _need(hf is not None, "Huffman weights do not form a tree")
    full, depth = hf
    return huf_codes(full, depth), depth, at


def _huf_stream(codes, depth: int, b: bytes, n: int) -> bytes:
    """n symbols of one Huffman stream"""
    look = [None] * (1 << depth)
    for s, (code, ln) in codes.items():
        lo = code << (depth - ln)
        for x in range(lo, lo + (1 << (depth - ln))):
            look[x] = (s, ln)
    bs, out = _Back(b), bytearray()
    for _ in range(n):
        e = look[bs.peek_msb(depth)]
        _need(e is not None, "no Huffman code for these bits")
        out.append(e[0])
        bs.left -= e[1]
    _need(bs.left == 0, "Huffman stream not used up exactly")
    return bytes(out)


def _literals(b: bytes, at: int, end: int, st: dict, feats: set):
    """-> (literal bytes, offset behind the section)"""
    _need(at < end, "no literals section")
    t, sf = b[at] & 3, (b[at] >> 2) & 3
    if t < 2:
        if sf in (0, 2):
            regen, hs = b[at] >> 3, 1
        elif sf == 1:
            regen, hs = int.from_bytes(b[at:at + 2], "little") >> 4, 2
        else:
            regen, hs = int.from_bytes(b[at:at + 3], "little") >> 4, 3
        _need(at + hs <= end and regen <= BLOCK_MAX, "raw / RLE literals header")
        at += hs
        if t == 0:
            _need(at + regen <= end, "raw literals cut short")
            feats.add("lit_raw_h%d" % hs)
            return b[at:at + regen], at + regen
        _need(at < end, "RLE literals without their byte")
        feats.add("lit_rle")
        return b[at:at + 1] * regen, at + 1
    bits, hs = {0: (10, 3), 1: (10, 3), 2: (14, 4), 3: (18, 5)}[sf]
    _need(at + hs <= end, "literals header cut short")
    h = int.from_bytes(b[at:at + hs], "little") >> 4
    regen, csize = h & ((1 << bits) - 1), h >> bits
    at += hs
    _need(regen <= BLOCK_MAX and at + csize <= end and regen > 0, "compressed literals sizes")
    send = at + csize
    fmt = "1s" if sf == 0 else "4s_%d" % bits
    if t == 2:
        codes, depth, at = _huf_tree(b, at, send, feats)
        st["huf"] = (codes, depth)
        feats.add("lit_huf_" + fmt)
        if depth == 11:
            feats.add("huf_depth_11")
    else:
        _need(st["huf"] is not None, "treeless literals without an earlier tree")
        codes, depth = st["huf"]
        feats.add("lit_treeless_" + fmt)
    if sf == 0:
        return _huf_stream(codes, depth, b[at:send], regen), send
    _need(at + 6 <= send, "no jump table")
    j = [int.from_bytes(b[at + 2 * i:at + 2 * i + 2], "little") for i in range(3)]
    at += 6
    _need(at + sum(j) < send, "jump table past the section")
    seg = (regen + 3) // 4
    _need(regen >= 3 * seg, "four streams for too few literals")
    cuts = [at, at + j[0], at + j[0] + j[1], at + sum(j), send]
    out = b"".join(_huf_stream(codes, depth, b[cuts[i]:cuts[i + 1]], seg if i < 3 else regen - 3 * seg)
                   for i in range(4))
    return out, send


_PRE = {}


def _seq_table(field: str, mode: int, b: bytes, at: int, end: int, st: dict, feats: set):
    dflt, dal, maxsym, maxal = FIELD[field]
    feats.add(field + ("_predefined", "_rle", "_fse", "_repeat")[mode])
    if mode == 0:
        if field not in _PRE:
            _PRE[field] = fse_table(dal, dflt)
        tab = _PRE[field]
    elif mode == 1:
        _need(at < end and b[at] <= maxsym, "RLE table symbol")
        tab, at = rle_table(b[at]), at + 1
    elif mode == 2:
        al, norm, at = read_ncount(b, at, end, maxal, maxsym)
        tab = fse_table(al, norm)
        _need(tab is not None, "sequence table does not build")
    else:
        tab = st[field]
        _need(tab is not None, "repeat mode without an earlier table")
        return tab, at
    st[field] = tab
    return tab, at


def _sequences(b: bytes, at: int, end: int, st: dict, feats: set):
    """-> [(literal length, match length, Offset_Value)]"""
    _need(at < end, "no sequences section")
    n = b[at]
    if n < 128:
        at += 1
        if n:
            feats.add("nbseq_1byte")
    elif n < 255:
        _need(at + 2 <= end, "sequence count cut short")
        n, at = ((n - 128) << 8) + b[at + 1], at + 2
        feats.add("nbseq_2byte")
    else:
        _need(at + 3 <= end, "sequence count cut short")
        n, at = b[at + 1] + (b[at + 2] << 8) + 0x7F00, at + 3
        feats.add("nbseq_3byte")
    if n in (127, 128):
        feats.add("nbseq_%d" % n)
    if n == 0:
        _need(at == end, "bytes behind a zero sequence count")
        feats.add("zero_sequences")
        return []
    _need(at < end, "no table modes")
    modes = b[at]
    at += 1
    _need(modes & 3 == 0, "reserved mode bits")
    tl, at = _seq_table("ll", modes >> 6, b, at, end, st, feats)
    to, at = _seq_table("of", (modes >> 4) & 3, b, at, end, st, feats)
    tm, at = _seq_table("ml", (modes >> 2) & 3, b, at, end, st, feats)
    _need(at < end, "no sequence bitstream")
    bs = _Back(b[at:end])
    sl, so, sm = bs.read(tl["al"]), bs.read(to["al"]), bs.read(tm["al"])
    out = []
    for i in range(n):
        llc, ofc, mlc = tl["sym"][sl], to["sym"][so], tm["sym"][sm]
        _need(llc <= 35 and mlc <= 52 and ofc <= 31, "sequence code past its alphabet")
        ofv = (1 << ofc) + bs.read(ofc)
        ml = ML_BASE[mlc] + bs.read(ML_BITS[mlc])
        ll = LL_BASE[llc] + bs.read(LL_BITS[llc])
        out.append((ll, ml, ofv))
        if i + 1 < n:
            sl = tl["base"][sl] + bs.read(tl["nb"][sl])
            sm = tm["base"][sm] + bs.read(tm["nb"][sm])
            so = to["base"][so] + bs.read(to["nb"][so])
        _need(bs.left >= 0, "sequence bitstream too short")
    _need(bs.left == 0, "sequence bitstream not used up exactly")
    return out


def _execute(out: bytearray, base: int, lits: bytes, seqs, rep, window: int, has_wd: bool, feats: set):
    lp = 0
    for ll, ml, ofv in seqs:
        if ofv > 3:
            off = ofv - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            feats.add("rep_offset_%d" % ofv)
            if ll == 0:
                feats.add("rep_ll0")
            k = ofv - 1 + (1 if ll == 0 else 0)
            if k == 0:
                off = rep[0]
            else:
                off = rep[0] - 1 if k == 3 else rep[k]
                _need(off > 0, "repeat offset of zero")
                rep[:] = [off, rep[0], rep[2]] if k == 1 else [off, rep[0], rep[1]]
        if ll >= 65536:
            feats.add("ll_ge_65536")
        if ml >= 65539:
            feats.add("ml_ge_65539")
        if ml in (65538, 65539, 65540):
            feats.add("ml_%d" % ml)
        if off > BLOCK_MAX:
            feats.add("offset_gt_128k")
        if has_wd and off > window - NEAR_WINDOW:
            feats.add("offset_near_window")
        _need(lp + ll <= len(lits), "sequences use more literals than there are")
        out += lits[lp:lp + ll]
        lp += ll
        _need(off <= len(out) - base and off <= window, "offset past the start of the window")
        if off >= ml:
            start = len(out) - off
            out += out[start:start + ml]
        else:
            pat = bytes(out[-off:])
            out += (pat * (ml // off + 1))[:ml]
    out += lits[lp:]


def census(frame: bytes):
    """One whole frame -> (decoded bytes, set of feature names); Corrupt when it does not decode."""
    b = bytes(frame)
    _need(len(b) >= 6 and int.from_bytes(b[:4], "little") == MAGIC, "magic number")
    feats = set()
    fhd, at = b[4], 5
    _need(fhd & 0x08 == 0 and fhd & 3 == 0, "reserved bit or dictionary id")
    single, check = bool(fhd & 0x20), bool(fhd & 0x04)
    window = None
    if not single:
        wd = b[at]
        at += 1
        wbase = 1 << (10 + (wd >> 3))
        window = wbase + (wbase >> 3) * (wd & 7)
        feats.add("window_descriptor")
    else:
        feats.add("single_segment")
    fw = {0: 1 if single else 0, 1: 2, 2: 4, 3: 8}[fhd >> 6]
    content = None
    if fw:
        _need(at + fw <= len(b), "frame content size cut short")
        content = int.from_bytes(b[at:at + fw], "little") + (256 if fw == 2 else 0)
        at += fw
        feats.add("fcs_%dbyte" % fw)
        if content in (255, 256, 65791, 65792):
            feats.add("size_%d" % content)
    if single:
        window = content
    st = {"huf": None, "ll": None, "of": None, "ml": None}
    rep, out, nblocks = [1, 4, 8], bytearray(), 0
    while True:
        _need(at + 3 <= len(b), "block header cut short")
        h = int.from_bytes(b[at:at + 3], "little")
        last, bt, size = h & 1, (h >> 1) & 3, h >> 3
        at += 3
        before = len(out)
        if bt == 0:
            _need(at + size <= len(b), "raw block cut short")
            out += b[at:at + size]
            at += size
            feats.add("block_raw")
        elif bt == 1:
            _need(at < len(b), "RLE block without its byte")
            out += b[at:at + 1] * size
            at += 1
            feats.add("block_rle")
        else:
            _need(bt == 2 and 3 <= size < BLOCK_MAX and at + size <= len(b), "compressed block header")
            lits, p = _literals(b, at, at + size, st, feats)
            seqs = _sequences(b, p, at + size, st, feats)
            _execute(out, 0, lits, seqs, rep, window, not single, feats)
            at += size
            feats.add("block_compressed")
            if nblocks == 0 and len(out) > 0 and out.count(out[0]) == len(out):
                feats.add("const_first_block_compressed")
        _need(len(out) - before <= BLOCK_MAX, "block decodes to more than 128 KiB")
        nblocks += 1
        if last:
            if nblocks > 1 and 1 <= len(out) - before <= 3:
                feats.add("last_block_%d" % (len(out) - before))
            break
    if check:
        _need(at + 4 <= len(b) and int.from_bytes(b[at:at + 4], "little") == xxh64(bytes(out)) & 0xFFFFFFFF,
              "content checksum")
        at += 4
    _need(at == len(b), "bytes behind the frame")
    _need(content is None or content == len(out), "frame content size differs from the content")
    assert feats <= set(FEATURES)
    return bytes(out), feats
