"""Test-only Zstandard frame writer, written from RFC 8878.

It turns an explicit description (plain dicts, see the constructors at the
end) into frame bytes -- every header field, block type, literal format,
sequence-table mode and bitstream detail is chosen by the caller, so frames no
encoder would emit (and corrupt ones) can be assembled by hand -- and models
the expected output: expand(description) replays literals and sequences and
returns the bytes a correct decoder must produce, or None for a corrupt
description.  Where RFC 8878 and libzstd differ (Huffman depth 12 is accepted,
the window size is not enforced by the one-shot API) the model follows libzstd.
"""
from __future__ import annotations

import struct

MAGIC = 0xFD2FB528
BLOCK_MAX = 128 << 10

LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512,
           1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
assert len(LL_BASE) == len(LL_BITS) == len(LL_DEF) == 36 and len(ML_BASE) == len(ML_BITS) == len(ML_DEF) == 53
assert len(OF_DEF) == 29
# field -> (predefined counts, predefined accuracy log, highest symbol, highest accuracy log)
FIELD = {"ll": (LL_DEF, 6, 35, 9), "of": (OF_DEF, 5, 31, 8), "ml": (ML_DEF, 6, 52, 9)}


# ------------------------------------------------------------------ XXH64
_P1, _P2, _P3, _P4, _P5 = (11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579,
                           2870177450012600261)
_M = (1 << 64) - 1


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _xround(acc, v):
    return (_rotl((acc + v * _P2) & _M, 31) * _P1) & _M


def xxh64(b: bytes, seed: int = 0) -> int:
    n, p = len(b), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        while p + 32 <= n:
            w = struct.unpack_from("<4Q", b, p)
            v = [_xround(v[i], w[i]) for i in range(4)]
            p += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for x in v:
            h = ((h ^ _xround(0, x)) * _P1 + _P4) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while p + 8 <= n:
        h = (_rotl(h ^ _xround(0, struct.unpack_from("<Q", b, p)[0]), 27) * _P1 + _P4) & _M
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", b, p)[0] * _P1) & _M, 23) * _P2 + _P3) & _M
        p += 4
    while p < n:
        h = (_rotl(h ^ (b[p] * _P5) & _M, 11) * _P1) & _M
        p += 1
    h = ((h ^ (h >> 33)) * _P2) & _M
    h = ((h ^ (h >> 29)) * _P3) & _M
    return h ^ (h >> 32)


# ------------------------------------------------------------- bit writers
class BitW:
    """LSB-first bit writer."""

    def __init__(self):
        self.out, self.v, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, val: int, nb: int):
        assert 0 <= val < (1 << nb) or (nb == 0 and val == 0), (val, nb)
        self.v |= val << self.n
        self.n += nb
        self.total += nb
        while self.n >= 8:
            self.out.append(self.v & 255)
            self.v >>= 8
            self.n -= 8

    def bytes(self) -> bytes:
        return bytes(self.out) + (bytes([self.v]) if self.n else b"")


def backward(reads, spare_bits: int = 0, drop_bits: int = 0) -> bytes:
    """The backward bitstream a decoder reads as `reads` = [(value, nbits)],
    first read at the top, closed by the padding 1-bit.  spare_bits zero bits
    are left below the last read (never consumed); drop_bits bits of the last
    reads are cut off the bottom (the decoder runs out of bits)."""
    w = BitW()
    w.put(0, spare_bits)
    for v, n in reversed(reads):
        if drop_bits:
            k = min(drop_bits, n)
            v, n, drop_bits = v >> k, n - k, drop_bits - k
        w.put(v, n)
    w.put(1, 1)
    return w.bytes()


# --------------------------------------------------------------------- FSE
def write_ncount(al: int, norm) -> bytes:
    """FSE table description: 4 bits of accuracy log - 5, then the counts
    (value count + 1, with the short code for small values, and 2-bit
    zero-run repeat flags after each zero)."""
    w = BitW()
    w.put(al - 5, 4)
    remaining, threshold, nb = (1 << al) + 1, 1 << al, al + 1
    s, n = 0, len(norm)
    while remaining > 1 and s < n:
        c = norm[s]
        s += 1
        mx = 2 * threshold - 1 - remaining
        remaining -= abs(c)
        v = c + 1
        if v >= threshold:
            v += mx
        w.put(v, nb - 1 if v < mx else nb)
        if c == 0:
            z = 0
            while s + z < n and norm[s + z] == 0:
                z += 1
            s += z
            while z >= 3:
                w.put(3, 2)
                z -= 3
            w.put(z, 2)
        assert remaining >= 1, "counts exceed the table size"
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    return w.bytes()


def fse_table(al: int, norm):
    """Decoding table (symbol, number of bits, baseline per state), or None
    when the counts do not fill the table."""
    size = 1 << al
    if sum(abs(c) for c in norm) != size:
        return None
    high, sym = size - 1, [0] * size
    nxt = []
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
        nxt.append(1 if c == -1 else c)
    step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    if pos != 0:
        return None
    nb, base = [0] * size, [0] * size
    for u in range(size):
        ns = nxt[sym[u]]
        nxt[sym[u]] += 1
        nb[u] = al - (ns.bit_length() - 1)
        base[u] = (ns << nb[u]) - size
    return {"al": al, "sym": sym, "nb": nb, "base": base}


def rle_table(symbol: int):
    return {"al": 0, "sym": [symbol], "nb": [0], "base": [0]}


def fse_states(tab, symbols, last_max_bits: bool = False):
    """The state sequence that decodes to `symbols`: the last state is free,
    every earlier one is the unique state of its symbol whose range holds the
    next state."""
    by = {}
    for u, s in enumerate(tab["sym"]):
        by.setdefault(s, []).append(u)
    for s in symbols:
        assert s in by, "symbol %d is not in the table" % s
    last = by[symbols[-1]]
    st = [max(last, key=lambda u: tab["nb"][u]) if last_max_bits else last[0]]
    for s in reversed(symbols[:-1]):
        t = st[-1]
        st.append(next(u for u in by[s] if tab["base"][u] <= t < tab["base"][u] + (1 << tab["nb"][u])))
    st.reverse()
    return st


# ----------------------------------------------------------------- Huffman
def huf_weights(nbits: dict):
    """Weights for symbols 0 .. highest - 1 from {symbol: code length}; the
    highest symbol's weight is implied."""
    mb = max(nbits.values())
    hi = max(nbits)
    return [mb + 1 - nbits[s] if s in nbits else 0 for s in range(hi)]


def huf_full(weights):
    """(all weights incl. the implied last one, depth), or None when a decoder
    must reject them (libzstd HUF_readStats rules)."""
    if any(w >= 12 for w in weights):
        return None
    total = sum(1 << (w - 1) for w in weights if w)
    if total == 0:
        return None
    mb = total.bit_length()
    if mb > 12:
        return None
    rest = (1 << mb) - total
    if rest & (rest - 1):
        return None
    full = list(weights) + [rest.bit_length()]
    r1 = sum(1 for w in full if w == 1)
    if r1 < 2 or r1 & 1:
        return None
    return full, mb


def huf_codes(full, mb):
    """{symbol: (code, length)}: cells by ascending weight, then symbol."""
    codes, acc = {}, 0
    for k in range(1, mb + 1):
        for s, w in enumerate(full):
            if w == k:
                codes[s] = (acc >> (k - 1), mb + 1 - k)
                acc += 1 << (k - 1)
    return codes


def huf_stream(codes, data: bytes) -> bytes:
    return backward([codes[b] for b in data])


def weights_norm(weights, al: int):
    """Normalized counts (sum 2^al) for the weight alphabet of `weights`."""
    hist = [0] * (max(weights) + 1)
    for w in weights:
        hist[w] += 1
    size, n = 1 << al, len(weights)
    norm = [max(1, h * size // n) if h else 0 for h in hist]
    big = max(range(len(norm)), key=lambda i: norm[i])
    norm[big] += size - sum(norm)
    assert norm[big] >= 1
    return norm


def huf_header(weights, wmode) -> bytes:
    """Huffman tree description: direct 4-bit weights (header byte 127 + n) or
    FSE-compressed weights (header byte = compressed size, two interleaved
    states, the stream ends by running out of bits)."""
    n = len(weights)
    if wmode == "direct":
        assert 1 <= n <= 128
        w = list(weights) + [0]
        return bytes([127 + n]) + bytes((w[i] << 4) | w[i + 1] for i in range(0, n, 2))
    al = wmode[1]
    norm = wmode[2] if len(wmode) > 2 else weights_norm(weights, al)
    tab = fse_table(al, norm)
    assert tab and n >= 2
    ev, od = list(weights[0::2]), list(weights[1::2])
    # the chain holding weight n-2 must end in a state that reads >= 1 bit
    se = fse_states(tab, ev, last_max_bits=(n - 2) % 2 == 0)
    so = fse_states(tab, od, last_max_bits=(n - 2) % 2 == 1)
    st = [se[i // 2] if i % 2 == 0 else so[i // 2] for i in range(n)]
    assert tab["nb"][st[n - 2]] >= 1
    reads = [(st[0], al), (st[1], al)]
    for i in range(n - 2):
        reads.append((st[i + 2] - tab["base"][st[i]], tab["nb"][st[i]]))
    body = write_ncount(al, norm) + backward(reads)
    assert len(body) < 128
    return bytes([len(body)]) + body


# ------------------------------------------------------------ frame state
class _State:
    """What a frame carries from block to block."""

    def __init__(self):
        self.huf = None  # {symbol: (code, length)} of the last Huffman block
        self.tab = {"ll": None, "of": None, "ml": None}
        self.tab_ok = {"ll": False, "of": False, "ml": False}
        self.rep = [1, 4, 8]


def _le(v: int, n: int) -> bytes:
    return v.to_bytes(n, "little")


def _lit_data(lit) -> bytes:
    d = lit["data"]
    return bytes([d[0]]) * d[1] if isinstance(d, tuple) else bytes(d)


def _literals(lit, st: _State):
    """-> (section bytes, literal bytes, ok)"""
    t, data = lit["type"], _lit_data(lit)
    regen = lit.get("regen", len(data))
    ok = "regen" not in lit and regen <= BLOCK_MAX
    if t in ("raw", "rle"):
        sf = lit.get("sf", 0 if regen < 32 else 1 if regen < 4096 else 3)
        tb = 0 if t == "raw" else 1
        if sf in (0, 2):  # one format bit (0); bit 3 is the low bit of the size: 00 when even, 10 when odd
            assert regen < 32
            hdr = bytes([tb | regen << 3])
        elif sf == 1:
            assert regen < 4096
            hdr = _le(tb | sf << 2 | regen << 4, 2)
        else:
            assert regen < (1 << 20)
            hdr = _le(tb | sf << 2 | regen << 4, 3)
        body = data if t == "raw" else bytes([lit["data"][0]])
        return hdr + body, data, ok
    assert t in ("huf", "treeless")
    streams = lit.get("streams", 1 if regen < 1024 and lit.get("sf", 0) == 0 else 4)
    tree = b""
    if t == "huf":
        weights = lit["weights"]
        hf = huf_full(weights)
        tree = huf_header(weights, lit.get("wmode", "direct"))
        if hf is None:
            ok = False
            # still writable: code the data with the valid weights `encode_as`
            hf = huf_full(lit["encode_as"])
        st.huf = huf_codes(*hf) if ok else None
        codes = huf_codes(*hf)
    else:
        codes = st.huf
        if codes is None:
            ok = False
            codes = huf_codes(*huf_full(lit["encode_as"]))
    if any(b not in codes for b in data):
        raise AssertionError("literal byte without a Huffman code")
    if streams == 1:
        body = lit.get("stream_bytes", huf_stream(codes, data))
    else:
        seg = (regen + 3) // 4
        parts = [huf_stream(codes, data[i * seg:(i + 1) * seg]) for i in range(4)]
        jump = lit.get("jump", [len(p) for p in parts[:3]])
        body = b"".join(_le(j, 2) for j in jump) + b"".join(parts)
    if any(k in lit for k in ("stream_bytes", "jump")):
        ok = False
    csize = len(tree) + len(body)
    sf = lit.get("sf", 0 if streams == 1 else 1 if regen < 1024 and csize < 1024 else 2 if regen < 16384 and
                 csize < 16384 else 3)
    assert (sf == 0) == (streams == 1)
    bits = {0: 10, 1: 10, 2: 14, 3: 18}[sf]
    assert regen < (1 << bits) and csize < (1 << bits), (regen, csize, sf)
    tb = 2 if t == "huf" else 3
    hdr = _le(tb | sf << 2 | regen << 4 | csize << (4 + bits), {10: 3, 14: 4, 18: 5}[bits])
    return hdr + tree + body, data, ok


def _code_of(v: int, base, bits):
    c = max(i for i in range(len(base)) if base[i] <= v)
    assert v - base[c] < (1 << bits[c]), v
    return c, v - base[c], bits[c]


def seq_codes(s):
    """One sequence, (ll, ml, Offset_Value) or a dict with explicit codes and
    extra bits -> (llc, llx, llb, mlc, mlx, mlb, ofc, ofx, ll, ml, ofv); a
    code past the alphabet has no extra bits and no value."""
    if not isinstance(s, dict):
        s = {"ll": s[0], "ml": s[1], "ofv": s[2]}
    if "llc" in s:
        llc, llx = s["llc"], s.get("llx", 0)
        llb = LL_BITS[llc] if llc < 36 else 0
        ll = LL_BASE[llc] + llx if llc < 36 else None
    else:
        llc, llx, llb = _code_of(s["ll"], LL_BASE, LL_BITS)
        ll = s["ll"]
    if "mlc" in s:
        mlc, mlx = s["mlc"], s.get("mlx", 0)
        mlb = ML_BITS[mlc] if mlc < 53 else 0
        ml = ML_BASE[mlc] + mlx if mlc < 53 else None
    else:
        mlc, mlx, mlb = _code_of(s["ml"], ML_BASE, ML_BITS)
        ml = s["ml"]
    if "ofc" in s:
        ofc, ofx = s["ofc"], s.get("ofx", 0)
    else:
        ofc = s["ofv"].bit_length() - 1
        ofx = s["ofv"] - (1 << ofc)
    ofv = (1 << ofc) + ofx if ofc < 32 else None
    return llc, llx, llb, mlc, mlx, mlb, ofc, ofx, ll, ml, ofv


def _table_for(field: str, mode, st: _State):
    """-> (mode bits, description bytes, table to code with, decoder accepts)"""
    dflt, dal, maxsym, maxal = FIELD[field]
    if mode == "pre":
        tab, ok, bits, desc = fse_table(dal, dflt), True, 0, b""
    elif mode[0] == "rle":
        tab, ok, bits, desc = rle_table(mode[1]), mode[1] <= maxsym, 1, bytes([mode[1]])
    elif mode[0] == "fse":
        al, norm = mode[1], mode[2]
        tab = fse_table(al, norm)
        assert tab is not None, "counts do not fill the table"
        ok = al <= maxal and len(norm) <= maxsym + 1
        bits, desc = 2, write_ncount(al, norm)
    else:
        assert mode == "rep"
        tab, ok, bits, desc = st.tab[field], st.tab_ok[field], 3, b""
        if tab is None:  # nothing to repeat: the frame is corrupt, code with the predefined table
            return bits, desc, fse_table(dal, dflt), False
        return bits, desc, tab, ok
    st.tab[field], st.tab_ok[field] = tab, ok
    return bits, desc, tab, ok


def _sequences(sec, st: _State):
    """-> (section bytes, [coded sequences], ok)"""
    seqs = [seq_codes(s) for s in sec.get("seqs", [])]
    n = sec.get("nbseq", len(seqs))
    form = sec.get("nbseq_form", 1 if n < 128 else 2 if n < 0x7F00 else 3)
    if form == 1:
        assert n < 128
        out = bytes([n])
    elif form == 2:
        assert n < 0x7F00
        out = bytes([128 + (n >> 8), n & 255])
    else:
        assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
        out = b"\xff" + _le(n - 0x7F00, 2)
    ok = n == len(seqs)
    if not seqs:
        if "tail" in sec:
            out, ok = out + sec["tail"], ok and not sec["tail"]
        return out, seqs, ok
    tabs, mbyte = {}, sec.get("reserved_modes", 0)
    ok = ok and mbyte == 0
    for field, sh in (("ll", 6), ("of", 4), ("ml", 2)):
        bits, desc, tab, tok = _table_for(field, sec.get(field, "pre"), st)
        mbyte |= bits << sh
        tabs[field] = (desc, tab)
        ok = ok and tok
    out += bytes([mbyte]) + tabs["ll"][0] + tabs["of"][0] + tabs["ml"][0]
    tl, to, tm = tabs["ll"][1], tabs["of"][1], tabs["ml"][1]
    sl = fse_states(tl, [q[0] for q in seqs])
    so = fse_states(to, [q[6] for q in seqs])
    sm = fse_states(tm, [q[3] for q in seqs])
    reads = [(sl[0], tl["al"]), (so[0], to["al"]), (sm[0], tm["al"])]
    for i, q in enumerate(seqs):
        reads += [(q[7], q[6] if q[6] < 32 else 0), (q[4], q[5]), (q[1], q[2])]
        if i + 1 < len(seqs):
            reads += [(sl[i + 1] - tl["base"][sl[i]], tl["nb"][sl[i]]), (sm[i + 1] - tm["base"][sm[i]], tm["nb"][sm[i]]),
                      (so[i + 1] - to["base"][so[i]], to["nb"][so[i]])]
    stream = backward(reads, sec.get("spare_bits", 0), sec.get("drop_bits", 0))
    if "want_stream_len" in sec:
        assert len(stream) == sec["want_stream_len"], len(stream)
    if "want_pad_pos" in sec:
        assert stream[-1].bit_length() - 1 == sec["want_pad_pos"], stream[-1]
    if "last_byte" in sec:
        stream = stream[:-1] + bytes([sec["last_byte"]])
    if any(k in sec for k in ("spare_bits", "drop_bits", "last_byte", "tail")):
        ok = False
    return out + sec.get("tail", stream), seqs, ok


def _run(out: bytearray, base: int, lits: bytes, seqs, rep):
    """Replay one compressed block; False when it is corrupt."""
    lp = 0
    for (llc, _, _, mlc, _, _, ofc, _, ll, ml, ofv) in seqs:
        if llc > 35 or mlc > 52 or ofc > 31:
            return False
        if ofv > 3:
            off = ofv - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            k = ofv - 1 + (1 if ll == 0 else 0)
            if k == 0:
                off = rep[0]
            else:
                off = rep[0] - 1 if k == 3 else rep[k]
                off = off or 1
                if k == 1:
                    rep[:] = [off, rep[0], rep[2]]
                else:
                    rep[:] = [off, rep[0], rep[1]]
        if lp + ll > len(lits):
            return False
        out += lits[lp:lp + ll]
        lp += ll
        if off > len(out) - base:
            return False
        if off >= ml:
            start = len(out) - off
            out += out[start:start + ml]
        else:
            pat = bytes(out[-off:])
            out += (pat * (ml // off + 1))[:ml]
    out += lits[lp:]
    return True


def _frame(fr, out: bytearray):
    """-> (frame bytes, ok); appends the frame's content to `out` while ok."""
    st = _State()
    base = len(out)
    ok = True
    body = bytearray()
    blocks = fr["blocks"]
    for i, b in enumerate(blocks):
        t = b["type"]
        last = b.get("last", i == len(blocks) - 1)
        if last != (i == len(blocks) - 1):
            ok = False
        if t == "raw":
            data = bytes(b["data"])
            size, payload = len(data), data
            if ok:
                out += data
        elif t == "rle":
            size, payload = b["n"], bytes([b["byte"]])
            if ok:
                out += payload * size
        else:
            assert t in ("comp", 3)
            lsec, lits, lok = _literals(b["lit"], st)
            ssec, seqs, sok = _sequences(b.get("seq", {}), st)
            payload = lsec + ssec
            ok = ok and lok and sok and 3 <= len(payload) < BLOCK_MAX and t != 3  # libzstd: MIN_CBLOCK_SIZE 3
            if ok:
                ok = _run(out, base, lits, seqs, st.rep)
            size = len(payload)
            if t == 3:
                ok = False
        if "size" in b:
            size, ok = b["size"], False
        bt = {"raw": 0, "rle": 1, "comp": 2, 3: 3}[t]
        body += _le((1 if last else 0) | bt << 1 | size << 3, 3) + payload
    content = len(out) - base
    single = fr.get("single", False)
    fcs_size = fr.get("fcs_size", 0)
    assert fcs_size in (0, 1, 2, 4, 8) and (fcs_size != 1 or single) and (fcs_size != 0 or not single)
    did_size = fr.get("did_size", 0)
    check = fr.get("checksum")
    fhd = ({0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_size] << 6 | (1 if single else 0) << 5 | fr.get("unused", 0) << 4 |
           fr.get("reserved", 0) << 3 | (1 if check else 0) << 2 | {0: 0, 1: 1, 2: 2, 4: 3}[did_size])
    hdr = _le(fr.get("magic", MAGIC), 4) + bytes([fhd])
    if fr.get("magic", MAGIC) != MAGIC or fr.get("reserved", 0):
        ok = False
    if not single:
        wlog = fr.get("wlog", 17)
        hdr += bytes([(wlog - 10) << 3 | fr.get("wmant", 0)])
        if wlog > 31:
            ok = False
    hdr += _le(fr.get("did", 0), did_size)
    if fr.get("did", 0):
        ok = False
    if fcs_size:
        fcs = fr.get("fcs", content)
        if fcs != content:
            ok = False
        hdr += _le(fcs - 256 if fcs_size == 2 else fcs, fcs_size)
    tail = b""
    if check:
        h = xxh64(bytes(out[base:])) & 0xFFFFFFFF if ok else 0
        if check == "bad":
            h ^= 0x00010000
        tail = _le(h, 4)
        if check == "cut":
            tail = tail[:fr.get("cut_to", 2)]
        if check != "ok":
            ok = False
    return hdr + bytes(body) + tail, ok


def _build(desc):
    out, src, ok = bytearray(), bytearray(), True
    for part in desc:
        if part["kind"] == "frame":
            b, fok = _frame(part, out)
            ok = ok and fok
        elif part["kind"] == "skip":
            data = bytes(part.get("data", b""))
            b = _le(0x184D2A50 + part.get("nibble", 0), 4) + _le(part.get("size", len(data)), 4) + data
            if "size" in part and part["size"] != len(data):
                ok = False
        else:
            assert part["kind"] == "bytes"  # stray bytes between or after frames
            b, ok = bytes(part["data"]), False
        src += b
    return bytes(src), (bytes(out) if ok else None)


def write(desc) -> bytes:
    """The bytes of a description: a list of frames, skippable frames and stray bytes."""
    return _build(desc)[0]


def expand(desc):
    """What a correct decoder produces for a description, or None if corrupt."""
    return _build(desc)[1]


# ------------------------------------------------------------ constructors
def frame(blocks, **kw):
    return dict(kind="frame", blocks=blocks, **kw)


def skip(data=b"", **kw):
    return dict(kind="skip", data=data, **kw)


def stray(data):
    return dict(kind="bytes", data=data)


def raw(data, **kw):
    return dict(type="raw", data=data, **kw)


def rle(byte, n, **kw):
    return dict(type="rle", byte=byte, n=n, **kw)


def comp(lit, seqs=None, **kw):
    seq = dict(kw.pop("seq", {}))
    if seqs is not None:
        seq["seqs"] = seqs
    return dict(type=kw.pop("type", "comp"), lit=lit, seq=seq, **kw)


def lit_raw(data, **kw):
    return dict(type="raw", data=data, **kw)


def lit_rle(byte, n, **kw):
    return dict(type="rle", data=(byte, n), **kw)


def lit_huf(data, weights, **kw):
    return dict(type="huf", data=data, weights=weights, **kw)


def lit_treeless(data, **kw):
    return dict(type="treeless", data=data, **kw)
