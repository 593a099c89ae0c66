// The seek table of a seekable Zstd object (the Zstandard
// seekable format): one skippable frame behind the object's frames,
//     u32 0x184D2A5E | u32 E nf + 9 | nf x (u32 compressed, u32 decompressed[, u32 checksum])
//     | u32 nf | u8 descriptor | u32 0x8F92EAB1
// all little-endian.  Descriptor 0x00: entries of E = 8 bytes; 0x80: entries of
// 12 bytes whose third word is the low 32 bits of XXH64 (seed 0) of the frame's
// content.  Everything here takes the byte fetch as a parameter (lz4_walkstep.h
// is the model), so the kernels of zstd_seek.hip and the CPU programs under
// tests/ run the same checks and the same placement.  Nothing outside the
// region handed in is ever fetched, and anything that is not a valid table is
// "no table", never an error.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JFS_ZSEEK_HD __host__ __device__ __forceinline__
#else
#define JFS_ZSEEK_HD inline
#endif

namespace jfs {
namespace zseek {

constexpr uint32_t SKIP_MAGIC = 0x184D2A5Eu;
constexpr uint32_t SEEK_MAGIC = 0x8F92EAB1u;
constexpr int32_t FRAME_BYTES = 128 << 10;  // content of one frame of the seekable encoder
constexpr int32_t TABLE_FIXED = 17;         // skippable header 8 + footer 9
constexpr int32_t FOOTER = 9;
constexpr int32_t ENTRY = 8;
constexpr int32_t ENTRY_CSUM = 12;
constexpr uint32_t DESC_CSUM = 0x80u;
// The most frames a table may list: what the encoder writes for its largest
// input (0x7FFFFF00 bytes).  The table comes from stored data, so the cap bounds
// what one stored object can ask of a decode: a scan of 256 rounds, a Rounds
// record of 5 KiB and 16,384 entries of the expanded list.  A table of hundreds
// of thousands of one-byte frames is "no table", and the object is decoded as
// any other.
constexpr int32_t MAX_FRAMES = 16384;

// bytes of the 8-byte-entry table of an object of nf frames
JFS_ZSEEK_HD int64_t table_bytes(int64_t nf) { return ENTRY * nf + TABLE_FIXED; }

template <class F>
JFS_ZSEEK_HD uint32_t le32(F fetch, int32_t p) {
    return (uint32_t)fetch(p) | ((uint32_t)fetch(p + 1) << 8) | ((uint32_t)fetch(p + 2) << 16) |
           ((uint32_t)fetch(p + 3) << 24);
}

// The footer alone, the 9 bytes [end - 9, end) (end >= 9 is the caller's): the
// frame count and the entry size, or false.  csum: descriptor 0x80 is accepted.
template <class F>
JFS_ZSEEK_HD bool footer_peek(F fetch, int32_t end, bool csum, int32_t *nf, int32_t *entry) {
    if (le32(fetch, end - 4) != SEEK_MAGIC) return false;
    const uint32_t desc = fetch(end - 5);
    if (desc != 0u && !(csum && desc == DESC_CSUM)) return false;  // reserved bits: not ours
    const uint32_t n = le32(fetch, end - FOOTER);
    if (n < 1u || n > (uint32_t)MAX_FRAMES) return false;
    *nf = (int32_t)n;
    *entry = desc ? ENTRY_CSUM : ENTRY;
    return true;
}

// The table at the end of the region [0, end): the frame count, where the table
// starts and the entry size, or false.  alone: the region is the table's own
// bytes, so it starts at 0 (a stand-alone table); otherwise the
// region is a whole object and tpos is the bytes its frames must take.  What
// the entries must add up to is seek_sums_ok's.
template <class F>
JFS_ZSEEK_HD bool seek_table(F fetch, int64_t end, bool csum, bool alone, int32_t *nf, int32_t *tpos, int32_t *entry) {
    if (end < TABLE_FIXED + ENTRY || end > 0x7FFFFFFFll) return false;
    int32_t n = 0, ent = 0;
    if (!footer_peek(fetch, (int32_t)end, csum, &n, &ent)) return false;
    const int32_t t = (int32_t)end - (ent * n + TABLE_FIXED);
    if (alone ? t != 0 : t < 0) return false;
    if (le32(fetch, t) != SKIP_MAGIC) return false;
    if (le32(fetch, t + 4) != (uint32_t)(ent * n + 9)) return false;
    *nf = n;
    *tpos = t;
    *entry = ent;
    return true;
}

// The bytes T of the table at the end of the region [0, len), either layout, by
// its placement alone -- the footer, and the skippable header where the footer
// says the table starts; 17 bytes are fetched -- or 0.  What the kernel of
// zstd_seek_tables.hip checks before it copies a table out; the
// copy then goes through seek_table and seek_sums_ok like any object.
template <class F>
JFS_ZSEEK_HD int32_t table_at_end(F fetch, int64_t len) {
    int32_t nf = 0, tpos = 0, entry = 0;
    return seek_table(fetch, len, true, false, &nf, &tpos, &entry) ? (int32_t)len - tpos : 0;
}

// entry k of the table at tpos whose entries take `entry` bytes: compressed
// size, decompressed size, checksum (0 without one)
template <class F>
JFS_ZSEEK_HD void seek_entry(F fetch, int32_t tpos, int32_t entry, int32_t k, uint32_t *c, uint32_t *d, uint32_t *x) {
    *c = le32(fetch, tpos + 8 + entry * k);
    *d = le32(fetch, tpos + 12 + entry * k);
    *x = entry == ENTRY_CSUM ? le32(fetch, tpos + 16 + entry * k) : 0u;
}

// the entries' totals: every frame has bytes (zeros = the number of entries
// with none), the frames end where the table starts, the content fits 32 bits
JFS_ZSEEK_HD bool seek_sums_ok(uint64_t csum, uint64_t dsum, uint32_t zeros, int32_t tpos) {
    return zeros == 0u && csum == (uint64_t)(uint32_t)tpos && dsum <= 0xFFFFFFFFull;
}

// the range asked of an object: lo' = max(lo, 0), hi' = min(hi, dst_cap)
JFS_ZSEEK_HD int32_t range_lo(int32_t lo) { return lo > 0 ? lo : 0; }
JFS_ZSEEK_HD int32_t range_hi(int32_t hi, int32_t dst_cap) { return hi < dst_cap ? hi : dst_cap; }

// Frame k, whose content is [d0, d0 + d) of the object: it comes before the
// range, meets it, or comes behind it.  A frame without content meets nothing.
JFS_ZSEEK_HD bool frame_before(uint64_t d0, uint32_t d, int32_t lo) { return d0 + d <= (uint64_t)(uint32_t)lo; }
JFS_ZSEEK_HD bool frame_from(uint64_t d0, int32_t hi) { return d0 >= (uint64_t)(uint32_t)hi; }
// The frames in front of the range are a prefix of the table and those behind
// it a suffix, so the rest is one run -- frames without content inside it included.
JFS_ZSEEK_HD bool frame_in_run(uint64_t d0, uint32_t d, int32_t lo, int32_t hi) {
    return !frame_before(d0, d, lo) && !frame_from(d0, hi);
}

struct Sel {
    int32_t table;    // 1: a valid table
    int32_t nf;       // its frames
    uint32_t total;   // D, the content of all frames
    int32_t first;    // first selected frame
    int32_t count;    // selected frames (they are consecutive); 0: the range meets none
    uint32_t coff;    // compressed offset of frame `first`
    uint32_t doff;    // content offset of frame `first`
};

// The whole answer for one object, serially.  lo < hi after the clamps is the
// caller's to check; an empty range selects nothing.  With D > dst_cap the
// selection is computed all the same: the caller answers -2 first.
template <class F>
JFS_ZSEEK_HD Sel seek_select(F fetch, int32_t src_len, int32_t dst_cap, int32_t lo, int32_t hi) {
    Sel s;
    s.table = 0; s.nf = 0; s.total = 0; s.first = 0; s.count = 0; s.coff = 0; s.doff = 0;
    int32_t nf = 0, tpos = 0, entry = 0;
    if (!seek_table(fetch, src_len, false, false, &nf, &tpos, &entry)) return s;
    const int32_t l = range_lo(lo), h = range_hi(hi, dst_cap);
    uint64_t cs = 0, ds = 0;
    uint32_t zeros = 0;
    int32_t before = 0, count = 0;
    uint64_t coff = 0, doff = 0;
    for (int32_t k = 0; k < nf; k++) {
        uint32_t c, d, x;
        seek_entry(fetch, tpos, entry, k, &c, &d, &x);
        zeros += c == 0u;
        if (frame_before(ds, d, l)) {
            before = k + 1;
            coff = cs + c;
            doff = ds + d;
        } else if (!frame_from(ds, h)) {
            count = k + 1 - before;
        }
        cs += c;
        ds += d;
    }
    if (!seek_sums_ok(cs, ds, zeros, tpos)) return s;
    s.table = 1;
    s.nf = nf;
    s.total = (uint32_t)ds;
    if (h > l && count > 0) {
        s.first = before;
        s.count = count;
        s.coff = (uint32_t)coff;
        s.doff = (uint32_t)doff;
    }
    return s;
}

// ---- a table that stands alone, with or without checksums ------
// The table's own bytes, [0, table_len) from the skippable magic through the
// footer, of an object of object_len bytes whose frames it follows, in either
// layout: seek_table with alone = true.  Every condition above holds here too;
// nothing outside [0, table_len) is fetched.
template <class F>
JFS_ZSEEK_HD bool table_header(F fetch, int64_t table_len, int64_t object_len, int32_t *nf, int32_t *entry) {
    int32_t tpos = 0;
    return table_len <= object_len && object_len <= 0x7FFFFFFFll && seek_table(fetch, table_len, true, true, nf, &tpos, entry);
}
// entry k of such a table: seek_entry at position 0
template <class F>
JFS_ZSEEK_HD void table_entry(F fetch, int32_t entry, int32_t k, uint32_t *c, uint32_t *d, uint32_t *x) {
    seek_entry(fetch, 0, entry, k, c, d, x);
}

struct TableSel {
    int32_t table;      // 1: a valid table
    int32_t checksums;  // 1: entries of 12 bytes
    int32_t nf;
    int32_t first, count;  // the selected frames; count 0: the range meets none
    uint64_t total;        // D
    uint64_t coff, cend;   // the selected frames' bytes in the object
    uint64_t doff, dend;   // and their content
};

// The whole answer for one stand-alone table, serially: seek_select's rule with
// lo' = max(lo, 0) and hi' = min(hi, cap), where cap < 0 stands for D.
template <class F>
JFS_ZSEEK_HD TableSel table_select(F fetch, int64_t table_len, int64_t object_len, int64_t cap, int64_t lo, int64_t hi) {
    TableSel s;
    s.table = 0; s.checksums = 0; s.nf = 0; s.first = 0; s.count = 0;
    s.total = 0; s.coff = 0; s.cend = 0; s.doff = 0; s.dend = 0;
    int32_t nf = 0, entry = 0;
    if (!table_header(fetch, table_len, object_len, &nf, &entry)) return s;
    uint64_t cs = 0, ds = 0;
    uint32_t zeros = 0;
    for (int32_t k = 0; k < nf; k++) {
        uint32_t c, d, x;
        seek_entry(fetch, 0, entry, k, &c, &d, &x);
        zeros += c == 0u;
        cs += c;
        ds += d;
    }
    if (zeros != 0u || cs != (uint64_t)(object_len - table_len) || ds > 0xFFFFFFFFull) return s;
    s.table = 1;
    s.checksums = entry == ENTRY_CSUM;
    s.nf = nf;
    s.total = ds;
    const uint64_t l = lo > 0 ? (uint64_t)lo : 0u;
    const int64_t top = cap < 0 ? (int64_t)ds : cap;
    const int64_t h = hi < top ? hi : top;
    if (h <= 0 || (uint64_t)h <= l) return s;
    uint64_t c0 = 0, d0 = 0;
    int32_t first = 0, count = 0;
    for (int32_t k = 0; k < nf; k++) {
        uint32_t c, d, x;
        seek_entry(fetch, 0, entry, k, &c, &d, &x);
        if (d0 + d <= l) {  // in front of the range
            first = k + 1;
            s.coff = c0 + c;
            s.doff = d0 + d;
        } else if (d0 < (uint64_t)h) {
            count = k + 1 - first;
            s.cend = c0 + c;
            s.dend = d0 + d;
        }
        c0 += c;
        d0 += d;
    }
    if (count > 0) {
        s.first = first;
        s.count = count;
    } else {
        s.coff = s.cend = s.doff = s.dend = 0;
    }
    return s;
}

// ---- several ranges of one object, either layout ---------------
// The table at the end of a whole object in either layout (seek_table with
// csum = true), and a list of ranges in place of one range.

// A list of ranges (any type with int32 lo, hi) is ascending and disjoint as
// given: lo <= hi for every range and hi <= the next one's lo.  Empty ranges
// may stand anywhere.  range_follows is the check of one range against the one
// in front of it (prev = null for the first).
template <class R>
JFS_ZSEEK_HD bool range_follows(const R *prev, const R &cur) {
    return cur.lo <= cur.hi && (prev == nullptr || prev->hi <= cur.lo);
}
template <class R>
JFS_ZSEEK_HD bool ranges_ok(const R *rng, int32_t nr) {
    for (int32_t r = 0; r < nr; r++)
        if (!range_follows(r > 0 ? &rng[r - 1] : (const R *)nullptr, rng[r])) return false;
    return true;
}

// a range is live when something of it is left after the clamps
template <class R>
JFS_ZSEEK_HD bool range_live(const R &r, int32_t dst_cap) { return range_hi(r.hi, dst_cap) > range_lo(r.lo); }

// Frame k, content [d0, d0 + d): selected iff d > 0 and some live range has
// lo' < d0 + d and hi' > d0.  The clamps keep the list's order, so hi' does not
// fall along it: a binary search finds the first range with hi' > d0, and the
// ranges from there on are tried while they start inside the frame (only
// ranges that are not live are passed over).
template <class R>
JFS_ZSEEK_HD bool frame_in_ranges(const R *rng, int32_t nr, int32_t dst_cap, uint64_t d0, uint32_t d) {
    if (d == 0u) return false;
    int32_t a = 0, z = nr;
    while (a < z) {
        const int32_t m = a + ((z - a) >> 1);
        if ((int64_t)range_hi(rng[m].hi, dst_cap) > (int64_t)d0) z = m;
        else a = m + 1;
    }
    const int64_t end = (int64_t)d0 + d;
    for (; a < nr && (int64_t)range_lo(rng[a].lo) < end; a++)
        if (range_live(rng[a], dst_cap)) return true;
    return false;
}

struct RangesSel {
    int32_t bad;        // 1: the list is not ascending and disjoint (nothing else is filled)
    int32_t live;       // its live ranges
    int32_t top;        // H, the largest hi' of the live ranges (0 without one)
    int32_t table;      // 1: a valid table of either layout
    int32_t checksums;  // 1: entries of 12 bytes
    int32_t nf;
    uint32_t total;     // D
    int32_t count;      // selected frames
};

// The whole answer for one object and its list, serially: the rule the sparse
// scan kernel (zstd_seek.hip) applies 64 frames a round.  emit(k, coff, doff, c,
// d, x) is called for every selected frame in ascending order: its number, where
// it starts (compressed, content) and its entry.  With D > dst_cap the selection
// is computed all the same: the caller answers -2 first.
template <class F, class R, class E>
JFS_ZSEEK_HD RangesSel ranges_select(F fetch, int32_t src_len, int32_t dst_cap, const R *rng, int32_t nr, E emit) {
    RangesSel s;
    s.bad = 0; s.live = 0; s.top = 0; s.table = 0; s.checksums = 0; s.nf = 0; s.total = 0; s.count = 0;
    if (!ranges_ok(rng, nr)) {
        s.bad = 1;
        return s;
    }
    for (int32_t r = 0; r < nr; r++)
        if (range_live(rng[r], dst_cap)) {
            s.live++;
            const int32_t h = range_hi(rng[r].hi, dst_cap);
            s.top = h > s.top ? h : s.top;
        }
    int32_t nf = 0, tpos = 0, entry = 0;
    if (!seek_table(fetch, src_len, true, false, &nf, &tpos, &entry)) return s;
    uint64_t cs = 0, ds = 0;
    uint32_t zeros = 0;
    for (int32_t k = 0; k < nf; k++) {
        uint32_t c, d, x;
        seek_entry(fetch, tpos, entry, k, &c, &d, &x);
        zeros += c == 0u;
        cs += c;
        ds += d;
    }
    if (!seek_sums_ok(cs, ds, zeros, tpos)) return s;
    s.table = 1;
    s.checksums = entry == ENTRY_CSUM;
    s.nf = nf;
    s.total = (uint32_t)ds;
    if (s.live == 0) return s;
    cs = ds = 0;
    for (int32_t k = 0; k < nf; k++) {
        uint32_t c, d, x;
        seek_entry(fetch, tpos, entry, k, &c, &d, &x);
        if (frame_in_ranges(rng, nr, dst_cap, ds, d)) {
            emit(k, (uint32_t)cs, (uint32_t)ds, c, d, x);
            s.count++;
        }
        cs += c;
        ds += d;
    }
    return s;
}

// ---- placement: where the j-th selected frame lies ----------------------------
// What a scan leaves per input for the expansion, whatever selected the frames:
// per round of 64 entries its selection word and what lies in front of it.
constexpr int32_t ROUNDS = MAX_FRAMES / 64;
struct Rounds {
    uint64_t word[ROUNDS];   // the round's selected frames, bit = lane
    uint32_t coff[ROUNDS];   // compressed bytes in front of the round
    uint32_t doff[ROUNDS];   // content in front of it
    int32_t before[ROUNDS];  // selected frames in front of it
};

// The j-th selected frame of a table of nf frames: its number k and where it
// starts, compressed and content.  Its round by binary search over the rounds'
// counts, k the (j - before)-th set bit of the round's word, the offsets the
// round's plus at most 63 entries.  False when fewer than j + 1 are selected.
template <class F>
JFS_ZSEEK_HD bool place_frame(F fetch, int32_t tpos, int32_t entry, int32_t nf, const Rounds &R, int32_t j, int32_t *k,
                              uint32_t *coff, uint32_t *doff) {
    int32_t r = 0, rz = ((nf + 63) >> 6) - 1;  // the last round with before <= j: the one that holds entry j
    while (r < rz) {
        const int32_t m = (r + rz + 1) >> 1;
        if (R.before[m] <= j) r = m;
        else rz = m - 1;
    }
    uint64_t w = R.word[r];
    for (int32_t t = j - R.before[r]; t > 0; t--) w &= w - 1;
    if (j < 0 || w == 0ull) return false;
    const int32_t b = __builtin_ctzll(w);
    uint32_t co = R.coff[r], dn = R.doff[r], c = 0, d = 0, x = 0;
    for (int32_t q = r * 64; q < r * 64 + b; q++) {
        seek_entry(fetch, tpos, entry, q, &c, &d, &x);
        co += c;
        dn += d;
    }
    *k = r * 64 + b;
    *coff = co;
    *doff = dn;
    return true;
}

// The record a scan must leave, serially: selects(k, d0, d) says whether frame k,
// content [d0, d0 + d), is selected.  Returns the number selected.
template <class F, class S>
JFS_ZSEEK_HD int32_t rounds_build(F fetch, int32_t tpos, int32_t entry, int32_t nf, S selects, Rounds *R) {
    uint64_t cs = 0, ds = 0;
    int32_t cnt = 0;
    for (int32_t k = 0; k < nf; k++) {
        if ((k & 63) == 0) {
            R->word[k >> 6] = 0ull;
            R->coff[k >> 6] = (uint32_t)cs;
            R->doff[k >> 6] = (uint32_t)ds;
            R->before[k >> 6] = cnt;
        }
        uint32_t c, d, x;
        seek_entry(fetch, tpos, entry, k, &c, &d, &x);
        if (selects(k, ds, d)) {
            R->word[k >> 6] |= 1ull << (k & 63);
            cnt++;
        }
        cs += c;
        ds += d;
    }
    return cnt;
}

}  // namespace zseek
}  // namespace jfs
