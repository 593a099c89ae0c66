// The seek table of a seekable Zstd object (the Zstandard seekable
// format): one skippable frame behind the object's frames,
//     u32 0x184D2A5E | u32 8 nf + 9 | nf x (u32 compressed, u32 decompressed)
//     | u32 nf | u8 descriptor | u32 0x8F92EAB1
// all little-endian.  The parser takes the byte fetch as a parameter
// (lz4_walkstep.h is the model), so the range decoder's scan kernel
// (zstd_seek.hip) and tests/zstd_seek_main.cc run the same checks.  It never
// fetches outside [0, src_len), and anything that is not a valid table --
// a table whose entries carry checksums included -- is "no table", never an
// error: such an object is decoded as any other Zstd object.
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
constexpr int32_t ENTRY = 8;
// The most frames a table may list: what the encoder writes for its largest
// input (0x7FFFFF00 bytes).  The table comes from stored data, and the range
// decoder's work per object grows with the square of the selected frames
// (zseek_expand walks on from the first one), so a table of hundreds of
// thousands of one-byte frames is "no table" and the object is decoded as any
// other: the walk is 16,384 entries at most.
constexpr int32_t MAX_FRAMES = 16384;

// bytes of the table of an object of nf frames
JFS_ZSEEK_HD int64_t table_bytes(int64_t nf) { return ENTRY * nf + TABLE_FIXED; }

template <class F>
JFS_ZSEEK_HD uint32_t le32(F fetch, int32_t p) {
    return (uint32_t)fetch(p) | ((uint32_t)fetch(p + 1) << 8) | ((uint32_t)fetch(p + 2) << 16) |
           ((uint32_t)fetch(p + 3) << 24);
}

// The footer and the skippable header: the frame count and where the table
// starts (= the bytes its frames must take), or false.  What the entries must
// add up to is seek_sums_ok's.
template <class F>
JFS_ZSEEK_HD bool seek_footer(F fetch, int32_t src_len, int32_t *nf, int32_t *tpos) {
    if (src_len < TABLE_FIXED + ENTRY) return false;
    if (le32(fetch, src_len - 4) != SEEK_MAGIC) return false;
    if (fetch(src_len - 5) != 0u) return false;  // checksum bit, reserved bits: not ours
    const uint32_t n = le32(fetch, src_len - 9);
    if (n < 1u || n > (uint32_t)MAX_FRAMES || (int64_t)n > ((int64_t)src_len - TABLE_FIXED) / ENTRY) return false;
    const int32_t t = src_len - (int32_t)table_bytes(n);
    if (le32(fetch, t) != SKIP_MAGIC) return false;
    if (le32(fetch, t + 4) != (uint32_t)(ENTRY * n + 9u)) return false;
    *nf = (int32_t)n;
    *tpos = t;
    return true;
}

// entry k of the table at tpos
template <class F>
JFS_ZSEEK_HD void seek_entry(F fetch, int32_t tpos, int32_t k, uint32_t *c, uint32_t *d) {
    *c = le32(fetch, tpos + 8 + ENTRY * k);
    *d = le32(fetch, tpos + 12 + ENTRY * k);
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
    int32_t nf = 0, tpos = 0;
    if (!seek_footer(fetch, src_len, &nf, &tpos)) return s;
    const int32_t l = range_lo(lo), h = range_hi(hi, dst_cap);
    uint64_t cs = 0, ds = 0;
    uint32_t zeros = 0;
    int32_t before = 0, count = 0;
    uint64_t coff = 0, doff = 0;
    for (int32_t k = 0; k < nf; k++) {
        uint32_t c, d;
        seek_entry(fetch, tpos, k, &c, &d);
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
// footer, of an object of object_len bytes whose frames it follows.  Descriptor
// 0x00: entries of 8 bytes as above; 0x80: entries of 12 bytes whose third word
// is the low 32 bits of XXH64 (seed 0) of the frame's content.  Every condition
// above holds here too; nothing outside [0, table_len) is fetched.
constexpr int32_t ENTRY_CSUM = 12;
constexpr uint32_t DESC_CSUM = 0x80u;

// the frame count and the entry size (8 or 12), or false
template <class F>
JFS_ZSEEK_HD bool table_header(F fetch, int64_t table_len, int64_t object_len, int32_t *nf, int32_t *entry) {
    if (table_len < TABLE_FIXED + ENTRY || table_len > object_len || object_len > 0x7FFFFFFFll) return false;
    const int32_t tl = (int32_t)table_len;
    if (le32(fetch, tl - 4) != SEEK_MAGIC) return false;
    const uint32_t desc = fetch(tl - 5);
    if (desc != 0u && desc != DESC_CSUM) return false;
    const int32_t ent = desc ? ENTRY_CSUM : ENTRY;
    const uint32_t n = le32(fetch, tl - 9);
    if (n < 1u || n > (uint32_t)MAX_FRAMES || (int64_t)ent * n + TABLE_FIXED != table_len) return false;
    if (le32(fetch, 0) != SKIP_MAGIC) return false;
    if (le32(fetch, 4) != (uint32_t)ent * n + 9u) return false;
    *nf = (int32_t)n;
    *entry = ent;
    return true;
}

// entry k: compressed size, decompressed size, checksum (0 without one)
template <class F>
JFS_ZSEEK_HD void table_entry(F fetch, int32_t entry, int32_t k, uint32_t *c, uint32_t *d, uint32_t *x) {
    *c = le32(fetch, 8 + entry * k);
    *d = le32(fetch, 12 + entry * k);
    *x = entry == ENTRY_CSUM ? le32(fetch, 16 + entry * k) : 0u;
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
        table_entry(fetch, entry, k, &c, &d, &x);
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
        table_entry(fetch, entry, k, &c, &d, &x);
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
// The table at the end of a whole object, as seek_footer finds it, with
// descriptor byte 0x00 (entries of 8 bytes) or 0x80 (entries of 12); any other
// descriptor is no table.  Every check of the two layouts above holds: the
// magics, 1 <= nf <= MAX_FRAMES, the size field; what the entries must add up to
// is seek_sums_ok's.  Nothing outside [0, src_len) is fetched.
template <class F>
JFS_ZSEEK_HD bool seek_footer_any(F fetch, int32_t src_len, int32_t *nf, int32_t *tpos, int32_t *entry) {
    if (src_len < TABLE_FIXED + ENTRY) return false;
    if (le32(fetch, src_len - 4) != SEEK_MAGIC) return false;
    const uint32_t desc = fetch(src_len - 5);
    if (desc != 0u && desc != DESC_CSUM) return false;
    const int32_t ent = desc ? ENTRY_CSUM : ENTRY;
    const uint32_t n = le32(fetch, src_len - 9);
    if (n < 1u || n > (uint32_t)MAX_FRAMES || (int64_t)n > ((int64_t)src_len - TABLE_FIXED) / ent) return false;
    const int32_t t = src_len - (ent * (int32_t)n + TABLE_FIXED);
    if (le32(fetch, t) != SKIP_MAGIC) return false;
    if (le32(fetch, t + 4) != (uint32_t)ent * n + 9u) return false;
    *nf = (int32_t)n;
    *tpos = t;
    *entry = ent;
    return true;
}

// entry k of the table at tpos whose entries take `entry` bytes: table_entry, inside the object
template <class F>
JFS_ZSEEK_HD void seek_entry_any(F fetch, int32_t tpos, int32_t entry, int32_t k, uint32_t *c, uint32_t *d, uint32_t *x) {
    *c = le32(fetch, tpos + 8 + entry * k);
    *d = le32(fetch, tpos + 12 + entry * k);
    *x = entry == ENTRY_CSUM ? le32(fetch, tpos + 16 + entry * k) : 0u;
}

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
    if (!seek_footer_any(fetch, src_len, &nf, &tpos, &entry)) return s;
    uint64_t cs = 0, ds = 0;
    uint32_t zeros = 0;
    for (int32_t k = 0; k < nf; k++) {
        uint32_t c, d, x;
        seek_entry_any(fetch, tpos, entry, k, &c, &d, &x);
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
        seek_entry_any(fetch, tpos, entry, k, &c, &d, &x);
        if (frame_in_ranges(rng, nr, dst_cap, ds, d)) {
            emit(k, (uint32_t)cs, (uint32_t)ds, c, d, x);
            s.count++;
        }
        cs += c;
        ds += d;
    }
    return s;
}

}  // namespace zseek
}  // namespace jfs
