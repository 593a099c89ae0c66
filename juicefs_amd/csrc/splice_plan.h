// Host-only planning of the spliced Zstd compaction (capi_chain.hip
// compact_splice_run): which 128 KiB pieces of an output are the stored bytes of
// a source's frame, the gather plan of everything else, and what that plan still
// reads of every source.  Plain C++17 integer code -- no HIP types -- with the
// byte fetch as a parameter, as in zstd_seek.h, whose table parser it uses for
// both layouts; tests/splice_plan_main.cc and tests/splice_tables_main.cc check
// it on a CPU under ASan + UBSan.
//
// The rule.  F = FRAME_BYTES.  Output j with total > F is cut into pieces p =
// [f F, min((f + 1) F, total)).  Piece p is PASS(i, k) iff
//   - one segment covers the whole piece, and its src = i >= 0;
//   - source i has a valid table: zstd_seek.h's, either layout, at most 16,384
//     frames, and its content D fits the block size the call states for it;
//   - frame k of that table has D_k == seg.src_off + (p.lo - seg.dst_off), d_k ==
//     |p| and d_k > 0;
//   - c_k <= d_k + 21, the seekable encoder's own worst case, so the spliced
//     object stays inside jfs_compress_bound(ZSTD, total) as n + 21 nb + 17 does;
//   - a 12-byte output layout has a 12-byte source table (the checksum word is
//     copied with the frame).
// Every other piece is FRESH.  An output is spliced iff total > F and at least
// one of its pieces is PASS; every other output is one encode unit, whole.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "chain_plan.h"
#include "zstd_seek.h"

namespace jfs_plan {

constexpr int32_t SPLICE_SLACK = 21;  // c_k - d_k of the seekable encoder's worst frame

// source i's table as the rule sees it
struct SpliceTable {
    int32_t valid = 0;  // 1: a valid table whose content fits the source's capacity
    int32_t entry = 0;  // 8 or 12
    int32_t nf = 0;
    uint32_t total = 0;              // D
    std::vector<uint32_t> c, d, x;   // the entries
    std::vector<uint64_t> coff, doff;  // what lies in front of frame k, nf + 1 entries
};

// one frame of a spliced output
struct SpliceFrame {
    int32_t src;    // PASS: the source; FRESH: -1
    int32_t k;      // PASS: the source's frame; FRESH: -1
    uint32_t coff;  // PASS: where the frame starts in the stored object
    uint32_t c;     // PASS: its stored bytes (FRESH: the encoder decides)
    uint32_t d;     // its content, |p|
    uint32_t x;     // PASS: its checksum word (0 from an 8-byte table)
    int32_t unit;   // FRESH: its encode unit; PASS: -1
};

// one encode unit of the derived plan: a whole output, or one FRESH piece
struct SpliceUnit {
    int32_t out;    // the output
    int32_t piece;  // -1: the whole output; else the piece's number f
    int32_t total;  // gathered bytes
};

struct SplicePlan {
    std::vector<SpliceTable> tab;       // per source
    std::vector<int32_t> frame_first;   // nout + 1; output j is spliced iff it owns frames
    std::vector<SpliceFrame> frames;
    std::vector<SpliceUnit> units;
    std::vector<int32_t> seg_first;     // the derived plan: units.size() + 1 entries
    std::vector<jfs_compact_seg> seg;   // each unit's segments, clipped, dst_off rebased to the unit
    uint64_t outs = 0, passed = 0, fresh = 0, passed_bytes = 0;  // spliced outputs, their frames, the PASS bytes
    bool spliced(int j) const { return frame_first[j + 1] > frame_first[j]; }
};

// The table at the end of the stored object [0, len) read through fetch(p); cap:
// the decoded block's capacity.
template <class F>
inline SpliceTable splice_table(F fetch, int64_t len, int64_t cap) {
    using namespace jfs::zseek;
    SpliceTable t;
    int32_t nf = 0, tpos = 0, entry = 0;
    if (!seek_table(fetch, len, true, false, &nf, &tpos, &entry)) return t;
    t.c.resize(nf);
    t.d.resize(nf);
    t.x.resize(nf);
    t.coff.assign(nf + 1, 0);
    t.doff.assign(nf + 1, 0);
    uint32_t zeros = 0;
    for (int32_t k = 0; k < nf; k++) {
        seek_entry(fetch, tpos, entry, k, &t.c[k], &t.d[k], &t.x[k]);
        zeros += t.c[k] == 0u;
        t.coff[k + 1] = t.coff[k] + t.c[k];
        t.doff[k + 1] = t.doff[k] + t.d[k];
    }
    if (!seek_sums_ok(t.coff[nf], t.doff[nf], zeros, tpos) || (int64_t)t.doff[nf] > cap) return SpliceTable();
    t.valid = 1;
    t.entry = entry;
    t.nf = nf;
    t.total = (uint32_t)t.doff[nf];
    return t;
}

// the frame of a valid table whose content is exactly [at, at + len), len > 0; or -1
inline int32_t splice_find_frame(const SpliceTable &t, int64_t at, int64_t len) {
    // the last k with D_k <= at: frames without content in front of it share its D_k
    const auto it = std::upper_bound(t.doff.begin(), t.doff.begin() + t.nf, (uint64_t)at);
    if (it == t.doff.begin()) return -1;
    const int32_t k = (int32_t)(it - t.doff.begin()) - 1;
    return (int64_t)t.doff[k] == at && (int64_t)t.d[k] == len && len > 0 ? k : -1;
}

// The whole answer.  fetch(i, p) = byte p of stored object i (p inside [0,
// src_len[i]) always); src_cap[i] = its decoded block's capacity; total[j] =
// compact_plan_ok's; use (nout entries, or null for "all") = the outputs the
// device works on -- the others get no unit; csum_out = the output table has
// 12-byte entries.  The plan is compact_plan_ok's: checked.
template <class F>
inline SplicePlan splice_plan(F fetch, int nsrc, const int64_t *src_len, const int64_t *src_cap, int nout,
                              const int32_t *seg_first, const jfs_compact_seg *seg, const int64_t *total,
                              const uint8_t *use, bool csum_out) {
    const int64_t FB = jfs::zseek::FRAME_BYTES;
    SplicePlan P;
    P.tab.resize(nsrc > 0 ? nsrc : 0);
    // every source's table: the caller answers src_n from it, whether a piece asks for it or not
    for (int i = 0; i < nsrc; i++) P.tab[i] = splice_table([&](int32_t p) { return fetch(i, p); }, src_len[i], src_cap[i]);
    auto table = [&](int i) -> const SpliceTable & { return P.tab[i]; };
    P.frame_first.assign(nout + 1, 0);
    P.seg_first.push_back(0);
    // [lo, hi) of output j's segments [k0, k1) as a unit of its own
    auto add_unit = [&](int j, int32_t piece, int64_t lo, int64_t hi, int k0, int k1) {
        for (int k = k0; k < k1; k++) {
            const jfs_compact_seg &g = seg[k];
            const int64_t a = std::max<int64_t>(g.dst_off, lo), b = std::min<int64_t>((int64_t)g.dst_off + g.len, hi);
            if (b <= a) continue;
            P.seg.push_back(jfs_compact_seg{g.src, g.src < 0 ? 0 : (int32_t)(g.src_off + (a - g.dst_off)), (int32_t)(a - lo),
                                            (int32_t)(b - a)});
        }
        P.units.push_back(SpliceUnit{j, piece, (int32_t)(hi - lo)});
        P.seg_first.push_back((int32_t)P.seg.size());
    };
    std::vector<SpliceFrame> fr;
    for (int j = 0; j < nout; j++) {
        P.frame_first[j] = (int32_t)P.frames.size();
        if (use && !use[j]) continue;
        const int k0 = seg_first[j], k1 = seg_first[j + 1];
        fr.clear();
        int npass = 0;
        if (total[j] > FB) {
            int k = k0;  // the segment that holds the piece's first byte
            for (int64_t lo = 0; lo < total[j]; lo += FB) {
                const int64_t hi = std::min(lo + FB, total[j]);
                while ((int64_t)seg[k].dst_off + seg[k].len <= lo) k++;
                const jfs_compact_seg &g = seg[k];
                SpliceFrame f{-1, -1, 0, 0, (uint32_t)(hi - lo), 0, -1};
                if (g.src >= 0 && (int64_t)g.dst_off + g.len >= hi) {
                    const SpliceTable &t = table(g.src);
                    const int32_t q = t.valid && (!csum_out || t.entry == jfs::zseek::ENTRY_CSUM)
                                          ? splice_find_frame(t, (int64_t)g.src_off + (lo - g.dst_off), hi - lo)
                                          : -1;
                    if (q >= 0 && (uint64_t)t.c[q] <= (uint64_t)t.d[q] + SPLICE_SLACK) {
                        f = SpliceFrame{g.src, q, (uint32_t)t.coff[q], t.c[q], t.d[q], t.x[q], -1};
                        npass++;
                    }
                }
                fr.push_back(f);
            }
        }
        if (npass == 0) {
            add_unit(j, -1, 0, total[j], k0, k1);
            continue;
        }
        int k = k0;
        for (size_t f = 0; f < fr.size(); f++) {
            if (fr[f].src < 0) {
                const int64_t lo = (int64_t)f * FB, hi = lo + fr[f].d;
                while ((int64_t)seg[k].dst_off + seg[k].len <= lo) k++;
                int ke = k;
                while (ke < k1 && (int64_t)seg[ke].dst_off < hi) ke++;
                fr[f].unit = (int32_t)P.units.size();
                add_unit(j, (int32_t)f, lo, hi, k, ke);
                P.fresh++;
            } else {
                P.passed++;
                P.passed_bytes += fr[f].c;
            }
            P.frames.push_back(fr[f]);
        }
        P.outs++;
    }
    P.frame_first[nout] = (int32_t)P.frames.size();
    return P;
}

// ---- the tables alone --------------------------------------------
// On a volume with object encryption the host never sees a source's plaintext:
// the sealed call opens the sources on the device, zstd_seek_tables.hip packs
// their tables into slots, and the rule above runs on those.

// Source i's slot: room for the 12-byte table of ceil(cap / F) frames -- what the
// seekable encoder and the spliced path write for a block of cap bytes -- rounded
// up to 16.  A table that does not fit is "no table" for the call.
inline int64_t splice_slot_bytes(int64_t cap) {
    const int64_t F = jfs::zseek::FRAME_BYTES, nf = cap > 0 ? (cap + F - 1) / F : 0;
    return align16(jfs::zseek::ENTRY_CSUM * nf + jfs::zseek::TABLE_FIXED);
}

// splice_plan's fetch over packed tables.  Source i's plaintext has len[i]
// bytes, of which only the last tlen[i], its table, are here, at tab + at[i];
// tlen[i] == 0: it has no table (also a failed open, len[i] < 0).  Every other
// position answers 0 and is counted in *outside (when given): the rule never
// asks for one -- zstd_seek.h's parser starts at the footer and reads nothing
// in front of the skippable header it points to.
struct PackedTables {
    const uint8_t *tab;
    const int64_t *at;
    const int32_t *tlen;
    const int64_t *len;
    uint64_t *outside;
    // what splice_plan is handed as src_len[i]: nothing to parse without a table
    int64_t src_len(int i) const { return tlen[i] > 0 && len[i] >= tlen[i] ? len[i] : 0; }
    uint8_t operator()(int i, int32_t p) const {
        const int64_t n = src_len(i), q = (int64_t)p - (n - tlen[i]);
        if (n == 0 || q < 0 || q >= tlen[i]) {
            if (outside) ++*outside;
            return 0;
        }
        return tab[at[i] + q];
    }
};

// What the derived plan still reads of every decoded source: chain_ranges' lists
// over the units.  A source that only PASS pieces reference has an empty list.
inline ChainRanges splice_ranges(const SplicePlan &P, int nsrc, const std::vector<ChainSrc> &st, int ns) {
    return chain_ranges(nsrc, (int)P.units.size(), P.seg_first.data(), P.seg.data(), st, ns);
}

}  // namespace jfs_plan
