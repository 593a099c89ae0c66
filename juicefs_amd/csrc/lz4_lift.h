// The LIFT of LZ4 compaction: an output chunk that is, byte for
// byte, one whole 64 KiB chunk of one source needs no parse -- its sequence
// records are read back from the source's stored token stream and handed to the
// fast encoder's stitch and emit (lz4_fast.hip).  Host and device, no HIP:
// tests/test_lz4_lift.py drives tests/lz4_lift_main.cc, which runs these rules
// and the serial restatement below against the fast encoder's host twin.
//
// The fast parse (lz4_fast.h) is deterministic in a chunk's content and in the
// block's end rules only: the table is zeroed per chunk, positions are
// chunk-relative and no byte outside the chunk is compared.  So:
//   interior  chunk c of a block of n bytes is INTERIOR iff (c + 1) * kChunk +
//             kMfLimit <= n: its parse ran with mend = clen and slim = clen - 4,
//             the block's end rules do not touch it.
//   plan      (host, lift_plan) output chunk j of block k is a CANDIDATE iff ONE
//             segment with src >= 0 covers [j * kChunk, (j + 1) * kChunk) whole,
//             that range is [i * kChunk, (i + 1) * kChunk) of the source for an
//             integer i, chunk j is interior in the output's total, and chunk i
//             is interior in the source's dst_cap.  A hole is never a candidate,
//             and neither is a chunk covered by two or more segments, even where
//             the segments continue each other: one segment is the whole test.
//   rule      (device, per candidate; the host only knows capacities) source
//             chunk i, F = i * kChunk, E = F + kChunk, is LIFTABLE iff
//             the source decoded to at least E + kMfLimit bytes (interior in its
//             true length), its token index settled, and of its sequences --
//             literals at [a, m), a match at [m, m + ml) of offset off, in
//             output coordinates as lz4_window.h phrases them --
//               none has m < F < m + ml           (a match straddles F),
//               none with F <= m < E has m - off < F   (copies from below F),
//               none has m < E < m + ml           (a match straddles E),
//               at most kMaxRec have F <= m < E,
//             and every field fits the u16 halves of a record (which the three
//             match conditions imply: 1 <= m - F, so ml <= 65,535; lit <= m - F).
//   result    what parse_kernel leaves for the chunk: recs[] = {pos | mlen << 16,
//             off | lit << 16} with pos = m - F and lit = m - max(a, F) (only the
//             first record's literals can begin below F: they are the trailing
//             literals of the chunks in front, which stitch adds back as the
//             carry), nrec, tail = E - (end of the last match) or kChunk without
//             one, lit0 = the first record's lit, and body by parse_kernel's sum.
// A wrong verdict can only send a chunk to the parse: the records of a liftable
// chunk describe the bytes the source's decode produced, whatever encoder wrote
// them, so the block emitted from them is a valid LZ4 block for the same bytes;
// for a fast-parse source they are the records a re-parse leaves.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/jfs_gpucodec.h"  // jfs_compact_seg, jfs_lz4_lift
#include "lz4_chase.h"                   // Tok, parse_rd: shared, not restated
#include "lz4_fast.h"                    // kChunk, kMfLimit, kMaxRec, len_bytes

namespace jfs {
namespace lz4l {

using lz4f::kChunk;
using lz4f::kChunkLog;
using lz4f::kMaxRec;
using lz4f::kMfLimit;
using lz4f::kMinMatch;
using lz4f::len_bytes;
using lz4f::nchunks;

JFS_LZ4F_HD bool interior(int64_t c, int64_t n) { return c >= 0 && (c + 1) * kChunk + kMfLimit <= n; }

// ---- the rule, per sequence ------------------------------------------------
enum : int { SEQ_OUT = 0, SEQ_REC = 1, SEQ_BAD = 2 };

// A sequence with its match at [m, m + ml) of offset off against the chunk at
// floor F: no part of the chunk's records (OUT), one of them (REC), or what
// refuses the chunk (BAD).  (m <= the block's total < 2^30 and ml < 2^30 + 2^9,
// as the index's count keeps them: no sum below overflows.)
JFS_LZ4F_HD int classify(int32_t F, int32_t m, int32_t ml, int32_t off) {
    const int32_t E = F + (int32_t)kChunk;
    if (m + ml <= F || m >= E) return SEQ_OUT;
    if (m < F || m + ml > E) return SEQ_BAD;  // straddles F, or E
    if (off < 1 || m - off < F || ml > 0xffff) return SEQ_BAD;
    return SEQ_REC;
}

// the record of a REC sequence whose literals begin at a
JFS_LZ4F_HD int32_t rec_lit(int32_t F, int32_t a, int32_t m) { return m - (a > F ? a : F); }
JFS_LZ4F_HD uint32_t rec_x(int32_t F, int32_t m, int32_t ml) { return (uint32_t)(m - F) | (uint32_t)ml << 16; }
JFS_LZ4F_HD uint32_t rec_y(int32_t off, int32_t lit) { return (uint32_t)off | (uint32_t)lit << 16; }
// its share of `body`, the length bytes of its literals included (parse_kernel
// leaves those of the chunk's first record to stitch: body_of_first takes them off)
JFS_LZ4F_HD uint32_t rec_body(int32_t lit, int32_t ml) {
    return (uint32_t)(1 + lit + 2 + len_bytes(ml - kMinMatch) + len_bytes(lit));
}
JFS_LZ4F_HD uint32_t body_of_first(int32_t lit0) { return (uint32_t)len_bytes(lit0); }

// ---- the serial restatement (host tests) -----------------------------------
struct Lifted {
    bool ok = false;
    std::vector<uint32_t> x, y;  // the records' halves
    int32_t nrec = 0, tail = 0, lit0 = 0;
    uint32_t body = 0;
    int64_t total = 0;  // the stream's output bytes, as its tokens count them
};

// Chunk i of the stored block s[0, n), walked token by token from byte 0.
inline Lifted lift_host(const uint8_t *s, int32_t n, int32_t i) {
    Lifted r;
    if (i < 0) return r;
    const int64_t F64 = (int64_t)i << kChunkLog;
    if (F64 + kChunk >= (1 << 30)) return r;
    const int32_t F = (int32_t)F64, E = F + (int32_t)kChunk;
    bool bad = false;
    int32_t end = F;
    int64_t op = 0;
    for (int32_t p = 0; p < n;) {
        const lz4s::Tok t = lz4s::parse_rd(s, n, p, true);
        if (t.cut || op + t.ll + t.ml >= (1 << 30)) return r;
        if (!t.last) {
            const int32_t a = (int32_t)op, m = a + t.ll;
            const int c = classify(F, m, t.ml, t.off);
            bad = bad || c == SEQ_BAD;
            if (c == SEQ_REC && !bad) {
                const int32_t lit = rec_lit(F, a, m);
                r.x.push_back(rec_x(F, m, t.ml));
                r.y.push_back(rec_y(t.off, lit));
                r.body += rec_body(lit, t.ml);
                end = m + t.ml;
            }
        }
        op += (int64_t)t.ll + t.ml;
        p = t.next;
    }
    r.total = op;
    // (matches are four bytes at least and lie inside the chunk: the count cannot pass kMaxRec)
    if (bad || !interior(i, op) || (int64_t)r.x.size() > kMaxRec) return r;
    r.ok = true;
    r.nrec = (int32_t)r.x.size();
    r.tail = E - end;
    r.lit0 = r.nrec ? (int32_t)(r.y[0] >> 16) : 0;
    r.body -= r.nrec ? body_of_first(r.lit0) : 0u;
    return r;
}

// ---- the host plan ---------------------------------------------------------
struct LiftPlan {
    std::vector<jfs_lz4_lift> chunk;  // per output chunk, flat: block after block, nchunks(total) each
    std::vector<int32_t> per_out;     // candidates per output block
    std::vector<int32_t> srcs;        // the distinct sources with a candidate, ascending
    int64_t candidates = 0;
};

// Output k owns seg[seg_first[k] .. seg_first[k + 1]), which tile [0, total[k])
// in order; src_cap[i]: source i's decode capacity (i < nsrc; a segment of any
// other source is no candidate).
inline LiftPlan lift_plan(int nout, const int32_t *seg_first, const jfs_compact_seg *seg, const int32_t *total, int nsrc,
                          const int32_t *src_cap) {
    LiftPlan P;
    std::vector<uint8_t> used(nsrc > 0 ? nsrc : 0, 0);
    P.per_out.assign(nout > 0 ? nout : 0, 0);
    for (int k = 0; k < nout; k++) {
        const int64_t n = total[k], nc = n >= 0 && n <= lz4f::kMaxInput ? nchunks(n) : 0;
        int32_t q = seg_first[k];
        for (int64_t j = 0; j < nc; j++) {
            jfs_lz4_lift c{-1, 0};
            const int64_t lo = j << kChunkLog, hi = lo + kChunk;
            // the segment that holds the chunk's first byte
            while (q < seg_first[k + 1] && (int64_t)seg[q].dst_off + seg[q].len <= lo) q++;
            if (q < seg_first[k + 1] && interior(j, n)) {
                const jfs_compact_seg &g = seg[q];
                const int64_t from = (int64_t)g.src_off + lo - g.dst_off;
                if (g.src >= 0 && g.src < nsrc && g.dst_off <= lo && (int64_t)g.dst_off + g.len >= hi && g.src_off >= 0 &&
                    from % kChunk == 0 && interior(from >> kChunkLog, src_cap[g.src])) {
                    c = jfs_lz4_lift{g.src, (int32_t)(from >> kChunkLog)};
                    used[g.src] = 1;
                    P.per_out[k]++;
                    P.candidates++;
                }
            }
            P.chunk.push_back(c);
        }
    }
    for (int i = 0; i < nsrc; i++)
        if (used[i]) P.srcs.push_back(i);
    return P;
}

}  // namespace lz4l
}  // namespace jfs
