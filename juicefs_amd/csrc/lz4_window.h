// The WINDOW decode of the LZ4 small-batch decoder (lz4_split.hip): the output
// bytes [lo, hi) of a block from the 64 KiB chunk boundary below lo, without
// the sequences in front of it.  Host and device, no HIP:
// tests/test_lz4_window.py drives tests/lz4_window_main.cc, which runs these
// rules against a serial LZ interpreter.
//
// The fast parse (lz4_fast.h) cuts a block into independent chunks of kChunk
// bytes: no match of it reaches before its chunk's first byte or past its
// last.  Nothing in the stored bytes says which encoder wrote them, so the
// property is CHECKED, per block and per window, on the sequences the window
// visits:
//   Fc(lo)   max(lo, 0) rounded down to kChunk: the floor the block is tried at;
//   H        the window's clamped upper end (the prefix decode's want);
//   reach    a sequence with literals at [op, op + ll) and a match at
//            [m, m + ml) of offset off REACHES BELOW F iff m + ml > F, m < H and
//            m - off < F: some match byte lies at or above F inside the window,
//            and the lowest byte the match can copy lies below F.  (A match
//            that straddles F has m < F, so it reaches below whatever its
//            offset; an overlapped match copies from m - off upwards only.)
//   floor    F = Fc if no sequence reaches below Fc, else 0 (the prefix decode).
//   entries  of a run of len output bytes at p (a sequence's literals, or its
//            match), the origin entries written are those in [F, E), E =
//            min(total, H): clip below.  They stay absolute output positions,
//            and by the floor rule every pointer among them points into [F, E).
//   checks   a token is checked (lz4_chase.h tok_ok) iff some output byte of
//            it lies in [F, H); the block's last token is checked whenever the
//            block ends within H, as in the prefix decode, because the verdict
//            asks for it.  A fault in a sequence wholly in front of F is unseen.
#pragma once
#include <stdint.h>

#include "lz4_chase.h"  // Tok, parse_rd, tok_ok: shared, not restated
#include "lz4_fast.h"   // kChunk

namespace jfs {
namespace lz4w {

constexpr int32_t CHUNK = (int32_t)lz4f::kChunk;
static_assert((CHUNK & (CHUNK - 1)) == 0, "the floor is a mask");

// Fc(lo)
JFS_LZ4_HD int32_t floor_of(int32_t lo) { return (lo > 0 ? lo : 0) & ~(CHUNK - 1); }

// the reach rule: a match at [m, m + ml) of offset off, floor F, window end H
// (m, ml < 2^30 + 2^9 and off < 2^16: no sum below overflows)
JFS_LZ4_HD bool reaches_below(int32_t F, int32_t H, int32_t m, int32_t ml, int32_t off) {
    return m + ml > F && m < H && m - off < F;
}

// whether a token with output [op, op + len) is visited: some byte of it in [F, H)
JFS_LZ4_HD bool visited(int32_t F, int32_t H, int32_t op, int32_t len) { return op + len > F && op < H; }

// the entries of a run of len output bytes at p that fall in [F, E): p + i for i0 <= i < i1 (none: i1 <= i0)
struct Clip {
    int32_t i0, i1;
};
JFS_LZ4_HD Clip clip(int32_t p, int32_t len, int32_t F, int32_t E) {
    Clip c;
    c.i0 = F - p > 0 ? F - p : 0;
    c.i1 = E - p < len ? E - p : len;
    return c;
}

}  // namespace lz4w
}  // namespace jfs
