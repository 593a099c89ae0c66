// The ORIGIN CHASE of the LZ4 ranges decode (lz4_chase.hip): one requested
// output byte of a block resolved on its own, from the index the small-batch
// decoder's spec / fix / count / scan leave behind (lz4_split.hip) and without
// any other output byte.  Host and device: tests/test_lz4_chase.py drives
// tests/lz4_chase_main.cc, which runs these rules for every output position
// against a serial LZ interpreter.
//
// The index: the compressed stream cut into SEG-byte segments; entry[k] = the
// position of the first token that starts at or behind segment k's first byte
// (n once there is none), cnt[k] = the output offset at that token.  A segment
// in which no token starts has entry[k] >= its end and shares cnt with its
// successor.
//
// The rule, per output position x < total:
//   locate   the last segment with cnt[k] <= x, then walk its tokens (the field
//            parsing of the decoders: parse_rd below) to the sequence holding x;
//   check    that token as the split decoder's emit checks it (tok_ok: the
//            acceptance conditions in the head comment of lz4_split.hip);
//   literal  the answer is its input position;
//   match    go on from mstart - off + (x - mstart) % off: an overlapped match
//            steps to its period position, so every step goes backwards and a
//            chain makes at most one step per sequence (origin_map.h states the
//            same for the dense map).
// The answer is a literal index, BAD (a visited token fails a condition, or the
// index does not lead to x) or DEEP (more than CHASE_HOPS steps).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "jfs_internal.h"
#define JFS_LZ4_HD __host__ __device__ __forceinline__
#define JFS_LZ4_UNROLL _Pragma("unroll")
#else
#define JFS_LZ4_HD inline
#define JFS_LZ4_UNROLL
#endif

namespace jfs {
namespace lz4s {

// one token at x (x < n): next token position, output bytes, and the fields
// the acceptance conditions need.  A token whose literals reach n is the last.
// 32-bit positions and lengths (the plan sends blocks with n or cap >= 2^30 to
// the exact kernel): the wave-per-segment emit parses in scalar registers, and
// 64-bit fields cost it two scalar ops per add and a VALU round trip per
// compare.  A length field stops growing at 2^30: such a token ends past n
// (or its match past cap) either way, so it is rejected as before.
constexpr int32_t LEN_CAP = 1 << 30;
struct Tok {
    uint32_t tok;    // the token byte
    int32_t lenip;   // input position after the literal-length bytes
    int32_t ll;      // literal length
    int32_t lit_end; // lenip + ll
    int32_t next;    // next token (n for the last token)
    int32_t mlip;    // input position after the match-length bytes
    int32_t ml;      // match length (0 for the last token)
    int32_t off;
    bool last, cut;  // cut: the stream ends inside the token's header fields
};

template <class RD>
JFS_LZ4_HD Tok parse_rd(RD s, int32_t n, int32_t x, bool want_off) {
    Tok t;
    t.cut = false;
    t.off = 0;
    t.ml = 0;
    const uint32_t tok = s[x];
    t.tok = tok;
    int32_t ip = x + 1;
    int32_t ll = (int32_t)(tok >> 4);
    if (ll == 15) {
        uint32_t b;
        do {
            if (ip >= n) {
                t.cut = true;
                break;
            }
            b = s[ip++];
            ll += (int32_t)b;
        } while (b == 255 && ll < LEN_CAP);
    }
    t.lenip = ip;
    t.ll = ll;
    t.lit_end = ip + ll;
    t.mlip = ip;
    if (t.cut || t.lit_end >= n) {
        t.last = true;
        t.next = n;
        return t;
    }
    t.last = false;
    int32_t q = t.lit_end;
    if (q + 2 > n) {
        t.cut = true;
        t.next = n;
        return t;
    }
    if (want_off) t.off = (int32_t)s[q] | ((int32_t)s[q + 1] << 8);
    q += 2;
    int32_t ml = (int32_t)(tok & 15);
    if (ml == 15) {
        uint32_t b;
        do {
            if (q >= n) {
                t.cut = true;
                break;
            }
            b = s[q++];
            ml += (int32_t)b;
        } while (b == 255 && ml < LEN_CAP);
    }
    t.mlip = q;
    t.ml = ml + 4;
    t.next = q;
    return t;
}

// the token checks the exact decoder makes (the emit keeps a token only if
// it would run it the same way)
JFS_LZ4_HD bool tok_ok(uint32_t tok, const Tok &t, int32_t n, int32_t op, int32_t cap) {
    // (op <= cap < 2^30 and every length < 2^30 + 2^8: no sum below overflows;
    // the last is evaluated only once op + ll <= cap - 12 holds)
    // literal-length bytes: liblz4 stops reading them (a "loop error" it
    // ignores) once its input position reaches iend-15 after a 255 byte;
    // lenip < iend-14 means the terminator was read before that point
    bool ok = !t.cut && ((tok >> 4) != 15 || t.lenip < n - 14);
    if (t.last) {
        ok = ok && t.lit_end == n && op + t.ll <= cap;
    } else {
        ok = ok && t.lit_end <= n - 8 && op + t.ll <= cap - 12 && t.off >= 1 && t.off <= op + t.ll &&
             ((tok & 15) != 15 || t.mlip < n - 4) && op + t.ll + t.ml <= cap - 5;
    }
    return ok;
}

// a rejected token that is a whole sequence, match included, and ends the
// stream: the block has no final literal run (BStat::bad = 2, the verdict's
// reason [5]; such a token always fails tok_ok -- its literals end past n - 8)
JFS_LZ4_HD bool ends_in_match(const Tok &t, int32_t n) { return !t.last && !t.cut && t.next >= n; }

}  // namespace lz4s

namespace lz4c {

constexpr int SEG = 256;  // compressed bytes per segment of the index (JFS_LZ4_SPLIT_SEG)
// Steps a chain may take.  A condition, not a tuning knob: the smallest power
// of two that is at least twice the deepest chain seen in 4 MiB blocks of every
// blockgen class from either encoder (DESIGN 12h has the histogram;
// tests/test_lz4_chase.py recomputes it on smaller blocks).  A block with a
// deeper chain is decoded by the exact prefix kernel instead.
constexpr int CHASE_HOPS = 2048;
constexpr int32_t BAD = -1, DEEP = -2;

// What one lookup finds: the run of output bytes [lo, hi) that one part of one
// sequence defines.  off == 0: its literals, byte lo at input position base.
// off > 0: its match, byte x copies output position base + (x - lo) % off
// (base = lo - off; the modulo only matters for an overlapped match).
struct Run {
    int32_t lo, hi, base, off;
};

// The run holding output position x (0 <= x < the block's total; cnt[0] == 0).
// s: the stream's bytes, s[p] for p < n; entry / cnt: the block's nseg index
// entries; cap: the block's dst_cap, which the token conditions refer to.
// false: BAD.  Reads s below n and the index below nseg only.
template <class S, class E>
JFS_LZ4_HD bool find_run(S s, int32_t n, int32_t cap, E entry, E cnt, int32_t nseg, int32_t x, Run &r) {
    if (nseg <= 0) return false;
    int32_t a = 0, z = nseg - 1;
    while (a < z) {  // the last segment whose offset is <= x (empty ones share their successor's)
        const int32_t m = (a + z + 1) >> 1;
        if (cnt[m] <= x) a = m;
        else z = m - 1;
    }
    const int32_t s1 = (a + 1) * SEG < n ? (a + 1) * SEG : n;
    int32_t p = entry[a], op = cnt[a];
    if (p < a * SEG || op < 0 || op > x) return false;
    while (p < s1) {
        const lz4s::Tok t = lz4s::parse_rd(s, n, p, true);
        const int32_t d = x - op;  // (>= 0; the lengths are below 2^30 + 2^9: no difference below overflows)
        if (d < t.ll || d - t.ll < t.ml) {
            if (!lz4s::tok_ok(t.tok, t, n, op, cap)) return false;
            if (d < t.ll) r = Run{op, op + t.ll, t.lenip, 0};
            else r = Run{op + t.ll, op + t.ll + t.ml, op + t.ll - t.off, t.off};
            return true;
        }
        if (t.last) return false;  // x lies behind the stream's output
        op += t.ll + t.ml;
        p = t.next;
    }
    return false;  // the segment's tokens end in front of x: not the index of this stream
}

// where a match byte comes from
JFS_LZ4_HD int32_t step(const Run &r, int32_t x) {
    const int32_t d = x - r.lo;
    return r.base + (r.off >= r.hi - r.lo ? d : (int32_t)((uint32_t)d % (uint32_t)r.off));
}

// The rule for one position: the literal index (>= 0), BAD or DEEP; hops += the steps taken.
template <class S, class E>
JFS_LZ4_HD int32_t chase_one(S s, int32_t n, int32_t cap, E entry, E cnt, int32_t nseg, int32_t x, uint32_t &hops) {
    for (int h = 0;; h++) {
        Run r;
        if (!find_run(s, n, cap, entry, cnt, nseg, x, r)) return BAD;
        if (r.off == 0) return r.base + (x - r.lo);
        if (h >= CHASE_HOPS) return DEEP;
        x = step(r, x);
        hops++;
    }
}

// The rule for the positions x0 + i, i < 4, whose bit is set in mask: idx[i] =
// the literal index of each.  Step by step, all positions together: a lookup
// serves every position of the quad that lies in its run, so a quad inside one
// literal run or one match run that does not wrap costs one lookup per step
// and stays together while that holds.  Returns 0, BAD or DEEP (idx is then
// not to be used); hops += the steps taken, per position.
template <class S, class E>
JFS_LZ4_HD int32_t chase_quad(S s, int32_t n, int32_t cap, E entry, E cnt, int32_t nseg, int32_t x0, uint32_t mask,
                              int32_t idx[4], uint32_t &hops) {
    int32_t x[4];
JFS_LZ4_UNROLL
    for (int i = 0; i < 4; i++) {
        x[i] = x0 + i;
        idx[i] = 0;
    }
    for (int h = 0;; h++) {
        Run r{0, 0, 0, 0};  // (holds nothing: the first open position looks up)
JFS_LZ4_UNROLL
        for (int i = 0; i < 4; i++) {
            if (!((mask >> i) & 1u)) continue;
            if (x[i] < r.lo || x[i] >= r.hi) {
                if (!find_run(s, n, cap, entry, cnt, nseg, x[i], r)) return BAD;
            }
            if (r.off == 0) {
                idx[i] = r.base + (x[i] - r.lo);
                mask &= ~(1u << i);
            } else {
                if (h >= CHASE_HOPS) return DEEP;
                x[i] = step(r, x[i]);
                hops++;
            }
        }
        if (!mask) return 0;
    }
}

}  // namespace lz4c
}  // namespace jfs
