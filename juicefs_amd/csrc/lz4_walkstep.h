// The step rule of the LZ4 decode kernel's segment-walk parser (SegWalk in
// lz4_decode.hip) with the byte fetch as a parameter, and the lanes' bit sets
// (BitSet<SEG>).  Host and device: tests/test_lz4_walkstep.py drives
// tests/walkstep_main.cc, tests/test_lz4_walk_seg.py tests/walkseg_main.cc
// (SEG = 128 and 256), which run these walks and a plain ws_next_exact walk
// over the same bytes.
//
// A step at p needs the token byte and the byte after it (one load round);
// from them follow the literal length and q, the position of the first
// match-length extension byte, and the next position x = q + mlx.  The byte at
// q (e2) matters only as `mlx && e2 == 255`: a match of >= 274 bytes, whose
// next position the exact rule finds.  So the step does not wait for e2: it is
// fetched, the lane goes on to x, and the test is made one iteration later,
// after the loads at x were issued (loads return in order: e2 is there once
// they are).  A lane whose test holds drops the bytes it fetched at the wrong
// x, takes the exact next position of the step it owes and goes on from there.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JFS_WALKSTEP_HD __host__ __device__ __forceinline__
#else
#define JFS_WALKSTEP_HD inline
#endif

namespace jfs {
namespace lz4d {

constexpr uint32_t WS_STOP = 0x80000000u;
constexpr int WS_KEXT = 64;  // max 255-extension bytes handled by the fast path

// Next token position after p (or WS_STOP | p): the exact chain rule.
template <class F>
JFS_WALKSTEP_HD uint32_t ws_next_exact(F fetch, int32_t n, int32_t p) {
    if (p > n - 18) return WS_STOP | (uint32_t)p;
    const uint32_t tb = fetch((uint32_t)p);
    int32_t q = p + 1;
    int32_t ll = (int32_t)(tb >> 4);
    if (ll == 15) {
        int k = 0;
        uint32_t sv;
        do {
            sv = fetch((uint32_t)q);
            q++;
            ll += (int32_t)sv;
            if (q >= n - 15 || ++k > WS_KEXT) return WS_STOP | (uint32_t)p;
        } while (sv == 255);
        if (q + ll > n - 32) return WS_STOP | (uint32_t)p;
    }
    q += ll + 2;
    if ((tb & 15u) == 15u) {
        int k = 0;
        uint32_t sv;
        do {
            sv = fetch((uint32_t)q);
            q++;
            if (q >= n - 4 || ++k > WS_KEXT) return WS_STOP | (uint32_t)p;
        } while (sv == 255);
    }
    return (uint32_t)q;
}

// The first load round of a step at p: all the step needs but e2.
// unsigned 32-bit offsets from a uniform base; bitwise 0/1 logic: no
// exec-mask branches.  A position past n - 18 reads index 0.
struct WsRound {
    uint32_t x;     // q + mlx
    uint32_t q;     // first match-length extension byte
    uint32_t halt;  // edge | lstop: WS_STOP | p without a further byte
    uint32_t ext;   // llx && e1 == 255: the exact rule, now
    uint32_t mlx;   // the token's match length is extended
};
// The owed byte pe2 is tested only after this round's loads were issued: on
// the device the three values pass through an empty volatile statement, which
// keeps the compiler from sinking the loads below the test or raising the
// test (and its wait for pe2) above them.
template <class F>
JFS_WALKSTEP_HD WsRound ws_round(F fetch, int32_t n, int32_t p, uint32_t &pe2) {
    const uint32_t edge = (uint32_t)(p > n - 18);
    const uint32_t up = (uint32_t)p;
    uint32_t tb = fetch(edge ? 0u : up), e1 = fetch(edge ? 0u : up + 1u);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(tb), "+v"(e1), "+v"(pe2));
#endif
    const uint32_t hi = tb >> 4;
    const uint32_t llx = (uint32_t)(hi == 15u);
    const uint32_t L = llx ? 15u + e1 : hi;
    const uint32_t lstop = llx & ((uint32_t)(p + 2 >= n - 15) | (uint32_t)(p + 2 + (int32_t)L > n - 32));
    WsRound r;
    r.q = up + 3u + llx + L;
    r.mlx = (uint32_t)((tb & 15u) == 15u);
    r.x = r.q + r.mlx;
    r.halt = edge | lstop;
    r.ext = (r.halt ^ 1u) & llx & (uint32_t)(e1 == 255u);
    return r;
}

// f(WsIdx<0>), f(WsIdx<1>) ... f(WsIdx<K - 1>): a loop whose index is a constant
// in every call, so that a word of a bit set is only ever named by a constant
// index and the set stays in registers.
template <int I>
struct WsIdx {
    static constexpr int v = I;
};
template <int K, int I = 0, class Fn>
JFS_WALKSTEP_HD void ws_each(Fn f) {
    if constexpr (I < K) {
        f(WsIdx<I>());
        ws_each<K, I + 1>(f);
    }
}

// SEG-bit sets as SEG / 64 u64 words (bit d = position plo + d); a bit index
// picks its word by compares.
template <int N>
struct BitSet {
    static_assert(N > 0 && N % 64 == 0, "whole u64 words");
    static constexpr int W = N / 64;
    uint64_t w[W];

    JFS_WALKSTEP_HD void clear() {
        ws_each<W>([&](auto i) { w[i.v] = 0ull; });
    }
    // d >= N reads the last word (callers discard the result)
    JFS_WALKSTEP_HD bool test(uint32_t d) const {
        uint64_t a = w[0];
        ws_each<W>([&](auto i) { a = i.v > 0 && d >= 64u * (uint32_t)i.v ? w[i.v] : a; });
        return ((a >> (d & 63u)) & 1ull) != 0;
    }
    // bit d of the set := on (d < N)
    JFS_WALKSTEP_HD void put(uint32_t d, bool on) {
        const uint64_t m = 1ull << (d & 63u);
        ws_each<W>([&](auto i) {
            const uint64_t v = on ? w[i.v] | m : w[i.v] & ~m;
            w[i.v] = (d >> 6) == (uint32_t)i.v ? v : w[i.v];
        });
    }
    // the bits >= d (none for d >= N)
    static JFS_WALKSTEP_HD BitSet from(uint32_t d) {
        BitSet r;
        const uint64_t part = ~0ull << (d & 63u);
        ws_each<W>([&](auto i) { r.w[i.v] = (d >> 6) < (uint32_t)i.v ? ~0ull : (d >> 6) == (uint32_t)i.v ? part : 0ull; });
        return r;
    }
    JFS_WALKSTEP_HD BitSet and_from(uint32_t d) const {
        BitSet r = from(d);
        ws_each<W>([&](auto i) { r.w[i.v] &= w[i.v]; });
        return r;
    }
    JFS_WALKSTEP_HD void or_in(const BitSet &o) {
        ws_each<W>([&](auto i) { w[i.v] |= o.w[i.v]; });
    }
    JFS_WALKSTEP_HD bool any() const {
        uint64_t a = 0ull;
        ws_each<W>([&](auto i) { a |= w[i.v]; });
        return a != 0ull;
    }
    // the first set bit >= d, or N
    JFS_WALKSTEP_HD uint32_t first_from(uint32_t d) const {
        const BitSet m = and_from(d);
        uint32_t r = (uint32_t)N;
        ws_each<W>([&](auto i) {  // from the last word down
            constexpr int k = W - 1 - i.v;
            r = m.w[k] ? 64u * (uint32_t)k + (uint32_t)__builtin_ctzll(m.w[k] | (1ull << 63)) : r;
        });
        return r;
    }
};

// What one iteration of a lane did (for the event counts of the profiling build).
enum { WS_STEPPED = 0, WS_REDONE = 1, WS_ARRIVED = 2 };

// The step at w.q, e2 left owing.  Returns its next position (or WS_STOP |
// w.q) unless *ext: then the exact rule gives it.  w.pend: the result stands
// only if the byte fetched into w.pe2 is not 255.
template <class W, class F>
JFS_WALKSTEP_HD uint32_t ws_take(W &w, uint32_t &pp, const WsRound &r, F fetch, int32_t n, bool *ext) {
    const uint32_t last = r.mlx & (uint32_t)((int32_t)r.x >= n - 4);
    const uint32_t pend = (r.halt ^ 1u) & (r.ext ^ 1u) & r.mlx & (last ^ 1u);
    w.pe2 = fetch(pend ? r.q : 0u);
    pp = (uint32_t)w.q;
    w.pend = pend != 0;
    *ext = r.ext != 0;
    return (r.halt | last) ? (WS_STOP | (uint32_t)w.q) : r.x;
}

// One iteration of a speculative walk (phase 0 of SegWalk::advance) for a
// moving lane.  W: q, plo, phi, sx, mv and the deferred state pe2 (the byte of
// the owed e2 test), pend; vs: the lane's speculative chain positions; the step
// that owes the test is kept in sx, which means nothing else while the lane
// moves.  A lane that owes a test keeps moving, past phi as well, until the
// test is made: sx is the exit once a settled step leaves.
template <int N, class W, class F, class X>
JFS_WALKSTEP_HD int ws_spec_iter(W &w, BitSet<N> &vs, F fetch, X exact, int32_t n) {
    const WsRound r = ws_round(fetch, n, w.q, w.pe2);
    // the step at pp is the exact rule's: the bytes at q are dropped
    const bool redo = w.pend && w.pe2 == 255u;
    const bool arr = w.pend && !redo && w.q >= w.phi;
    const int32_t at = redo ? (int32_t)w.sx : w.q;  // the step this iteration settles
    uint32_t x = (uint32_t)w.q;
    bool ex = redo;
    if (redo || arr) w.pend = false;
    else x = ws_take(w, w.sx, r, fetch, n, &ex);
    if (ex) x = exact(at);
    const bool stop = (x & WS_STOP) != 0;
    if (!arr && at >= w.plo) vs.put((uint32_t)(at - w.plo), !stop);
    const bool out = stop || (!w.pend && (int32_t)x >= w.phi);
    w.sx = out ? x : w.sx;
    w.mv = !out;
    w.q = (int32_t)x;
    return redo ? WS_REDONE : arr ? WS_ARRIVED : WS_STEPPED;
}

// One iteration of a fix-up walk (phase 1) for a moving lane: the walk ends
// where it joins the speculative chain vs, stops or leaves the segment.  W as
// above and ex; here ex keeps the step that owes the test while the lane moves
// (sx is the speculative exit a joining walk takes).  vt, the lane's true
// chain positions, takes the walk's positions directly: the caller clears it
// when the walk starts (nothing reads a walking lane's vt), a join ORs the
// speculative chain's suffix in.
template <int N, class W, class F, class X>
JFS_WALKSTEP_HD int ws_fix_iter(W &w, const BitSet<N> &vs, BitSet<N> &vt, F fetch, X exact, int32_t n) {
    const WsRound r = ws_round(fetch, n, w.q, w.pe2);
    const bool redo = w.pend && w.pe2 == 255u;
    const bool arr = w.pend && !redo && w.q >= w.phi;
    const int32_t at = redo ? (int32_t)w.ex : w.q;
    const uint32_t d = (uint32_t)(at - w.plo);
    const bool join = !redo && !arr && vs.test(d);
    uint32_t x = (uint32_t)w.q;
    bool ex = redo;
    if (redo || arr || join) w.pend = false;
    else x = ws_take(w, w.ex, r, fetch, n, &ex);
    if (ex) x = exact(at);
    const bool stop = (x & WS_STOP) != 0;
    if (!arr && !join) vt.put(d, !stop);
    if (join) vt.or_in(vs.and_from(d));
    const bool out = join || stop || (!w.pend && (int32_t)x >= w.phi);
    if (out) w.ex = join ? w.sx : x;
    w.mv = !out;
    w.q = (int32_t)x;
    return redo ? WS_REDONE : arr ? WS_ARRIVED : WS_STEPPED;
}

// The two-word form of a 128-bit set and of the two iterations, for a W that
// keeps its sets as vs0, vs1 / vt0, vt1 (tests/walkstep_main.cc).
JFS_WALKSTEP_HD BitSet<128> ws_set2(uint64_t a0, uint64_t a1) {
    BitSet<128> s;
    s.w[0] = a0;
    s.w[1] = a1;
    return s;
}
JFS_WALKSTEP_HD bool tbit2(uint64_t a0, uint64_t a1, uint32_t d) { return ws_set2(a0, a1).test(d); }
JFS_WALKSTEP_HD void sbit2(uint64_t &a0, uint64_t &a1, uint32_t d) {
    BitSet<128> s = ws_set2(a0, a1);
    s.put(d, true);
    a0 = s.w[0];
    a1 = s.w[1];
}
JFS_WALKSTEP_HD uint64_t from_lo(uint32_t d) { return BitSet<128>::from(d).w[0]; }
JFS_WALKSTEP_HD uint64_t from_hi(uint32_t d) { return BitSet<128>::from(d).w[1]; }
template <class W, class F, class X>
JFS_WALKSTEP_HD int ws_spec_iter(W &w, F fetch, X exact, int32_t n) {
    BitSet<128> vs = ws_set2(w.vs0, w.vs1);
    const int kind = ws_spec_iter(w, vs, fetch, exact, n);
    w.vs0 = vs.w[0];
    w.vs1 = vs.w[1];
    return kind;
}
template <class W, class F, class X>
JFS_WALKSTEP_HD int ws_fix_iter(W &w, F fetch, X exact, int32_t n) {
    BitSet<128> vt = ws_set2(w.vt0, w.vt1);
    const int kind = ws_fix_iter(w, ws_set2(w.vs0, w.vs1), vt, fetch, exact, n);
    w.vt0 = vt.w[0];
    w.vt1 = vt.w[1];
    return kind;
}

}  // namespace lz4d
}  // namespace jfs
