// The ORIGIN MAP of the small-batch decoders (lz4_split.hip, zstd_split.inc):
// everything both codecs mean by it, once.  Host and device:
// tests/test_origin_map.py drives tests/origin_map_main.cc, which runs these
// rules against a serial LZ interpreter.
//
// A decode writes one uint32 per output byte: a literal byte's entry is
// -(literal index + 1), any other entry is the output position the byte
// copies (an overlapped match points before the match, so every pointer goes
// backwards).  Pointer jumping settles the map in place -- a pointer only ever
// moves to an ancestor, so concurrent rounds are safe -- and the gather writes
// dst[p] = literal[index of org[p]], or reports a quad that still holds a
// pointer: its block goes to the codec's exact kernel.
#pragma once
#include <stdint.h>

#include <algorithm>

#if defined(__HIPCC__)
#include "jfs_internal.h"
#define JFS_OM_HD __host__ __device__ __forceinline__
#define JFS_OM_UNROLL _Pragma("unroll")
#else
#define JFS_OM_HD inline
#define JFS_OM_UNROLL
#endif

namespace jfs {
namespace om {

#if !defined(__HIPCC__)
// a host build: jfs_internal.h's pointer types as plain ones (may_alias keeps
// the kernels' 16-byte and 32-bit casts defined)
struct __attribute__((may_alias)) uint4 {
    uint32_t x, y, z, w;
};
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
typedef uint8_t g_u8;
typedef uint32_t __attribute__((may_alias)) g_u32;
typedef uint4 g_u4;
#endif

constexpr int HOPS = 6;         // pointer hops per entry per jump round
constexpr int MAX_ROUNDS = 12;  // jump rounds a launch makes at most (BStat::jmp, SIn::jmp)
constexpr int THREADS = 256;    // threads per workgroup of emit / jump / gather

// ---- entry encoding
JFS_OM_HD uint32_t lit_entry(int64_t i) { return (uint32_t)(-i - 1); }
JFS_OM_HD bool is_lit(uint32_t e) { return (int32_t)e < 0; }
JFS_OM_HD int64_t lit_index(uint32_t e) { return -(int64_t)(int32_t)e - 1; }

// ---- entry writers, one thread per run: 16-byte stores where the run is
// 4-aligned (the map starts 16-byte aligned).  P: the codec's position type.

// entries [p, p + n) = the literals from index i0 on (v0 = lit_entry(i0), v0 - 1, ...)
template <class P>
JFS_OM_HD void put_lits(g_u32 *org, P p, P n, uint32_t v0) {
    P i = 0;
    for (; i < n && ((p + i) & 3); i++) org[p + i] = v0 - (uint32_t)i;
    for (; i + 4 <= n; i += 4) {
        const uint32_t v = v0 - (uint32_t)i;
        *(g_u4 *)(org + p + i) = make_uint4(v, v - 1u, v - 2u, v - 3u);
    }
    for (; i < n; i++) org[p + i] = v0 - (uint32_t)i;
}

// entries [p, p + n) of a match at p with offset off: entry i = p - off +
// (i mod off), the modulo as a running j (n may stop short of the match).
// FROM: only the entries [p + i0, p + n) (a decode from a floor above 0).
template <class P, bool FROM = false>
JFS_OM_HD void put_match(g_u32 *org, P p, P n, uint32_t off, P i0 = 0) {
    const P base = p - (P)off;
    uint32_t j = FROM ? (uint32_t)i0 % off : 0u;
    auto next = [&]() {
        const uint32_t e = (uint32_t)(base + j);
        j = j + 1 == off ? 0u : j + 1;
        return e;
    };
    P i = FROM ? i0 : 0;
    for (; i < n && ((p + i) & 3); i++) org[p + i] = next();
    for (; i + 4 <= n; i += 4) {
        uint32_t e[4];
JFS_OM_UNROLL
        for (int q = 0; q < 4; q++) e[q] = next();
        *(g_u4 *)(org + p + i) = make_uint4(e[0], e[1], e[2], e[3]);
    }
    for (; i < n; i++) org[p + i] = next();
}

// ---- jump step: one thread's walk over the quads first, first + stride, ...
// below total.  Each entry makes up to HOPS hops, the four entries' hops
// interleaved (four independent loads in flight), and the quad is stored if
// it changed.  load(o) reads entry o (o < total: an entry at or above total is
// neither followed nor changed).  Returns whether anything was stored.
// FROM: the map holds the entries [start, total) only (a decode from a floor
// above 0); the walk covers the quads from start's on, `first` counted from
// there, and an entry below start is neither followed nor changed.
template <bool FROM = false, class LD>
JFS_OM_HD bool jump_walk(g_u32 *org, int64_t total, int64_t first, int64_t stride, LD load, int64_t start = 0) {
    bool any = false;
    for (int64_t p = FROM ? (start & ~(int64_t)3) + first : first; p < total; p += stride) {
        const int lim = total - p < 4 ? (int)(total - p) : 4;
        const int low = FROM && start > p ? (int)(start - p) : 0;
        const uint4 v = *(const g_u4 *)(org + p);
        const uint32_t e0[4] = {v.x, v.y, v.z, v.w};
        int32_t o[4];  // (negative: a literal, or past total)
JFS_OM_UNROLL
        for (int i = 0; i < 4; i++) o[i] = i < lim && (!FROM || i >= low) ? (int32_t)e0[i] : -1;
        for (int h = 0; h < HOPS; h++) {
            if (o[0] < 0 && o[1] < 0 && o[2] < 0 && o[3] < 0) break;
            int32_t nx[4];
JFS_OM_UNROLL
            for (int i = 0; i < 4; i++) nx[i] = o[i] >= 0 ? (int32_t)load(o[i]) : o[i];
JFS_OM_UNROLL
            for (int i = 0; i < 4; i++) o[i] = nx[i];
        }
        uint32_t e[4];
        bool changed = false;
JFS_OM_UNROLL
        for (int i = 0; i < 4; i++) {
            e[i] = i < lim && (!FROM || i >= low) ? (uint32_t)o[i] : e0[i];
            changed |= e[i] != e0[i];
        }
        if (changed) {
            *(g_u4 *)(org + p) = make_uint4(e[0], e[1], e[2], e[3]);
            any = true;
        }
    }
    return any;
}

// ---- gather step: the quad at p (a multiple of 4, below total).  Writes
// dst[p + i] = lit[index of org[p + i]] for p + i < total and returns true, or
// writes nothing and returns false when one of those entries is not a literal.
// FROM: only the positions at or above start (the map holds nothing below it).
template <bool FROM = false>
JFS_OM_HD bool gather_quad(const g_u32 *org, const g_u8 *lit, g_u8 *dst, int64_t p, int64_t total, int64_t start = 0) {
    const uint4 v = *(const g_u4 *)(org + p);
    const uint32_t e[4] = {v.x, v.y, v.z, v.w};
    bool settled = true;
JFS_OM_UNROLL
    for (int i = 0; i < 4; i++) settled &= p + i >= total || (FROM && p + i < start) || is_lit(e[i]);
    if (!settled) return false;
    if (p + 4 <= total && (!FROM || p >= start) && (((uintptr_t)(dst + p)) & 3u) == 0) {
        uint32_t w = 0;
JFS_OM_UNROLL
        for (int i = 0; i < 4; i++) w |= (uint32_t)lit[lit_index(e[i])] << (8 * i);
        *(g_u32 *)(dst + p) = w;
    } else {
        for (int i = 0; i < 4 && p + i < total; i++)
            if (!FROM || p + i >= start) dst[p + i] = lit[lit_index(e[i])];
    }
    return true;
}

// ---- launch rules (host).  Jump rounds for maps of at most max_entries
// entries: the smallest count with HOPS^rounds > max_entries / unit + 1, at
// most MAX_ROUNDS.  After round r every entry points >= HOPS^r steps up its
// chain (or to a literal).  A step from a match byte lands in an earlier
// sequence's output or in its own sequence's literals (overlaps point before
// their match), so a chain has at most one step per sequence, and a sequence
// with a match makes at least `unit` bytes: 4 for LZ4 (a step per token), 3
// for Zstd.  So these rounds settle every well-formed block (8 for 4 MiB;
// each idle launch cost ~6 us of a lone decode); the gather checks every
// entry regardless.
inline int rounds(int64_t max_entries, int unit) {
    int jr = 1;
    for (double reach = HOPS; reach <= (double)max_entries / unit + 1 && jr < MAX_ROUNDS; reach *= HOPS) jr++;
    return jr;
}
// Test only (jfs_test_set_split_jump_rounds): the rounds the launchers of LZ4
// ([0], unit 4) and Zstd ([1], unit 3) make instead; 0 = rounds().
inline int test_rounds[2] = {0, 0};
inline int launch_rounds(int64_t max_entries, int unit) {
    const int t = test_rounds[unit == 3];
    return t > 0 ? t : rounds(max_entries, unit);
}

// workgroups that cover max_entries entries at one quad per thread (the gather)
inline unsigned quad_groups(int64_t max_entries) { return (unsigned)((max_entries / 4 + THREADS) / THREADS); }
// Jump grid width per block: about 2,048 workgroups in all (every entry of a
// 4 MiB block is covered after a few strides; the rounds after the first
// mostly find their block settled, and a workgroup per 1,024 entries for them
// cost more than the hops), at most one per 1,024 entries.
inline unsigned jump_groups(int64_t max_entries, int nb) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(quad_groups(max_entries), (2048 + nb - 1) / nb));
}

// A scratch layout, described once: the areas in order behind the 256-aligned
// base, each 256-byte aligned.  With a null base only `bytes` means anything
// (the size query); the launcher takes the pointers.
struct Carve {
    uintptr_t at;
    int64_t bytes = 256;  // (room to align the base)
    explicit Carve(void *base) : at(((uintptr_t)base + 255) & ~(uintptr_t)255) {}
    template <class T>
    void take(T *&p, int64_t n) {
        p = (T *)at;
        at += (uintptr_t)((n + 255) & ~255ll);
        bytes += (n + 255) & ~255ll;
    }
};

}  // namespace om
}  // namespace jfs
