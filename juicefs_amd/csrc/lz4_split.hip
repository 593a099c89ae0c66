// LZ4 block decode for SMALL batches: every block is spread over the whole
// GPU instead of one workgroup (lz4_decode.hip).  This is the latency path of
// the one-call API: cachedStore.load (pkg/chunk/cached_store.go:755-823)
// decodes exactly one 4 MiB block per cache miss, and one workgroup's serial
// token chain takes ~21 ms on it; here a lone block takes a few hundred
// microseconds of kernel time.
//
// Parallel formulation of LZ4_decompress_safe (the C routine lz4.DecompressSafe
// reaches, compress.go:120-125), in eight steps, all on one stream:
//   plan     per-block scratch offsets and segment counts (one tiny kernel);
//   spec     the compressed stream is cut into SEG-byte segments, one lane
//            each; a lane walks the token chain from its segment's first byte
//            (a guess: that byte need not start a token), marks every chain
//            position in a bitmap and records where the chain leaves;
//   fix      repeated rounds: a lane walks the chain from its segment's
//            current entry until it meets a marked position (the two chains
//            have merged, so its exit is the speculative one) or leaves the
//            segment; a changed exit becomes the next segment's entry.  A round
//            that changes nothing proves every entry is the true one (entry 0
//            is 0, and each exit is the chain function of its entry);
//   count    output bytes of each segment's true tokens;
//   scan     exclusive prefix sum per block -> output offset of each segment;
//   emit     each lane walks its true tokens again, checks liblz4's
//            acceptance conditions (below) and writes the block's ORIGIN map
//            (origin_map.h: the entries, the jump and gather rules and the
//            round count); a literal's index is its input position;
//   jump     pointer jumping over the map until every entry is a literal;
//   gather   the output bytes, from the settled map.
// Any block that this formulation does not cover EXACTLY -- a fix-up or jump
// that did not converge in its rounds, or a token that fails one of the
// conditions below -- is flagged and re-run by the exact one-workgroup kernel
// (lz4_decode.hip), which reproduces liblz4 1.9.3 return values on every
// input.  The conditions are sufficient for LZ4_decompress_safe to accept the
// stream with standard semantics (oracle/lz4_oracle.c, the liblz4 1.9.3 check
// order): for every sequence but the last, literal-length bytes end before
// iend-14, literals end at or before iend-8 and oend-12, 1 <= offset <= bytes
// produced, match-length bytes end before iend-4, the match ends at or before
// oend-5; the last sequence is literals only, ends exactly at iend and within
// oend (literal-length bytes before iend-14).  Encoder output always meets
// them; anything else takes the exact path.
//
// Prefix decode (jfs_launch_lz4_split_prefix): a block also carries `want`, the
// output bytes its caller needs.  Origin pointers only point backwards, so the
// entries of [0, want) never depend on one at or above want: spec, fix, count
// and scan (which walk compressed bytes) run whole, emit writes only the
// entries below want (a token that starts below want is still checked in
// full, one that starts at or above it is not looked at), jump and gather run
// over min(total, want) entries, and the result is that minimum.  The full
// launcher is the same kernels with want = cap.
//
// Window decode (jfs_launch_lz4_split_window): a block carries [lo, hi), and
// is decoded from the floor F of lz4_window.h: the 64 KiB chunk boundary below
// lo where the probe finds no sequence of the window reaching below it, else 0.
// The index steps run whole, as above; the probe walks the segments whose
// output meets [Fc, hi); emit skips the segments that end at or below F and
// writes the entries of [F, min(total, hi)) only, at their absolute positions;
// jump and gather run over that range, their grids sized as the prefix
// launcher's (the host cannot know F: threads are counted from F's quad and
// the ones past the end exit at once).  With F = 0 it is the prefix decode.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jfs_internal.h"
#include "lz4_chase.h"  // Tok, parse_rd, tok_ok: the token parse and its checks, shared with the host tests
#include "lz4_window.h"  // the window decode's floor, reach and clipping rules, shared with the host tests
#include "origin_map.h"
#include "wave.cuh"

namespace jfs {
namespace lz4s {

// ---- shared with the ranges decode: lz4_chase.hip includes this file with
// JFS_LZ4_SPLIT_RECORDS_ONLY defined and takes the records the kernels keep in
// scratch and the launch of the INDEX steps (plan, spec, fix, count, scan, which
// walk compressed bytes only), not the kernels.
constexpr int SEG = JFS_LZ4_SPLIT_SEG;  // compressed bytes per segment (one lane)
constexpr int FIX_ROUNDS = 6;
constexpr int T = om::THREADS;  // threads per workgroup
static_assert(SEG == lz4c::SEG, "lz4_chase.h restates the segment size");

struct SBlock {
    const uint8_t *src;
    uint8_t *dst;
    int32_t n, cap;
    int32_t want;  // output bytes asked for, in [0, cap] (the full decode: cap)
    int32_t seg0, nseg;
    int64_t bits_off;  // dwords into the bitmap area
    int64_t org_off;   // entries into the origin area (multiple of 4)
};

struct BStat {
    int32_t bad, last_ok, total, todo;  // bad: 1 = outside the proven cases, 2 = the stream ends in a match
    int32_t unsettled;  // the gather met an entry that is not a literal yet
    int32_t fc, below;  // window decode: the chunk floor tried, and the probe's flag (a sequence reaches below it)
    int32_t fix[FIX_ROUNDS];
    int32_t jmp[om::MAX_ROUNDS];
};

struct Scratch {
    SBlock *blk;
    BStat *st;
    int32_t *spec_exit, *entry, *cnt;
    uint32_t *bits;
    int32_t *org;
    int32_t *hwant;  // window decode: the want of the hand-over (0 for an empty window), per block
};

// the block holding segment g: the last b with seg0 <= g (binary search)
__device__ __forceinline__ int block_of(const SBlock *blk, int nb, int g) {
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blk[mid].seg0 <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Carves the index areas (everything but the todo mask and the origin map) for
// nb blocks of nseg_all segments in all; the caller goes on carving behind them.
void carve_index(om::Carve &c, int64_t nb, int64_t nseg_all, Scratch &sc);

// Queues plan, spec, the fix rounds, count and scan on st.  d_want (null: the
// full decode), max_cap, norg_all and max_want as the launchers below take
// them; a caller without an origin area passes norg_all = INT64_MAX.
void launch_index(const jfs_dev_block *d_desc, const int32_t *d_want, int nb, const Scratch &sc, int64_t nseg_all,
                  int64_t max_cap, int64_t norg_all, int64_t max_want, hipStream_t st);

#ifndef JFS_LZ4_SPLIT_RECORDS_ONLY

__device__ __forceinline__ Tok parse(const gc_u8 *s, int32_t n, int32_t x, bool want_off) {
    return parse_rd(s, n, x, want_off);
}

// The scratch and the grids were sized on the host from its own (src_len,
// dst_cap) copies (nseg_all, max_cap, norg_all).  A block whose device
// descriptor asks for more than that budget leaves -- it would overrun the
// segment or origin-map scratch -- is planned empty and marked bad, so the
// exact one-workgroup kernel decodes it from its descriptor instead.
// want (null: the full decode) is clamped to [0, cap] and to max_want, the
// bound the host sized the jump and gather grids with.
__global__ void plan_kernel(const jfs_dev_block *__restrict__ desc, const int32_t *__restrict__ want, int nb,
                            Scratch sc, int64_t nseg_all, int64_t max_cap, int64_t norg_all, int64_t max_want) {
    for (int i = threadIdx.x; i < nb * (int)(sizeof(BStat) / 4); i += blockDim.x) ((int32_t *)sc.st)[i] = 0;
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int32_t seg = 0;
        int64_t bits = 0, org = 0;
        for (int b = 0; b < nb; b++) {
            const jfs_dev_block d = ((const gc_blk *)desc)[b];
            SBlock &s = sc.blk[b];
            s.src = d.src;
            s.dst = d.dst;
            s.n = d.src && d.src_len > 0 ? d.src_len : 0;  // (a NULL src: planned empty, the exact kernel answers)
            s.cap = d.dst_cap > 0 ? d.dst_cap : 0;
            const int64_t ns = (s.n + SEG - 1) / SEG, no = ((int64_t)s.cap + 3) & ~3ll;
            if (s.cap > max_cap || seg + ns > nseg_all || org + no > norg_all || s.n >= LEN_CAP || s.cap >= LEN_CAP) {
                s.n = 0;
                s.cap = 0;
                sc.st[b].bad = 1;
            }
            const int64_t hi = s.cap < max_want ? (int64_t)s.cap : max_want, w = want ? (int64_t)want[b] : hi;
            s.want = (int32_t)(w < 0 ? 0 : w < hi ? w : hi);
            s.seg0 = seg;
            s.nseg = (s.n + SEG - 1) / SEG;
            s.bits_off = bits;
            s.org_off = org;
            seg += s.nseg;
            bits += (int64_t)s.nseg * (SEG / 32);
            org += ((int64_t)s.cap + 3) & ~3ll;
        }
    }
}

__global__ __launch_bounds__(T) void spec_kernel(int nb, int nseg_all, Scratch sc) {
    const int g = blockIdx.x * T + threadIdx.x;
    if (g >= nseg_all) return;
    const int b = block_of(sc.blk, nb, g);
    const SBlock B = sc.blk[b];
    const gc_u8 *s = (const gc_u8 *)B.src;
    const int32_t n = B.n, k = g - B.seg0;
    const int32_t s0 = k * SEG, s1 = s0 + SEG < n ? s0 + SEG : n;
    uint32_t m[SEG / 32];
#pragma unroll
    for (int w = 0; w < SEG / 32; w++) m[w] = 0;
    int32_t x = s0;
    while (x < s1) {
        const uint32_t rel = (uint32_t)(x - s0), w = rel >> 5, bit = 1u << (rel & 31);
#pragma unroll
        for (int i = 0; i < SEG / 32; i++) m[i] |= (w == (uint32_t)i) ? bit : 0u;
        x = parse(s, n, x, false).next;
    }
    g_u32 *bits = (g_u32 *)(sc.bits + B.bits_off + k * (SEG / 32));
#pragma unroll
    for (int i = 0; i < SEG / 32; i++) bits[i] = m[i];
    const int32_t ex = x < n ? x : n;
    sc.spec_exit[g] = ex;
    if (k + 1 < B.nseg) sc.entry[g + 1] = ex;
    if (k == 0) sc.entry[g] = 0;
}

// exit of segment (s0, s1) entered at x: walk until the chain meets a marked
// position (then it is the speculative chain, whose exit is known) or leaves
__device__ __forceinline__ int32_t seg_exit(const gc_u8 *s, int32_t n, int32_t s0, int32_t s1, int32_t x,
                                           const gc_u32 *bits, int32_t spec_ex) {
    while (x < s1) {
        const uint32_t rel = (uint32_t)(x - s0);
        if ((bits[rel >> 5] >> (rel & 31)) & 1u) return spec_ex;
        x = parse(s, n, x, false).next;
    }
    return x < n ? x : n;
}

// One fix-up round.  Inside a workgroup the segments' entries live in LDS and
// the workgroup iterates to its own fixed point (a token that spans several
// segments, or a speculative chain that never merged, moves the next entry;
// every iteration settles at least the lowest unsettled lane).  Only a changed
// entry that crosses into the next workgroup needs another round, so rounds
// count workgroup-boundary cascades, not segments.
__global__ __launch_bounds__(T) void fix_kernel(int nb, int nseg_all, Scratch sc, int round) {
    __shared__ int32_t ent[T];
    const int t = threadIdx.x;
    const int g = blockIdx.x * T + t;
    const bool valid = g < nseg_all;
    int b = 0;
    SBlock B{};
    int32_t k = 0;
    bool active = false;
    if (valid) {
        b = block_of(sc.blk, nb, g);
        B = sc.blk[b];
        k = g - B.seg0;
        active = k + 1 < B.nseg && !(round > 0 && !sc.st[b].fix[round - 1]);
    }
    const int32_t e0 = valid ? sc.entry[g] : 0;
    ent[t] = e0;
    const gc_u8 *s = (const gc_u8 *)B.src;
    const int32_t n = B.n, s0 = k * SEG, s1 = s0 + SEG < n ? s0 + SEG : n;
    const gc_u32 *bits = (const gc_u32 *)(sc.bits + B.bits_off + k * (SEG / 32));
    const int32_t spec_ex = active ? sc.spec_exit[g] : 0;
    int32_t last_in = -1, ex = -1;
    __syncthreads();
    for (int it = 0; it <= T; it++) {
        int changed = 0;
        if (active) {
            const int32_t e = ent[t];
            if (e != last_in) {
                last_in = e;
                ex = seg_exit(s, n, s0, s1, e, bits, spec_ex);
                if (t + 1 < T && ent[t + 1] != ex) {
                    ent[t + 1] = ex;
                    changed = 1;
                }
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
    if (valid && t > 0 && ent[t] != e0) sc.entry[g] = ent[t];
    if (active && t == T - 1 && sc.entry[g + 1] != ex) {  // the next workgroup's first entry
        sc.entry[g + 1] = ex;
        sc.st[b].fix[round] = 1;
    }
}

__global__ __launch_bounds__(T) void count_kernel(int nb, int nseg_all, Scratch sc) {
    const int g = blockIdx.x * T + threadIdx.x;
    if (g >= nseg_all) return;
    const int b = block_of(sc.blk, nb, g);
    if (sc.st[b].fix[FIX_ROUNDS - 1]) return;  // did not converge: exact path
    const SBlock B = sc.blk[b];
    const gc_u8 *s = (const gc_u8 *)B.src;
    const int32_t n = B.n, k = g - B.seg0;
    // (a segment the host counted for a block that was planned empty falls behind the last block's own: it has
    // no entry of this call, and whatever the scratch holds there is not a position to walk from)
    if (k >= B.nseg) return;
    const int32_t s0 = k * SEG, s1 = s0 + SEG < n ? s0 + SEG : n;
    int32_t x = sc.entry[g];
    int64_t c = 0;
    while (x < s1) {
        const Tok t = parse(s, n, x, false);
        c += (int64_t)t.ll + t.ml;
        if (c > B.cap) break;
        x = t.next;
    }
    sc.cnt[g] = (int32_t)(c <= B.cap ? c : (int64_t)B.cap + 1);
}

// one workgroup per block: cnt -> exclusive output offsets, block total
__global__ __launch_bounds__(T) void scan_kernel(Scratch sc) {
    const int b = blockIdx.x;
    const SBlock B = sc.blk[b];
    BStat &st = sc.st[b];
    if (st.fix[FIX_ROUNDS - 1]) return;
    __shared__ int64_t part[T];
    const int per = (B.nseg + T - 1) / T, t = threadIdx.x;
    const int i0 = B.seg0 + t * per, i1 = min(i0 + per, B.seg0 + B.nseg);
    int64_t a = 0;
    for (int i = i0; i < i1; i++) a += sc.cnt[i];
    part[t] = a;
    __syncthreads();
    for (int o = 1; o < T; o <<= 1) {
        const int64_t y = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += y;
        __syncthreads();
    }
    int64_t run = part[t] - a;
    for (int i = i0; i < i1; i++) {
        const int64_t c = sc.cnt[i];
        sc.cnt[i] = (int32_t)(run < B.cap ? run : B.cap);
        run += c;
    }
    if (t == T - 1) {
        if (part[t] > B.cap || B.n == 0 || B.cap == 0) st.bad = 1;
        st.total = (int32_t)(part[t] < B.cap ? part[t] : B.cap);
    }
}

// One WAVE per segment: the segment's true tokens are parsed wave-uniformly
// and each token's origin run is written by the whole wave (consecutive
// entries per lane: coalesced stores).  (One thread per segment wrote ~2 KB
// of scattered 16-byte stores each: 147 us of a lone 4 MiB block's 426.)
constexpr int EWV = T / 64;  // segments per workgroup
constexpr int ESTG = 1024;   // compressed bytes staged per segment (its tokens' fields, mostly)
constexpr int64_t EMIT_WAVE_MAX = 65536;  // segments (about 4 blocks of 4 MiB text)
// PREFIX: only the origin entries below the block's `want` are written, and a
// segment (or the rest of one) whose output starts at or above it is skipped
// when the block is longer than want (cut).  A block that ends within want is
// emitted whole, final token included: its last_ok is still required.
// WINDOW: the prefix form from the block's floor F (lz4_window.h): a segment
// whose output ends at or below F is skipped (unless the block ends within
// want and the segment reaches its end: the final token is still required), a
// token with no output byte in [F, want) is walked but not checked, and only
// the entries at or above F are written.
enum : int { FORM_FULL = 0, FORM_PREFIX = 1, FORM_WINDOW = 2 };
template <int FORM>
__global__ __launch_bounds__(T) void emit_kernel(int nb, int nseg_all, Scratch sc) {
    constexpr bool PREFIX = FORM != FORM_FULL, WINDOW = FORM == FORM_WINDOW;
    __shared__ alignas(16) uint8_t stg[EWV][ESTG];
    const int l = lane_id();
    const int g = (int)uniform((uint32_t)(blockIdx.x * EWV + (threadIdx.x >> 6)));
    if (g >= nseg_all) return;
    const int b = (int)uniform((uint32_t)block_of(sc.blk, nb, g));
    BStat &st = sc.st[b];
    if (st.fix[FIX_ROUNDS - 1] || st.bad) return;
    const SBlock B = sc.blk[b];
    const gc_u8 *s = (const gc_u8 *)(((uint64_t)uniform((uint32_t)((uint64_t)(uintptr_t)B.src >> 32)) << 32) |
                                     uniform((uint32_t)(uintptr_t)B.src));
    g_u32 *org = (g_u32 *)(sc.org + B.org_off);
    const int32_t n = (int32_t)uniform((uint32_t)B.n), cap = (int32_t)uniform((uint32_t)B.cap),
                  k = g - (int32_t)uniform((uint32_t)B.seg0);
    if (k >= (int32_t)uniform((uint32_t)B.nseg)) return;  // (behind the last block's own segments: see count_kernel)
    const int32_t s0 = k * SEG, s1 = s0 + SEG < n ? s0 + SEG : n;
    int32_t x = (int32_t)uniform((uint32_t)sc.entry[g]), op = (int32_t)uniform((uint32_t)sc.cnt[g]);
    const int32_t want = PREFIX ? (int32_t)uniform((uint32_t)B.want) : cap;
    const bool cut = PREFIX && want < (int32_t)uniform((uint32_t)st.total);
    if (cut && op >= want) return;
    const int32_t F = WINDOW ? (int32_t)uniform((uint32_t)(st.below ? 0 : st.fc)) : 0;
    if (WINDOW) {
        const int32_t total = (int32_t)uniform((uint32_t)st.total);
        const int32_t end = k + 1 < (int32_t)uniform((uint32_t)B.nseg) ? (int32_t)uniform((uint32_t)sc.cnt[g + 1]) : total;
        if (end <= F && (cut || end < total)) return;
    }
    // the parse reads the segment's bytes from LDS (one wave-uniform LDS round
    // trip per field instead of an L2 one); bytes past the staging from HBM
    uint8_t *buf = stg[threadIdx.x >> 6];
    const uintptr_t a0 = ((uintptr_t)(s + s0)) & ~(uintptr_t)15, aend = (uintptr_t)(s + n);
    {
        const uintptr_t a = a0 + 16u * (uint32_t)l;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (a < aend) v = *(const gc_u4 *)a;  // (an aligned chunk holding a valid byte: same page)
        *(uint4 *)(buf + 16 * l) = v;
        __builtin_amdgcn_wave_barrier();
    }
    struct Rd {
        const gc_u8 *s;
        const uint8_t *buf;
        int32_t A;  // stream position of buf[0] (a0 - s: s0 less its misalignment)
        __device__ uint32_t operator[](int32_t p) const {  // (p wave-uniform: scalar branch)
            const uint32_t r = (uint32_t)(p - A);
            uint32_t v;
            if (r < (uint32_t)ESTG) v = buf[r];
            else v = s[p];
            return uniform(v);
        }
    } rd{s, buf, s0 - (int32_t)((uintptr_t)(s + s0) & 15u)};
    while (x < s1) {
        const Tok t = parse_rd(rd, n, x, true);
        if (WINDOW && !t.last && !lz4w::visited(F, want, op, t.ll + t.ml)) {  // (in front of F: unseen)
            op += t.ll + t.ml;
            x = t.next;
            continue;
        }
        const bool ok = tok_ok(t.tok, t, n, op, cap);
        if (!ok) {
            if (l == 0) st.bad = ends_in_match(t, n) ? 2 : 1;
            return;
        }
        const uint32_t v0 = om::lit_entry(t.lenip);  // literal entry i = v0 - i
        // (PREFIX: the entries below want; want - op <= 0 leaves none.  WINDOW: and at or above F)
        const int32_t ll = PREFIX ? min(t.ll, want - op) : t.ll;
        for (int32_t i = l + (WINDOW ? lz4w::clip(op, t.ll, F, want).i0 : 0); i < ll; i += 64) org[op + i] = v0 - (uint32_t)i;
        op += t.ll;
        if (t.last) {
            if (l == 0) st.last_ok = 1;
            return;
        }
        const int32_t ml = PREFIX ? min(t.ml, want - op) : t.ml;
        // match entry i = op - off + (i mod off): overlapped matches point before the match
        const int32_t base = op - t.off;
        const uint32_t off = (uint32_t)t.off;
        const int32_t m0 = WINDOW ? lz4w::clip(op, t.ml, F, want).i0 : 0;
        if (off >= (uint32_t)t.ml) {  // no overlap (most matches): no modulo
            for (int32_t i = l + m0; i < ml; i += 64) org[op + i] = (uint32_t)(base + i);
        } else {
            for (int32_t i = l + m0; i < ml; i += 64) {
                const uint32_t ui = (uint32_t)i;
                org[op + i] = (uint32_t)(base + (ui < off ? ui : ui % off));
            }
        }
        op += t.ml;
        x = t.next;
        if (cut && op >= want) return;
    }
}

// One THREAD per segment (large batches: 64 segments per wave do the most
// work per instruction; the wave form above wins only while the segments are
// too few to fill the GPU -- a 16-block chunk ran 20 % slower in it).
template <int FORM>
__global__ __launch_bounds__(T) void emit_thread_kernel(int nb, int nseg_all, Scratch sc) {
    constexpr bool PREFIX = FORM != FORM_FULL, WINDOW = FORM == FORM_WINDOW;
    const int g = blockIdx.x * T + threadIdx.x;
    if (g >= nseg_all) return;
    const int b = block_of(sc.blk, nb, g);
    BStat &st = sc.st[b];
    if (st.fix[FIX_ROUNDS - 1] || st.bad) return;
    const SBlock B = sc.blk[b];
    const gc_u8 *s = (const gc_u8 *)B.src;
    g_u32 *org = (g_u32 *)(sc.org + B.org_off);
    const int32_t n = B.n, cap = B.cap, k = g - B.seg0;
    if (k >= B.nseg) return;  // (behind the last block's own segments: see count_kernel)
    const int32_t s0 = k * SEG, s1 = s0 + SEG < n ? s0 + SEG : n;
    int32_t x = sc.entry[g], op = sc.cnt[g];
    const int32_t want = PREFIX ? B.want : cap;
    const bool cut = PREFIX && want < st.total;
    if (cut && op >= want) return;
    const int32_t F = WINDOW ? (st.below ? 0 : st.fc) : 0;
    if (WINDOW) {
        const int32_t end = k + 1 < B.nseg ? sc.cnt[g + 1] : st.total;
        if (end <= F && (cut || end < st.total)) return;
    }
    while (x < s1) {
        const Tok t = parse(s, n, x, true);
        if (WINDOW && !t.last && !lz4w::visited(F, want, op, t.ll + t.ml)) {  // (in front of F: unseen)
            op += t.ll + t.ml;
            x = t.next;
            continue;
        }
        const bool ok = tok_ok(t.tok, t, n, op, cap);
        if (!ok) {
            st.bad = ends_in_match(t, n) ? 2 : 1;
            return;
        }
        // (PREFIX: the entries below want; want - op <= 0 leaves none.  WINDOW: and at or above F)
        if (WINDOW) {
            const lz4w::Clip c = lz4w::clip(op, t.ll, F, want);
            if (c.i1 > c.i0) om::put_lits(org, op + c.i0, c.i1 - c.i0, om::lit_entry(t.lenip + c.i0));
        } else {
            om::put_lits(org, op, PREFIX ? min(t.ll, want - op) : t.ll, om::lit_entry(t.lenip));
        }
        op += t.ll;
        if (t.last) {
            st.last_ok = 1;
            return;
        }
        if (WINDOW) {
            const lz4w::Clip c = lz4w::clip(op, t.ml, F, want);
            if (c.i1 > c.i0) om::put_match<int32_t, true>(org, op, c.i1, (uint32_t)t.off, c.i0);
        } else {
            om::put_match(org, op, PREFIX ? min(t.ml, want - op) : t.ml, (uint32_t)t.off);
        }
        op += t.ml;
        x = t.next;
        if (cut && op >= want) return;
    }
}

// Window decode, after the index steps: the window's clamps, per block, from
// the descriptor (a block over the host's sizes was planned empty, and the
// hand-over decodes it from its descriptor): lo' = max(lo, 0), hi' = min(hi,
// dst_cap).  An empty window (hi' <= lo') becomes want = 0, for this path and
// for the hand-over: the prefix decode's answer for it is the window's (0
// behind the early answers, nothing written).  Any other block is tried at
// the floor Fc(lo'); its want is the plan's (hi' within the host's bounds).
__global__ void window_plan_kernel(const jfs_dev_block *__restrict__ desc, const int32_t *__restrict__ lo,
                                   const int32_t *__restrict__ hi, int nb, Scratch sc) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const int32_t cap = ((const gc_blk *)desc)[b].dst_cap;
    const int32_t l = lo[b] > 0 ? lo[b] : 0, h = hi[b] < cap ? hi[b] : cap;
    const bool empty = h <= l;
    if (empty) sc.blk[b].want = 0;
    sc.hwant[b] = empty ? 0 : h;
    sc.st[b].fc = empty ? 0 : lz4w::floor_of(l);
}

// Window decode: the probe.  One lane per segment whose output meets [Fc, H):
// it walks the segment's true tokens, as the count does, and flags the block
// when a sequence reaches below Fc (lz4_window.h).  Segments in front of Fc or
// behind H are not walked: the probe reads compressed bytes of the window only.
// An offset it reads is unchecked: whatever it holds, the flag only ever sends
// the block to floor 0, and the emit checks every token the window visits.
__global__ __launch_bounds__(T) void probe_kernel(int nb, int nseg_all, Scratch sc) {
    const int g = blockIdx.x * T + threadIdx.x;
    if (g >= nseg_all) return;
    const int b = block_of(sc.blk, nb, g);
    BStat &st = sc.st[b];
    const int32_t F = st.fc;
    if (F <= 0 || st.fix[FIX_ROUNDS - 1] || st.bad) return;
    const SBlock B = sc.blk[b];
    const int32_t n = B.n, k = g - B.seg0, H = B.want;
    if (k >= B.nseg) return;  // (behind the last block's own segments: see count_kernel)
    int32_t op = sc.cnt[g];
    const int32_t end = k + 1 < B.nseg ? sc.cnt[g + 1] : st.total;
    if (end <= F || op >= H) return;
    const gc_u8 *s = (const gc_u8 *)B.src;
    const int32_t s0 = k * SEG, s1 = s0 + SEG < n ? s0 + SEG : n;
    int32_t x = sc.entry[g];
    while (x < s1 && op < H) {
        const Tok t = parse(s, n, x, true);
        if (t.last) return;
        op += t.ll;  // (the count kept the block's total within cap < 2^30: no sum here overflows)
        if (lz4w::reaches_below(F, H, op, t.ml, t.off)) {
            st.below = 1;
            return;
        }
        op += t.ml;
        x = t.next;
    }
}

// grid (x: workgroups per block, y: block)
template <bool WINDOW>
__global__ __launch_bounds__(T) void jump_kernel(Scratch sc, int round) {
    const int b = blockIdx.y;
    BStat &st = sc.st[b];
    if (st.fix[FIX_ROUNDS - 1] || st.bad) return;
    if (round > 0 && !st.jmp[round - 1]) return;
    const SBlock B = sc.blk[b];
    const int64_t total = min(st.total, B.want);  // (the entries the emit wrote; the full decode: st.total)
    g_u32 *org = (g_u32 *)(sc.org + B.org_off);
    if (!WINDOW) {
        if (om::jump_walk(org, total, ((int64_t)blockIdx.x * T + threadIdx.x) * 4, (int64_t)gridDim.x * T * 4,
                          [org](int32_t o) -> uint32_t { return org[o]; }))
            st.jmp[round] = 1;
    } else {
        // (the floor rule keeps every pointer of [F, total) inside it; one that is not is left standing, never
        // followed into entries no one wrote, and the gather then hands the block over)
        const int32_t F = st.below ? 0 : st.fc, E = (int32_t)total;
        if (om::jump_walk<true>(org, total, ((int64_t)blockIdx.x * T + threadIdx.x) * 4, (int64_t)gridDim.x * T * 4,
                                [org, F, E](int32_t o) -> uint32_t { return o >= F && o < E ? org[o] : (uint32_t)o; }, F))
            st.jmp[round] = 1;
    }
}

// window decode, on the current device since the last reset: blocks decoded from a floor above 0, blocks whose
// probe sent them to floor 0, blocks handed to the exact kernel, origin entries written
__device__ unsigned long long g_window_counts[4];

// blocks decoded by this path / handed to the exact kernel (diagnostics)
__device__ unsigned long long g_split_counts[6];

// per block: the verdict (exact path or not) and the result of the good ones
template <bool WINDOW>
__global__ void verdict_kernel(int nb, Scratch sc, int32_t *__restrict__ ret, int32_t *__restrict__ todo) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    BStat &st = sc.st[b];
    // (a block cut at want never reaches its final token: no last_ok to ask for)
    const int32_t want = sc.blk[b].want;
    const bool bad = st.bad || (!st.last_ok && st.total <= want) || st.fix[FIX_ROUNDS - 1] || st.unsettled;
    st.todo = bad;
    todo[b] = bad;
    if (!bad) ret[b] = min(st.total, want);
    atomicAdd(&g_split_counts[bad ? 1 : 0], 1ull);
    // why a block was handed over: fix-up / jumping did not converge, a token
    // outside the proven cases, no final literal run
    if (st.fix[FIX_ROUNDS - 1]) atomicAdd(&g_split_counts[2], 1ull);
    else if (st.bad == 1) atomicAdd(&g_split_counts[4], 1ull);
    else if (st.bad || (!st.last_ok && st.total <= want)) atomicAdd(&g_split_counts[5], 1ull);
    else if (st.unsettled) atomicAdd(&g_split_counts[3], 1ull);
    if (WINDOW) {
        const int32_t F = st.below ? 0 : st.fc;
        if (!bad && F > 0) atomicAdd(&g_window_counts[0], 1ull);
        if (st.below) atomicAdd(&g_window_counts[1], 1ull);
        if (bad) atomicAdd(&g_window_counts[2], 1ull);
        else if (min(st.total, want) > F) atomicAdd(&g_window_counts[3], (unsigned long long)(min(st.total, want) - F));
    }
}

// (runs before the verdict: an entry that is still not a literal flags its
// block, whose output the exact kernel then rewrites whole)
// (WINDOW: the quads are counted from the floor's; no byte below the floor is written)
template <bool WINDOW>
__global__ __launch_bounds__(T) void gather_kernel(Scratch sc) {
    const int b = blockIdx.y;
    BStat &st = sc.st[b];
    const SBlock B = sc.blk[b];
    if (st.bad || (!st.last_ok && st.total <= B.want) || st.fix[FIX_ROUNDS - 1]) return;  // (entries not all written: never read)
    const int64_t F = WINDOW ? (st.below ? 0 : st.fc) : 0;
    const int64_t p = (F & ~(int64_t)3) + ((int64_t)blockIdx.x * T + threadIdx.x) * 4;
    const int64_t total = min(st.total, B.want);  // no byte at or above it is written
    if (p >= total) return;
    const gc_u32 *org = (const gc_u32 *)(sc.org + B.org_off);
    if (!om::gather_quad<WINDOW>(org, (const gc_u8 *)B.src, (g_u8 *)B.dst, p, total, F)) st.unsettled = 1;
}

#endif  // JFS_LZ4_SPLIT_RECORDS_ONLY

}  // namespace lz4s
}  // namespace jfs

#ifndef JFS_LZ4_SPLIT_RECORDS_ONLY

using namespace jfs::lz4s;
namespace om = jfs::om;

// Scratch layout: carves the areas from d_scratch (null: only the size
// counts) and returns the bytes it takes, for the host's size query and the launcher.
void jfs::lz4s::carve_index(om::Carve &c, int64_t nb, int64_t nseg_all, Scratch &sc) {
    c.take(sc.blk, nb * (int64_t)sizeof(SBlock));
    c.take(sc.st, nb * (int64_t)sizeof(BStat));
    c.take(sc.spec_exit, nseg_all * 4);
    c.take(sc.entry, nseg_all * 4);
    c.take(sc.cnt, nseg_all * 4);
    c.take(sc.bits, nseg_all * (SEG / 8));
    sc.org = nullptr;
    sc.hwant = nullptr;
}

static int64_t layout(void *d_scratch, int64_t nb, int64_t nseg_all, int64_t norg_all, Scratch &sc, int32_t *&todo) {
    om::Carve c(d_scratch);
    carve_index(c, nb, nseg_all, sc);
    c.take(todo, nb * 4);
    c.take(sc.hwant, nb * 4);
    c.take(sc.org, norg_all * 4);
    return c.bytes;
}

void jfs::lz4s::launch_index(const jfs_dev_block *d_desc, const int32_t *d_want, int nb, const Scratch &sc,
                             int64_t nseg_all, int64_t max_cap, int64_t norg_all, int64_t max_want, hipStream_t st) {
    const int gs = (int)((nseg_all + T - 1) / T);
    hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(T), 0, st, d_desc, d_want, nb, sc, nseg_all, max_cap, norg_all, max_want);
    if (nseg_all > 0) {
        hipLaunchKernelGGL(spec_kernel, dim3(gs), dim3(T), 0, st, nb, (int)nseg_all, sc);
        for (int r = 0; r < FIX_ROUNDS; r++) hipLaunchKernelGGL(fix_kernel, dim3(gs), dim3(T), 0, st, nb, (int)nseg_all, sc, r);
        hipLaunchKernelGGL(count_kernel, dim3(gs), dim3(T), 0, st, nb, (int)nseg_all, sc);
    }
    hipLaunchKernelGGL(scan_kernel, dim3(nb), dim3(T), 0, st, sc);
}

extern "C" int64_t jfs_lz4_split_scratch_bytes(int nb, const int32_t *src_len, const int32_t *cap) {
    int64_t seg = 0, org = 0;
    for (int b = 0; b < nb; b++) {
        const int64_t n = src_len[b] > 0 ? src_len[b] : 0, c = cap[b] > 0 ? cap[b] : 0;
        seg += (n + SEG - 1) / SEG;
        org += (c + 3) & ~3ll;
    }
    Scratch sc;
    int32_t *todo;
    return layout(nullptr, nb, seg, org, sc, todo);
}

// nseg_all / max_cap: Σ segments and the largest dst_cap (grid sizes); the
// host computes both from the same (src_len, cap) it sized the scratch with.
// d_want (null: the full decode): the output bytes asked for per block;
// max_want: an upper bound of them on the host (at most max_cap), which sizes
// the jump and gather grids -- the device values are clamped to it.
// FORM_WINDOW: d_want is the windows' upper ends and d_lo their lower ends.
template <int FORM>
static int launch_split(const jfs_dev_block *d_desc, int nb, int32_t *d_ret, const int32_t *d_want, void *d_scratch,
                        int64_t nseg_all, int64_t max_cap, int64_t norg_all, int64_t max_want, hipStream_t st,
                        const int32_t *d_lo = nullptr) {
    constexpr bool PREFIX = FORM != FORM_FULL, WINDOW = FORM == FORM_WINDOW;
    if (nb <= 0) return 0;
    max_want = std::max<int64_t>(0, std::min(max_want, max_cap));
    Scratch sc;
    int32_t *todo;
    layout(d_scratch, nb, nseg_all, norg_all, sc, todo);
    const int gs = (int)((nseg_all + T - 1) / T);
    launch_index(d_desc, d_want, nb, sc, nseg_all, max_cap, norg_all, max_want, st);
    if (WINDOW) {
        hipLaunchKernelGGL(window_plan_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, d_desc, d_lo, d_want, nb, sc);
        if (nseg_all > 0) hipLaunchKernelGGL(probe_kernel, dim3((unsigned)gs), dim3(T), 0, st, nb, (int)nseg_all, sc);
    }
    if (nseg_all > 0) {
        // a wave per segment while that leaves the GPU short of waves (a lone
        // block: ~16 k segments), a thread per segment beyond
        if (nseg_all <= EMIT_WAVE_MAX)
            hipLaunchKernelGGL(emit_kernel<FORM>, dim3((unsigned)((nseg_all + EWV - 1) / EWV)), dim3(T), 0, st, nb, (int)nseg_all, sc);
        else
            hipLaunchKernelGGL(emit_thread_kernel<FORM>, dim3((unsigned)gs), dim3(T), 0, st, nb, (int)nseg_all, sc);
    }
    const unsigned jx = om::jump_groups(max_want, nb);
    const int jr = om::launch_rounds(max_want, 4);
    for (int r = 0; r < jr; r++) hipLaunchKernelGGL(jump_kernel<WINDOW>, dim3(jx, (unsigned)nb), dim3(T), 0, st, sc, r);
    hipLaunchKernelGGL(gather_kernel<WINDOW>, dim3(om::quad_groups(max_want), (unsigned)nb), dim3(T), 0, st, sc);
    hipLaunchKernelGGL(verdict_kernel<WINDOW>, dim3((nb + 63) / 64), dim3(64), 0, st, nb, sc, d_ret, todo);
    if (hipGetLastError() != hipSuccess) return -1;
    // the exact one-workgroup kernel for the flagged blocks (the others exit at once)
    if (WINDOW) return jfs_launch_lz4_decode_prefix(d_desc, nb, d_ret, sc.hwant, todo, st);
    if (PREFIX) return jfs_launch_lz4_decode_prefix(d_desc, nb, d_ret, d_want, todo, st);
    return jfs_launch_lz4_decode_todo(d_desc, nb, d_ret, todo, st);
}

extern "C" int jfs_launch_lz4_split(const jfs_dev_block *d_desc, int nb, int32_t *d_ret, void *d_scratch,
                                    int64_t nseg_all, int64_t max_cap, int64_t norg_all, hipStream_t st) {
    return launch_split<FORM_FULL>(d_desc, nb, d_ret, nullptr, d_scratch, nseg_all, max_cap, norg_all, max_cap, st);
}

extern "C" int jfs_launch_lz4_split_prefix(const jfs_dev_block *d_desc, int nb, int32_t *d_ret, const int32_t *d_want,
                                           void *d_scratch, int64_t nseg_all, int64_t max_cap, int64_t norg_all,
                                           int64_t max_want, hipStream_t st) {
    if (!d_want) return -1;
    return launch_split<FORM_PREFIX>(d_desc, nb, d_ret, d_want, d_scratch, nseg_all, max_cap, norg_all, max_want, st);
}

// d_lo / d_hi: the windows (device); max_want: an upper bound of the hi on the host, as the prefix launcher's
extern "C" int jfs_launch_lz4_split_window(const jfs_dev_block *d_desc, int nb, int32_t *d_ret, const int32_t *d_lo,
                                           const int32_t *d_hi, void *d_scratch, int64_t nseg_all, int64_t max_cap,
                                           int64_t norg_all, int64_t max_want, hipStream_t st) {
    if (!d_lo || !d_hi) return -1;
    return launch_split<FORM_WINDOW>(d_desc, nb, d_ret, d_hi, d_scratch, nseg_all, max_cap, norg_all, max_want, st, d_lo);
}

extern "C" int jfs_lz4_window_counts(uint64_t out[4], int reset) {
    if (!out) return -1;
    unsigned long long v[4] = {0, 0, 0, 0};
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_window_counts), sizeof(v)) != hipSuccess) return -1;
    for (int i = 0; i < 4; i++) out[i] = v[i];
    if (reset) {
        unsigned long long z[4] = {0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_window_counts), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}

// Test hook (include/jfs_gpucodec_test.h)
extern "C" int jfs_test_set_split_jump_rounds(int lz4_rounds, int zstd_rounds) {
    om::test_rounds[0] = std::max(0, std::min(lz4_rounds, om::MAX_ROUNDS));
    om::test_rounds[1] = std::max(0, std::min(zstd_rounds, om::MAX_ROUNDS));
    return 0;
}

// Diagnostics: blocks the small-batch path decoded itself (out[0]) and blocks
// it handed to the exact kernel (out[1]) on the current device since the
// last reset; synchronous.
extern "C" int jfs_lz4_split_counts(uint64_t *out, int reset) {
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_split_counts), sizeof(v)) != hipSuccess) return -1;
    for (int i = 0; i < 6; i++) out[i] = v[i];
    if (reset) {
        unsigned long long z[6] = {0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_split_counts), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}

#endif  // JFS_LZ4_SPLIT_RECORDS_ONLY
