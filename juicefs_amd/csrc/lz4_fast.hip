// Fast LZ4 encode: valid LZ4 blocks, not liblz4's bytes.  Every
// block is cut into independent 64 KiB chunks; one wave parses a chunk 64
// positions at a time (parse), one thread per block turns the chunks' sequence
// lists into output offsets and the block's size (stitch), and one wave per
// chunk writes the bytes of the blocks that fit (emit).  lz4_fast_host.cc
// restates the parse on the host and gives the same bytes.
// The LIFT form (jfs_launch_lz4_fast_lift; lz4_lift.h) runs
// lz4_lift.hip's kernels between plan and parse: they fill the parse results of
// the chunks whose records a compaction source's stored stream already holds,
// and parse_kernel<true> returns at once for those.
#include "jfs_internal.h"
#include "lz4_fast.h"
#include "wave.cuh"

#include <algorithm>

namespace jfs {
namespace lz4f {

typedef JFS_GLOBAL int32_t g_i32;
typedef JFS_GLOBAL const int32_t gc_i32;
typedef JFS_GLOBAL uint2 g_u2;

constexpr int kCapLen = kMinMatch + kTile;  // a lane extends its own match this far; longer ones end the tile
constexpr int kGroupChunks = 8192;          // chunks parsed per launch group (bounds the scratch: 1 GiB of records)
constexpr int kInlineLits = 16;             // emit: a lane copies this many literals itself
constexpr int kInlineLenBytes = 8;          // emit: and writes this many length bytes itself

// scratch views of one launch group (B blocks, at most C chunks)
struct Ctl {
    int nblk, cap_chunks;
    int32_t *cfirst;                                      // [B + 1] first chunk of every block
    int32_t *nrec, *tail, *lit0, *body;                   // [C] parse results
    int32_t *start, *cin, *delta;                         // [C] stitch results
    int32_t *fin_off, *fin_lit;                           // [B] the block's last (literal-only) sequence; off < 0: no emit
    uint2 *recs;                                          // [C * kMaxRec] {pos | mlen << 16, off | lit << 16}
    const int32_t *lifted;                                // [C] the LIFT form: the chunk's results are in place
};

__device__ __forceinline__ uint32_t ld32u(const gc_u8 *p) {
    uintptr_t a = (uintptr_t)p;
    const gc_u32 *w = (const gc_u32 *)(a & ~(uintptr_t)3);
    uint32_t sh = (uint32_t)(a & 3);
    uint32_t w0 = w[0];
    if (sh == 0) return w0;
    uint32_t w1 = w[1];
    return __builtin_amdgcn_alignbyte(w1, w0, sh);
}

__device__ __forceinline__ bool block_ok(int64_t n, int nc) { return n >= 0 && n <= kMaxInput && nc == (int)nchunks(n); }

// the block that owns chunk g: the last b with cfirst[b] <= g < cfirst[b + 1]
__device__ __forceinline__ int find_block(gc_i32 *cfirst, int nblk, int g) {
    int lo = 0, hi = nblk;  // cfirst[lo] <= g < cfirst[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cfirst[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Chunk counts and their prefix over the group's blocks.  A block the scratch
// has no room for (the host's lengths did not match the descriptors) gets
// fewer chunks than it needs, which every later kernel reads as "failed".
__global__ __launch_bounds__(256) void plan_kernel(const jfs_dev_block *__restrict__ blocks_, Ctl c) {
    __shared__ uint32_t part[256];
    gc_blk *blocks = (gc_blk *)blocks_;
    g_i32 *cfirst = (g_i32 *)c.cfirst;
    const int t = threadIdx.x, per = (c.nblk + 255) / 256;
    const int lo = t * per < c.nblk ? t * per : c.nblk, hi = lo + per < c.nblk ? lo + per : c.nblk;
    uint32_t sum = 0;
    for (int b = lo; b < hi; ++b) {
        const int64_t n = blocks[b].src_len;
        sum += n >= 0 && n <= kMaxInput ? (uint32_t)nchunks(n) : 0u;
    }
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const uint32_t v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    uint32_t run = part[t];
    const uint32_t cap = (uint32_t)c.cap_chunks;
    for (int b = lo; b < hi; ++b) {
        const int64_t n = blocks[b].src_len;
        cfirst[b] = (int32_t)(run < cap ? run : cap);
        run += n >= 0 && n <= kMaxInput ? (uint32_t)nchunks(n) : 0u;
    }
    if (hi == c.nblk) cfirst[c.nblk] = (int32_t)(run < cap ? run : cap);  // every such thread holds the total
}

template <bool LIFT>
__global__ __launch_bounds__(64) void parse_kernel(const jfs_dev_block *__restrict__ blocks_, Ctl c) {
    __shared__ uint16_t tab[1 << kHashLog];
    gc_blk *blocks = (gc_blk *)blocks_;
    gc_i32 *cfirst = (gc_i32 *)c.cfirst;
    const int lane = lane_id();
    const int g = (int)blockIdx.x;
    if (g >= cfirst[c.nblk]) return;
    if (LIFT && ((gc_i32 *)c.lifted)[g]) return;  // (the lift left this chunk's records and counts)
    const int b = find_block(cfirst, c.nblk, g);
    const int64_t n = blocks[b].src_len;
    if (!block_ok(n, cfirst[b + 1] - cfirst[b])) return;
    const int64_t cbase = (int64_t)(g - cfirst[b]) << kChunkLog;
    const int clen = (int)(n - cbase < kChunk ? n - cbase : kChunk);
    gc_u8 *src = (gc_u8 *)blocks[b].src + cbase;
    g_u2 *recs = (g_u2 *)c.recs + (int64_t)g * kMaxRec;
    for (int i = lane; i < (1 << kHashLog) / 2; i += 64) ((uint32_t *)tab)[i] = 0;
    __syncthreads();
    // the block's end rules in chunk coordinates (see the twin)
    const int64_t mend64 = n - kLastLits - cbase, slim64 = n - kMfLimit - cbase;
    const int mend = (int)(clen < mend64 ? clen : mend64);
    const int slim = (int)(clen - kMinMatch < slim64 ? clen - kMinMatch : slim64);
    int anchor = 0, cur = 0, nrec = 0, lit0 = 0;
    uint32_t body = 0;
    for (int t0 = 0; t0 <= slim;) {
        const int p = t0 + lane;
        const bool act = p <= slim;
        uint32_t v = 0, h = 0;
        int cand = -1, len = 0;
        if (act) {
            if (p >= kNear) {
                // bytes [p - 4, p + 4): p + 10 < n, so the three dwords lie inside the block
                const uintptr_t a = (uintptr_t)(src + p - 4);
                const gc_u32 *w = (const gc_u32 *)(a & ~(uintptr_t)3);
                const uint32_t sh = (uint32_t)(a & 3);
                const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
                const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sh);
                v = __builtin_amdgcn_alignbyte(w2, w1, sh);
                const uint64_t win = (uint64_t)v << 32 | lo;
                if ((uint32_t)(win >> 24) == v) cand = p - 1;
                else if ((uint32_t)(win >> 16) == v) cand = p - 2;
                else if ((uint32_t)(win >> 8) == v) cand = p - 3;
                else if (lo == v) cand = p - 4;
            } else {
                v = ld32u(src + p);
            }
            h = hash4(v);
            if (cand < 0) {
                const int e = tab[h];
                if (e < p && ld32u(src + e) == v) cand = e;
            }
            if (cand >= 0) {
                const int limit = mend - p < kCapLen ? mend - p : kCapLen;
                len = kMinMatch;
                while (len < limit) {
                    const uint32_t x = ld32u(src + p + len) ^ ld32u(src + cand + len);
                    if (x) {
                        len += (int)(__builtin_ctz(x) >> 3);
                        break;
                    }
                    len += 4;
                }
                len = len < limit ? len : limit;
            }
        }
        // greedy choice in position order
        const uint64_t have = __ballot(cand >= 0);
        for (;;) {
            const int rel = cur - t0;
            const uint64_t m = rel <= 0 ? have : (rel >= 64 ? 0ull : have & (~0ull << rel));
            if (!m) break;
            const int l = __ffsll((unsigned long long)m) - 1;
            const int pl = t0 + l;
            const int cl = (int)lane_read((uint32_t)cand, l);
            int ml = (int)lane_read((uint32_t)len, l);
            if (ml == kCapLen && pl + ml < mend) {
                // the whole wave extends this one: 256 bytes a step
                for (;;) {
                    const int q = pl + ml + 4 * lane;
                    int eq = 0;
                    if (q < mend) {
                        const uint32_t x = ld32u(src + q) ^ ld32u(src + cl + ml + 4 * lane);
                        eq = x ? (int)(__builtin_ctz(x) >> 3) : 4;
                        eq = eq < mend - q ? eq : mend - q;
                    }
                    const uint64_t stop = __ballot(eq < 4);
                    if (stop) {
                        const int f = __ffsll((unsigned long long)stop) - 1;
                        ml += 4 * f + (int)lane_read((uint32_t)eq, f);
                        break;
                    }
                    ml += 256;
                }
            }
            const int lit = pl - anchor;
            if (lane == 0 && nrec < kMaxRec)
                recs[nrec] = make_uint2((uint32_t)pl | (uint32_t)ml << 16, (uint32_t)(pl - cl) | (uint32_t)lit << 16);
            body += (uint32_t)(1 + lit + 2 + len_bytes(ml - kMinMatch) + (nrec ? len_bytes(lit) : 0));
            if (!nrec) lit0 = lit;
            ++nrec;
            anchor = cur = pl + ml;
        }
        // insert: the highest position of the tile wins a table entry, whatever
        // order the lanes' writes land in
        bool pend = act;
        while (__ballot(pend)) {
            if (pend) tab[h] = (uint16_t)p;
            __syncthreads();
            if (pend) pend = tab[h] < p;
            __syncthreads();
        }
        t0 = t0 + kTile > cur ? t0 + kTile : cur;
    }
    if (lane == 0) {
        ((g_i32 *)c.nrec)[g] = nrec < kMaxRec ? nrec : kMaxRec;
        ((g_i32 *)c.tail)[g] = clen - anchor;
        ((g_i32 *)c.lit0)[g] = lit0;
        ((g_i32 *)c.body)[g] = (int32_t)body;
    }
}

// One thread per block: where every chunk's first token goes once the literals
// left over by the chunks before it have joined its first sequence.
__global__ __launch_bounds__(64) void stitch_kernel(const jfs_dev_block *__restrict__ blocks_, Ctl c,
                                                    int32_t *__restrict__ ret_) {
    gc_blk *blocks = (gc_blk *)blocks_;
    gc_i32 *cfirst = (gc_i32 *)c.cfirst;
    gc_i32 *nrec = (gc_i32 *)c.nrec, *tail = (gc_i32 *)c.tail, *lit0 = (gc_i32 *)c.lit0, *body = (gc_i32 *)c.body;
    g_i32 *start = (g_i32 *)c.start, *cin = (g_i32 *)c.cin, *delta = (g_i32 *)c.delta;
    g_i32 *ret = (g_i32 *)ret_;
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= c.nblk) return;
    const int64_t n = blocks[b].src_len, cap = blocks[b].dst_cap;
    const int c0 = cfirst[b], nc = cfirst[b + 1] - c0;
    ((g_i32 *)c.fin_off)[b] = -1;
    if (!block_ok(n, nc)) {
        ret[b] = 0;
        return;
    }
    int64_t off = 0, carry = 0;
    int pend0 = 0;  // chunks [pend0, ci) hold literals of the sequence not yet placed
    for (int ci = 0; ci < nc; ++ci) {
        const int g = c0 + ci;
        if (nrec[g] == 0) {
            carry += tail[g];
            continue;
        }
        const int64_t L = carry + lit0[g];
        const int64_t lit_area = off + 1 + len_bytes(L);
        const int64_t S = ((int64_t)ci << kChunkLog) - carry;  // block position of the sequence's first literal
        for (int k = pend0; k < ci; ++k) delta[c0 + k] = (int32_t)(lit_area - S);
        start[g] = (int32_t)off;
        cin[g] = (int32_t)carry;
        off += (int64_t)(uint32_t)body[g] + carry + len_bytes(L);
        carry = tail[g];
        pend0 = ci;
    }
    const int64_t lit_area = off + 1 + len_bytes(carry);
    for (int k = pend0; k < nc; ++k) delta[c0 + k] = (int32_t)(lit_area - (n - carry));
    const int64_t total = lit_area + carry;
    const bool fits = total <= cap;
    ret[b] = fits ? (int32_t)total : 0;
    if (fits) {
        ((g_i32 *)c.fin_off)[b] = (int32_t)off;
        ((g_i32 *)c.fin_lit)[b] = (int32_t)carry;
    }
}

struct Out {
    g_u8 *dst;
    int64_t cap;
    gc_u8 *src;  // the block
    int64_t n;
};

__device__ __forceinline__ void put(const Out &o, int64_t at, uint32_t v) {
    if (at >= 0 && at < o.cap) o.dst[at] = (uint8_t)v;
}

__device__ __forceinline__ int64_t bcast64(int64_t v, int l) {
    const uint32_t lo = lane_read((uint32_t)v, l), hi = lane_read((uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)((uint64_t)hi << 32 | lo);
}

// the length bytes of `v` (>= 15) at `at`, by the whole wave
__device__ void fill_len(const Out &o, int64_t at, int64_t v) {
    const int64_t nb = len_bytes(v);
    for (int64_t j = lane_id(); j < nb; j += 64) put(o, at + j, j == nb - 1 ? (uint32_t)((v - 15) % 255) : 255u);
}

// src[spos, spos + len) -> dst[dpos, ...), by the whole wave: bytes up to a
// 16-byte boundary of dst, then uint4 stores fed by dword reads + v_alignbyte
// (the segment encoder's copy_direct, with explicit bounds)
__device__ void copy_wide(const Out &o, int64_t dpos, int64_t spos, int64_t len) {
    const int l = lane_id();
    int64_t end = dpos + len;
    if (end > o.cap) end = o.cap;
    if (dpos < 0 || spos < 0 || end <= dpos || spos + (end - dpos) > o.n) return;
    const int64_t delta = spos - dpos;
    int64_t a = dpos + (int64_t)((16u - (uint32_t)((uintptr_t)(o.dst + dpos) & 15u)) & 15u);
    if (a > end) a = end;
    if (l < a - dpos) o.dst[dpos + l] = o.src[dpos + l + delta];
    int64_t lim = end;
    if (lim > o.n - 4 - delta) lim = o.n - 4 - delta;  // the dword reads stay inside the source
    const int64_t b = lim > a ? a + ((lim - a) & ~(int64_t)15) : a;
    for (int64_t x0 = a + 16 * l; x0 < b; x0 += 4096) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t x = x0 + 1024 * u;
            if (x < b) {
                const uintptr_t p = (uintptr_t)(o.src + x + delta);
                const gc_u32 *w = (const gc_u32 *)(p & ~(uintptr_t)3);
                const uint32_t sh = (uint32_t)(p & 3);
                const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
                v[u] = make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                                  __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t x = x0 + 1024 * u;
            if (x < b) *(g_u4 *)(o.dst + x) = v[u];
        }
    }
    for (int64_t x = b + l; x < end; x += 64) o.dst[x] = o.src[x + delta];
}

__global__ __launch_bounds__(64) void emit_kernel(const jfs_dev_block *__restrict__ blocks_, Ctl c) {
    gc_blk *blocks = (gc_blk *)blocks_;
    gc_i32 *cfirst = (gc_i32 *)c.cfirst;
    const int lane = lane_id();
    const int g = (int)blockIdx.x;
    if (g >= cfirst[c.nblk]) return;
    const int b = find_block(cfirst, c.nblk, g);
    const int fin_off = ((gc_i32 *)c.fin_off)[b];
    if (fin_off < 0) return;  // failed, or does not fit: not a byte of dst is written
    const int ci = g - cfirst[b], nc = cfirst[b + 1] - cfirst[b];
    Out o;
    o.dst = (g_u8 *)blocks[b].dst;
    o.cap = blocks[b].dst_cap;
    o.src = (gc_u8 *)blocks[b].src;
    o.n = blocks[b].src_len;
    const int64_t cbase = (int64_t)ci << kChunkLog;
    const int clen = (int)(o.n - cbase < kChunk ? o.n - cbase : kChunk);
    const int R = ((gc_i32 *)c.nrec)[g];
    const int64_t carry = R ? ((gc_i32 *)c.cin)[g] : 0;
    gc_u2 *recs = (gc_u2 *)c.recs + (int64_t)g * kMaxRec;
    int64_t at = R ? ((gc_i32 *)c.start)[g] : 0;  // where the next 64 sequences begin
    for (int i0 = 0; i0 < R; i0 += 64) {
        const int i = i0 + lane;
        const bool has = i < R;
        uint2 r = make_uint2(kMinMatch << 16, 0);
        if (has) {
            const gc_u32 *rw = (const gc_u32 *)(recs + i);
            r.x = rw[0];
            r.y = rw[1];
        }
        const int p = (int)(r.x & 0xffff), mlen = (int)(r.x >> 16), moff = (int)(r.y & 0xffff), lit = (int)(r.y >> 16);
        const int64_t cin = i == 0 ? carry : 0;
        const int64_t L = lit + cin;
        const int ml = mlen - kMinMatch;
        const int64_t lb = len_bytes(L), mb = len_bytes(ml);
        const uint32_t size = has ? (uint32_t)(1 + lb + L + 2 + mb) : 0u;
        uint32_t total;
        const int64_t my = at + wave_scan_excl(size, &total);
        const int64_t litdst = my + 1 + lb + cin;  // this chunk's own literals
        const int64_t litsrc = cbase + p - lit;
        if (has) {
            put(o, my, (uint32_t)((L >= 15 ? 15 : (int)L) << 4 | (ml >= 15 ? 15 : ml)));
            if (L >= 15 && lb <= kInlineLenBytes)
                for (int64_t j = 0; j < lb; ++j) put(o, my + 1 + j, j == lb - 1 ? (uint32_t)((L - 15) % 255) : 255u);
            if (lit <= kInlineLits)
                for (int j = 0; j < lit; ++j) put(o, litdst + j, o.src[litsrc + j]);
            int64_t q = litdst + lit;
            put(o, q++, (uint32_t)moff & 255u);
            put(o, q++, (uint32_t)moff >> 8);
            if (ml >= 15) {
                int rem = ml - 15;
                for (; rem >= 255; rem -= 255) put(o, q++, 255u);
                put(o, q, (uint32_t)rem);
            }
        }
        for (uint64_t m = __ballot(has && lb > kInlineLenBytes); m; m &= m - 1) {
            const int l = __ffsll((unsigned long long)m) - 1;
            fill_len(o, bcast64(my + 1, l), bcast64(L, l));
        }
        for (uint64_t m = __ballot(has && lit > kInlineLits); m; m &= m - 1) {
            const int l = __ffsll((unsigned long long)m) - 1;
            copy_wide(o, bcast64(litdst, l), bcast64(litsrc, l), (int64_t)lane_read((uint32_t)lit, l));
        }
        at += total;
    }
    // the literals after the chunk's last match belong to a later sequence
    const int tl = ((gc_i32 *)c.tail)[g];
    if (tl > 0) {
        const int64_t spos = cbase + clen - tl;
        copy_wide(o, spos + ((gc_i32 *)c.delta)[g], spos, tl);
    }
    if (ci == nc - 1) {
        const int64_t L = ((gc_i32 *)c.fin_lit)[b];
        if (lane == 0) put(o, fin_off, (uint32_t)((L >= 15 ? 15 : (int)L) << 4));
        if (L >= 15) fill_len(o, (int64_t)fin_off + 1, L);
    }
}

namespace {
int64_t a16(int64_t x) { return (x + 15) & ~(int64_t)15; }
struct Layout {
    int64_t o_chunk, o_blk, o_rec, total;
};
Layout layout(int64_t B, int64_t C) {
    Layout y;
    y.o_chunk = a16(4 * (B + 1));
    y.o_blk = a16(y.o_chunk + 4 * 7 * C);
    y.o_rec = a16(y.o_blk + 4 * 2 * B);
    y.total = y.o_rec + (int64_t)sizeof(uint2) * kMaxRec * C;
    return y;
}
int64_t host_chunks(int32_t n) { return n >= 0 && n <= kMaxInput ? nchunks(n) : 0; }
int g_group_chunks = kGroupChunks;  // (jfs_test_set_lz4_fast_group_chunks)
// blocks [b0, return) form the next launch group
int next_group(int nblk, const int32_t *lens, int b0, int64_t *chunks) {
    int64_t C = 0;
    int b = b0;
    while (b < nblk && (b == b0 || C + host_chunks(lens[b]) <= g_group_chunks)) C += host_chunks(lens[b++]);
    *chunks = C;
    return b;
}
// the scratch views of a group of B blocks and C chunks
Ctl views(uint8_t *base, const Layout &y, int B, int64_t C) {
    Ctl c{};
    c.nblk = B;
    c.cap_chunks = (int)C;
    c.cfirst = (int32_t *)base;
    int32_t *pc = (int32_t *)(base + y.o_chunk);
    c.nrec = pc;
    c.tail = pc + C;
    c.lit0 = pc + 2 * C;
    c.body = pc + 3 * C;
    c.start = pc + 4 * C;
    c.cin = pc + 5 * C;
    c.delta = pc + 6 * C;
    c.fin_off = (int32_t *)(base + y.o_blk);
    c.fin_lit = c.fin_off + B;
    c.recs = (uint2 *)(base + y.o_rec);
    return c;
}
// the LIFT form's scratch: [the groups' areas | lifted, one per chunk of the largest group | the index areas]
struct LiftLayout {
    int64_t o_lifted, o_index, total;
};
LiftLayout lift_layout(int nblk, const int32_t *lens, int64_t index_bytes) {
    int64_t need = 0, cmax = 1;
    for (int b0 = 0; b0 < nblk;) {
        int64_t C;
        const int b1 = next_group(nblk, lens, b0, &C);
        C = C > 0 ? C : 1;
        need = std::max(need, layout(b1 - b0, C).total);
        cmax = std::max(cmax, C);
        b0 = b1;
    }
    LiftLayout y;
    y.o_lifted = a16(need);
    y.o_index = (y.o_lifted + 4 * cmax + 255) & ~(int64_t)255;
    y.total = y.o_index + index_bytes;
    return y;
}
}  // namespace

}  // namespace lz4f
}  // namespace jfs

extern "C" int64_t jfs_lz4_fast_scratch_bytes(int nblk, const int32_t *lens) {
    using namespace jfs::lz4f;
    int64_t need = 0;
    for (int b0 = 0; b0 < nblk;) {
        int64_t C;
        const int b1 = next_group(nblk, lens, b0, &C);
        const int64_t t = layout(b1 - b0, C > 0 ? C : 1).total;
        need = t > need ? t : need;
        b0 = b1;
    }
    return need;
}

extern "C" int jfs_launch_lz4_fast(const jfs_dev_block *d_blocks, int nblk, const int32_t *lens, int32_t *d_ret,
                                   void *scratch, int64_t scratch_cap, hipStream_t st) {
    using namespace jfs::lz4f;
    if (nblk <= 0) return 0;
    uint8_t *base = (uint8_t *)scratch;
    // groups run one after the other on the stream and reuse the scratch
    for (int b0 = 0; b0 < nblk;) {
        int64_t C;
        const int b1 = next_group(nblk, lens, b0, &C);
        const int B = b1 - b0;
        if (C < 1) C = 1;
        const Layout y = layout(B, C);
        if (!scratch || y.total > scratch_cap) return -1;
        const Ctl c = views(base, y, B, C);
        hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(256), 0, st, d_blocks + b0, c);
        hipLaunchKernelGGL(parse_kernel<false>, dim3((unsigned)C), dim3(64), 0, st, d_blocks + b0, c);
        hipLaunchKernelGGL(stitch_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, d_blocks + b0, c,
                           d_ret + b0);
        hipLaunchKernelGGL(emit_kernel, dim3((unsigned)C), dim3(64), 0, st, d_blocks + b0, c);
        b0 = b1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int64_t jfs_lz4_fast_lift_scratch_bytes(int nblk, const int32_t *lens, int nsrc, int nsel,
                                                   const int32_t *sel_len) {
    return jfs::lz4f::lift_layout(nblk, lens, jfs_lz4_lift_index_bytes(nsrc, nsel, sel_len)).total;
}

extern "C" int jfs_launch_lz4_fast_lift(const jfs_dev_block *d_blocks, int nblk, const int32_t *lens,
                                        const jfs_lz4_lift *d_lift, const jfs_lz4_lift_srcs *S, int32_t *d_ret,
                                        int32_t *d_lifted, void *scratch, int64_t scratch_cap, hipStream_t st) {
    using namespace jfs::lz4f;
    if (nblk <= 0) return 0;
    if (!S || S->nsrc <= 0 || S->nsel <= 0 || !d_lift) return -1;
    uint8_t *base = (uint8_t *)scratch;
    const LiftLayout ly = lift_layout(nblk, lens, jfs_lz4_lift_index_bytes(S->nsrc, S->nsel, S->sel_len));
    if (!scratch || ly.total > scratch_cap) return -1;
    // the index: once, in front of the first group, behind every group's areas
    if (jfs_launch_lz4_lift_index(S, base + ly.o_index, st) != 0) return -1;
    int64_t chunk0 = 0;  // the flat candidate array is offset per group
    for (int b0 = 0; b0 < nblk;) {
        int64_t C;
        const int b1 = next_group(nblk, lens, b0, &C);
        const int B = b1 - b0;
        const int64_t own = C;
        if (C < 1) C = 1;
        Ctl c = views(base, layout(B, C), B, C);
        int32_t *lifted = (int32_t *)(base + ly.o_lifted);
        c.lifted = lifted;
        const jfs_lz4_lift_group grp{B, (int)own, c.cfirst, c.nrec, c.tail, c.lit0, c.body, lifted, c.recs};
        hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(256), 0, st, d_blocks + b0, c);
        if (jfs_launch_lz4_lift(d_blocks + b0, &grp, (int)C, d_lift + chunk0, S, base + ly.o_index,
                                d_lifted ? d_lifted + b0 : nullptr, st) != 0)
            return -1;
        hipLaunchKernelGGL(parse_kernel<true>, dim3((unsigned)C), dim3(64), 0, st, d_blocks + b0, c);
        hipLaunchKernelGGL(stitch_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, d_blocks + b0, c,
                           d_ret + b0);
        hipLaunchKernelGGL(emit_kernel, dim3((unsigned)C), dim3(64), 0, st, d_blocks + b0, c);
        chunk0 += own;
        b0 = b1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Test hook (include/jfs_gpucodec_lz4_fast_test.h)
extern "C" int jfs_test_set_lz4_fast_group_chunks(int chunks) {
    const int prev = jfs::lz4f::g_group_chunks;
    jfs::lz4f::g_group_chunks = chunks > 0 ? chunks : jfs::lz4f::kGroupChunks;
    return prev;
}
