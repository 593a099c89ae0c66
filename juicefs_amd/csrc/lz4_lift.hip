// The lift of LZ4 compaction (lz4_lift.h): the kernels between the
// fast encoder's plan and its parse.
//
//   select   the sources that have a candidate, packed for the index (a call
//            that does not know them on the host indexes every source);
//   index    lz4_split.hip's plan, spec, fix, count and scan (launch_index) over
//            those sources' stored bytes: every 256-byte segment's true entry
//            position and the output offset at that entry.  Once per call;
//   lift     one wave per output chunk of a launch group.  A candidate's wave
//            finds, by binary search in its source's cnt, the segments whose
//            output meets [F, F + kChunk), takes them 64 at a time, walks each
//            lane's true tokens twice -- the rule and the count of records, then,
//            behind a wave prefix sum, the records themselves -- and leaves what
//            parse_kernel leaves for a chunk, with lifted[g] = 1.  A refused
//            chunk gets lifted[g] = 0 and nothing else, and is parsed;
//   count    per output block, the chunks lifted.
// An offset or a length the rule reads is unchecked beyond the stream's bounds:
// a wrong verdict can only send the chunk to the parse, and the source's own
// decode has judged the stream (the rule asks for its result).  No LDS, no
// atomics, no host wait.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "jfs_internal.h"
#include "lz4_lift.h"
#define JFS_LZ4_SPLIT_RECORDS_ONLY  // the small-batch decoder's records and its index launch, not its kernels
#include "lz4_split.hip"
#undef JFS_LZ4_SPLIT_RECORDS_ONLY

namespace jfs {
namespace lz4l {

using lz4s::BStat;
using lz4s::FIX_ROUNDS;
using lz4s::SBlock;
using lz4s::Scratch;
using lz4s::SEG;
using lz4s::T;

typedef JFS_GLOBAL int32_t g_i32;
typedef JFS_GLOBAL const int32_t gc_i32;

// what the index of a call keeps in scratch behind the fast encoder's areas
struct Index {
    Scratch sc;
    jfs_dev_block *desc;  // [nsel] the packed descriptors (select), or the caller's
    int32_t *slot;        // [nsrc] source -> its place in the index, or -1
    int nsrc, nsel;
};

__global__ __launch_bounds__(T) void select_kernel(const jfs_dev_block *__restrict__ src, const int32_t *__restrict__ sel,
                                                   Index ix) {
    for (int i = threadIdx.x; i < ix.nsrc; i += T) ix.slot[i] = sel ? -1 : i;
    __syncthreads();
    if (!sel) return;
    for (int k = threadIdx.x; k < ix.nsel; k += T) {
        const int32_t s = sel[k];
        const bool ok = s >= 0 && s < ix.nsrc;
        jfs_dev_block d{nullptr, nullptr, 0, 0};  // (not a source: planned empty)
        if (ok) d = ((const gc_blk *)src)[s];
        ix.desc[k] = d;
        if (ok) ix.slot[s] = k;
    }
}

constexpr int kRounds = 6;  // rounds of 64 segments a chunk is taken in

// the last segment j of [0, nseg) with cnt[j] <= x (cnt[0] == 0 <= x)
__device__ __forceinline__ int32_t seg_at(gc_i32 *cnt, int32_t nseg, int32_t x) {
    int32_t a = 0, z = nseg - 1;
    while (a < z) {
        const int32_t m = (a + z + 1) >> 1;
        if (cnt[m] <= x) a = m;
        else z = m - 1;
    }
    return a;
}

// One lane's walk of the true tokens of segment k of a block (stored bytes
// s[0, n)) against the chunk at floor F: every REC sequence goes to `rec` in
// stream order; false: a sequence refuses the chunk.  parse_rd reads below n only.
template <class Rec>
__device__ __forceinline__ bool walk(const gc_u8 *s, int32_t n, int32_t k, int32_t x, int32_t op, int32_t F, Rec rec) {
    const int32_t s1 = (k + 1) * SEG < n ? (k + 1) * SEG : n, E = F + (int32_t)kChunk;
    while (x < s1 && op < E) {
        const lz4s::Tok t = lz4s::parse_rd(s, n, x, true);
        if (t.cut) return false;  // (the stream ends inside a token: as lift_host refuses it)
        if (t.last) break;
        const int32_t m = op + t.ll;
        const int c = classify(F, m, t.ml, t.off);
        if (c == SEQ_BAD) return false;
        if (c == SEQ_REC) rec(op, m, t.ml, t.off);
        op = m + t.ml;
        x = t.next;
    }
    return true;
}

__global__ __launch_bounds__(64) void lift_kernel(const jfs_dev_block *__restrict__ blocks_, jfs_lz4_lift_group c,
                                                  const jfs_lz4_lift *__restrict__ lift, const int32_t *__restrict__ src_n,
                                                  Index ix) {
    gc_blk *blocks = (gc_blk *)blocks_;
    gc_i32 *cfirst = (gc_i32 *)c.cfirst;
    const int lane = lane_id();
    const int g = (int)blockIdx.x;
    if (g >= cfirst[c.nblk]) return;
    g_i32 *lifted = (g_i32 *)c.lifted;
    if (lane == 0) lifted[g] = 0;
    // the output chunk: interior in a block the fast encoder takes
    int b = 0;
    {
        int hi = c.nblk;  // cfirst[b] <= g < cfirst[hi]
        while (hi - b > 1) {
            const int mid = (b + hi) >> 1;
            if (cfirst[mid] <= g) b = mid;
            else hi = mid;
        }
    }
    const int64_t n_out = blocks[b].src_len;
    if (n_out < 0 || n_out > lz4f::kMaxInput || cfirst[b + 1] - cfirst[b] != (int)nchunks(n_out)) return;
    if (!interior(g - cfirst[b], n_out) || g >= c.ncand) return;
    // the candidate: a source of the index, a chunk interior in what it decoded to
    const jfs_lz4_lift cand = ((const JFS_GLOBAL jfs_lz4_lift *)lift)[g];
    if (cand.src < 0 || cand.src >= ix.nsrc || cand.src_chunk < 0 || cand.src_chunk >= (1 << 30 >> kChunkLog) - 1) return;
    const int32_t slot = ((gc_i32 *)ix.slot)[cand.src];
    if (slot < 0) return;
    if (!interior(cand.src_chunk, ((gc_i32 *)src_n)[cand.src])) return;
    const SBlock B = ix.sc.blk[slot];
    const BStat &st = ix.sc.st[slot];
    if (B.n <= 0 || B.nseg <= 0 || st.bad || st.fix[FIX_ROUNDS - 1]) return;
    const int32_t F = cand.src_chunk << kChunkLog, E = F + (int32_t)kChunk;
    if (st.total < E) return;
    const gc_u8 *s = (const gc_u8 *)B.src;
    gc_i32 *entry = (gc_i32 *)(ix.sc.entry + B.seg0), *cnt = (gc_i32 *)(ix.sc.cnt + B.seg0);
    const int32_t k0 = seg_at(cnt, B.nseg, F), k1 = seg_at(cnt, B.nseg, E - 1);
    // Segment k0 holds the token of the sequence that reaches F.  Its literals may begin any distance below F --
    // the trailing literals of the chunks in front, whole chunks without a match among them -- so the segments
    // behind k0 may hold no token for any length: they share the cnt of kA, the next segment that holds one.  The
    // chunk is taken as k0, then kA .. k1.  From kA on the tokens' output lies inside the chunk, whose stored bytes
    // span some 260 segments at most (a sequence of four output bytes takes three stored ones at least): kRounds
    // rounds of 64.  A stream that spreads a chunk wider is none of the fast encoder's.
    const int32_t kA = k0 < k1 ? seg_at(cnt, B.nseg, cnt[k0 + 1]) : k0 + 1;
    if (k1 - kA + 2 > 64 * kRounds) return;
    const auto seg_of = [&](int32_t idx) { return idx == 0 ? k0 : kA + idx - 1; };  // (> k1: none)
    // pass 1: the rule, and per round every lane's first record index (a wave prefix sum of its count), its body
    // and its last match's end
    int32_t first[kRounds];
    int32_t nrec = 0, end = F;
    uint32_t body = 0;
    bool good = true;
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
        const int32_t k = seg_of(64 * r + lane);
        int32_t mine = 0, mend = 0;
        uint32_t mbody = 0;
        bool ok = true;
        if (good && k <= k1)
            ok = walk(s, B.n, k, entry[k], cnt[k], F, [&](int32_t a, int32_t m, int32_t ml, int32_t) {
                mine++;
                mbody += rec_body(rec_lit(F, a, m), ml);
                mend = m + ml;
            });
        good = good && __ballot(!ok) == 0;
        uint32_t round;
        first[r] = nrec + (int32_t)wave_scan_excl((uint32_t)mine, &round);
        nrec += (int32_t)round;
        body += wave_sum(mbody);
        const int32_t top = (int32_t)wave_max((uint32_t)mend);  // (ends are positions above F >= 0, or 0)
        end = top > end ? top : end;
    }
    // (matches are four bytes at least and lie inside the chunk: the count cannot pass kMaxRec; the test stays
    // beside the stores it guards)
    if (!good || nrec > kMaxRec) return;
    // pass 2: the records
    JFS_GLOBAL uint2 *recs = (JFS_GLOBAL uint2 *)c.recs + (int64_t)g * kMaxRec;
    int32_t lit0 = 0;
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
        const int32_t k = seg_of(64 * r + lane);
        int32_t at = first[r];
        if (k <= k1)
            walk(s, B.n, k, entry[k], cnt[k], F, [&](int32_t a, int32_t m, int32_t ml, int32_t off) {
                const int32_t lit = rec_lit(F, a, m);
                if (at < kMaxRec) recs[at] = make_uint2(rec_x(F, m, ml), rec_y(off, lit));
                if (at == 0) lit0 = lit;
                at++;
            });
    }
    lit0 = (int32_t)wave_max((uint32_t)lit0);  // (one lane holds record 0; the others 0)
    if (lane == 0) {
        ((g_i32 *)c.nrec)[g] = nrec;
        ((g_i32 *)c.tail)[g] = E - end;
        ((g_i32 *)c.lit0)[g] = lit0;
        ((g_i32 *)c.body)[g] = (int32_t)(body - (nrec ? body_of_first(lit0) : 0u));
        lifted[g] = 1;
    }
}

// per output block of the group: the chunks lifted
__global__ __launch_bounds__(64) void count_kernel(jfs_lz4_lift_group c, int32_t *__restrict__ out) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= c.nblk) return;
    int32_t sum = 0;
    for (int g = c.cfirst[b]; g < c.cfirst[b + 1]; g++) sum += c.lifted[g];
    out[b] = sum;
}

static int64_t segments(int n, const int32_t *len) {
    int64_t seg = 0;
    for (int b = 0; b < n; b++) seg += ((int64_t)(len[b] > 0 ? len[b] : 0) + SEG - 1) / SEG;
    return seg;
}

static int64_t layout(void *base, int64_t nsrc, int64_t nsel, int64_t nseg_all, Index &ix) {
    om::Carve c(base);
    lz4s::carve_index(c, nsel, nseg_all, ix.sc);
    c.take(ix.desc, nsel * (int64_t)sizeof(jfs_dev_block));
    c.take(ix.slot, nsrc * 4);
    return c.bytes;
}

}  // namespace lz4l
}  // namespace jfs

using namespace jfs::lz4l;

// The index areas of a call over nsrc sources of which nsel are indexed
// (sel_len: their stored lengths on the host): some 44 bytes per 256 stored bytes.
extern "C" int64_t jfs_lz4_lift_index_bytes(int nsrc, int nsel, const int32_t *sel_len) {
    Index ix;
    return layout(nullptr, nsrc, nsel, segments(nsel, sel_len), ix);
}

// the index of a call as both launches below carve it from d_scratch
static Index index_of(const jfs_lz4_lift_srcs &S, void *d_scratch) {
    Index ix;
    layout(d_scratch, S.nsrc, S.nsel, segments(S.nsel, S.sel_len), ix);
    ix.nsrc = S.nsrc;
    ix.nsel = S.nsel;
    if (!S.d_sel) ix.desc = const_cast<jfs_dev_block *>(S.d_src);
    return ix;
}

// Queues select and the index steps over S (jfs_internal.h), once per call.
extern "C" int jfs_launch_lz4_lift_index(const jfs_lz4_lift_srcs *S, void *d_scratch, hipStream_t st) {
    if (S->nsrc <= 0 || S->nsel <= 0) return -1;
    Index ix = index_of(*S, d_scratch);
    const int64_t nseg_all = segments(S->nsel, S->sel_len);
    int64_t max_cap = 0;
    for (int b = 0; b < S->nsel; b++) max_cap = std::max<int64_t>(max_cap, S->sel_cap[b]);
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(T), 0, st, S->d_src, S->d_sel, ix);
    jfs::lz4s::launch_index(ix.desc, nullptr, S->nsel, ix.sc, nseg_all, max_cap, INT64_MAX, max_cap, st);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Queues lift and count for one launch group of the fast encoder, between its
// plan and its parse.  d_lift: the candidate of the group's first chunk;
// d_lifted (may be null): the count of the group's first block.
extern "C" int jfs_launch_lz4_lift(const jfs_dev_block *d_blocks, const jfs_lz4_lift_group *grp, int chunks,
                                   const jfs_lz4_lift *d_lift, const jfs_lz4_lift_srcs *S, void *d_scratch,
                                   int32_t *d_lifted, hipStream_t st) {
    const Index ix = index_of(*S, d_scratch);
    hipLaunchKernelGGL(lift_kernel, dim3((unsigned)chunks), dim3(64), 0, st, d_blocks, *grp, d_lift, S->d_src_n, ix);
    if (d_lifted)
        hipLaunchKernelGGL(count_kernel, dim3((unsigned)((grp->nblk + 63) / 64)), dim3(64), 0, st, *grp, d_lifted);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
