// LZ4 RANGES decode: only the requested bytes of a block are produced, each by
// the origin chase of lz4_chase.h -- no origin map, no other output byte.
//
// On one stream:
//   index    lz4_split.hip's plan, spec, fix, count and scan (launch_index): they
//            walk compressed bytes only and leave every 256-byte segment's true
//            entry position and the output offset at that entry;
//   plan     per block: the early answers' blocks and the blocks the index does
//            not cover are marked for the hand-over; the range list is checked
//            by the rules of the Zstd ranges call (zstd_seek.h range_follows /
//            range_live); H = the largest clamped hi; the live bytes below
//            min(total, dst_cap) are laid out on a flat grid of QUADS, 4-aligned
//            groups of output positions, by an exclusive sum over the blocks;
//   tail     the block's last token: a literal-only sequence that ends exactly
//            at n (the one thing the verdict needs that no requested byte visits);
//   chase    one thread per quad of requested positions: chase_quad, then the
//            bytes from src to dst (an aligned whole quad as one 32-bit store);
//            BAD or DEEP flags the block and writes nothing for the quad;
//   verdict  ret = min(total, H) for a block whose fix-up settled, whose last
//            token is good, whose total fits dst_cap and that no quad flagged;
//            any other goes, through the todo mask, to the exact prefix kernel
//            (lz4_decode.hip) with want = H.
// No LDS, no dependence between threads, no host wait.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "jfs_internal.h"
#include "lz4_chase.h"
#define JFS_LZ4_SPLIT_RECORDS_ONLY  // the small-batch decoder's records and its index launch, not its kernels
#include "lz4_split.hip"
#undef JFS_LZ4_SPLIT_RECORDS_ONLY
#include "zstd_seek.h"

namespace jfs {
namespace lz4c {

using lz4s::BStat;
using lz4s::FIX_ROUNDS;
using lz4s::SBlock;
using lz4s::Scratch;
using lz4s::T;

enum : int32_t { S_CHASE = 0, S_ANSWERED = 1, S_HAND = 2 };

struct CBlock {
    int32_t state;
    int32_t r0, r1;   // the block's ranges, d_rng[r0 .. r1) (a checked list)
    int32_t lim;      // min(total, dst_cap): no position at or above it is chased
    int32_t top;      // H
    int32_t quads;    // quads of the live bytes below lim
    int32_t bytes;    // those bytes
    int32_t flag;     // a quad met BAD (1) or DEEP (2)
    int32_t last_ok;  // the last token is literals only and ends at n, within dst_cap
};

struct CScratch {
    CBlock *cb;
    int64_t *qf;    // exclusive sum of CBlock::quads, nb + 1
    int32_t *want;  // H per block: the hand-over's want
    int32_t *todo;
};

// blocks resolved by the chase, bytes requested of them, steps taken, blocks handed over
__device__ unsigned long long g_chase_counts[4];

// the clamps of range c: lo' and hi' against the capacity, then the end of the chased bytes
__device__ __forceinline__ bool quad_span(const jfs_range c, int32_t cap, int32_t lim, int32_t &lo, int32_t &hi) {
    lo = zseek::range_lo(c.lo);
    hi = zseek::range_hi(c.hi, cap);
    hi = hi < lim ? hi : lim;
    return hi > lo;
}

__global__ __launch_bounds__(T) void plan_kernel(const jfs_dev_block *__restrict__ desc, const int32_t *__restrict__ rf,
                                                 const jfs_range *__restrict__ rng, int nb, Scratch sc, CScratch cs,
                                                 int32_t *__restrict__ ret) {
    for (int b = threadIdx.x; b < nb; b += T) {
        const jfs_dev_block d = ((const gc_blk *)desc)[b];
        const BStat &st = sc.st[b];
        CBlock c{};
        cs.want[b] = 0;
        if (!d.src || d.src_len <= 0 || d.dst_cap <= 0) {
            c.state = S_HAND;  // the full decoder's early answers, in front of the list's
        } else {
            const int32_t r0 = rf[b], r1 = rf[b + 1];
            bool bad = r0 < 0 || r1 < r0, live = false;
            int32_t top = 0;
            for (int32_t q = bad ? r1 : r0; q < r1; q++) {
                const jfs_range r = rng[q];
                bad = bad || !zseek::range_follows(q > r0 ? &rng[q - 1] : (const jfs_range *)nullptr, r);
                if (zseek::range_live(r, d.dst_cap)) {
                    live = true;
                    top = max(top, zseek::range_hi(r.hi, d.dst_cap));
                }
            }
            if (bad || !live) {
                c.state = S_ANSWERED;
                ret[b] = bad ? -1 : 0;
            } else {
                c.r0 = r0;
                c.r1 = r1;
                c.top = top;
                cs.want[b] = top;
                // (planned empty: over the host's budget; bad: total over dst_cap, or an empty block)
                if (sc.blk[b].n <= 0 || st.bad || st.fix[FIX_ROUNDS - 1]) {
                    c.state = S_HAND;
                } else {
                    c.lim = min(st.total, d.dst_cap);
                    int64_t quads = 0, bytes = 0;
                    for (int32_t q = r0; q < r1; q++) {
                        int32_t lo, hi;
                        if (!quad_span(rng[q], d.dst_cap, c.lim, lo, hi)) continue;
                        quads += ((hi + 3) >> 2) - (lo >> 2);
                        bytes += hi - lo;
                    }
                    c.quads = (int32_t)quads;  // (disjoint ranges below lim < 2^30: at most lim / 4 + their count)
                    c.bytes = (int32_t)bytes;
                }
            }
        }
        cs.cb[b] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t q = 0;
        for (int b = 0; b < nb; b++) {
            cs.qf[b] = q;
            q += cs.cb[b].state == S_CHASE ? cs.cb[b].quads : 0;
        }
        cs.qf[nb] = q;
    }
}

// The segment that holds the block's last token start walks to it: the one
// whose own entry lies inside it and whose successor's entry is n.
__global__ __launch_bounds__(T) void tail_kernel(int nb, int nseg_all, Scratch sc, CScratch cs) {
    const int g = blockIdx.x * T + threadIdx.x;
    if (g >= nseg_all) return;
    const int b = lz4s::block_of(sc.blk, nb, g);
    if (cs.cb[b].state != S_CHASE) return;
    const SBlock B = sc.blk[b];
    const int32_t n = B.n, k = g - B.seg0;
    const int32_t s0 = k * SEG, s1 = s0 + SEG < n ? s0 + SEG : n;
    int32_t x = sc.entry[g], op = sc.cnt[g];
    if (x < s0 || x >= s1 || (k + 1 < B.nseg && sc.entry[g + 1] < n)) return;
    const gc_u8 *s = (const gc_u8 *)B.src;
    while (x < s1) {
        const lz4s::Tok t = lz4s::parse_rd(s, n, x, false);
        if (t.last) {
            if (lz4s::tok_ok(t.tok, t, n, op, B.cap)) cs.cb[b].last_ok = 1;
            return;
        }
        op += t.ll + t.ml;  // (the count kept the block's total within cap < 2^30)
        x = t.next;
    }
}

// the block of quad q: the last b with qf[b] <= q (blocks without quads share their successor's)
__device__ __forceinline__ int block_of_quad(const int64_t *qf, int nb, int64_t q) {
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (qf[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One thread per quad, grid-strided: the grid is sized on the host from what
// it knows (its own copy of the lists, or the capacities), the quads on the
// device from the lists themselves.
__global__ __launch_bounds__(T) void chase_kernel(const jfs_range *__restrict__ rng, int nb, Scratch sc, CScratch cs) {
    const int64_t nq = cs.qf[nb];
    uint32_t hops = 0;
    for (int64_t q = (int64_t)blockIdx.x * T + threadIdx.x; q < nq; q += (int64_t)gridDim.x * T) {
        const int b = block_of_quad(cs.qf, nb, q);
        const CBlock c = cs.cb[b];
        const SBlock B = sc.blk[b];
        // the quad's place: the block's live ranges in order, each a run of quads
        int32_t rel = (int32_t)(q - cs.qf[b]), x0 = -1;
        uint32_t mask = 0;
        for (int32_t r = c.r0; r < c.r1; r++) {
            int32_t lo, hi;
            if (!quad_span(rng[r], B.cap, c.lim, lo, hi)) continue;
            const int32_t cnt = ((hi + 3) >> 2) - (lo >> 2);
            if (rel < cnt) {
                x0 = ((lo >> 2) + rel) << 2;
#pragma unroll
                for (int i = 0; i < 4; i++) mask |= (x0 + i >= lo && x0 + i < hi) ? 1u << i : 0u;
                break;
            }
            rel -= cnt;
        }
        if (x0 < 0) continue;  // (the plan counted these quads from the same list: not reached)
        const gc_u8 *s = (const gc_u8 *)B.src;
        const JFS_GLOBAL int32_t *entry = (const JFS_GLOBAL int32_t *)(sc.entry + B.seg0);
        const JFS_GLOBAL int32_t *cnt = (const JFS_GLOBAL int32_t *)(sc.cnt + B.seg0);
        int32_t idx[4];
        const int32_t rc = chase_quad(s, B.n, B.cap, entry, cnt, B.nseg, x0, mask, idx, hops);
        if (rc != 0) {
            cs.cb[b].flag = rc == BAD ? 1 : 2;
            continue;
        }
        g_u8 *dst = (g_u8 *)B.dst;
        if (mask == 15u && (((uintptr_t)(dst + x0)) & 3u) == 0) {
            uint32_t w = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) w |= (uint32_t)s[idx[i]] << (8 * i);
            *(g_u32 *)(dst + x0) = w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if ((mask >> i) & 1u) dst[x0 + i] = s[idx[i]];
        }
    }
    if (hops) atomicAdd(&g_chase_counts[2], (unsigned long long)hops);
}

__global__ void verdict_kernel(int nb, Scratch sc, CScratch cs, int32_t *__restrict__ ret) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const CBlock c = cs.cb[b];
    const bool hand = c.state == S_HAND || (c.state == S_CHASE && (c.flag || !c.last_ok));
    cs.todo[b] = hand;
    if (hand) {
        atomicAdd(&g_chase_counts[3], 1ull);
    } else if (c.state == S_CHASE) {
        ret[b] = min(sc.st[b].total, c.top);
        atomicAdd(&g_chase_counts[0], 1ull);
        atomicAdd(&g_chase_counts[1], (unsigned long long)c.bytes);
    }
}

}  // namespace lz4c
}  // namespace jfs

using namespace jfs::lz4c;
namespace om = jfs::om;

static int64_t layout(void *d_scratch, int64_t nb, int64_t nseg_all, Scratch &sc, CScratch &cs) {
    om::Carve c(d_scratch);
    jfs::lz4s::carve_index(c, nb, nseg_all, sc);
    c.take(cs.cb, nb * (int64_t)sizeof(CBlock));
    c.take(cs.qf, (nb + 1) * 8);
    c.take(cs.want, nb * 4);
    c.take(cs.todo, nb * 4);
    return c.bytes;
}

static int64_t segments(int nb, const int32_t *src_len) {
    int64_t seg = 0;
    for (int b = 0; b < nb; b++) seg += ((int64_t)(src_len[b] > 0 ? src_len[b] : 0) + SEG - 1) / SEG;
    return seg;
}

// The split layout without the origin area: some 44 bytes per 256 compressed bytes.
extern "C" int64_t jfs_lz4_chase_scratch_bytes(int nb, const int32_t *src_len) {
    Scratch sc;
    CScratch cs;
    return layout(nullptr, nb, segments(nb, src_len), sc, cs);
}

// src_len / cap: the host's copies of the descriptors' sizes (they size the
// scratch and the index grids; a block whose device descriptor asks for more
// is handed over).  max_quads: an upper bound of the quads the lists ask for,
// where the host knows one (< 0: it does not; the capacities bound them).  It
// only sizes the grid: the threads stride over the quads the device counted.
extern "C" int jfs_launch_lz4_chase(const jfs_dev_block *d_desc, const int32_t *src_len, const int32_t *cap,
                                    const int32_t *d_rf, const jfs_range *d_rng, int nb, int32_t *d_ret, void *d_scratch,
                                    int64_t max_quads, hipStream_t st) {
    if (nb <= 0) return 0;
    const int64_t nseg_all = segments(nb, src_len);
    int64_t max_cap = 0, cap_quads = 0;
    for (int b = 0; b < nb; b++) {
        const int64_t c = cap[b] > 0 ? cap[b] : 0;
        max_cap = std::max(max_cap, c);
        cap_quads += (c + 3) / 4;
    }
    Scratch sc;
    CScratch cs;
    layout(d_scratch, nb, nseg_all, sc, cs);
    jfs::lz4s::launch_index(d_desc, nullptr, nb, sc, nseg_all, max_cap, INT64_MAX, max_cap, st);
    hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(T), 0, st, d_desc, d_rf, d_rng, nb, sc, cs, d_ret);
    if (nseg_all > 0)
        hipLaunchKernelGGL(tail_kernel, dim3((unsigned)((nseg_all + T - 1) / T)), dim3(T), 0, st, nb, (int)nseg_all, sc, cs);
    const int64_t quads = max_quads >= 0 ? std::min(max_quads, cap_quads + nb) : cap_quads;
    const unsigned groups = (unsigned)std::max<int64_t>(1, std::min<int64_t>((quads + T - 1) / T, 16384));
    hipLaunchKernelGGL(chase_kernel, dim3(groups), dim3(T), 0, st, d_rng, nb, sc, cs);
    hipLaunchKernelGGL(verdict_kernel, dim3((nb + 63) / 64), dim3(64), 0, st, nb, sc, cs, d_ret);
    if (hipGetLastError() != hipSuccess) return -1;
    // the exact one-workgroup prefix kernel for the flagged blocks (the others exit at once)
    return jfs_launch_lz4_decode_prefix(d_desc, nb, d_ret, cs.want, cs.todo, st);
}

extern "C" int jfs_lz4_chase_counts(uint64_t out[4], int reset) {
    if (!out) return -1;
    unsigned long long v[4] = {0, 0, 0, 0};
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_chase_counts), sizeof(v)) != hipSuccess) return -1;
    for (int i = 0; i < 4; i++) out[i] = v[i];
    if (reset) {
        unsigned long long z[4] = {0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_chase_counts), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
