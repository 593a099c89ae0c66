// Slice compaction's stitch step on the GPU (pkg/vfs/compact.go:54-108): every
// output block is a list of byte ranges of decoded source blocks and holes
// (jfs_compact_seg, include/jfs_gpucodec.h), gathered into one buffer that the
// encoders then read -- the decoded bytes never leave HBM.
//
// Two kernels, chained on the caller's stream:
//   gather_plan_kernel  one workgroup per output block: checks the block's
//                       segments (tiling, indices, source lengths as the
//                       decoder wrote them) and writes the verdict to ret[j]:
//                       the block's total, -1 (bad plan) or JFS_CHAIN_FAILED;
//   gather_copy_kernel  grid (output tiles, blocks): moves the bytes of the
//                       blocks whose verdict is a total;
//   gather_copy_flat_kernel  the same tile body on a one-dimensional grid over
//                       a per-output tile prefix, for the read path's batches
//                       of very different output sizes.
// Work is split by OUTPUT position: a tile is TILE bytes of one block,
// whatever segments it is made of, so one 4 MiB single-segment block spreads
// over 256 workgroups and a block of thousands of one-byte segments does not
// queue on one lane.  A lane owns destination-aligned 16-byte words: a word
// that lies inside one segment is one 16-byte store, fed by the one or two
// aligned 16-byte source words that hold its bytes (shifted into place in
// registers); a hole is a zero store without a load; a word that straddles a
// segment boundary, or the block's head or tail, goes byte by byte.  Loads
// therefore touch only aligned words that contain a requested byte, and
// stores stay inside dst[0, total).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jfs_internal.h"

namespace jfs {
namespace compact {

constexpr int LANES = 256;
constexpr int TILE = 16 << 10;     // output bytes per workgroup: 4 words per lane
constexpr int WORDS = TILE / 16;

typedef JFS_GLOBAL const jfs_compact_seg gc_seg;
typedef JFS_GLOBAL const jfs_compact_out gc_out;
typedef JFS_GLOBAL const int32_t gc_i32;

constexpr int F_BAD = 1, F_FAILED = 2;

// merge != 0: ret[j] already holds the encoder's result for block j; only a
// negative verdict replaces it (the encoder may have run on a failed block)
__global__ __launch_bounds__(LANES) void gather_plan_kernel(const jfs_dev_block *__restrict__ src,
                                                            const int32_t *__restrict__ src_n, int nsrc,
                                                            const jfs_compact_out *__restrict__ out,
                                                            const jfs_compact_seg *__restrict__ seg,
                                                            int32_t *__restrict__ ret, int merge) {
    __shared__ int flags;
    const int j = blockIdx.x, t = threadIdx.x;
    if (t == 0) flags = 0;
    __syncthreads();
    const jfs_compact_out o = ((gc_out *)out)[j];
    const bool head_ok = o.dst_cap >= 0 && o.seg_first >= 0 && o.seg_count >= 0 && (o.seg_count == 0 || o.dst != nullptr);
    const gc_seg *sg = (gc_seg *)seg + (head_ok ? o.seg_first : 0);
    int f = head_ok ? 0 : F_BAD;
    for (int k = t; head_ok && k < o.seg_count; k += LANES) {
        const jfs_compact_seg s = sg[k];
        int64_t expect = 0;
        if (k > 0) {
            const jfs_compact_seg p = sg[k - 1];
            expect = (int64_t)p.dst_off + p.len;
        }
        if (s.len <= 0 || (int64_t)s.dst_off != expect || s.src < -1 || s.src >= nsrc ||
            (int64_t)s.dst_off + s.len > (int64_t)o.dst_cap || (s.src >= 0 && s.src_off < 0)) {
            f |= F_BAD;
        } else if (s.src >= 0) {
            const int32_t n = ((gc_i32 *)src_n)[s.src];
            const int32_t cap = ((gc_blk *)src)[s.src].dst_cap;
            if (n < 0 || (int64_t)s.src_off + s.len > (int64_t)(n < cap ? n : cap)) f |= F_FAILED;
        }
    }
    if (f) atomicOr(&flags, f);
    __syncthreads();
    if (t == 0) {
        const int fl = flags;
        int32_t v = 0;
        if (fl & F_BAD) {
            v = -1;
        } else if (fl & F_FAILED) {
            v = JFS_CHAIN_FAILED;
        } else if (o.seg_count > 0) {
            const jfs_compact_seg l = sg[o.seg_count - 1];
            v = l.dst_off + l.len;  // <= dst_cap: checked above
        }
        if (!merge || v < 0) ret[j] = v;
    }
}

// last segment of sg[lo .. hi] that starts at or before output position p
__device__ inline int find_seg(const gc_seg *sg, int lo, int hi, int32_t p) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (sg[mid].dst_off <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// bytes [sm, sm + 16) of the 32 bytes x | y  (0 < sm < 16)
__device__ inline uint4 shift_bytes(const uint4 x, const uint4 y, int sm) {
    const uint32_t c[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    const int q = sm >> 2, r = (sm & 3) * 8;
    uint32_t d[5], o[4];
#pragma unroll
    for (int i = 0; i < 5; i++) d[i] = q == 0 ? c[i] : q == 1 ? c[i + 1] : q == 2 ? c[i + 2] : c[i + 3];
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = (uint32_t)(((((uint64_t)d[i + 1]) << 32) | d[i]) >> r);
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// One TILE of output block o (its segments sg, its verdict total > 0): the body
// both copy kernels run, so the 2-D and the flat grid move the same words the
// same way.  Every lane of the workgroup calls it (it synchronises).
__device__ __forceinline__ void gather_tile(const jfs_dev_block *__restrict__ src, const jfs_compact_out o,
                                            const gc_seg *sg, const int32_t total, const int64_t tile) {
    __shared__ int krange[2];
    const int t = threadIdx.x;
    g_u8 *dst = (g_u8 *)o.dst;
    // word w of the block holds output positions [16 w - m, 16 w - m + 16): aligned in memory
    const int m = (int)((uintptr_t)o.dst & 15u);
    const int64_t nwords = ((int64_t)m + total + 15) >> 4;
    const int64_t w0 = tile * WORDS;
    if (w0 >= nwords) return;
    const int64_t w1 = w0 + WORDS < nwords ? w0 + WORDS : nwords;
    if (t < 2) {  // the segments this tile touches
        const int64_t p0 = 16 * w0 - m > 0 ? 16 * w0 - m : 0;
        const int64_t p1 = 16 * w1 - m < total ? 16 * w1 - m : total;
        krange[t] = find_seg(sg, 0, o.seg_count - 1, (int32_t)(t == 0 ? p0 : p1 - 1));
    }
    __syncthreads();
    const int klo = krange[0], khi = krange[1];
    for (int64_t w = w0 + t; w < w1; w += LANES) {
        const int64_t lo = 16 * w - m, hi = lo + 16;
        const int64_t a = lo > 0 ? lo : 0, b = hi < total ? hi : total;
        int k = find_seg(sg, klo, khi, (int32_t)a);
        jfs_compact_seg s = sg[k];
        if (a == lo && b == hi && hi <= (int64_t)s.dst_off + s.len) {
            uint4 v = make_uint4(0, 0, 0, 0);  // a hole: zeros, no load
            if (s.src >= 0) {
                const uintptr_t sa = (uintptr_t)((gc_blk *)src)[s.src].dst + (uintptr_t)s.src_off + (uintptr_t)(lo - s.dst_off);
                const int sm = (int)(sa & 15u);
                const gc_u4 *q = (const gc_u4 *)(sa - sm);
                v = q[0];
                if (sm) v = shift_bytes(v, q[1], sm);  // q[1] holds byte sa + 15
            }
            *(g_u4 *)(dst + lo) = v;
        } else {
            for (int64_t p = a; p < b; p++) {
                while (p >= (int64_t)s.dst_off + s.len) s = sg[++k];  // p < total: a segment holds it
                uint8_t c = 0;
                if (s.src >= 0) c = ((gc_u8 *)((gc_blk *)src)[s.src].dst)[(int64_t)s.src_off + (p - s.dst_off)];
                dst[p] = c;
            }
        }
    }
}

__global__ __launch_bounds__(LANES) void gather_copy_kernel(const jfs_dev_block *__restrict__ src,
                                                            const jfs_compact_out *__restrict__ out,
                                                            const jfs_compact_seg *__restrict__ seg,
                                                            const int32_t *__restrict__ ret) {
    const int j = blockIdx.y;
    const int32_t total = ((gc_i32 *)ret)[j];  // the plan kernel's verdict
    if (total <= 0) return;
    const jfs_compact_out o = ((gc_out *)out)[j];
    gather_tile(src, o, (gc_seg *)seg + o.seg_first, total, (int64_t)blockIdx.x);
}

// Tiles a block of `cap` bytes may need: it has at most (15 + cap + 15) / 16
// destination-aligned words.  The host sizes both grids with it, and the flat
// grid's prefix (below) is its running sum.
__host__ __device__ inline int64_t tiles_of(int64_t cap) { return cap > 0 ? (cap + 30 + TILE - 1) / TILE : 0; }

// The read path's grid (capi.hip, read_run): a batch mixes 4 KiB and 4 MiB
// outputs, so a (largest output's tiles) x nout grid would be almost all empty
// workgroups.  Here the grid is one-dimensional over tile_first, the running
// sum of every output's own tile count (nout + 1 entries, tile_first[0] = 0):
// a workgroup finds its output by binary search and runs the same tile body.
__global__ __launch_bounds__(LANES) void gather_copy_flat_kernel(const jfs_dev_block *__restrict__ src,
                                                                 const jfs_compact_out *__restrict__ out, int nout,
                                                                 const jfs_compact_seg *__restrict__ seg,
                                                                 const int32_t *__restrict__ ret,
                                                                 const int32_t *__restrict__ tile_first) {
    const gc_i32 *tf = (gc_i32 *)tile_first;
    const int32_t b = (int32_t)blockIdx.x;
    if (b >= tf[nout]) return;
    int lo = 0, hi = nout - 1;  // the last output whose first tile is at or before b (empty outputs share a start)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tf[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    const int j = lo;
    const int32_t total = ((gc_i32 *)ret)[j];  // the plan kernel's verdict
    if (total <= 0) return;
    const jfs_compact_out o = ((gc_out *)out)[j];
    gather_tile(src, o, (gc_seg *)seg + o.seg_first, total, (int64_t)(b - tf[j]));
}

// tile_first from the outputs' dst_cap on the device (jfs_read_gather_device:
// its caller has no staged prefix).  One workgroup: lane t sums a run of
// outputs, lane 0 scans the 256 sums, every lane writes its run's prefix.
__global__ __launch_bounds__(LANES) void gather_prefix_kernel(const jfs_compact_out *__restrict__ out, int nout,
                                                              int32_t *__restrict__ tile_first) {
    __shared__ int64_t part[LANES];
    const int t = threadIdx.x;
    const int per = (nout + LANES - 1) / LANES;
    const int j0 = t * per < nout ? t * per : nout, j1 = j0 + per < nout ? j0 + per : nout;
    int64_t sum = 0;
    for (int j = j0; j < j1; j++) sum += tiles_of(((gc_out *)out)[j].dst_cap);
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < LANES; i++) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    int64_t run = part[t];
    JFS_GLOBAL int32_t *tf = (JFS_GLOBAL int32_t *)tile_first;
    for (int j = j0; j < j1; j++) {
        tf[j] = (int32_t)(run < INT32_MAX ? run : INT32_MAX);
        run += tiles_of(((gc_out *)out)[j].dst_cap);
    }
    if (t == LANES - 1) tf[nout] = (int32_t)(run < INT32_MAX ? run : INT32_MAX);  // the last lane's run ends at nout
}

// The sealed chain (capi.hip, compact_seal_run) opens every source before it
// decodes it.  A failed open zeroes its output (aead.hip), and zeros can be a
// valid block -- for the "none" codec they always are -- so the open's verdict
// has to reach the gather: one lane per source writes a negative open result
// over src_n[i], which the plan kernel then reads as "that source failed".
// Runs after the decoders (they write every src_n[i], and take the zeroed
// payload like any other untrusted input) and before the gather.
__global__ __launch_bounds__(LANES) void chain_merge_kernel(const int32_t *__restrict__ open_ret, int nsrc,
                                                            int32_t *__restrict__ src_n) {
    const int i = blockIdx.x * LANES + threadIdx.x;
    if (i >= nsrc) return;
    const int32_t r = ((gc_i32 *)open_ret)[i];
    if (r < 0) ((JFS_GLOBAL int32_t *)src_n)[i] = r;
}

// The spliced compaction (capi.hip, compact_splice_run) finishes every output
// with one seal and one checksum launch, which read the payload's length on the
// device: a whole output's is its encode unit's result, a spliced one's the
// splice scan's verdict.  One lane per output k: idx[k] >= 0 picks a[idx[k]],
// else b[~idx[k]].
__global__ __launch_bounds__(LANES) void chain_pick_kernel(const int32_t *__restrict__ idx, int n,
                                                           const int32_t *__restrict__ a,
                                                           const int32_t *__restrict__ b, int32_t *__restrict__ out) {
    const int k = blockIdx.x * LANES + threadIdx.x;
    if (k >= n) return;
    const int32_t q = ((gc_i32 *)idx)[k];
    ((JFS_GLOBAL int32_t *)out)[k] = q >= 0 ? ((gc_i32 *)a)[q] : ((gc_i32 *)b)[~q];
}

// The read chain (capi.hip, read_run) checks every stored object's CRC-32C
// before anything else sees a byte of it (pkg/object/checksum.go:55-85).  The
// decoders still run on a mismatching object; like a failed open, only its
// verdict is replaced.  One lane per staged object i: lens[i] > 0 means "has an
// expected value" and crc[i] is what crc32c.hip computed; crc_got[i] receives
// it (0 without an expected value), and a mismatch on one of the first ndec
// objects (the decoded sources) writes JFS_CHECKSUM_FAILED over src_n[i].
// Runs after the decoders and the open's merge, before the gather's plan.
__global__ __launch_bounds__(LANES) void verify_gate_kernel(const uint32_t *__restrict__ crc,
                                                            const int32_t *__restrict__ lens,
                                                            const uint32_t *__restrict__ expect, int n, int ndec,
                                                            int32_t *__restrict__ src_n,
                                                            uint32_t *__restrict__ crc_got) {
    const int i = blockIdx.x * LANES + threadIdx.x;
    if (i >= n) return;
    const bool has = ((gc_i32 *)lens)[i] > 0;
    const uint32_t got = has ? ((gc_u32 *)crc)[i] : 0u;
    ((g_u32 *)crc_got)[i] = got;
    if (has && got != ((gc_u32 *)expect)[i] && i < ndec) ((JFS_GLOBAL int32_t *)src_n)[i] = JFS_CHECKSUM_FAILED;
}

}  // namespace compact
}  // namespace jfs

extern "C" int jfs_launch_chain_merge(const int32_t *d_open_ret, int nsrc, int32_t *d_src_n, hipStream_t stream) {
    using namespace jfs::compact;
    if (nsrc <= 0) return 0;
    hipLaunchKernelGGL(chain_merge_kernel, dim3((unsigned)((nsrc + LANES - 1) / LANES)), dim3(LANES), 0, stream,
                       d_open_ret, nsrc, d_src_n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int jfs_launch_chain_pick(const int32_t *d_idx, int n, const int32_t *d_a, const int32_t *d_b, int32_t *d_out,
                                     hipStream_t stream) {
    using namespace jfs::compact;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(chain_pick_kernel, dim3((unsigned)((n + LANES - 1) / LANES)), dim3(LANES), 0, stream, d_idx, n, d_a,
                       d_b, d_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// plan (verdicts into d_ret; merge: see gather_plan_kernel) and, unless merge,
// the copy.  max_dst_cap: host value >= every d_out[j].dst_cap.
extern "C" int jfs_launch_gather(const jfs_dev_block *d_src, const int32_t *d_src_n, int nsrc,
                                 const jfs_compact_out *d_out, int nout, const jfs_compact_seg *d_seg,
                                 int32_t max_dst_cap, int32_t *d_ret, int merge, hipStream_t stream) {
    using namespace jfs::compact;
    if (nout <= 0) return 0;
    hipLaunchKernelGGL(gather_plan_kernel, dim3(nout), dim3(LANES), 0, stream, d_src, d_src_n, nsrc, d_out, d_seg, d_ret,
                       merge);
    if (hipGetLastError() != hipSuccess) return -1;
    if (merge) return 0;
    if (max_dst_cap <= 0) return 0;
    // a block has at most (15 + cap + 15) / 16 destination-aligned words
    const int64_t tiles = ((int64_t)max_dst_cap + 30 + TILE - 1) / TILE;
    for (int y0 = 0; y0 < nout; y0 += 65535) {  // grid.y limit
        const int ny = nout - y0 < 65535 ? nout - y0 : 65535;
        hipLaunchKernelGGL(gather_copy_kernel, dim3((unsigned)tiles, (unsigned)ny), dim3(LANES), 0, stream, d_src,
                           d_out + y0, d_seg, d_ret + y0);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

extern "C" int64_t jfs_gather_tiles(int64_t cap) { return jfs::compact::tiles_of(cap); }

// d_tile_first[j] = running sum of jfs_gather_tiles(d_out[j].dst_cap), nout + 1 entries
extern "C" int jfs_launch_gather_prefix(const jfs_compact_out *d_out, int nout, int32_t *d_tile_first,
                                        hipStream_t stream) {
    using namespace jfs::compact;
    if (nout < 0) return -1;
    hipLaunchKernelGGL(gather_prefix_kernel, dim3(1), dim3(LANES), 0, stream, d_out, nout, d_tile_first);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// plan (verdicts into d_ret) and the copy on the flat grid.  d_tile_first: the
// device copy of the tile prefix (nout + 1 entries); ntiles: its last entry, a
// host value (it sizes the launch).
extern "C" int jfs_launch_gather_flat(const jfs_dev_block *d_src, const int32_t *d_src_n, int nsrc,
                                      const jfs_compact_out *d_out, int nout, const jfs_compact_seg *d_seg,
                                      int32_t *d_ret, const int32_t *d_tile_first, int64_t ntiles,
                                      hipStream_t stream) {
    using namespace jfs::compact;
    if (nout <= 0) return 0;
    if (ntiles < 0 || ntiles > INT32_MAX) return -1;
    hipLaunchKernelGGL(gather_plan_kernel, dim3(nout), dim3(LANES), 0, stream, d_src, d_src_n, nsrc, d_out, d_seg, d_ret,
                       0);
    if (hipGetLastError() != hipSuccess) return -1;
    if (ntiles == 0) return 0;
    hipLaunchKernelGGL(gather_copy_flat_kernel, dim3((unsigned)ntiles), dim3(LANES), 0, stream, d_src, d_out, nout, d_seg,
                       d_ret, d_tile_first);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int jfs_launch_verify_gate(const uint32_t *d_crc, const int32_t *d_lens, const uint32_t *d_expect, int n,
                                      int ndec, int32_t *d_src_n, uint32_t *d_crc_got, hipStream_t stream) {
    using namespace jfs::compact;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(verify_gate_kernel, dim3((unsigned)((n + LANES - 1) / LANES)), dim3(LANES), 0, stream, d_crc,
                       d_lens, d_expect, n, ndec, d_src_n, d_crc_got);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
