// Fast Zstd parse: valid RFC 8878 frames, not libzstd's bytes.
// Every 128 KiB block is cut into at most two independent 64 KiB chunks; one
// wave parses a chunk 64 positions at a time (zfast_parse, modelled on
// lz4f::parse_kernel), and one wave per block turns the chunks' records into
// the sequence records, counts and flags that the entropy stage of
// zstd_encode.hip reads (zfast_seq), with repeat offsets that never reach
// outside the block.  zstd_fast_host.cc restates both on the host and gives the
// same records.
#include <string.h>

#include <vector>

#include "../../include/jfs_gpucodec_zstd_fast_test.h"
#include "wave.cuh"
#include "zstd_fast.h"
#include "zstd_l1.h"

namespace jfs {
namespace zfast {

using zl1::BInfo;
using zl1::FInfo;
using zl1::Src;

typedef JFS_GLOBAL int32_t g_i32;
typedef JFS_GLOBAL const int32_t gc_i32;
typedef JFS_GLOBAL uint64_t g_u64;

static_assert(kBlock == zl1::BLK, "zstd_fast.h restates the block size");

// 4 bytes at byte `b` of the buffer (b >= 0): two aligned dwords + v_alignbyte.
// Dwords past the input read 0 and never reach a decision: every caller clamps
// what it takes from them to the chunk.
__device__ __forceinline__ uint32_t ld32(const Src &S, int32_t b) {
    const int32_t o = b & ~3;
    return __builtin_amdgcn_alignbyte(zl1::ldw(S, o + 4), zl1::ldw(S, o), (uint32_t)b & 3u);
}

// the records of chunk ci of a block live in the block's own sequence area,
// which seq_cap sizes for one record per 4 bytes: chunk 1's start at kMaxRec
__device__ __forceinline__ g_u64 *chunk_recs(uint64_t *seqs, const BInfo &B, int ci) {
    return (g_u64 *)(seqs + B.seq_off + (int64_t)ci * kMaxRec);
}

__global__ __launch_bounds__(64) void zfast_parse(const FInfo *__restrict__ fi, const int32_t *__restrict__ blist,
                                                  const BInfo *__restrict__ bi, uint64_t *seqs,
                                                  int32_t *__restrict__ cmeta) {
    __shared__ uint16_t tab[1 << kHashLog];
    const int lane = lane_id();
    const int bid = blist[blockIdx.x >> 1], ci = (int)(blockIdx.x & 1);
    const BInfo B = bi[bid];
    const FInfo F = fi[B.frame];
    if (F.status < 0) return;
    const int32_t bsz = B.be - B.bs, cb = ci << kChunkLog;
    if (bsz < kNoCompBelow || cb >= bsz) return;  // zfast_seq reads no record of such a chunk
    const int clen = bsz - cb < kChunk ? bsz - cb : kChunk;
    const Src S = zl1::make_src(F.src, F.n);
    const int32_t base = B.bs + cb + S.sh;  // buffer byte of chunk position 0
    g_u64 *recs = chunk_recs(seqs, B, ci);
    const int maxrec = clen / kMinMatch;
    for (int i = lane; i < (1 << kHashLog) / 2; i += 64) ((uint32_t *)tab)[i] = 0;
    __syncthreads();
    const int mend = clen;              // a match may end at the chunk's last byte
    const int slim = clen - kMinMatch;  // last position with 4 bytes inside the chunk
    int anchor = 0, cur = 0, nrec = 0;
    for (int t0 = 0; t0 <= slim;) {
        const int p = t0 + lane;
        const bool act = p <= slim;
        uint32_t v = 0, h = 0;
        int cand = -1, len = 0;
        if (act) {
            if (p >= kNear) {
                // bytes [p - 4, p + 4) of the chunk
                const int32_t b = base + p - 4, o = b & ~3;
                const uint32_t sh = (uint32_t)b & 3u;
                const uint32_t w0 = zl1::ldw(S, o), w1 = zl1::ldw(S, o + 4), w2 = zl1::ldw(S, o + 8);
                const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sh);
                v = __builtin_amdgcn_alignbyte(w2, w1, sh);
                const uint64_t win = (uint64_t)v << 32 | lo;
                if ((uint32_t)(win >> 24) == v) cand = p - 1;
                else if ((uint32_t)(win >> 16) == v) cand = p - 2;
                else if ((uint32_t)(win >> 8) == v) cand = p - 3;
                else if (lo == v) cand = p - 4;
            } else {
                v = ld32(S, base + p);
            }
            h = hash4(v);
            if (cand < 0) {
                const int e = tab[h];
                if (e < p && ld32(S, base + e) == v) cand = e;
            }
            if (cand >= 0) {
                const int limit = mend - p < kCapLen ? mend - p : kCapLen;
                len = kMinMatch;
                while (len < limit) {
                    const uint32_t x = ld32(S, base + p + len) ^ ld32(S, base + cand + len);
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
                        const uint32_t x = ld32(S, base + q) ^ ld32(S, base + cl + ml + 4 * lane);
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
            if (lane == 0 && nrec < maxrec)
                recs[nrec] = (uint64_t)rec_hi((uint32_t)(pl - cl), (uint32_t)(pl - anchor)) << 32 |
                             rec_lo((uint32_t)pl, (uint32_t)ml);
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
        g_i32 *cm = (g_i32 *)cmeta + ((int64_t)bid * 2 + ci) * 2;
        cm[0] = nrec < maxrec ? nrec : maxrec;  // (every match covers 4 bytes: never more)
        cm[1] = clen - anchor;
    }
}

// all bytes of the block equal (ZSTD_isRLE)
__device__ bool all_equal(const Src &S, int32_t bs, int32_t be) {
    const int lane = lane_id();
    const uint32_t c4 = zl1::ldb(S, bs) * 0x01010101u;
    for (int32_t p0 = bs; p0 < be; p0 += 256) {
        const int32_t p = p0 + 4 * lane;
        bool bad = false;
        if (p < be) {
            uint32_t x = ld32(S, p + S.sh) ^ c4;
            if (be - p < 4) x &= (1u << (8 * (be - p))) - 1u;
            bad = x != 0;
        }
        if (__ballot(bad)) return false;
    }
    return true;
}

// One wave per block.  The chunks' records become the block's sequence records
// in place (a sequence's slot never lies past the record it comes from, and 64
// records are read before 64 sequences are written).  Repeat offsets: RepHist.
// The history scan is serial: 64 records sit one per lane and a scalar loop
// walks the lanes.
__global__ __launch_bounds__(64) void zfast_seq(const FInfo *__restrict__ fi, const int32_t *__restrict__ blist,
                                                BInfo *__restrict__ bi, uint64_t *seqs,
                                                const int32_t *__restrict__ cmeta) {
    const int lane = lane_id();
    const int bid = blist[blockIdx.x];
    BInfo &B = bi[bid];
    const FInfo F = fi[B.frame];
    if (F.status < 0) return;
    const int32_t bs = B.bs, be = B.be, bsz = be - bs;
    // the repeat offsets handed on are those handed in: a fast block takes none
    // from its predecessors, so no outcome of theirs can make it wrong and the
    // literal kernel never asks for another parse; F_ASSUMED stays clear
    if (bsz < kNoCompBelow) {
        if (lane == 0) {
            B.ns = 0;
            B.nl = bsz;
            B.rin0 = B.rout0 = 0;
            B.rin1 = B.rout1 = 0;
            B.flags = zl1::F_NOCOMP;
        }
        return;
    }
    const int nc = bsz > kChunk ? 2 : 1;
    g_u64 *sq = (g_u64 *)(seqs + B.seq_off);
    RepHist hist;
    hist.start(bs == 0);
    uint32_t carry = 0, mlsum = 0;
    int w = 0;
    for (int ci = 0; ci < nc; ++ci) {
        gc_i32 *cm = (gc_i32 *)cmeta + ((int64_t)bid * 2 + ci) * 2;
        const int nr = cm[0];
        const uint32_t tail = (uint32_t)cm[1];
        const g_u64 *recs = chunk_recs(seqs, B, ci);
        for (int i0 = 0; i0 < nr; i0 += 64) {
            const int i = i0 + lane;
            const bool has = i < nr;
            const uint64_t r = has ? recs[i] : 0ull;
            const uint32_t ml = (uint32_t)r >> 16, off = (uint32_t)(r >> 32) & 0xffffu;
            const uint32_t ll = (uint32_t)(r >> 48) + (i == 0 ? carry : 0u);
            const int nj = nr - i0 < 64 ? nr - i0 : 64;
            uint32_t ofv = 0;
            for (int jj = 0; jj < nj; ++jj) {
                const uint32_t c = hist.code(readlane(ll, jj), readlane(off, jj));
                if (lane == jj) ofv = c;
            }
            if (has) {
                sq[w + i] = seq_rec(ll, ml, ofv);
                mlsum += ml;
            }
        }
        // the literals a chunk leaves over join the next chunk's first sequence
        carry = nr ? tail : carry + tail;
        w += nr;
    }
    // all equal: a chunk of equal bytes parses into one match at most
    const bool rle = bs > 0 && w <= 2 && all_equal(zl1::make_src(F.src, F.n), bs, be);
    const uint32_t nl = (uint32_t)bsz - wave_sum(mlsum);  // a block's trailing literals stay in the block
    if (lane == 0) {
        B.ns = w;
        B.nl = (int32_t)nl;
        B.rin0 = B.rout0 = 0;
        B.rin1 = B.rout1 = 0;
        B.flags = rle ? zl1::F_RLE : 0;
    }
}

}  // namespace zfast

namespace zl1 {
int launch_zfast(const FInfo *d_fi, BInfo *d_bi, const int32_t *d_blist, int nb, uint64_t *d_seq, int32_t *d_cmeta,
                 hipStream_t st) {
    if (nb <= 0) return 0;
    hipLaunchKernelGGL(zfast::zfast_parse, dim3(2u * (unsigned)nb), dim3(64), 0, st, d_fi, d_blist,
                       (const BInfo *)d_bi, d_seq, d_cmeta);
    hipLaunchKernelGGL(zfast::zfast_seq, dim3((unsigned)nb), dim3(64), 0, st, d_fi, d_blist, d_bi, d_seq,
                       (const int32_t *)d_cmeta);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace zl1
}  // namespace jfs

extern "C" int64_t jfs_test_zstd_fast_seqs_device(const uint8_t *d_src, int64_t n, uint64_t *out_u64, int64_t cap,
                                                  int32_t *ns_per_block, int32_t *nl_per_block) {
    using namespace jfs::zl1;
    if (n < 0 || n > 0x7FFFFF00ll || cap < 0) return -1;
    const int nb = (int)jfs::zfast::nblocks(n);
    if (nb == 0) return 0;
    FInfo F;
    memset(&F, 0, sizeof(F));
    F.src = d_src;
    F.n = (int32_t)n;
    F.nb = nb;
    std::vector<BInfo> bi(nb);
    std::vector<int32_t> blist(nb);
    int64_t seq_total = 0;
    for (int k = 0; k < nb; ++k) {
        BInfo &B = bi[k];
        memset(&B, 0, sizeof(B));
        B.bs = k * BLK;
        B.be = (int32_t)(n - B.bs < BLK ? n : B.bs + BLK);
        B.seq_off = seq_total;
        seq_total += seq_cap(B.be - B.bs);
        blist[k] = k;
    }
    const size_t o_bi = 256, o_bl = o_bi + sizeof(BInfo) * nb, o_cm = o_bl + sizeof(int32_t) * nb,
                 o_sq = (o_cm + sizeof(int32_t) * 4 * nb + 255) & ~(size_t)255;
    uint8_t *d = nullptr;
    if (hipMalloc((void **)&d, o_sq + sizeof(uint64_t) * (size_t)seq_total) != hipSuccess) return -1;
    std::vector<uint64_t> seqs((size_t)seq_total);
    bool ok = hipMemcpy(d, &F, sizeof(F), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_bi, bi.data(), sizeof(BInfo) * nb, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + o_bl, blist.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice) == hipSuccess &&
              launch_zfast((const FInfo *)d, (BInfo *)(d + o_bi), (const int32_t *)(d + o_bl), nb,
                           (uint64_t *)(d + o_sq), (int32_t *)(d + o_cm), nullptr) == 0 &&
              hipDeviceSynchronize() == hipSuccess &&
              hipMemcpy(bi.data(), d + o_bi, sizeof(BInfo) * nb, hipMemcpyDeviceToHost) == hipSuccess &&
              hipMemcpy(seqs.data(), d + o_sq, sizeof(uint64_t) * (size_t)seq_total, hipMemcpyDeviceToHost) ==
                  hipSuccess;
    (void)hipFree(d);
    if (!ok) return -1;
    int64_t total = 0;
    for (const BInfo &B : bi) {
        if (B.ns < 0 || B.ns > seq_cap(B.be - B.bs)) return -1;
        total += B.ns;
    }
    if (total > cap) return -1;
    int64_t at = 0;
    for (int k = 0; k < nb; ++k) {
        const BInfo &B = bi[k];
        if (B.ns) memcpy(out_u64 + at, seqs.data() + B.seq_off, sizeof(uint64_t) * (size_t)B.ns);
        at += B.ns;
        ns_per_block[k] = B.ns;
        nl_per_block[k] = B.nl;
    }
    return total;
}
