// Assembling seekable Zstd objects from frames that already exist (DESIGN 11d;
// the contract is jfs_zstd_splice_device's in the header).  Two kernels, chained
// on the caller's stream:
//   zsplice_scan  one wave per output, 64 frames a round: every lane takes one
//                 frame's compressed length (its record's, or the encoder's
//                 result of its unit), a wave prefix sum places the frames, the
//                 round's carry stays in a scalar; then the verdict, and for a
//                 good output the seek table behind its last frame;
//   zsplice_copy  one workgroup per frame on a flat grid: the frame's bytes,
//                 from the stored source object or from its unit's encode
//                 buffer, to where the scan placed them.
// Neither uses LDS.  Everything is written with plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "copy_any.cuh"
#include "jfs_internal.h"
#include "wave.cuh"
#include "zstd_seek.h"

namespace jfs {
namespace zsplice {

using namespace jfs::zseek;

constexpr int32_t MAX_C = 1 << 24;  // the longest frame a record may name: a round's sum fits 32 bits
constexpr int COPY_LANES = 256;

typedef JFS_GLOBAL const jfs_splice_out gc_sout;
typedef JFS_GLOBAL const jfs_splice_frame gc_sframe;
typedef JFS_GLOBAL const int32_t gc_i32;
typedef JFS_GLOBAL const uint64_t gc_u64;

__device__ __forceinline__ void put32(g_u8 *p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// what an output record must satisfy before any of its frames is looked at
__device__ __forceinline__ bool out_ok(const jfs_splice_out &o, int nframes) {
    return o.dst != nullptr && o.dst_cap >= 0 && o.frame_first >= 0 && o.frame_count >= 1 && o.frame_count <= MAX_FRAMES &&
           (int64_t)o.frame_first + o.frame_count <= (int64_t)nframes;
}

// frame f's compressed length: its record's, or its unit's encode result
__device__ __forceinline__ int32_t frame_len(const jfs_splice_frame &fr, const gc_i32 *unit_len) {
    return fr.unit < 0 ? fr.c : unit_len[fr.unit];
}

__global__ __launch_bounds__(64) void zsplice_scan(const jfs_splice_out *__restrict__ out, int nout,
                                                   const jfs_splice_frame *__restrict__ frames, int nframes,
                                                   const int32_t *__restrict__ unit_len,
                                                   const uint64_t *__restrict__ unit_hash, uint32_t *__restrict__ off,
                                                   int32_t *__restrict__ ret) {
    const int j = blockIdx.x, lane = lane_id();
    if (j >= nout) return;
    const jfs_splice_out o = ((gc_sout *)out)[j];
    if (!out_ok(o, nframes)) {
        if (lane == 0) ret[j] = -1;
        return;
    }
    const gc_sframe *fr = (gc_sframe *)frames + o.frame_first;
    const gc_i32 *ul = (gc_i32 *)unit_len;
    g_u32 *po = (g_u32 *)off + o.frame_first;
    const int32_t nf = o.frame_count;
    const int32_t entry = unit_hash ? ENTRY_CSUM : ENTRY;
    uint64_t carry = 0;  // bytes of the frames in front of the round
    bool bad = false, chain = false, failed = false;
    int32_t fail_v = 0;  // the first FRESH result <= 0
    for (int32_t k0 = 0; k0 < nf; k0 += 64) {
        const int32_t k = k0 + lane;
        int32_t c = 0;
        bool b = false, fl = false;
        if (k < nf) {
            const jfs_splice_frame f = fr[k];
            c = frame_len(f, ul);
            b = f.out != j || f.src == nullptr || f.d < 0 || c > MAX_C || (f.unit < 0 && c < 1);
            fl = f.unit >= 0 && c <= 0;
        }
        const uint64_t mb = __ballot(b), mf = __ballot(fl);
        bad = bad || mb != 0;
        chain = chain || __ballot(fl && c == JFS_CHAIN_FAILED) != 0;
        if (mf != 0 && !failed) {
            failed = true;
            fail_v = (int32_t)lane_read((uint32_t)c, __builtin_ctzll(mf));
        }
        uint32_t tot = 0;
        const uint32_t x = wave_scan_excl(b || fl ? 0u : (uint32_t)c, &tot);
        // only a verdict > 0 lets the copy use it: the sum then fits dst_cap, and 32 bits
        if (k < nf) po[k] = (uint32_t)(carry + x);
        carry += uniform(tot);
    }
    const int64_t size = (int64_t)carry + (int64_t)entry * nf + TABLE_FIXED;
    const int32_t v = bad ? -1 : chain ? JFS_CHAIN_FAILED : failed ? fail_v : size > (int64_t)o.dst_cap ? 0 : (int32_t)size;
    if (lane == 0) ret[j] = v;
    if (v <= 0) return;  // nothing is written for a failed output
    g_u8 *T = (g_u8 *)o.dst + carry;
    for (int32_t k = lane; k < nf; k += 64) {
        const jfs_splice_frame f = fr[k];
        g_u8 *e = T + 8 + entry * k;
        put32(e, (uint32_t)frame_len(f, ul));
        put32(e + 4, (uint32_t)f.d);
        if (unit_hash) put32(e + 8, f.unit < 0 ? f.x : (uint32_t)((gc_u64 *)unit_hash)[f.unit]);
    }
    if (lane == 0) {
        put32(T, SKIP_MAGIC);
        put32(T + 4, (uint32_t)(entry * nf + FOOTER));
        g_u8 *ft = T + 8 + entry * nf;
        put32(ft, (uint32_t)nf);
        ft[4] = (uint8_t)(unit_hash ? DESC_CSUM : 0u);
        put32(ft + 5, SEEK_MAGIC);
    }
}

// Frame f of the call, c bytes from src to dst at any two alignments (copy_any.cuh).
__global__ __launch_bounds__(COPY_LANES) void zsplice_copy(const jfs_splice_out *__restrict__ out, int nout,
                                                           const jfs_splice_frame *__restrict__ frames, int nframes,
                                                           const int32_t *__restrict__ unit_len,
                                                           const uint32_t *__restrict__ off,
                                                           const int32_t *__restrict__ ret) {
    const int32_t f = (int32_t)blockIdx.x, t = (int32_t)threadIdx.x;
    if (f >= nframes) return;
    const jfs_splice_frame fr = ((gc_sframe *)frames)[f];
    const int j = fr.out;
    if (j < 0 || j >= nout || ((gc_i32 *)ret)[j] <= 0) return;  // the scan's verdict
    const jfs_splice_out o = ((gc_sout *)out)[j];
    // a verdict > 0 vouches for the frames of [frame_first, frame_first + frame_count) only
    if (f < o.frame_first || f - o.frame_first >= o.frame_count) return;
    const int32_t c = frame_len(fr, (gc_i32 *)unit_len);
    g_u8 *dst = (g_u8 *)o.dst + ((JFS_GLOBAL const uint32_t *)off)[f];
    gc_u8 *src = (gc_u8 *)fr.src;
    copy_any<COPY_LANES>(dst, src, c, t);
}

}  // namespace zsplice
}  // namespace jfs

extern "C" int jfs_launch_zstd_splice(const jfs_splice_out *d_out, int nout, const jfs_splice_frame *d_frames,
                                      int nframes, const int32_t *d_unit_len, const uint64_t *d_unit_hash,
                                      uint32_t *d_off, int32_t *d_ret, hipStream_t stream) {
    using namespace jfs::zsplice;
    if (nout <= 0) return 0;
    hipLaunchKernelGGL(zsplice_scan, dim3((unsigned)nout), dim3(64), 0, stream, d_out, nout, d_frames, nframes, d_unit_len,
                       d_unit_hash, d_off, d_ret);
    if (hipGetLastError() != hipSuccess) return -1;
    if (nframes <= 0) return 0;
    hipLaunchKernelGGL(zsplice_copy, dim3((unsigned)nframes), dim3(COPY_LANES), 0, stream, d_out, nout, d_frames, nframes,
                       d_unit_len, (const uint32_t *)d_off, (const int32_t *)d_ret);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
