// Checksummed seekable Zstd encode (the contract is
// jfs_zstd_compress_seekable_csum_device's in the header): the seekable encode
// as it is, XXH64 (xxh64.hip) of every source's 128 KiB pieces, and one small
// kernel per object that rewrites the 8-byte table in place as the 12-byte one.
// No kernel of zstd_encode.hip changes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "jfs_internal.h"
#include "wave.cuh"
#include "zstd_seek.h"

namespace jfs {
namespace zseek {

__device__ __forceinline__ uint32_t get32(const g_u8 *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
__device__ __forceinline__ void put32(g_u8 *p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// One wave per object.  Entry k moves from 8 + 8 k to 8 + 12 k of the table, so
// the new entries of a round of 64 cover old entries of that round and of later
// ones only: the rounds run from the back, and a round reads all its entries
// before it writes any.
__global__ __launch_bounds__(64) void zcsum_widen(const jfs_dev_block *__restrict__ blocks, int nblk,
                                                  const int32_t *__restrict__ piece0, const uint64_t *__restrict__ hash,
                                                  int32_t *__restrict__ ret) {
    const int i = blockIdx.x, lane = lane_id();
    if (i >= nblk) return;
    const jfs_dev_block b = blocks[i];
    const int32_t r = ret[i];
    if (b.src == nullptr || b.src_len <= FRAME_BYTES || r <= 0) return;  // one frame, no table; or the encoder's refusal
    const int32_t nb = (int32_t)(((int64_t)b.src_len + FRAME_BYTES - 1) / FRAME_BYTES);
    const int64_t t = (int64_t)r - table_bytes(nb);
    // Unreachable, kept as a bound on the stores below: the encoder answers r > 0 only with dst_cap >=
    // CompressBound(src_len), its frames and table take n + 21 nb + 17 at most, and n + 25 nb + 17 stays
    // within that bound (tests/test_zstd_seek_csum.py sweeps it), so r + 4 nb <= dst_cap.
    if (t < 0 || (int64_t)r + 4 * nb > (int64_t)b.dst_cap) {
        if (lane == 0) ret[i] = -2;
        return;
    }
    g_u8 *T = (g_u8 *)b.dst + t;
    const int32_t p0 = piece0[i];
    for (int32_t k0 = (nb - 1) & ~63; k0 >= 0; k0 -= 64) {
        const int32_t k = k0 + lane;
        uint32_t c = 0, d = 0;
        if (k < nb) {
            c = get32(T + 8 + ENTRY * k);
            d = get32(T + 12 + ENTRY * k);
        }
        wait_vm();
        if (k < nb) {
            put32(T + 8 + ENTRY_CSUM * k, c);
            put32(T + 12 + ENTRY_CSUM * k, d);
            put32(T + 16 + ENTRY_CSUM * k, (uint32_t)hash[p0 + k]);
        }
        wait_vm();
    }
    if (lane == 0) {
        put32(T + 4, (uint32_t)(ENTRY_CSUM * nb + 9));
        g_u8 *f = T + 8 + ENTRY_CSUM * nb;
        put32(f, (uint32_t)nb);
        f[4] = (uint8_t)DESC_CSUM;
        put32(f + 5, SEEK_MAGIC);
        ret[i] = r + 4 * nb;
    }
}

namespace {
struct CsumScratch {
    std::mutex mu;
    uint8_t *d = nullptr;
    size_t cap = 0;
};
CsumScratch g_csum[16];
}  // namespace

}  // namespace zseek
}  // namespace jfs

// host-synchronous, as the seekable encode is
extern "C" int jfs_launch_zstd_encode_seek_csum(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret,
                                                hipStream_t stream) {
    using namespace jfs::zseek;
    if (jfs_launch_zstd_encode(d_blocks, nblk, d_ret, stream, JFS_ZSTD_PARSE_SEEKABLE) != 0) return -1;
    if (nblk <= 0) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return -1;
    std::vector<jfs_dev_block> hb((size_t)nblk);
    if (hipMemcpyAsync(hb.data(), d_blocks, sizeof(jfs_dev_block) * (size_t)nblk, hipMemcpyDeviceToHost, stream) !=
            hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return -1;
    std::vector<int32_t> piece0((size_t)nblk);
    std::vector<jfs_dev_block> pieces;
    for (int i = 0; i < nblk; i++) {
        piece0[(size_t)i] = (int32_t)pieces.size();
        const jfs_dev_block &b = hb[(size_t)i];
        if (b.src == nullptr || b.src_len <= FRAME_BYTES) continue;
        for (int64_t o = 0; o < b.src_len; o += FRAME_BYTES)
            pieces.push_back(jfs_dev_block{b.src + o, nullptr, (int32_t)(b.src_len - o < FRAME_BYTES ? b.src_len - o : FRAME_BYTES), 0});
        if (pieces.size() > 0x7FFFFFFFull / 64) return -1;
    }
    const size_t np = pieces.size();
    if (np == 0) return 0;  // nothing has a table
    const size_t o_hash = sizeof(jfs_dev_block) * np, o_p0 = o_hash + 8 * np, bytes = o_p0 + 4 * (size_t)nblk;
    CsumScratch &z = g_csum[dev];
    std::lock_guard<std::mutex> lk(z.mu);
    if (z.cap < bytes) {
        if (z.d) (void)hipFree(z.d);
        z.d = nullptr;
        z.cap = 0;
        size_t n = 1 << 16;
        while (n < bytes) n <<= 1;
        if (hipMalloc((void **)&z.d, n) != hipSuccess) return -1;
        z.cap = n;
    }
    jfs_dev_block *d_pieces = (jfs_dev_block *)z.d;
    uint64_t *d_hash = (uint64_t *)(z.d + o_hash);
    int32_t *d_p0 = (int32_t *)(z.d + o_p0);
    if (hipMemcpyAsync(d_pieces, pieces.data(), o_hash, hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(d_p0, piece0.data(), 4 * (size_t)nblk, hipMemcpyHostToDevice, stream) != hipSuccess)
        return -1;
    if (jfs_launch_xxh64(d_pieces, (int)np, d_hash, nullptr, stream) != 0) return -1;
    hipLaunchKernelGGL(zcsum_widen, dim3((unsigned)nblk), dim3(64), 0, stream, d_blocks, nblk, (const int32_t *)d_p0,
                       (const uint64_t *)d_hash, d_ret);
    if (hipGetLastError() != hipSuccess) return -1;
    return hipStreamSynchronize(stream) == hipSuccess ? 0 : -1;
}
