// XXH64 (seed 0) of device-resident pieces (the contract is
// jfs_xxh64_device's in the header): the per-frame checksum of the Zstandard
// seekable format is its low 32 bits.  A message is four independent 64-bit
// accumulator chains over 32-byte stripes and has no more parallelism than
// that, so a piece takes 4 lanes (lane j owns accumulator j and the j-th 8
// bytes of every stripe) and a wave takes 16 pieces.  Each chain step is a
// dependent add, rotate and 64-bit multiply; the words are fetched DEPTH
// stripes ahead of their use so that no step waits for its load.  Lane 0 of a
// group merges the accumulators and walks the tail of fewer than 32 bytes.
// Every load is of exactly the bytes it uses, at any alignment (gfx950 serves
// unaligned global loads): nothing outside src[0, src_len) is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jfs_internal.h"
#include "wave.cuh"

namespace jfs {
namespace xxh {

constexpr uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull,
                   P4 = 0x85EBCA77C2B2AE63ull, P5 = 0x27D4EB2F165667C5ull;
constexpr int DEPTH = 8;  // stripes in flight per lane: 2 x 16 VGPRs of words, no scratch

struct __attribute__((packed)) U64 { uint64_t v; };
struct __attribute__((packed)) U32 { uint32_t v; };
__device__ __forceinline__ uint64_t ld64(gc_u8 *p) { return ((JFS_GLOBAL const U64 *)p)->v; }
__device__ __forceinline__ uint32_t ld32(gc_u8 *p) { return ((JFS_GLOBAL const U32 *)p)->v; }

__device__ __forceinline__ uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t round1(uint64_t acc, uint64_t w) { return rotl(acc + w * P2, 31) * P1; }
__device__ __forceinline__ uint64_t merge(uint64_t h, uint64_t v) { return (h ^ round1(0, v)) * P1 + P4; }
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int l) {
    return (uint64_t)lane_read((uint32_t)(v >> 32), l) << 32 | lane_read((uint32_t)v, l);
}

__global__ __launch_bounds__(64) void xxh64_kernel(const jfs_dev_block *__restrict__ blocks, int nblk,
                                                   uint64_t *__restrict__ hash, int32_t *__restrict__ ret) {
    const int lane = lane_id(), j = lane & 3;
    const int64_t g = (int64_t)blockIdx.x * 16 + (lane >> 2);
    const bool has = g < nblk;
    int32_t len = 0;
    gc_u8 *src = nullptr;
    if (has) {
        len = blocks[g].src_len;
        src = (gc_u8 *)blocks[g].src;
    }
    const bool bad = len < 0 || (src == nullptr && len > 0);
    if (bad) len = 0;
    const int32_t ns = len >> 5;  // whole stripes
    uint64_t acc = j == 0 ? P1 + P2 : j == 1 ? P2 : j == 2 ? 0ull : 0ull - P1;
    gc_u8 *p = src + 8 * j;
    const int32_t full = ns / DEPTH;
    if (full > 0) {
        uint64_t w[DEPTH];
#pragma unroll
        for (int t = 0; t < DEPTH; t++) w[t] = ld64(p + 32 * t);
        for (int32_t c = 0; c < full; c++) {
            p += 32 * DEPTH;
            uint64_t nx[DEPTH];
            if (c + 1 < full) {
#pragma unroll
                for (int t = 0; t < DEPTH; t++) nx[t] = ld64(p + 32 * t);
            } else {
#pragma unroll
                for (int t = 0; t < DEPTH; t++) nx[t] = 0;
            }
#pragma unroll
            for (int t = 0; t < DEPTH; t++) acc = round1(acc, w[t]);
#pragma unroll
            for (int t = 0; t < DEPTH; t++) w[t] = nx[t];
        }
    }
    for (int32_t s = full * DEPTH; s < ns; s++, p += 32) acc = round1(acc, ld64(p));
    // (the four lanes of a group run the same trip counts, so they meet here)
    const int l0 = lane & ~3;
    const uint64_t v1 = shfl64(acc, l0), v2 = shfl64(acc, l0 + 1), v3 = shfl64(acc, l0 + 2), v4 = shfl64(acc, l0 + 3);
    if (!has || j != 0) return;
    uint64_t h;
    if (ns > 0) {
        h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
        h = merge(merge(merge(merge(h, v1), v2), v3), v4);
    } else {
        h = P5;
    }
    h += (uint64_t)(uint32_t)len;
    gc_u8 *q = src + ((int64_t)ns << 5);
    int32_t rem = len & 31;
    for (; rem >= 8; rem -= 8, q += 8) h = rotl(h ^ round1(0, ld64(q)), 27) * P1 + P4;
    if (rem >= 4) {
        h = rotl(h ^ (uint64_t)ld32(q) * P1, 23) * P2 + P3;
        q += 4;
        rem -= 4;
    }
    for (; rem > 0; rem--, q++) h = rotl(h ^ (uint64_t)*q * P5, 11) * P1;
    h ^= h >> 33;
    h *= P2;
    h ^= h >> 29;
    h *= P3;
    h ^= h >> 32;
    hash[g] = bad ? 0ull : h;
    if (ret) ret[g] = bad ? -1 : 0;
}

}  // namespace xxh
}  // namespace jfs

extern "C" int jfs_launch_xxh64(const jfs_dev_block *d_blocks, int nblk, uint64_t *d_hash, int32_t *d_ret,
                                hipStream_t stream) {
    if (nblk <= 0) return 0;
    hipLaunchKernelGGL(jfs::xxh::xxh64_kernel, dim3((unsigned)((nblk + 15) / 16)), dim3(64), 0, stream, d_blocks, nblk,
                       d_hash, d_ret);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
