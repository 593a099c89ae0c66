// c bytes from src to dst at any two alignments, by LANES lanes of which the
// caller is lane t (zstd_splice.hip's frames, zstd_seek_tables.hip's tables).
// The body is destination-aligned 16-byte stores; word w's bytes come from the
// five dwords at the 4-byte-aligned address below its first source byte, shifted
// into place (lz4_decode.hip's long-literal copy is the model).  The head runs
// byte-wise up to the first aligned store whose loads start inside the source,
// and the tail from the last word whose loads end inside it, so no byte outside
// [src, src + c) is read and none outside [dst, dst + c) is written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jfs_internal.h"

namespace jfs {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef JFS_GLOBAL const u32x4 gc_x4;

template <int LANES>
__device__ __forceinline__ void copy_any(g_u8 *dst, gc_u8 *src, int32_t c, int32_t t) {
    int32_t h0 = (int32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
    const uint32_t sm = (uint32_t)(((uintptr_t)src + (uint32_t)h0) & 3u);
    if ((uint32_t)h0 < sm) h0 += 16;  // the first word's loads start at src + h0 - sm
    const int32_t past = sm ? 4 - (int32_t)sm : 0;  // a word's loads end `past` bytes behind its 16
    const int32_t nw = c - h0 - past >= 16 ? (c - h0 - past) >> 4 : 0;
    if (h0 > c) h0 = c;
    for (int32_t p = t; p < h0; p += LANES) dst[p] = src[p];
    if (sm == 0) {
        for (int32_t w = t; w < nw; w += LANES) {
            const u32x4 v = *(const gc_x4 *)(src + h0 + 16 * w);
            *(g_u4 *)(dst + h0 + 16 * w) = make_uint4(v.x, v.y, v.z, v.w);
        }
    } else {
        for (int32_t w = t; w < nw; w += LANES) {
            gc_u8 *a = src + h0 + 16 * w - sm;
            const u32x4 v = *(const gc_x4 *)a;
            const uint32_t e = *(const gc_u32 *)(a + 16);
            uint4 q;
            q.x = __builtin_amdgcn_alignbyte(v.y, v.x, sm);
            q.y = __builtin_amdgcn_alignbyte(v.z, v.y, sm);
            q.z = __builtin_amdgcn_alignbyte(v.w, v.z, sm);
            q.w = __builtin_amdgcn_alignbyte(e, v.w, sm);
            *(g_u4 *)(dst + h0 + 16 * w) = q;
        }
    }
    for (int32_t p = h0 + 16 * nw + t; p < c; p += LANES) dst[p] = src[p];
}

}  // namespace jfs
