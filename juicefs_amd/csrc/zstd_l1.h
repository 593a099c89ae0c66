// Zstd level-1 encoder (zstd_encode.hip): the frame and block records, the
// sequence record and the range-checked source access that the exact parse and
// the fast parse (zstd_fast.hip) share with the entropy stage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jfs_internal.h"

namespace jfs {
namespace zl1 {

constexpr int32_t BLK = 128 << 10;  // ZSTD_BLOCKSIZE_MAX

// ---------------------------------------------------------------------------
// parameters: ZSTD_getCParams(1, n, 0) (level-1 row of the size tier, then
// ZSTD_adjustCParams_internal); strategy fast, targetLength 0 (step 2)
// ---------------------------------------------------------------------------
struct Params {
    uint32_t wlog, hlog, mls;
};
__host__ __device__ inline uint32_t hbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
__host__ __device__ inline Params params_of(int64_t n) {
    Params p;
    if (n > (256 << 10)) { p.wlog = 19; p.hlog = 14; p.mls = 7; }
    else if (n > (128 << 10)) { p.wlog = 18; p.hlog = 14; p.mls = 6; }
    else if (n > (16 << 10)) { p.wlog = 17; p.hlog = 13; p.mls = 6; }
    else { p.wlog = 14; p.hlog = 15; p.mls = 5; }
    const uint32_t t = (uint32_t)n;
    const uint32_t srclog = t < 64 ? 6u : hbit(t - 1) + 1;
    if (p.wlog > srclog) p.wlog = srclog;
    if (p.hlog > p.wlog + 1) p.hlog = p.wlog + 1;
    if (p.wlog < 10) p.wlog = 10;
    return p;
}
__host__ __device__ inline int64_t zbound(int64_t n) { return n + (n >> 8) + (n < BLK ? (BLK - n) >> 11 : 0); }

// per frame / per block records (host-built, device-updated)
struct FInfo {
    const uint8_t *src;
    uint8_t *dst;
    int32_t n, cap;
    int32_t nb, b0;  // blocks, index of the first in the block array
    uint32_t wlog, hlog, mls;
    int32_t status;  // 0 done, 1 parse again (a confirmation guess was wrong), -2 dst too small
};
enum : int32_t { F_NOCOMP = 1, F_RLE = 2, F_ASSUMED = 4, F_LASTNC = 8 };
struct BInfo {
    int64_t seq_off;  // u64 records in the sequence scratch
    int64_t lit_off;  // bytes: literals (bsz), then the sequences section (bsz + 512)
    int32_t frame, bs, be;
    int32_t ns, nl;                    // sequences, literals
    uint32_t rin0, rin1, rout0, rout1;  // repeat offsets in / out (offset_1, offset_2)
    int32_t flags;
    int32_t conf;   // outcome known from an earlier pass: 0 unknown, 1 confirmed, 2 not
    int32_t secsz;  // sequences section bytes, -1 = larger than the block
};
constexpr int64_t SEC_EXTRA = 512;
__host__ __device__ inline int64_t seq_cap(int32_t bsz) { return bsz / 4 + 4; }

// sequence record: ll | mlb << 17 | Offset_Value << 34
__device__ __forceinline__ uint64_t seq_pack(uint32_t ll, uint32_t mlb, uint32_t ofv) {
    return (uint64_t)ll | ((uint64_t)mlb << 17) | ((uint64_t)ofv << 34);
}

// ---------------------------------------------------------------------------
// source access through a buffer resource: the descriptor covers exactly the
// dwords that hold input bytes, so every load is range-checked by the
// hardware (out-of-range dwords read 0, nothing past the input is touched)
// and needs only a 32-bit offset -- no per-load guards or 64-bit address math
// ---------------------------------------------------------------------------
struct Src {
    __amdgpu_buffer_rsrc_t r;
    int32_t sh;  // input byte 0 sits at byte sh of the first dword
};
__device__ __forceinline__ Src make_src(const uint8_t *p, int32_t n) {
    Src s;
    const uintptr_t a = (uintptr_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(a & ~(uintptr_t)3));
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    s.sh = (int32_t)__builtin_amdgcn_readfirstlane((uint32_t)(a & 3u));
    const int32_t nb = n > 0 ? (int32_t)((n + s.sh + 3) & ~3) : 0;
    s.r = __builtin_amdgcn_make_buffer_rsrc((void *)(((uintptr_t)hi << 32) | lo), 0,
                                            (int)__builtin_amdgcn_readfirstlane((uint32_t)nb), 0x00020000);
    return s;
}
__device__ __forceinline__ uint32_t ldw(const Src &S, int32_t byteoff) {
    return __builtin_amdgcn_raw_buffer_load_b32(S.r, (uint32_t)byteoff, 0, 0);
}
// byte at position p
__device__ __forceinline__ uint32_t ldb(const Src &S, int32_t p) {
    return __builtin_amdgcn_raw_buffer_load_b8(S.r, (uint32_t)(p + S.sh), 0, 0);
}

// the fast parse (zstd_fast.hip) of the blocks d_blist[0, nb): fills their
// sequence records at seq_off and ns, nl, flags, rin / rout of their BInfo;
// d_cmeta: 4 int32 per block of the whole block array (per chunk: records,
// trailing literals)
int launch_zfast(const FInfo *d_fi, BInfo *d_bi, const int32_t *d_blist, int nb, uint64_t *d_seq, int32_t *d_cmeta,
                 hipStream_t st);

}  // namespace zl1
}  // namespace jfs
