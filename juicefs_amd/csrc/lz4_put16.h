// Byte masks of one <= 16-byte ring write of the LZ4 decode copier (put16 in
// lz4_decode.hip).  Host and device: tests/test_lz4_put16_masks.py drives
// tests/put16_masks_main.cc over every (ha, m) against the byte-wise
// definition.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JFS_PUT16_HD __host__ __device__ __forceinline__
#else
#define JFS_PUT16_HD inline
#endif

namespace jfs {
namespace lz4d {

JFS_PUT16_HD uint32_t sat_sub(uint32_t a, uint32_t b) { return a > b ? a - b : 0u; }  // v_sub_u32 clamp

struct Put16Masks {
    uint32_t k[5];
};

// A write of m bytes (1..16) whose first byte is byte ha (0..3) of dword 0
// covers bits [8 ha, E), E = 8 (ha + m), of five dwords.  Three shared shifts
// instead of a clamp and a shift per dword:
//   dwords 0,1: E >= 8, so the low min(E, 64) bits are ~0 >> (64 - E) with the
//               shift saturated at 0 (never the empty mask);
//   dword 2:    the high half of 0x00000000FFFFFFFF << clamp(E - 64, 0, 32);
//   dwords 3,4: E <= 152, so the low E - 96 <= 56 bits are ~(~0 << (E - 96))
//               with the shift saturated at 0 (never the full mask).
JFS_PUT16_HD Put16Masks put16_masks(uint32_t ha, uint32_t m) {
    Put16Masks r;
    const uint32_t lo = 8u * ha, E = lo + 8u * m;
    const uint64_t a = ~0ull >> sat_sub(64u, E);
    r.k[0] = (uint32_t)a & (0xFFFFFFFFu << lo);
    r.k[1] = (uint32_t)(a >> 32);
    const uint32_t s2 = sat_sub(E, 64u);
    r.k[2] = (uint32_t)((0xFFFFFFFFull << (s2 < 32u ? s2 : 32u)) >> 32);
    const uint64_t b = ~0ull << sat_sub(E, 96u);
    r.k[3] = ~(uint32_t)b;
    r.k[4] = ~(uint32_t)(b >> 32);
    return r;
}

}  // namespace lz4d
}  // namespace jfs
