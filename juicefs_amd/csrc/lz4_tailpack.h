// One-word descriptor of a match left to the ordered tail of the LZ4 decode
// copier (batch() in lz4_decode.hip): the wave reads it with one lane read per
// match instead of three and branches on its sign.  Host and device:
// tests/test_lz4_tailpack.py drives tests/tailpack_main.cc over the whole
// stated range against the byte-wise definition of wave_near.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JFS_TAILPACK_HD __host__ __device__ __forceinline__
#else
#define JFS_TAILPACK_HD inline
#endif

namespace jfs {
namespace lz4d {

constexpr uint32_t TP_RING = 4096;      // ring bytes: slots take TP_SLOT_BITS bits
constexpr uint32_t TP_SLOT_BITS = 12;
constexpr uint32_t TP_LEN_MAX = 64;     // a lane-parallel match is at most this long (7 bits)
constexpr uint32_t TP_DIRECT = 0x80000000u;
static_assert((1u << TP_SLOT_BITS) == TP_RING, "a ring slot fills its field exactly");
static_assert(TP_LEN_MAX < (1u << (31 - 2 * TP_SLOT_BITS)), "length field: bits 24..30");

// ds, ss: ring slots (< TP_RING) of the first destination / source byte;
// rem: bytes left (1..TP_LEN_MAX); D: match distance (>= 1).
// Bits 0..11 ds, 12..23 ss, 24..30 rem, 31 direct.  Direct: the whole match
// is one chunk of wave_near (rem <= min(D, 64), i.e. rem <= D as rem <= 64)
// and neither byte range crosses the ring's end, so lane i < rem copies
// ring[ss + i] to ring[ds + i] with no mask and no step loop.
JFS_TAILPACK_HD uint32_t tail_pack(uint32_t ds, uint32_t ss, uint32_t rem, uint32_t D) {
    const bool direct = rem <= D && ss + rem <= TP_RING && ds + rem <= TP_RING;
    return ds | (ss << TP_SLOT_BITS) | (rem << (2 * TP_SLOT_BITS)) | (direct ? TP_DIRECT : 0u);
}
JFS_TAILPACK_HD bool tail_direct(uint32_t w) { return (int32_t)w < 0; }
JFS_TAILPACK_HD uint32_t tail_ds(uint32_t w) { return w & (TP_RING - 1u); }
JFS_TAILPACK_HD uint32_t tail_ss(uint32_t w) { return (w >> TP_SLOT_BITS) & (TP_RING - 1u); }
JFS_TAILPACK_HD uint32_t tail_rem(uint32_t w) { return (w >> (2 * TP_SLOT_BITS)) & 127u; }

}  // namespace lz4d
}  // namespace jfs
