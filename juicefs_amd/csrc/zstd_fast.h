// Fast Zstd parse: the constants, the chunk record and the
// block-local repeat-offset rule that the kernels (zstd_fast.hip) and their
// host twin (zstd_fast_host.cc) share.  The two restate the same parse; these
// are the numbers and the one rule both must agree on.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JFS_ZF_HD __host__ __device__ __forceinline__
#else
#define JFS_ZF_HD inline
#endif

namespace jfs {
namespace zfast {

constexpr int32_t kBlock = 128 << 10;      // Zstd block (zl1::BLK)
constexpr int kChunkLog = 16;
constexpr int32_t kChunk = 1 << kChunkLog;  // independent parse unit: at most two per block
constexpr int kTile = 64;                   // positions searched at once (one per lane)
constexpr int kHashLog = 13;                // 8,192 u16 entries
constexpr int kNear = 4;                    // in-tile candidates: offsets 1..kNear tested directly
constexpr int kMinMatch = 4;                // seq_cap(bsz) = bsz / 4 + 4 records rests on this
constexpr int kCapLen = kMinMatch + kTile;  // a lane extends its own match this far
constexpr int kMaxRec = kChunk / kMinMatch;  // sequences one chunk can hold
constexpr int32_t kNoCompBelow = 7;         // blocks under 7 bytes: F_NOCOMP (ZSTD_buildSeqStore)

// A match lies inside its chunk, so its offset is at most kChunk - 1 = 65,535.
// Every window a frame header of params_of can declare holds that: a frame of
// n <= 512 KiB is single-segment (window = n, and an offset never exceeds the
// match's own position), a larger one declares 1 << 19.
static_assert(kChunk - 1 <= 0xFFFF, "offsets and chunk positions must fit u16");
static_assert(2 * kChunk == kBlock, "a block is at most two chunks");

JFS_ZF_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashLog); }

// chunk record: {pos | mlen << 16, off | lit << 16}; pos, mlen, off and lit
// (the literals between the previous match of the chunk and this one) are u16
JFS_ZF_HD uint32_t rec_lo(uint32_t pos, uint32_t mlen) { return pos | mlen << 16; }
JFS_ZF_HD uint32_t rec_hi(uint32_t off, uint32_t lit) { return off | lit << 16; }

// sequence record of the entropy stage (zl1::seq_pack): ll | (ml - 3) << 17 | Offset_Value << 34
JFS_ZF_HD uint64_t seq_rec(uint32_t ll, uint32_t ml, uint32_t ofv) {
    return (uint64_t)ll | ((uint64_t)(ml - 3) << 17) | ((uint64_t)ofv << 34);
}

// The decoder's repeat-offset history (RFC 8878 3.1.1.5) as the encoder may
// rely on it: an entry is known only when a sequence of this block (or the
// frame's start values, in block 0) determined it.  Blocks before this one
// that end up raw or RLE leave the decoder's history alone and compressed
// ones move it, so what it holds at a later block's start depends on choices
// made after the parse; an unknown entry is never named by a repeat code.
struct RepHist {
    uint32_t v0, v1, v2;  // 0 = unknown (no offset is 0)
    JFS_ZF_HD void start(bool frame_start) {
        v0 = frame_start ? 1u : 0u;
        v1 = frame_start ? 4u : 0u;
        v2 = frame_start ? 8u : 0u;
    }
    // Offset_Value of a match at offset `off` after `ll` literals; moves the
    // history exactly as the decoder will
    JFS_ZF_HD uint32_t code(uint32_t ll, uint32_t off) {
        if (ll != 0) {
            if (off == v0) return 1;
            if (off == v1) {
                v1 = v0;
                v0 = off;
                return 2;
            }
            if (off == v2) {
                v2 = v1;
                v1 = v0;
                v0 = off;
                return 3;
            }
        } else {  // no literals: the codes mean repeat 2, repeat 3, repeat 1 minus 1
            if (off == v1) {
                v1 = v0;
                v0 = off;
                return 1;
            }
            if (off == v2) {
                v2 = v1;
                v1 = v0;
                v0 = off;
                return 2;
            }
            if (v0 > 1 && off == v0 - 1) {
                v2 = v1;
                v1 = v0;
                v0 = off;
                return 3;
            }
        }
        v2 = v1;
        v1 = v0;
        v0 = off;
        return off + 3;
    }
};

JFS_ZF_HD int64_t nblocks(int64_t n) { return (n + kBlock - 1) / kBlock; }

}  // namespace zfast
}  // namespace jfs
