// Fast LZ4 parse: the constants and the byte-size arithmetic that
// the kernels (lz4_fast.hip) and their host twin (lz4_fast_host.cc) share.
// The two restate the same algorithm; these are the numbers both must agree on.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JFS_LZ4F_HD __host__ __device__ __forceinline__
#else
#define JFS_LZ4F_HD inline
#endif

namespace jfs {
namespace lz4f {

constexpr int kChunkLog = 16;
constexpr int64_t kChunk = 1 << kChunkLog;  // independent parse unit; offsets fit u16
constexpr int kTile = 64;                   // positions searched at once (one per lane)
constexpr int kHashLog = 13;                // 8,192 u16 entries (liblz4's byU16 size)
constexpr int kNear = 4;                    // in-tile candidates: offsets 1..kNear tested directly
constexpr int kMinMatch = 4;
constexpr int kMfLimit = 12;    // no match starts within the last 12 bytes of the block
constexpr int kLastLits = 5;    // the last 5 bytes of the block are literals
constexpr int64_t kMaxInput = 0x7E000000;
constexpr int kMaxRec = (int)(kChunk / kMinMatch);  // sequences one chunk can hold

JFS_LZ4F_HD uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - kHashLog); }
// extra length bytes after a token nibble
JFS_LZ4F_HD int64_t len_bytes(int64_t v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }
JFS_LZ4F_HD int64_t nchunks(int64_t n) { return n <= 0 ? 1 : (n + kChunk - 1) >> kChunkLog; }

}  // namespace lz4f
}  // namespace jfs
