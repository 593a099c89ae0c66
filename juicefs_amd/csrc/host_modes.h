// The run-time switches of the C ABI (include/jfs_gpucodec.h), each described
// once: the nine enumerated ones by environment name, default, accepted
// spellings and what their setters take; the two integer ones by name, default
// and closed range.  The initial value is read once from the environment,
// case-insensitively; an unknown or malformed value gives the default.  A
// setter answers the previous value, or -1 for a value it refuses, and then
// changes nothing.  Plain C++17, no HIP: tests/host_modes_main.cc runs the
// parse functions under the host sanitizers.
#pragma once
#include <ctype.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>

#include "../../include/jfs_gpucodec.h"

namespace jfs_host __attribute__((visibility("hidden"))) {

struct ModeWord {
    const char *word;  // lower case
    int value;
};
// An enumerated switch: its values are 0 .. ext_max.  The plain setter takes
// 0 .. set_max, the values the switch was introduced with; the _ext setter
// (where there is one) all of them.
struct ModeDesc {
    const char *env;
    int def;
    ModeWord words[3];  // unused entries: a null word
    int set_max, ext_max;
};
// An integer switch: a decimal in [lo, hi].
struct IntDesc {
    const char *env;
    int64_t def, lo, hi;
};

// the value `s` (the environment's, or null) gives the switch
inline int mode_parse(const ModeDesc &d, const char *s) {
    if (!s) return d.def;
    for (const ModeWord &w : d.words) {
        if (!w.word) continue;
        const char *a = s, *b = w.word;
        while (*b && (char)tolower((unsigned char)*a) == *b) a++, b++;
        if (!*a && !*b) return w.value;
    }
    return d.def;
}
inline int64_t int_parse(const IntDesc &d, const char *s) {
    if (!s) return d.def;
    char *end = nullptr;
    const long long v = strtoll(s, &end, 10);
    return end != s && *end == 0 && v >= d.lo && v <= d.hi ? (int64_t)v : d.def;
}

template <const ModeDesc &D>
struct Mode {
    static std::atomic<int> &var() {
        static std::atomic<int> m{mode_parse(D, getenv(D.env))};
        return m;
    }
    static int get() { return var().load(std::memory_order_relaxed); }
    static int set(int v) { return v < 0 || v > D.set_max ? -1 : var().exchange(v); }
    static int set_ext(int v) { return v < 0 || v > D.ext_max ? -1 : var().exchange(v); }
};
template <const IntDesc &D>
struct IntSwitch {
    static std::atomic<int64_t> &var() {
        static std::atomic<int64_t> m{int_parse(D, getenv(D.env))};
        return m;
    }
    static int64_t get() { return var().load(std::memory_order_relaxed); }
    static int64_t set(int64_t v) { return v < D.lo || v > D.hi ? -1 : var().exchange(v); }
};

// clang-format off
inline constexpr ModeDesc MODE_LZ4_PARSE{"JFS_LZ4_PARSE", JFS_LZ4_PARSE_EXACT,
    {{"exact", JFS_LZ4_PARSE_EXACT}, {"fast", JFS_LZ4_PARSE_FAST}, {nullptr, 0}}, JFS_LZ4_PARSE_FAST, JFS_LZ4_PARSE_FAST};
inline constexpr ModeDesc MODE_READ_DECODE{"JFS_READ_DECODE", JFS_READ_DECODE_FULL,
    {{"full", JFS_READ_DECODE_FULL}, {"prefix", JFS_READ_DECODE_PREFIX}, {"prefix-all", JFS_READ_DECODE_PREFIX_ALL}},
    JFS_READ_DECODE_PREFIX, JFS_READ_DECODE_PREFIX_ALL};
inline constexpr ModeDesc MODE_READ_SEEK{"JFS_READ_SEEK", JFS_READ_SEEK_OFF,
    {{"off", JFS_READ_SEEK_OFF}, {"on", JFS_READ_SEEK_ON}, {"sparse", JFS_READ_SEEK_SPARSE}},
    JFS_READ_SEEK_ON, JFS_READ_SEEK_SPARSE};
inline constexpr ModeDesc MODE_READ_LZ4_CHASE{"JFS_READ_LZ4_CHASE", JFS_READ_LZ4_CHASE_OFF,
    {{"off", JFS_READ_LZ4_CHASE_OFF}, {"on", JFS_READ_LZ4_CHASE_ON}, {nullptr, 0}},
    JFS_READ_LZ4_CHASE_ON, JFS_READ_LZ4_CHASE_ON};
inline constexpr ModeDesc MODE_READ_LZ4_WINDOW{"JFS_READ_LZ4_WINDOW", JFS_READ_LZ4_WINDOW_OFF,
    {{"off", JFS_READ_LZ4_WINDOW_OFF}, {"on", JFS_READ_LZ4_WINDOW_ON}, {nullptr, 0}},
    JFS_READ_LZ4_WINDOW_ON, JFS_READ_LZ4_WINDOW_ON};
inline constexpr ModeDesc MODE_ZSTD_PARSE{"JFS_ZSTD_PARSE", JFS_ZSTD_PARSE_EXACT,
    {{"exact", JFS_ZSTD_PARSE_EXACT}, {"fast", JFS_ZSTD_PARSE_FAST}, {"seekable", JFS_ZSTD_PARSE_SEEKABLE}},
    JFS_ZSTD_PARSE_FAST, JFS_ZSTD_PARSE_SEEKABLE};
inline constexpr ModeDesc MODE_ZSTD_SEEK_CSUM{"JFS_ZSTD_SEEK_CSUM", JFS_ZSTD_SEEK_CSUM_OFF,
    {{"off", JFS_ZSTD_SEEK_CSUM_OFF}, {"on", JFS_ZSTD_SEEK_CSUM_ON}, {nullptr, 0}},
    JFS_ZSTD_SEEK_CSUM_ON, JFS_ZSTD_SEEK_CSUM_ON};
inline constexpr ModeDesc MODE_COMPACT_SPLICE{"JFS_COMPACT_SPLICE", JFS_COMPACT_SPLICE_OFF,
    {{"off", JFS_COMPACT_SPLICE_OFF}, {"on", JFS_COMPACT_SPLICE_ON}, {"all", JFS_COMPACT_SPLICE_ALL}},
    JFS_COMPACT_SPLICE_ON, JFS_COMPACT_SPLICE_ALL};
inline constexpr ModeDesc MODE_COMPACT_LZ4_LIFT{"JFS_COMPACT_LZ4_LIFT", JFS_COMPACT_LZ4_LIFT_OFF,
    {{"off", JFS_COMPACT_LZ4_LIFT_OFF}, {"on", JFS_COMPACT_LZ4_LIFT_ON}, {nullptr, 0}},
    JFS_COMPACT_LZ4_LIFT_ON, JFS_COMPACT_LZ4_LIFT_ON};
// bytes per source, default 0 (the measured crossover)
inline constexpr IntDesc INT_LZ4_CHASE_MAX{"JFS_LZ4_CHASE_MAX", 0, 0, INT32_MAX};
inline constexpr IntDesc INT_ZSTD_SPLIT_FRAMES{"JFS_ZSTD_SPLIT_FRAMES", JFS_ZSTD_SPLIT_FRAMES_MAX, 1, JFS_ZSTD_SPLIT_FRAMES_MAX};
// clang-format on

using Lz4Parse = Mode<MODE_LZ4_PARSE>;
using ReadDecode = Mode<MODE_READ_DECODE>;
using ReadSeek = Mode<MODE_READ_SEEK>;
using ReadLz4Chase = Mode<MODE_READ_LZ4_CHASE>;
using ReadLz4Window = Mode<MODE_READ_LZ4_WINDOW>;
using ZstdParse = Mode<MODE_ZSTD_PARSE>;
using ZstdSeekCsum = Mode<MODE_ZSTD_SEEK_CSUM>;
using CompactSplice = Mode<MODE_COMPACT_SPLICE>;
using CompactLz4Lift = Mode<MODE_COMPACT_LZ4_LIFT>;
using Lz4ChaseMax = IntSwitch<INT_LZ4_CHASE_MAX>;
using ZstdSplitFrames = IntSwitch<INT_ZSTD_SPLIT_FRAMES>;

}  // namespace jfs_host
