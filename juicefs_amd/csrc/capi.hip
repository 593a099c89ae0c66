// libjfsgpu.so host side: the C ABI declared in include/jfs_gpucodec.h.
//
// Mirrors pkg/compress (compress.go:31-125) for the Go/cgo caller and adds the
// batch and device-resident entry points.  Every LZ4 byte is produced by the
// HIP kernels; if no gfx950 device is usable the codec calls fail with
// JFS_ERR_NO_DEVICE -- there is no CPU fallback.  Only the "none" codec is a
// host memcpy, because that is what noOp is (compress.go:55-68).
//
// Concurrency model (pkg/chunk runs up to 20 Compress + 200 Decompress calls
// at once, cmd/flags.go:133-139): single-block calls enqueue on a per-process
// coalescer; NLANE worker threads per device drain the queue, each gathering a
// burst of calls (a short gather window, Gather below) into one batch, and a
// device runs the next batch while the previous one is in flight (one lane of
// staging and streams per worker).  Batches go host -> pinned staging -> HBM
// -> kernel -> HBM -> pinned -> host, pipelined in chunks (run_batch).
#include <hip/hip_runtime.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/jfs_gpucodec_test.h"
#include "batch_plan.h"
#include "blockgen.h"
#include "chain_plan.h"
#include "jfs_internal.h"
#include "splice_plan.h"
#include "zstd_seek.h"

#define JFS_VERSION "jfs-gpucodec 0.1.0 (gfx950)"

namespace {

constexpr int64_t LZ4_MAX_INPUT = 0x7E000000;

using jfs_plan::align16;
using jfs_plan::envelope_parse;

// JFS_HOST_TRACE=1: per-chunk host timings on stderr (diagnostics)
bool host_trace() {
    static bool v = getenv("JFS_HOST_TRACE") != nullptr;
    return v;
}
double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// (trace) a staging or scratch allocation: hipFree waits for the whole device
void trace_alloc(const char *what, int64_t bytes, double t0) {
    if (host_trace())
        fprintf(stderr, "[jfs host] t=%.2f alloc %s %.1f MiB %.2f ms\n", now_ms(), what, bytes / 1048576.0,
                now_ms() - t0);
}

// One pinned host + device staging area: chunk k of a batch uses slot
// k % NSLOT, so chunk k+1's H2D and chunk k-1's D2H run while chunk k's
// kernel runs.  (Four slots measured 42.8 vs 42.0 GiB/s on a lone 4,096-block
// host-to-host decode, but 28 vs 41 right after a configs[0] round trip had
// grown the staging: kept at three.)
#ifndef JFS_NSLOT
#define JFS_NSLOT 3
#endif
constexpr int NSLOT = JFS_NSLOT;
static_assert(NSLOT >= 2, "the staging pipeline overlaps a chunk's copies with the next chunk's");
// disk-cache checksum piece (pkg/chunk/disk_cache_file.go:139-152: csBlock)
constexpr int64_t CSUM_SEG = 32 << 10;

// Upper bound on one slot's staging (JFS_STAGING_MAX_MB; default none): a
// request that needs more fails alone with JFS_ERR_NO_MEMORY.
// Footprint without a cap: a slot holds one chunk's input + output, at most
// the chunk limit (2 GiB decode, 4 GiB LZ4 / Zstd compress) plus one block;
// a lane has NSLOT = 3 slots and a device NLANE = 2 lanes, each slot pinned
// on the host and mirrored in HBM.  Peak per device: 2 x 3 x 4 GiB = 24 GiB
// pinned + 24 GiB HBM when both lanes run compress batches (e.g. LZ4 and Zstd
// at once), 12 + 12 GiB for two decode lanes; freed after JFS_STAGING_IDLE_MS
// of inactivity or by jfs_release_staging().  Hosts with less memory to pin
// set JFS_STAGING_MAX_MB (and JFS_HOST_CHUNK_MB[_LZ4C] to keep chunks under it).
int64_t staging_max_bytes() {
    static int64_t v = [] {
        const char *e = getenv("JFS_STAGING_MAX_MB");
        return e ? (int64_t)atoll(e) << 20 : INT64_MAX;
    }();
    return v;
}

// The output D2H of a (non-encrypted) chunk goes in up to NPIECE pieces, each
// with its own event, so the host copy-out of a piece overlaps the D2H of the
// next -- at the end of a batch only the last piece's copy-out is left.
#ifndef JFS_NPIECE
#define JFS_NPIECE 4
#endif
constexpr int NPIECE = JFS_NPIECE;

// Output pieces of a one-block chunk (a lone cache miss): its output D2H goes
// in NPIECE byte ranges and the caller copies each out as soon as it lands,
// spinning on the piece's event (a blocking wait per piece cost more than the
// overlap saved).  Lone 4 MiB one-call decode in the full bench: LZ4 0.81 ->
// 0.70 ms, Zstd 2.34 -> 2.23 ms (scripts/r6_bpiece3.sh).
// JFS_BYTE_PIECES=n overrides (0 or 1 = whole output).
int byte_npiece() {
    static int v = [] {
        const char *e = getenv("JFS_BYTE_PIECES");
        return e ? std::min(NPIECE, std::max(0, atoi(e))) : NPIECE;
    }();
    return v;
}

static_assert(NPIECE >= 1, "at least one output piece per chunk (finish() waits on ev_p[npiece - 1])");
struct Slot {
    hipEvent_t ev_in = nullptr, ev_k = nullptr, ev = nullptr;  // H2D done, kernel done, D2H done
    hipEvent_t ev_p[NPIECE] = {};                              // output piece p landed
    uint8_t *h = nullptr;
    int64_t h_cap = 0;
    uint8_t *d = nullptr;
    int64_t d_cap = 0;
    // Zstd decode scratch of this slot (planned on the host per chunk)
    uint8_t *z_lit = nullptr, *z_items = nullptr;
    uint16_t *z_tabs = nullptr;
    uint64_t z_lit_cap = 0, z_items_cap = 0, z_tabs_cap = 0;
    // small-batch decode scratch (LZ4: lz4_split.hip, Zstd: zstd_split.inc)
    uint8_t *sp = nullptr;
    int64_t sp_cap = 0;

    bool ensure_split(int64_t bytes) {
        if (bytes <= sp_cap) return true;
        const double t0 = host_trace() ? now_ms() : 0.0;
        if (sp) (void)hipFree(sp);
        sp = nullptr;
        sp_cap = 0;
        int64_t want = 64ll << 20;
        while (want < bytes) want <<= 1;
        if (hipMalloc((void **)&sp, (size_t)want) != hipSuccess) return false;
        sp_cap = want;
        trace_alloc("split", want, t0);
        return true;
    }

    bool ensure_zstd(const uint64_t *t) {  // t: items, literal bytes, table cells
        auto grow = [](auto **p, uint64_t *cap, uint64_t want, size_t elem) {
            if (*cap >= want) return true;
            const double t0 = host_trace() ? now_ms() : 0.0;
            if (*p) (void)hipFree(*p);
            *p = nullptr;
            *cap = 0;
            const uint64_t n = want + want / 4;
            if (hipMalloc((void **)p, (size_t)(n * elem)) != hipSuccess) return false;
            *cap = n;
            trace_alloc("zstd", (int64_t)(n * elem), t0);
            return true;
        };
        return grow(&z_items, &z_items_cap, t[0], 16) && grow(&z_lit, &z_lit_cap, t[1], 1) &&
               grow(&z_tabs, &z_tabs_cap, t[2], 2);
    }

    bool ensure(int64_t bytes) {
        // grow to the next power of two (at least 64 MiB): pinning costs about
        // 0.1 s per GiB, so a growing workload should re-pin rarely
        int64_t want = 64ll << 20;
        while (want < bytes) want <<= 1;
        if (bytes > staging_max_bytes()) return false;
        const double t0 = host_trace() ? now_ms() : 0.0;
        if (bytes > h_cap) {
            if (h) (void)hipHostFree(h);
            if (hipHostMalloc((void **)&h, (size_t)want, hipHostMallocDefault) != hipSuccess) {
                h = nullptr;
                h_cap = 0;
                return false;
            }
            h_cap = want;
            trace_alloc("pinned", want, t0);
        }
        if (bytes > d_cap) {
            if (d) (void)hipFree(d);
            if (hipMalloc((void **)&d, (size_t)want) != hipSuccess) {
                d = nullptr;
                d_cap = 0;
                return false;
            }
            d_cap = want;
            trace_alloc("device", want, t0);
        }
        return true;
    }
};

// Streams: a process gets GPU_MAX_HW_QUEUES (4 by default) hardware queues
// per device, and work on two streams that share one runs in submission
// order -- kernels "on different streams" then serialise (measured: five
// streams of one 0.5 s kernel each take 1.0 s; scripts/stream_probe.py).  So
// the library uses exactly four streams per device: one for every H2D copy,
// one for every D2H copy (a D2H waiting for its kernel must not hold up the
// next chunk's H2D), and one kernel stream per lane.
// A lane is one staging pipeline (NSLOT slots + its kernel stream); a device
// has NLANE of them, so a second batch (the coalescer's next one, or another
// caller's jfs_*_batch) runs while the first is still in flight.
struct Lane {
    std::mutex mu;  // serialises use of this lane's slots
    Slot slot[NSLOT];
    hipStream_t s_k = nullptr;  // this lane's kernels, in chunk order
    std::atomic<int> kind{-1};  // algo * 2 + dir of the batch it last ran (acquire_lane)
    // free the pinned host and HBM staging (caller holds mu)
    void release_staging() {
        for (Slot &sl : slot) {
            if (sl.h) (void)hipHostFree(sl.h);
            if (sl.d) (void)hipFree(sl.d);
            if (sl.z_lit) (void)hipFree(sl.z_lit);
            if (sl.z_items) (void)hipFree(sl.z_items);
            if (sl.z_tabs) (void)hipFree(sl.z_tabs);
            if (sl.sp) (void)hipFree(sl.sp);
            sl.sp = nullptr;
            sl.sp_cap = 0;
            sl.h = sl.d = sl.z_lit = sl.z_items = nullptr;
            sl.z_tabs = nullptr;
            sl.h_cap = sl.d_cap = 0;
            sl.z_lit_cap = sl.z_items_cap = sl.z_tabs_cap = 0;
        }
    }
    bool holds_staging() const {
        for (const Slot &sl : slot)
            if (sl.h || sl.d || sl.z_items || sl.sp) return true;
        return false;
    }
};
constexpr int NLANE = 2;

struct DevCtx {
    int id = -1;
    Lane lane[NLANE];
    hipStream_t s_in = nullptr, s_out = nullptr;  // all H2D / all D2H copies of the device
    std::atomic<unsigned> next_lane{0};
    std::mutex vocab_mu;
    uint8_t *d_vocab = nullptr;
    std::atomic<int64_t> last_use_ms{0};  // staging janitor: release after an idle period
    std::atomic<uint64_t> batches{0}, blocks{0};  // per-device counters (jfs_device_stats)

    // a lane for a batch call: a free one if any, else wait for one
    // (kind = algo * 2 + dir, or -1: a free lane that last ran the same kind
    // first, since its staging and scratch already fit such batches -- a lane
    // that must grow them waits on hipFree, i.e. on the whole device)
    Lane &acquire_lane(std::unique_lock<std::mutex> &lk, int kind = -1) {
        for (int pass = kind < 0 ? 1 : 0; pass < 2; pass++)
            for (int k = 0; k < NLANE; k++) {
                if (pass == 0 && lane[k].kind.load(std::memory_order_relaxed) != kind) continue;
                std::unique_lock<std::mutex> t(lane[k].mu, std::try_to_lock);
                if (t.owns_lock()) {
                    lk = std::move(t);
                    return lane[k];
                }
            }
        Lane &l = lane[next_lane.fetch_add(1) % NLANE];
        lk = std::unique_lock<std::mutex>(l.mu);
        return l;
    }
};

// The library never leaves the caller on another device: every entry point
// that selects a device restores the caller's current device on return (the
// caller's runtime -- e.g. PyTorch's current stream and events -- reads it).
struct DevGuard {
    int prev = -1;
    DevGuard() {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// JFS_GPU_CODEC (include/jfs_gpucodec.h): off | auto (default) | force
int gpu_mode() {
    static int m = [] {
        const char *e = getenv("JFS_GPU_CODEC");
        if (!e) return JFS_MODE_AUTO;
        std::string v(e);
        for (auto &ch : v) ch = (char)tolower((unsigned char)ch);
        if (v == "off" || v == "0" || v == "false") return JFS_MODE_OFF;
        if (v == "force") return JFS_MODE_FORCE;
        return JFS_MODE_AUTO;
    }();
    return m;
}

// JFS_LZ4_PARSE (include/jfs_gpucodec.h): exact (default) | fast
std::atomic<int> &lz4_parse() {
    static std::atomic<int> m{[] {
        const char *e = getenv("JFS_LZ4_PARSE");
        if (!e) return JFS_LZ4_PARSE_EXACT;
        std::string v(e);
        for (auto &ch : v) ch = (char)tolower((unsigned char)ch);
        return v == "fast" ? JFS_LZ4_PARSE_FAST : JFS_LZ4_PARSE_EXACT;
    }()};
    return m;
}
inline bool lz4_fast_mode() { return lz4_parse().load(std::memory_order_relaxed) == JFS_LZ4_PARSE_FAST; }

// JFS_READ_DECODE (include/jfs_gpucodec.h): full (default) | prefix | prefix-all
std::atomic<int> &read_decode() {
    static std::atomic<int> m{[] {
        const char *e = getenv("JFS_READ_DECODE");
        if (!e) return JFS_READ_DECODE_FULL;
        std::string v(e);
        for (auto &ch : v) ch = (char)tolower((unsigned char)ch);
        return v == "prefix" ? JFS_READ_DECODE_PREFIX : v == "prefix-all" ? JFS_READ_DECODE_PREFIX_ALL : JFS_READ_DECODE_FULL;
    }()};
    return m;
}

// JFS_READ_SEEK (include/jfs_gpucodec.h): off (default) | on | sparse
std::atomic<int> &read_seek() {
    static std::atomic<int> m{[] {
        const char *e = getenv("JFS_READ_SEEK");
        if (!e) return JFS_READ_SEEK_OFF;
        std::string v(e);
        for (auto &ch : v) ch = (char)tolower((unsigned char)ch);
        return v == "on" ? JFS_READ_SEEK_ON : v == "sparse" ? JFS_READ_SEEK_SPARSE : JFS_READ_SEEK_OFF;
    }()};
    return m;
}

// JFS_READ_LZ4_CHASE (include/jfs_gpucodec.h): off (default) | on
std::atomic<int> &read_lz4_chase() {
    static std::atomic<int> m{[] {
        const char *e = getenv("JFS_READ_LZ4_CHASE");
        if (!e) return JFS_READ_LZ4_CHASE_OFF;
        std::string v(e);
        for (auto &ch : v) ch = (char)tolower((unsigned char)ch);
        return v == "on" ? JFS_READ_LZ4_CHASE_ON : JFS_READ_LZ4_CHASE_OFF;
    }()};
    return m;
}

// JFS_LZ4_CHASE_MAX (include/jfs_gpucodec.h): bytes per source, default 0 (the measured crossover);
// anything else in the environment leaves the default
std::atomic<int64_t> &lz4_chase_max() {
    static std::atomic<int64_t> m{[] {
        const char *e = getenv("JFS_LZ4_CHASE_MAX");
        if (!e) return (int64_t)0;
        char *end = nullptr;
        const long long v = strtoll(e, &end, 10);
        return end != e && *end == 0 && v >= 0 && v <= INT32_MAX ? (int64_t)v : (int64_t)0;
    }()};
    return m;
}

// JFS_ZSTD_SPLIT_FRAMES (include/jfs_gpucodec.h): 1 .. 16384 (default 16384);
// anything else in the environment leaves the default
std::atomic<int> &zstd_split_frames() {
    static std::atomic<int> m{[] {
        const char *e = getenv("JFS_ZSTD_SPLIT_FRAMES");
        if (!e) return JFS_ZSTD_SPLIT_FRAMES_MAX;
        char *end = nullptr;
        const long v = strtol(e, &end, 10);
        return end != e && *end == 0 && v >= 1 && v <= JFS_ZSTD_SPLIT_FRAMES_MAX ? (int)v : JFS_ZSTD_SPLIT_FRAMES_MAX;
    }()};
    return m;
}

// JFS_ZSTD_PARSE (include/jfs_gpucodec.h): exact (default) | fast | seekable
std::atomic<int> &zstd_parse() {
    static std::atomic<int> m{[] {
        const char *e = getenv("JFS_ZSTD_PARSE");
        if (!e) return JFS_ZSTD_PARSE_EXACT;
        std::string v(e);
        for (auto &ch : v) ch = (char)tolower((unsigned char)ch);
        return v == "fast" ? JFS_ZSTD_PARSE_FAST : v == "seekable" ? JFS_ZSTD_PARSE_SEEKABLE : JFS_ZSTD_PARSE_EXACT;
    }()};
    return m;
}
inline int zstd_parse_now() { return zstd_parse().load(std::memory_order_relaxed); }

// JFS_ZSTD_SEEK_CSUM (include/jfs_gpucodec.h): off (default) | on
std::atomic<int> &zstd_seek_csum() {
    static std::atomic<int> m{[] {
        const char *e = getenv("JFS_ZSTD_SEEK_CSUM");
        if (!e) return JFS_ZSTD_SEEK_CSUM_OFF;
        std::string v(e);
        for (auto &ch : v) ch = (char)tolower((unsigned char)ch);
        return v == "on" ? JFS_ZSTD_SEEK_CSUM_ON : JFS_ZSTD_SEEK_CSUM_OFF;
    }()};
    return m;
}
// JFS_COMPACT_SPLICE (include/jfs_gpucodec.h): off (default) | on | all
std::atomic<int> &compact_splice() {
    static std::atomic<int> m{[] {
        const char *e = getenv("JFS_COMPACT_SPLICE");
        if (!e) return JFS_COMPACT_SPLICE_OFF;
        std::string v(e);
        for (auto &ch : v) ch = (char)tolower((unsigned char)ch);
        return v == "on" ? JFS_COMPACT_SPLICE_ON : v == "all" ? JFS_COMPACT_SPLICE_ALL : JFS_COMPACT_SPLICE_OFF;
    }()};
    return m;
}
// What a host-buffer compress call encodes with: the parse mode, or this value
// (no parse mode of the public switch) for seekable objects with checksums.
constexpr int ZSTD_ENCODE_SEEK_CSUM = 3;
inline int zstd_encode_now() {
    const int p = zstd_parse_now();
    return p == JFS_ZSTD_PARSE_SEEKABLE && zstd_seek_csum().load(std::memory_order_relaxed) == JFS_ZSTD_SEEK_CSUM_ON
               ? ZSTD_ENCODE_SEEK_CSUM
               : p;
}

// JFS_GPU_DEVICES: "all" (default), a comma list of ordinals, or a 0x mask
uint64_t device_select_mask() {
    const char *e = getenv("JFS_GPU_DEVICES");
    if (!e || !*e || !strcmp(e, "all")) return ~0ull;
    if (e[0] == '0' && (e[1] == 'x' || e[1] == 'X')) return strtoull(e + 2, nullptr, 16);
    uint64_t m = 0;
    for (const char *p = e; *p;) {
        char *end = nullptr;
        const long v = strtol(p, &end, 10);
        if (end == p) break;
        if (v >= 0 && v < 64) m |= 1ull << v;
        p = *end == ',' ? end + 1 : end;
    }
    return m;
}

// per-(algo, dir) counters behind jfs_stats()
struct OpStats {
    std::atomic<uint64_t> calls{0}, blocks{0}, bytes_in{0}, bytes_out{0}, errors{0}, nanos{0}, batches{0};
};
OpStats g_stats[JFS_STATS_N];

inline OpStats *op_stats(int algo, int dir) {
    return (algo >= 0 && algo <= 2 && (dir == 0 || dir == 1)) ? &g_stats[algo * 2 + dir] : nullptr;
}

int64_t steady_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// one host-path block's outcome
inline void stat_block(OpStats *st, int64_t in, int64_t out) {
    if (!st) return;
    st->blocks.fetch_add(1, std::memory_order_relaxed);
    if (out >= 0) {
        st->bytes_in.fetch_add((uint64_t)(in > 0 ? in : 0), std::memory_order_relaxed);
        st->bytes_out.fetch_add((uint64_t)out, std::memory_order_relaxed);
    } else {
        st->errors.fetch_add(1, std::memory_order_relaxed);
    }
}

// a host batch call that began at t0: the call, its time and, when it ran
// (rc), every block's outcome
inline void stat_call(int algo, int dir, int64_t rc, int nblk, const jfs_iov *iov, const int64_t *out_n, int64_t t0) {
    OpStats *st = op_stats(algo, dir);
    if (!st) return;
    st->calls.fetch_add(1, std::memory_order_relaxed);
    if (rc == JFS_OK)
        for (int i = 0; i < nblk; i++) stat_block(st, iov[i].src_len, out_n[i]);
    st->nanos.fetch_add((uint64_t)(steady_ns() - t0), std::memory_order_relaxed);
}

inline void stat_launch(int algo, int dir, int nblk) {
    if (OpStats *st = op_stats(algo, dir)) {
        st->calls.fetch_add(1, std::memory_order_relaxed);
        if (nblk > 0) st->blocks.fetch_add((uint64_t)nblk, std::memory_order_relaxed);
    }
}

std::once_flag g_once;
// never destroyed: the coalescer workers and the staging janitor are detached
// threads that may still look at it while static destructors run at exit
std::vector<DevCtx *> &g_devs = *new std::vector<DevCtx *>();
std::atomic<bool> g_exiting{false};

void init_devices() {
    if (gpu_mode() == JFS_MODE_OFF) return;
    DevGuard guard;
    const uint64_t sel = device_select_mask();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    for (int i = 0; i < n; i++) {
        if (i >= 64 || !((sel >> i) & 1ull)) continue;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, i) != hipSuccess) continue;
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) continue;
        DevCtx *d = new DevCtx();
        d->id = i;
        (void)hipSetDevice(i);
        bool ok = true;
        ok = ok && hipStreamCreateWithFlags(&d->s_in, hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipStreamCreateWithFlags(&d->s_out, hipStreamNonBlocking) == hipSuccess;
        for (Lane &ln : d->lane) {
            ok = ok && hipStreamCreateWithFlags(&ln.s_k, hipStreamNonBlocking) == hipSuccess;
            for (Slot &sl : ln.slot) {
                ok = ok && hipEventCreateWithFlags(&sl.ev_in, hipEventDisableTiming) == hipSuccess;
                ok = ok && hipEventCreateWithFlags(&sl.ev_k, hipEventDisableTiming) == hipSuccess;
                ok = ok && hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) == hipSuccess;
                for (hipEvent_t &e : sl.ev_p)
                    ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
            }
        }
        if (!ok) {
            delete d;
            continue;
        }
        g_devs.push_back(d);
    }
}

std::vector<DevCtx *> &devices() {
    std::call_once(g_once, init_devices);
    return g_devs;
}

int64_t steady_ms() {
    return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// Pinned staging (up to NSLOT x 2 GiB host + HBM per device) is released after
// JFS_STAGING_IDLE_MS (default 15 s; 0 = keep forever) without a batch, so an
// idle FUSE daemon does not hold it.  jfs_release_staging() frees it at once.
int64_t staging_idle_ms() {
    static int64_t v = [] {
        const char *e = getenv("JFS_STAGING_IDLE_MS");
        return e ? (int64_t)atoll(e) : (int64_t)15000;
    }();
    return v;
}

void release_lane_staging(DevCtx *d, Lane &ln) {
    (void)hipSetDevice(d->id);  // janitor thread / explicit release: no caller device to keep
    ln.release_staging();
}

// At exit the janitor must not call into a HIP runtime that is being torn
// down: the handler raises g_exiting and then takes every lane lock once,
// which waits out a release already in progress.
void on_exit_handler() {
    g_exiting = true;
    for (DevCtx *d : g_devs)
        for (Lane &ln : d->lane) {
            std::lock_guard<std::mutex> lk(ln.mu);
        }
}

void start_janitor() {
    static std::once_flag once;
    if (staging_idle_ms() <= 0) return;
    std::call_once(once, [] {
        atexit(on_exit_handler);
        std::thread([] {
            while (!g_exiting) {
                std::this_thread::sleep_for(std::chrono::milliseconds(std::min<int64_t>(1000, staging_idle_ms())));
                for (DevCtx *d : g_devs) {
                    if (steady_ms() - d->last_use_ms.load() < staging_idle_ms()) continue;
                    for (Lane &ln : d->lane) {
                        std::unique_lock<std::mutex> lk(ln.mu, std::try_to_lock);
                        if (!lk.owns_lock() || g_exiting) continue;
                        if (ln.holds_staging()) release_lane_staging(d, ln);
                    }
                }
            }
        }).detach();
    });
}

// crc32.Update(crc, crc32c, p[0:n]) on the host (pkg/object/checksum.go:30-45):
// table-driven, for the few hundred header bytes of an envelope and the
// "none" codec; block payloads are summed by crc32c.hip
uint32_t host_crc32c(uint32_t crc, const uint8_t *p, int64_t n) {
    static uint32_t tab[256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0x82F63B78u : 0u);
            tab[i] = c;
        }
    });
    crc = ~crc;
    for (int64_t i = 0; i < n; i++) crc = tab[(crc ^ p[i]) & 255u] ^ (crc >> 8);
    return ~crc;
}

enum Dir { COMPRESS = 0, DECOMPRESS = 1 };
constexpr int COMPRESS_DIR = COMPRESS, DECOMPRESS_DIR = DECOMPRESS;

// Per-block result conversion from the kernel's raw value to the C-ABI value.
// DataDog/zstd v1.5.6 decompressSizeHint: the first frame's content size if
// known and non-zero, else max(50*len(src), 1e6); capped at that bound.
int64_t zstd_size_hint(const uint8_t *src, int64_t n) {
    int64_t upper = std::max<int64_t>(50 * n, 1000000);
    int64_t hint = upper;
    if (n >= 5 && src[0] == 0x28 && src[1] == 0xB5 && src[2] == 0x2F && src[3] == 0xFD) {
        int fhd = src[4];
        int fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, did = fhd & 3;
        int64_t p = 5 + (single ? 0 : 1) + (did == 0 ? 0 : did == 1 ? 1 : did == 2 ? 2 : 4);
        int fs = fcs_flag == 0 ? (single ? 1 : 0) : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8;
        if (fs && p + fs <= n && !(fhd & 8)) {
            uint64_t v = 0;
            for (int i = 0; i < fs; i++) v |= (uint64_t)src[p + i] << (8 * i);
            if (fs == 2) v += 256;
            if (v > 0 && v < (uint64_t)INT64_MAX) hint = (int64_t)v;
        }
    }
    return std::min(hint, upper);
}

int64_t finish_result(int algo, int dir, int32_t raw) {
    if (algo == JFS_ALGO_LZ4) {
        if (dir == COMPRESS) return raw > 0 ? raw : JFS_ERR_COMPRESS_FAIL;
        return raw;  // LZ4_decompress_safe value, passed through like lz4.DecompressSafe
    }
    if (algo == JFS_ALGO_ZSTD) {
        if (raw >= 0) return raw;
        if (dir == COMPRESS) return raw == -2 ? JFS_ERR_SHORT_BUFFER : JFS_ERR_COMPRESS_FAIL;
        if (raw == -2) return JFS_ERR_SHORT_BUFFER;
        return JFS_ERR_CORRUPT;
    }
    return JFS_ERR_INVALID;
}

// Staged output capacity of one block (what the kernel may write).
int64_t staged_cap(int algo, int dir, const jfs_iov &v) {
    int64_t cap = v.dst_cap;
    // LZ4 compress: the kernel never writes at/after cap; stage at most the bound
    if (algo == JFS_ALGO_LZ4 && dir == COMPRESS) cap = std::min<int64_t>(cap, v.src_len + v.src_len / 255 + 16);
    // Zstd decompress with cap(dst) < DataDog's size hint: DataDog decodes into
    // a buffer of its own, so compress.go:99-101 answers "buffer too short"
    // unless the frames decode to nothing ((0, nil)) or are corrupt (their own
    // error).  Decoding into zero bytes of staging tells those three apart
    // without staging a size the caller cannot hold.
    if (algo == JFS_ALGO_ZSTD && dir == DECOMPRESS && cap < zstd_size_hint(v.src, v.src_len)) cap = 0;
    if (algo == JFS_ALGO_ZSTD && dir == COMPRESS) cap = std::min<int64_t>(cap, jfs_compress_bound(JFS_ALGO_ZSTD, v.src_len));
    // the kernels take int32 capacities (jfs_dev_block)
    return std::min<int64_t>(std::max<int64_t>(cap, 0), INT32_MAX);
}

// HBM/pinned bytes one block occupies in a chunk
int64_t staged_bytes(int algo, int dir, const jfs_iov &v) { return align16(v.src_len) + align16(staged_cap(algo, dir, v)); }

// Host staging chunk (input + output bytes per pipeline stage); default 2 GiB,
// JFS_HOST_CHUNK_MB overrides.  The decode kernel needs many blocks in flight
// (one workgroup per block), so chunks stay large.
int64_t chunk_limit() {
    static int64_t v = [] {
        const char *e = getenv("JFS_HOST_CHUNK_MB");
        long long mb = e ? atoll(e) : 2048;
        return (int64_t)std::max(mb, 16ll) << 20;
    }();
    return v;
}

// Decode chunk ramp (run_batch): the number of small first chunks (32, 64,
// 128, then 128 blocks); JFS_HOST_RAMP overrides (0 = off).
int host_ramp_len() {
    static int v = [] {
        const char *e = getenv("JFS_HOST_RAMP");
        return e ? std::min(8, std::max(0, atoi(e))) : 3;  // 32 << k stays well inside int
    }();
    return v;
}
// blocks in the first full chunk after the ramp (0: no cap)
#ifndef JFS_HOST_FIRST_BIG
#define JFS_HOST_FIRST_BIG 192
#endif

// LZ4 compress chunks: the serial-parse encoder holds 8 blocks per CU and a
// launch lasts one block's parse (~0.5 s) whatever its size, so a 2 GiB chunk
// (256 blocks at ~8 MiB staged each) fills an eighth of the GPU; 4 GiB chunks
// (512 blocks) with two chunk kernels side by side fill half of it.  The
// same holds for Zstd compress (one frame's serial parse, ~0.7 s at 4 MiB):
// a mixed 64 KiB-4 MiB batch in 1 GiB chunks paid its longest chain per chunk.
// JFS_HOST_CHUNK_MB_LZ4C overrides.
int64_t chunk_limit_lz4c() {
    static int64_t v = [] {
        const char *e = getenv("JFS_HOST_CHUNK_MB_LZ4C");
        long long mb = e ? atoll(e) : 4096;
        return (int64_t)std::max(mb, 16ll) << 20;
    }();
    return v;
}

// Batches of at most this many LZ4 decode blocks take the small-batch path
// (lz4_split.hip: every block spread over the whole GPU) instead of one
// workgroup per block; JFS_LZ4_SPLIT_MAX overrides (0 = never).
int split_max() {
    static int v = [] {
        const char *e = getenv("JFS_LZ4_SPLIT_MAX");
        return e ? std::max(0, atoi(e)) : 128;
    }();
    return v;
}

// memcpy jobs spread over host threads (pageable <-> pinned is CPU-bound)
struct CopyJob {
    uint8_t *dst;
    const uint8_t *src;
    int64_t n;
};
// One process-wide pool of copy threads shared by every lane of every device:
// concurrent batches (two lanes per GPU, up to eight GPUs) interleave their
// pieces instead of each spawning its own 16 threads, which oversubscribed the
// CPU quota (a 38 MiB stage-in took 65 ms next to another lane's copy-out).
// Size: JFS_COPY_THREADS, default min(16, CPUs this process may run on).
class CopyPool {
   public:
    static CopyPool &get() {
        static CopyPool *p = new CopyPool();  // never destroyed: workers outlive static dtors
        return *p;
    }
    int threads() const { return nthr_; }
    void run(std::vector<CopyJob> &pc) {
        Task t;
        t.pc = pc.data();
        t.n = pc.size();
        {
            std::lock_guard<std::mutex> lk(mu_);
            q_.push_back(&t);
        }
        cv_.notify_all();
        work(t);  // the caller copies too
        std::unique_lock<std::mutex> lk(mu_);
        q_.erase(std::find(q_.begin(), q_.end(), &t));  // no worker picks it up any more
        done_cv_.wait(lk, [&] { return t.done.load() == t.n && t.active == 0; });
    }

   private:
    struct Task {
        CopyJob *pc = nullptr;
        size_t n = 0;
        std::atomic<size_t> next{0}, done{0};
        int active = 0;  // workers inside work(*this) (guarded by mu_)
    };
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::deque<Task *> q_;
    int nthr_ = 1;

    static int cpu_share() {
        cpu_set_t set;
        CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof(set), &set) == 0) return std::max(1, CPU_COUNT(&set));
        return (int)std::max(1u, std::thread::hardware_concurrency());
    }
    CopyPool() {
        const char *e = getenv("JFS_COPY_THREADS");
        nthr_ = e ? std::max(1, atoi(e)) : std::min(16, cpu_share());
        for (int i = 1; i < nthr_; i++) std::thread([this] { loop(); }).detach();
    }
    static void work(Task &t) {
        for (size_t i; (i = t.next.fetch_add(1)) < t.n;) {
            memcpy(t.pc[i].dst, t.pc[i].src, (size_t)t.pc[i].n);
            t.done.fetch_add(1);
        }
    }
    void loop() {
        for (;;) {
            Task *t = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] {
                    for (Task *x : q_)
                        if (x->next.load() < x->n) return true;
                    return false;
                });
                for (Task *x : q_)  // the oldest task with pieces left
                    if (x->next.load() < x->n) { t = x; break; }
                if (t) t->active++;
            }
            if (!t) continue;
            work(*t);
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (--t->active == 0) done_cv_.notify_all();
            }
        }
    }
};

void par_copy(std::vector<CopyJob> &jobs) {
    int64_t total = 0;
    for (const CopyJob &j : jobs) total += j.n;
    CopyPool &pool = CopyPool::get();
    if (total < (16ll << 20) || pool.threads() == 1) {
        for (const CopyJob &j : jobs) memcpy(j.dst, j.src, (size_t)j.n);
        return;
    }
    // cut into <= 4 MiB pieces, handed out one at a time
    constexpr int64_t PIECE = 4ll << 20;
    std::vector<CopyJob> pc;
    for (const CopyJob &j : jobs)
        for (int64_t o = 0; o < j.n; o += PIECE) pc.push_back({j.dst + o, j.src + o, std::min(PIECE, j.n - o)});
    pool.run(pc);
}

// LZ4 encode batches of at most this many blocks take the segment-parallel
// parse (lz4_encode.hip, lz4_eseg): latency of a few segment parses instead of
// one whole-block parse per wave
int eseg_max() {
    static int v = [] {
        const char *e = getenv("JFS_LZ4E_SEG_MAX");
        return e ? atoi(e) : 256;
    }();
    return v;
}

// zparse: the Zstd parse mode of the call this launch belongs to (Zstd compress only)
int launch_kernel(int algo, int dir, const jfs_dev_block *d_desc, int nblk, int32_t *d_ret, hipStream_t st,
                  int zparse) {
    if (algo == JFS_ALGO_LZ4 && dir == DECOMPRESS) return jfs_launch_lz4_decode(d_desc, nblk, d_ret, st);
    if (algo == JFS_ALGO_LZ4 && dir == COMPRESS) return jfs_launch_lz4_encode(d_desc, nblk, d_ret, st);
    if (algo == JFS_ALGO_ZSTD && dir == DECOMPRESS) return jfs_launch_zstd_decode(d_desc, nblk, d_ret, nullptr, st);
    if (algo == JFS_ALGO_ZSTD && dir == COMPRESS)
        return zparse == ZSTD_ENCODE_SEEK_CSUM ? jfs_launch_zstd_encode_seek_csum(d_desc, nblk, d_ret, st)
                                               : jfs_launch_zstd_encode(d_desc, nblk, d_ret, st, zparse);
    return -1;
}

// Object encryption around the codec (pkg/object/encrypt.go
// dataEncryptor, installed after compression on PUT and before decompression
// on GET, cmd/format.go:289-302).  Arrays are parallel to the iov run_batch
// gets (whose src/src_len/dst_cap are the staged payload and capacity); orig
// holds the caller's buffers, which receive the envelope (seal) or the
// plaintext block (open).
struct Aead {
    int cipher;
    bool seal;
    const jfs_iov *orig;
    const uint8_t *const *key;    // data key per block
    const uint8_t *const *nonce;  // 12-byte nonce per block
    const jfs_seal_param *sp;     // seal: wrapped key per block
    const int64_t *hdr;           // seal: header bytes per block
    Aead at(int64_t h) const {
        Aead a = *this;
        a.orig += h;
        a.key += h;
        a.nonce += h;
        if (a.sp) a.sp += h;
        if (a.hdr) a.hdr += h;
        return a;
    }
};

// The envelope header of one sealed block (encrypt.go:244-254:
// be16(len(wrapped)) | len(nonce) | wrapped | nonce), host-known: its CRC-32C
// (the seed of the payload's checksum on the device) and its bytes
uint32_t seal_header_crc(const jfs_seal_param &p) {
    const uint8_t h3[3] = {(uint8_t)(p.wrapped_len >> 8), (uint8_t)(p.wrapped_len & 0xFF), 12};
    uint32_t v = host_crc32c(0, h3, 3);
    v = host_crc32c(v, p.wrapped, p.wrapped_len);
    return host_crc32c(v, p.nonce, 12);
}
void seal_header_write(uint8_t *dst, const jfs_seal_param &p) {
    dst[0] = (uint8_t)(p.wrapped_len >> 8);
    dst[1] = (uint8_t)(p.wrapped_len & 0xFF);
    dst[2] = 12;
    if (p.wrapped_len > 0) memcpy(dst + 3, p.wrapped, (size_t)p.wrapped_len);
    memcpy(dst + 3 + p.wrapped_len, p.nonce, 12);
}

// What every run on a lane begins and ends with: the caller's device is kept
// and the lane's selected, the device's counters and idle clock move on, the
// staging janitor runs; the idle clock starts anew when the run ends.
struct LaneRun {
    DevGuard guard;
    DevCtx *dev;
    LaneRun(DevCtx *d, Lane &ln, int kind, uint64_t nblk) : dev(d) {
        (void)hipSetDevice(d->id);
        d->last_use_ms = steady_ms();
        ln.kind.store(kind, std::memory_order_relaxed);
        d->batches.fetch_add(1, std::memory_order_relaxed);
        d->blocks.fetch_add(nblk, std::memory_order_relaxed);
        start_janitor();
    }
    ~LaneRun() { dev->last_use_ms = steady_ms(); }
};

inline int64_t launch_rc(int lk) { return lk == 0 ? JFS_OK : JFS_ERR_HIP; }

// src_len / dst_cap of staged descriptors, as the small-batch launchers take them
std::vector<int32_t> desc_lens(const jfs_dev_block *h_desc, int n) {
    std::vector<int32_t> v(n);
    for (int k = 0; k < n; k++) v[k] = h_desc[k].src_len;
    return v;
}
std::vector<int32_t> desc_caps(const jfs_dev_block *h_desc, int n) {
    std::vector<int32_t> v(n);
    for (int k = 0; k < n; k++) v[k] = h_desc[k].dst_cap;
    return v;
}

// LZ4 encode of n staged blocks (h_desc = d_desc's host copy): the fast parse
// when `fast`, else the segment-parallel parse for small batches (eseg_max)
// and one whole-block parse per wave for large ones.  lz4_encode_scratch: the
// slot scratch that launch will ask for (a caller that shares a slot's scratch
// between launches sizes it first: growing it waits for the whole device).
int64_t lz4_encode_scratch(int n, const int32_t *lens, bool fast) {
    if (fast) return jfs_lz4_fast_scratch_bytes(n, lens);
    return n <= eseg_max() ? jfs_lz4_eseg_scratch_bytes(n, lens) : 0;
}
int64_t launch_lz4_encode(Slot &sl, const jfs_dev_block *h_desc, const jfs_dev_block *d_desc, int n, int32_t *d_ret,
                          hipStream_t st, bool fast) {
    if (!fast && n > eseg_max()) return launch_rc(jfs_launch_lz4_encode(d_desc, n, d_ret, st));
    const std::vector<int32_t> lens = desc_lens(h_desc, n);
    if (!sl.ensure_split(lz4_encode_scratch(n, lens.data(), fast))) return JFS_ERR_NO_MEMORY;
    return launch_rc(fast ? jfs_launch_lz4_fast(d_desc, n, lens.data(), d_ret, sl.sp, sl.sp_cap, st)
                          : jfs_launch_lz4_encode_seg(d_desc, n, lens.data(), d_ret, sl.sp, sl.sp_cap, st));
}

static_assert(jfs_plan::LZ4_SPLIT_SEG == JFS_LZ4_SPLIT_SEG, "batch_plan.h restates the small-batch segment size");

// LZ4 decode of n staged blocks: the small-batch path up to split_max()
// blocks, else one workgroup per block.  lz4_decode_scratch: the slot scratch
// that launch will ask for (lens / caps: the descriptors' src_len / dst_cap).
int64_t lz4_decode_scratch(int n, const int32_t *lens, const int32_t *caps) {
    return n <= split_max() ? jfs_lz4_split_scratch_bytes(n, lens, caps) : 0;
}
int64_t launch_lz4_decode(Slot &sl, const jfs_dev_block *h_desc, const jfs_dev_block *d_desc, int n, int32_t *d_ret,
                          hipStream_t st) {
    if (n > split_max()) return launch_rc(jfs_launch_lz4_decode(d_desc, n, d_ret, st));
    const std::vector<int32_t> lens = desc_lens(h_desc, n), caps = desc_caps(h_desc, n);
    if (!sl.ensure_split(lz4_decode_scratch(n, lens.data(), caps.data()))) return JFS_ERR_NO_MEMORY;
    const jfs_plan::Lz4SplitGeom g = jfs_plan::lz4_split_geom(n, lens.data(), caps.data());
    return launch_rc(jfs_launch_lz4_split(d_desc, n, d_ret, sl.sp, g.nseg, g.max_cap, g.norg, st));
}
// The same choice for a prefix decode: block k stops at d_want[k] output bytes
// (max_want: the largest of them, known on the host).  The scratch is
// lz4_decode_scratch's.
int64_t launch_lz4_decode_prefix(Slot &sl, const jfs_dev_block *h_desc, const jfs_dev_block *d_desc, int n,
                                 int32_t *d_ret, const int32_t *d_want, int64_t max_want, hipStream_t st) {
    if (n > split_max()) return launch_rc(jfs_launch_lz4_decode_prefix(d_desc, n, d_ret, d_want, nullptr, st));
    const std::vector<int32_t> lens = desc_lens(h_desc, n), caps = desc_caps(h_desc, n);
    if (!sl.ensure_split(lz4_decode_scratch(n, lens.data(), caps.data()))) return JFS_ERR_NO_MEMORY;
    const jfs_plan::Lz4SplitGeom g = jfs_plan::lz4_split_geom(n, lens.data(), caps.data());
    return launch_rc(
        jfs_launch_lz4_split_prefix(d_desc, n, d_ret, d_want, sl.sp, g.nseg, g.max_cap, g.norg, max_want, st));
}

// One run_batch call: the chunk plan (batch_plan.h), every chunk's staging
// layout and the call's options; launch(k) queues chunk k, finish(k) waits for
// it and hands its results and outputs to the caller.  Every pointer into a
// slot's staging comes from the chunk's ChunkLayout, applied to the pinned
// (sl.h) and the HBM (sl.d) copy alike.
struct BatchRun {
    using Chunk = jfs_plan::Chunk;
    using Layout = jfs_plan::ChunkLayout;

    DevCtx *const dev;
    Lane &ln, &other;  // chunk kernels alternate between the two lanes' kernel streams
    const int algo, dir;
    const jfs_iov *const iov;
    int64_t *const out;
    const Aead *const ae;
    uint32_t *const crc_out;
    uint8_t *const *const csum_out;  // decode-side disk-cache checksums, or null
    const bool zplan;                // Zstd decode: the per-input scratch plan (ZInfo) rides in the chunk
    const int64_t zib;
    const bool lz4_fast;  // the parse mode when this batch started
    const int zparse;     // and the Zstd one
    const jfs_plan::Pieces pieces{NPIECE, byte_npiece()};
    std::vector<jfs_plan::Block> blk;  // staged input bytes and capacity per block
    jfs_plan::Plan plan;
    std::vector<Layout> lay;  // per chunk

    BatchRun(DevCtx *dev, Lane &ln, int algo, int dir, int nblk, const jfs_iov *iov, int64_t *out, const Aead *ae,
             uint32_t *crc_out, int max_chunk_blocks, uint8_t *const *csum)
        : dev(dev), ln(ln), other(dev->lane[(&ln - dev->lane + 1) % NLANE]), algo(algo), dir(dir), iov(iov), out(out),
          ae(ae), crc_out(crc_out), csum_out(dir == DECOMPRESS ? csum : nullptr),
          zplan(algo == JFS_ALGO_ZSTD && dir == DECOMPRESS && !ae), zib(zplan ? (int64_t)jfs_zstd_info_bytes() : 0),
          lz4_fast(lz4_fast_mode()), zparse(zstd_encode_now()), blk(nblk) {
        for (int i = 0; i < nblk; i++) blk[i] = {iov[i].src_len, ae ? iov[i].dst_cap : staged_cap(algo, dir, iov[i])};
        const int64_t limit =
            (algo == JFS_ALGO_LZ4 || algo == JFS_ALGO_ZSTD) && dir == COMPRESS && !ae ? chunk_limit_lz4c()
                                                                                      : chunk_limit();
        const bool ramp_ok = dir == DECOMPRESS && !ae && max_chunk_blocks <= 0;
        plan = jfs_plan::plan_chunks(blk.data(), nblk,
                                     {limit, max_chunk_blocks, ramp_ok, host_ramp_len(), JFS_HOST_FIRST_BIG, NSLOT});
        lay.reserve(plan.ch.size());
        for (const Chunk &c : plan.ch)
            lay.emplace_back(c.e - c.s, c.tin, c.tout, zib, ae != nullptr, crc_out != nullptr, csum_out != nullptr,
                             csum_out ? csum_bytes(c) : 0);
    }

    // Chunk kernels alternate between this lane's kernel stream and the other
    // lane's: an encode launch lasts one block's latency (~0.5 s) whatever its
    // size, so two chunks' kernels must run side by side (a device has only
    // two kernel streams: see Lane).
    hipStream_t kstream(int k) const { return (k & 1) ? other.s_k : ln.s_k; }
    bool h2d(void *d, const void *h, int64_t n) const {
        return hipMemcpyAsync(d, h, (size_t)n, hipMemcpyHostToDevice, dev->s_in) == hipSuccess;
    }
    bool d2h(void *h, const void *d, int64_t n) const {
        return hipMemcpyAsync(h, d, (size_t)n, hipMemcpyDeviceToHost, dev->s_out) == hipSuccess;
    }
    // what block i's codec descriptor holds (launch), known before it is staged (presize)
    int32_t desc_len(int i) const { return (int32_t)iov[i].src_len; }
    int32_t desc_cap(int i) const { return (int32_t)std::min<int64_t>(blk[i].cap, INT32_MAX); }
    // a block's disk-cache checksums: ((cap-1)/32 KiB+1)*4 bytes, 16-aligned in the chunk's area
    int64_t csum_words(int i) const { return blk[i].cap > 0 ? (blk[i].cap - 1) / CSUM_SEG + 1 : 1; }
    int64_t csum_bytes(const Chunk &c) const {
        int64_t t = 0;
        for (int i = c.s; i < c.e; i++) t += align16(4 * csum_words(i));
        return t;
    }

    // stage the checksum descriptors (the decoded output is the data, the
    // checksum bytes go to the chunk's checksum area) and queue their H2D
    bool stage_csum(const Chunk &c, const Layout &L, Slot &sl) const {
        if (!csum_out) return true;
        jfs_dev_block *h_cd = Layout::at<jfs_dev_block>(sl.h, L.csum_desc);
        uint8_t *d_out = Layout::at(sl.d, L.out), *d_area = Layout::at(sl.d, L.csum);
        for (int i = c.s; i < c.e; i++) {
            const int64_t bytes = 4 * csum_words(i);
            h_cd[i - c.s] = jfs_dev_block{d_out + plan.out_off[i], d_area, 0, (int32_t)bytes};
            d_area += align16(bytes);
        }
        return h2d(Layout::at(sl.d, L.csum_desc), h_cd, (int64_t)(c.e - c.s) * (int64_t)sizeof(jfs_dev_block));
    }
    bool run_csum(const Chunk &c, const Layout &L, Slot &sl, const int32_t *d_lens, hipStream_t ks) const {
        const jfs_dev_block *d_cd = Layout::at<jfs_dev_block>(sl.d, L.csum_desc);
        return !csum_out || jfs_launch_crc32c_segs_lens(d_cd, c.e - c.s, CSUM_SEG, d_lens, ks) == 0;
    }
    bool fetch_csum(const Layout &L, Slot &sl) const {
        return !csum_out || d2h(Layout::at(sl.h, L.csum), Layout::at(sl.d, L.csum), L.csum_bytes);
    }
    // PUT-payload checksums: stage the descriptors (payload = the codec's
    // output area) and the seeds (the envelope header's CRC for a seal) and
    // queue their H2D; after the kernels the checksum launch (lengths from the
    // device), then its D2H
    bool stage_crc(const Chunk &c, const Layout &L, Slot &sl) const {
        if (!crc_out) return true;
        jfs_dev_block *h_cd = Layout::at<jfs_dev_block>(sl.h, L.crc_desc);
        uint32_t *h_seed = Layout::at<uint32_t>(sl.h, L.crc_seed);
        for (int i = c.s; i < c.e; i++) {
            const int k = i - c.s;
            h_cd[k] = jfs_dev_block{Layout::at(sl.d, L.out) + plan.out_off[i], nullptr, 0, 0};
            h_seed[k] = ae && ae->seal ? seal_header_crc(ae->sp[i]) : 0;
        }
        return h2d(Layout::at(sl.d, L.crc_desc), h_cd, L.crc - L.crc_desc);  // descriptors and seeds
    }
    bool run_crc(const Chunk &c, const Layout &L, Slot &sl, const int32_t *d_lens, hipStream_t ks) const {
        const jfs_dev_block *d_cd = Layout::at<jfs_dev_block>(sl.d, L.crc_desc);
        uint32_t *d_seed = Layout::at<uint32_t>(sl.d, L.crc_seed), *d_crc = Layout::at<uint32_t>(sl.d, L.crc);
        return !crc_out || jfs_launch_crc32c_lens(d_cd, c.e - c.s, d_lens, d_seed, d_crc, ks) == 0;
    }
    bool fetch_crc(const Chunk &c, const Layout &L, Slot &sl) const {
        return !crc_out || d2h(Layout::at(sl.h, L.crc), Layout::at(sl.d, L.crc), (int64_t)(c.e - c.s) * 4);
    }

    // Size every slot for all of its chunks (staging, LZ4 small-batch scratch)
    // before the first launch: growing a slot mid-batch frees the old buffer,
    // and hipFree waits for the whole device -- the batch's own chunks in
    // flight (64 ms of a 273 ms 1,024-block decode).  A size that cannot be
    // had is left to the chunk's own ensure(), which reports it.
    void presize() {
        int64_t need[NSLOT] = {}, need_sp[NSLOT] = {};
        for (size_t k = 0; k < plan.ch.size(); k++) {
            const Chunk &c = plan.ch[k];
            need[c.slot] = std::max(need[c.slot], lay[k].total);
            const int n = c.e - c.s;
            if (algo == JFS_ALGO_LZ4 && dir == DECOMPRESS && !ae) {
                std::vector<int32_t> lens(n), caps(n);
                for (int i = 0; i < n; i++) {
                    lens[i] = desc_len(c.s + i);
                    caps[i] = desc_cap(c.s + i);
                }
                need_sp[c.slot] = std::max(need_sp[c.slot], lz4_decode_scratch(n, lens.data(), caps.data()));
            }
        }
        for (int s = 0; s < NSLOT; s++) {
            if (need[s] > 0) (void)ln.slot[s].ensure(need[s]);
            if (need_sp[s] > 0) (void)ln.slot[s].ensure_split(need_sp[s]);
        }
    }

    // Stage a chunk and queue its H2D (s_in), kernels (its kernel stream) and D2H (s_out).
    int64_t launch(int chunk) {
        const Chunk &c = plan.ch[chunk];
        const Layout &L = lay[chunk];
        Slot &sl = ln.slot[c.slot];
        if (!sl.ensure(L.total)) return JFS_ERR_NO_MEMORY;
        const hipStream_t ks = kstream(chunk);
        const int n = c.e - c.s;
        uint8_t *h_in = Layout::at(sl.h, L.in), *h_out = Layout::at(sl.h, L.out);
        uint8_t *d_in = Layout::at(sl.d, L.in), *d_out = Layout::at(sl.d, L.out);
        jfs_dev_block *h_desc = Layout::at<jfs_dev_block>(sl.h, L.desc);
        jfs_dev_block *d_desc = Layout::at<jfs_dev_block>(sl.d, L.desc);
        int32_t *h_ret = Layout::at<int32_t>(sl.h, L.ret), *d_ret = Layout::at<int32_t>(sl.d, L.ret);
        for (int i = c.s; i < c.e; i++)
            h_desc[i - c.s] = jfs_dev_block{d_in + plan.in_off[i], d_out + plan.out_off[i], desc_len(i), desc_cap(i)};
        const double t0 = host_trace() ? now_ms() : 0.0;
        // Stage the inputs in pieces (NPIECE), each piece's H2D issued as soon as
        // it is staged so that it overlaps the staging of the next (the
        // encrypted path stages everything first: launch_aead issues its H2D).
        for (int p = 0; p < pieces.in_npiece(c); p++) {
            const int b0 = pieces.in_piece_b(c, p), b1 = pieces.in_piece_b(c, p + 1);
            std::vector<CopyJob> jobs;
            for (int i = b0; i < b1; i++)
                if (iov[i].src_len > 0) jobs.push_back({h_in + plan.in_off[i], iov[i].src, iov[i].src_len});
            par_copy(jobs);
            if (ae) continue;
            const int64_t o0 = plan.in_off[b0], o1 = b1 < c.e ? plan.in_off[b1] : c.tin;
            if (o1 > o0 && !h2d(d_in + o0, h_in + o0, o1 - o0)) return JFS_ERR_HIP;
        }
        if (host_trace())
            fprintf(stderr, "[jfs host] t=%.2f lane %d algo %d dir %d chunk %d-%d stage-in %.1f MiB %.2f ms\n",
                    now_ms(), (int)(&ln - dev->lane), algo, dir, c.s, c.e, c.tin / 1048576.0, now_ms() - t0);
        if (ae) return launch_aead(c, L, sl, ks);
        if (algo != JFS_ALGO_LZ4 && algo != JFS_ALGO_ZSTD) return JFS_ERR_UNSUPPORTED;
        uint64_t ztot[6] = {0, 0, 0, 0, 0, 0};
        uint8_t *h_zi = Layout::at(sl.h, L.zinfo), *d_zi = Layout::at(sl.d, L.zinfo);
        if (zplan) {  // plan the Zstd scratch from the staged inputs: no device round trip
            std::vector<const uint8_t *> srcs(n);
            for (int i = 0; i < n; i++) srcs[i] = h_in + plan.in_off[c.s + i];
            jfs_zstd_plan_host(srcs.data(), desc_lens(h_desc, n).data(), desc_caps(h_desc, n).data(), n, h_zi, ztot);
            if (!sl.ensure_zstd(ztot)) return JFS_ERR_NO_MEMORY;
            if (jfs_zstd_split_ok(n, ztot) && !sl.ensure_split(jfs_zstd_split_bytes(n, ztot))) return JFS_ERR_NO_MEMORY;
        }
        if (!h2d(d_desc, h_desc, (int64_t)n * (int64_t)sizeof(jfs_dev_block))) return JFS_ERR_HIP;
        if (zplan && !h2d(d_zi, h_zi, n * zib)) return JFS_ERR_HIP;
        if (dir == COMPRESS && !stage_crc(c, L, sl)) return JFS_ERR_HIP;
        if (!stage_csum(c, L, sl)) return JFS_ERR_HIP;
        if (hipEventRecord(sl.ev_in, dev->s_in) != hipSuccess) return JFS_ERR_HIP;
        if (hipStreamWaitEvent(ks, sl.ev_in, 0) != hipSuccess) return JFS_ERR_HIP;
        int64_t r;
        if (zplan)
            r = launch_rc(jfs_launch_zstd_decode_planned(d_desc, n, d_ret, d_zi, sl.z_lit, sl.z_tabs, sl.z_items,
                                                         jfs_zstd_split_ok(n, ztot) ? sl.sp : nullptr, ztot, ks));
        else if (algo == JFS_ALGO_LZ4 && dir == DECOMPRESS)
            r = launch_lz4_decode(sl, h_desc, d_desc, n, d_ret, ks);
        else if (algo == JFS_ALGO_LZ4)
            r = launch_lz4_encode(sl, h_desc, d_desc, n, d_ret, ks, lz4_fast);
        else
            r = launch_rc(launch_kernel(algo, dir, d_desc, n, d_ret, ks, zparse));
        if (r != JFS_OK) return r;
        if (dir == COMPRESS && !run_crc(c, L, sl, d_ret, ks)) return JFS_ERR_HIP;
        if (!run_csum(c, L, sl, d_ret, ks)) return JFS_ERR_HIP;
        if (hipEventRecord(sl.ev_k, ks) != hipSuccess) return JFS_ERR_HIP;
        if (hipStreamWaitEvent(dev->s_out, sl.ev_k, 0) != hipSuccess) return JFS_ERR_HIP;
        if (!d2h(h_ret, d_ret, (int64_t)n * 4)) return JFS_ERR_HIP;
        if (dir == COMPRESS && !fetch_crc(c, L, sl)) return JFS_ERR_HIP;
        if (!fetch_csum(L, sl)) return JFS_ERR_HIP;
        for (int p = 0; p < pieces.npiece(c); p++) {  // output bytes [piece_o(c, p), piece_o(c, p + 1))
            const int64_t o0 = pieces.piece_o(c, p, plan.out_off.data());
            const int64_t o1 = pieces.piece_o(c, p + 1, plan.out_off.data());
            if (o1 > o0 && !d2h(h_out + o0, d_out + o0, o1 - o0)) return JFS_ERR_HIP;
            if (hipEventRecord(sl.ev_p[p], dev->s_out) != hipSuccess) return JFS_ERR_HIP;
        }
        if (hipEventRecord(sl.ev, dev->s_out) != hipSuccess) return JFS_ERR_HIP;
        return JFS_OK;
    }

    // compress -> seal, or open -> decompress (the staged inputs and the
    // codec descriptors are already in place; run on the chunk's kernel stream)
    int64_t launch_aead(const Chunk &c, const Layout &L, Slot &sl, hipStream_t ks) {
        const int n = c.e - c.s;
        uint8_t *d_in = Layout::at(sl.d, L.in), *d_out = Layout::at(sl.d, L.out);
        jfs_dev_block *h_desc = Layout::at<jfs_dev_block>(sl.h, L.desc);
        jfs_dev_block *d_desc = Layout::at<jfs_dev_block>(sl.d, L.desc);
        jfs_aead_block *h_ad = Layout::at<jfs_aead_block>(sl.h, L.aead_desc);
        jfs_aead_block *d_ad = Layout::at<jfs_aead_block>(sl.d, L.aead_desc);
        int32_t *d_ret = Layout::at<int32_t>(sl.d, L.ret), *d_r2 = Layout::at<int32_t>(sl.d, L.aead_ret);
        uint8_t *h_kn = Layout::at(sl.h, L.aead_kn), *d_kn = Layout::at(sl.d, L.aead_kn);
        const int klen = jfs_cipher_key_size(ae->cipher);
        for (int k = 0; k < n; k++) {
            const int i = c.s + k;
            const int64_t cap = blk[i].cap, io = plan.in_off[i], oo = plan.out_off[i];
            memcpy(h_kn + 64 * k, ae->key[i], (size_t)klen);
            memcpy(h_kn + 64 * k + 32, ae->nonce[i], 12);
            jfs_aead_block &a = h_ad[k];
            a.key = d_kn + 64 * k;
            a.nonce = d_kn + 64 * k + 32;
            if (ae->seal) {
                // the codec writes the payload area; the seal runs in place over it
                h_desc[k].dst_cap = (int32_t)(cap - 16);
                a.src = algo == JFS_ALGO_NONE ? d_in + io : d_out + oo;
                a.dst = d_out + oo;
                a.src_len = (int32_t)iov[i].src_len;
                a.dst_cap = (int32_t)cap;
            } else {
                // open in place over the staged payload (into the output for "none"),
                // then the codec reads the plaintext: the payload minus its tag
                h_desc[k].src_len = (int32_t)std::max<int64_t>(iov[i].src_len - 16, 0);
                a.src = d_in + io;
                a.dst = algo == JFS_ALGO_NONE ? d_out + oo : d_in + io;
                a.src_len = (int32_t)iov[i].src_len;
                a.dst_cap = algo == JFS_ALGO_NONE ? (int32_t)cap : (int32_t)iov[i].src_len;
            }
        }
        if (!h2d(d_in, Layout::at(sl.h, L.in), c.tin)) return JFS_ERR_HIP;
        if (!h2d(d_desc, h_desc, (int64_t)n * (int64_t)sizeof(jfs_dev_block))) return JFS_ERR_HIP;
        if (!h2d(d_ad, h_ad, L.aead_bytes)) return JFS_ERR_HIP;
        if (!stage_crc(c, L, sl)) return JFS_ERR_HIP;
        if (!stage_csum(c, L, sl)) return JFS_ERR_HIP;
        if (hipEventRecord(sl.ev_in, dev->s_in) != hipSuccess) return JFS_ERR_HIP;
        if (hipStreamWaitEvent(ks, sl.ev_in, 0) != hipSuccess) return JFS_ERR_HIP;
        int64_t r = JFS_OK;
        if (ae->seal) {
            if (algo == JFS_ALGO_LZ4) r = launch_lz4_encode(sl, h_desc, d_desc, n, d_ret, ks, lz4_fast);
            else if (algo != JFS_ALGO_NONE) r = launch_rc(launch_kernel(algo, COMPRESS, d_desc, n, d_ret, ks, zparse));
            if (r == JFS_OK)
                r = launch_rc(
                    jfs_launch_aead(ae->cipher, d_ad, n, 0, d_r2, algo != JFS_ALGO_NONE ? d_ret : nullptr, ks));
        } else {
            r = launch_rc(jfs_launch_aead(ae->cipher, d_ad, n, 1, d_r2, nullptr, ks));
            if (r == JFS_OK && algo == JFS_ALGO_LZ4) r = launch_lz4_decode(sl, h_desc, d_desc, n, d_ret, ks);
            // Zstd: the host holds ciphertext only, the device API plans the scratch itself
            if (r == JFS_OK && algo == JFS_ALGO_ZSTD)
                r = launch_rc(jfs_launch_zstd_decode(d_desc, n, d_ret, nullptr, ks));
        }
        if (r != JFS_OK) return r;
        if (ae->seal && !run_crc(c, L, sl, d_r2, ks)) return JFS_ERR_HIP;
        // the opened block's checksums: its length is the codec's result, for "none" the open's
        // (a failed open's zeros may decode: finish() hands out nothing for it)
        if (!run_csum(c, L, sl, algo == JFS_ALGO_NONE ? d_r2 : d_ret, ks)) return JFS_ERR_HIP;
        if (hipEventRecord(sl.ev_k, ks) != hipSuccess) return JFS_ERR_HIP;
        if (hipStreamWaitEvent(dev->s_out, sl.ev_k, 0) != hipSuccess) return JFS_ERR_HIP;
        if (!d2h(Layout::at(sl.h, L.ret), d_ret, (int64_t)n * 4)) return JFS_ERR_HIP;
        if (!d2h(Layout::at(sl.h, L.aead_ret), d_r2, (int64_t)n * 4)) return JFS_ERR_HIP;
        if (ae->seal && !fetch_crc(c, L, sl)) return JFS_ERR_HIP;
        if (!fetch_csum(L, sl)) return JFS_ERR_HIP;
        if (!d2h(Layout::at(sl.h, L.out), d_out, c.tout)) return JFS_ERR_HIP;
        if (hipEventRecord(sl.ev, dev->s_out) != hipSuccess) return JFS_ERR_HIP;
        return JFS_OK;
    }

    // Wait for a chunk and copy its results and outputs to the caller.
    int64_t finish(int chunk) {
        const Chunk &c = plan.ch[chunk];
        const Layout &L = lay[chunk];
        Slot &sl = ln.slot[c.slot];
        const double t0 = host_trace() ? now_ms() : 0.0;
        // (results, CRCs and checksums land before the first output piece)
        if (hipEventSynchronize(ae ? sl.ev : sl.ev_p[0]) != hipSuccess) return JFS_ERR_HIP;
        const double t1 = host_trace() ? now_ms() : 0.0;
        const uint8_t *h_out = Layout::at(sl.h, L.out);
        const int32_t *h_ret = Layout::at<int32_t>(sl.h, L.ret);
        const int64_t *out_off = plan.out_off.data();
        std::vector<CopyJob> jobs;
        if (ae) {
            const int32_t *h_r2 = Layout::at<int32_t>(sl.h, L.aead_ret);
            for (int i = c.s; i < c.e; i++) {
                const int k = i - c.s;
                const jfs_iov &o = ae->orig[i];
                if (ae->seal) {
                    // encrypt.go:244-254: be16(len(wrapped)) | len(nonce) | wrapped | nonce | sealed
                    const int64_t rc = algo == JFS_ALGO_NONE ? iov[i].src_len : finish_result(algo, COMPRESS, h_ret[k]);
                    const int64_t hdr = ae->hdr[i];
                    if (rc < 0) {
                        out[i] = rc;
                    } else if (h_r2[k] != rc + 16) {
                        out[i] = JFS_ERR_HIP;
                    } else if (hdr + rc + 16 > o.dst_cap) {
                        out[i] = JFS_ERR_SHORT_BUFFER;
                    } else {
                        seal_header_write(o.dst, ae->sp[i]);
                        jobs.push_back({o.dst + hdr, h_out + out_off[i], rc + 16});
                        out[i] = hdr + rc + 16;
                    }
                } else {
                    // aead.Open first (encrypt.go:283), then the codec
                    const int64_t r = h_r2[k] < 0 ? JFS_ERR_AUTH
                                      : algo == JFS_ALGO_NONE ? (int64_t)h_r2[k]
                                                              : finish_result(algo, DECOMPRESS, h_ret[k]);
                    if (r > 0) jobs.push_back({o.dst, h_out + out_off[i], r});
                    out[i] = r;
                }
            }
        } else {
            for (int i = c.s; i < c.e; i++) out[i] = finish_result(algo, dir, h_ret[i - c.s]);
            const bool bytewise = pieces.byte_pieces(c);
            for (int p = 0; p < pieces.npiece(c); p++) {  // each piece's copy-out as soon as it landed
                if (p > 0 && bytewise) {  // (a piece of a lone block: spin, it lands within microseconds)
                    hipError_t q;
                    while ((q = hipEventQuery(sl.ev_p[p])) == hipErrorNotReady) {
                    }
                    if (q != hipSuccess) return JFS_ERR_HIP;
                } else if (p > 0 && hipEventSynchronize(sl.ev_p[p]) != hipSuccess) {
                    return JFS_ERR_HIP;
                }
                std::vector<CopyJob> pj;
                const int64_t p0 = pieces.piece_o(c, p, out_off), p1 = pieces.piece_o(c, p + 1, out_off);
                const int i0 = bytewise ? c.s : pieces.piece_b(c, p), i1 = bytewise ? c.e : pieces.piece_b(c, p + 1);
                for (int i = i0; i < i1; i++) {  // the part of block i's output inside the piece
                    if (out[i] <= 0) continue;
                    const int64_t lo = std::max(out_off[i], p0), hi = std::min(out_off[i] + out[i], p1);
                    if (hi > lo) pj.push_back({iov[i].dst + (lo - out_off[i]), h_out + lo, hi - lo});
                }
                par_copy(pj);
            }
        }
        if (crc_out) {
            const uint32_t *h_crc = Layout::at<uint32_t>(sl.h, L.crc);
            for (int i = c.s; i < c.e; i++) crc_out[i] = out[i] >= 0 ? h_crc[i - c.s] : 0u;
        }
        if (csum_out) {
            const uint8_t *h_area = Layout::at(sl.h, L.csum);
            int64_t o = 0;
            for (int i = c.s; i < c.e; i++) {
                if (csum_out[i] && out[i] >= 0) {
                    const int64_t nw = out[i] > 0 ? (out[i] - 1) / CSUM_SEG + 1 : 1;
                    jobs.push_back({csum_out[i], h_area + o, 4 * nw});
                }
                o += align16(4 * csum_words(i));
            }
        }
        par_copy(jobs);
        if (host_trace())
            fprintf(stderr, "[jfs host] t=%.2f chunk %d-%d wait %.2f ms copy-out %.1f MiB %.2f ms\n", now_ms(), c.s, c.e,
                    t1 - t0, c.tout / 1048576.0, now_ms() - t1);
        return JFS_OK;
    }

    // after a failure: leave no copy in flight into the staging slots
    void drain() const {
        (void)hipStreamSynchronize(dev->s_in);
        (void)hipStreamSynchronize(ln.s_k);
        (void)hipStreamSynchronize(other.s_k);
        (void)hipStreamSynchronize(dev->s_out);
    }
};

// Run blocks [0,nblk) of iov on one device through one lane (the caller holds
// ln.mu); returns when every result is in out[].  Blocks that the C-ABI
// answers without a kernel (empty input, noOp) are handled by the caller.  The
// batch is cut into chunks pipelined over the lane's NSLOT (stream, pinned,
// HBM) slots: host copy-in of chunk k (threads) | H2D k+1, kernel k, D2H k-1
// (streams) | host copy-out of chunk k-NSLOT.  A chunk holds at most
// chunk_limit() staging bytes; the lane's kernels run in chunk order, so a
// batch is not cut finer than that (a decode kernel over fewer blocks than
// CUs lasts about one block's latency whatever its size).
// max_chunk_blocks (> 0) also caps a chunk's block count; on_chunk (optional)
// is called with [s, e) as soon as those blocks' results and outputs are final
// (the coalescer releases their callers there, before later chunks finish).
int64_t run_batch(DevCtx *dev, Lane &ln, int algo, int dir, int nblk, const jfs_iov *iov, int64_t *out,
                  const Aead *ae = nullptr, uint32_t *crc_out = nullptr, int max_chunk_blocks = 0,
                  const std::function<void(int, int)> *on_chunk = nullptr, uint8_t *const *csum_out = nullptr) {
    if (nblk <= 0) return JFS_OK;
    LaneRun scope(dev, ln, algo * 2 + dir, (uint64_t)nblk);
    if (OpStats *st = op_stats(algo, dir)) st->batches.fetch_add(1, std::memory_order_relaxed);
    BatchRun b(dev, ln, algo, dir, nblk, iov, out, ae, crc_out, max_chunk_blocks, csum_out);
    b.presize();
    const int nch = (int)b.plan.ch.size();
    int64_t rc = JFS_OK;
    int done = 0;  // chunks [0, done) finished
    auto finish_next = [&]() -> int64_t {
        const jfs_plan::Chunk &c = b.plan.ch[done];
        const int64_t r = b.finish(done++);
        if (r == JFS_OK && on_chunk) (*on_chunk)(c.s, c.e);
        return r;
    };
    for (int k = 0; k < nch && rc == JFS_OK; k++) {
        if (k >= NSLOT) rc = finish_next();
        if (rc == JFS_OK) rc = b.launch(k);
    }
    while (done < nch && rc == JFS_OK) rc = finish_next();
    if (rc != JFS_OK) b.drain();
    return rc;
}

// run_batch with per-block error isolation (a GPU codec
// reports per-block errors): when a batch fails as a whole (staging
// allocation, a copy or launch error), it is split in halves and each half
// re-run, down to single blocks, so a failure is charged only to the blocks
// that fail alone and a few bad blocks cost O(log n) re-runs, not n.  After a
// sticky HIP error (the lane's streams no longer synchronise) nothing is
// re-run: the remaining blocks report JFS_ERR_HIP at once.
bool lane_healthy(DevCtx *dev, Lane &ln) {
    DevGuard guard;
    (void)hipSetDevice(dev->id);
    return hipStreamSynchronize(dev->s_in) == hipSuccess && hipStreamSynchronize(ln.s_k) == hipSuccess &&
           hipStreamSynchronize(dev->s_out) == hipSuccess;
}

void run_isolated(DevCtx *dev, Lane &ln, int algo, int dir, int nblk, const jfs_iov *iov, int64_t *out,
                  const Aead *ae = nullptr, uint32_t *crc = nullptr, uint8_t *const *csum = nullptr) {
    if (nblk <= 0) return;
    const int64_t rc = run_batch(dev, ln, algo, dir, nblk, iov, out, ae, crc, 0, nullptr, csum);
    if (rc == JFS_OK) return;
    if (nblk == 1 || (rc == JFS_ERR_HIP && !lane_healthy(dev, ln))) {
        for (int i = 0; i < nblk; i++) out[i] = rc;
        return;
    }
    const int h = nblk / 2;
    run_isolated(dev, ln, algo, dir, h, iov, out, ae, crc, csum);
    if (ae) {
        const Aead a2 = ae->at(h);
        run_isolated(dev, ln, algo, dir, nblk - h, iov + h, out + h, &a2, crc ? crc + h : nullptr,
                     csum ? csum + h : nullptr);
    } else {
        run_isolated(dev, ln, algo, dir, nblk - h, iov + h, out + h, nullptr, crc ? crc + h : nullptr,
                     csum ? csum + h : nullptr);
    }
}

// ---------------------------------------------------------------------------
// coalescer for the one-call-per-block API
// ---------------------------------------------------------------------------
struct Pending {
    int algo, dir;
    jfs_iov iov;
    int64_t res;
    bool done;
    // the caller's own wake-up: a release wakes only the callers it answers
    // (one shared condition woke all ~200 waiting callers per released chunk,
    // each re-taking the queue mutex that the gathering worker needs)
    std::condition_variable cv;
};

// Gather window (microseconds): a worker that finds work waits until no new
// call has arrived for `gap` (or `max` has passed since it started), so a
// burst of concurrent calls (pkg/chunk runs up to 20 uploads and 200
// downloads at once, cmd/flags.go:133-139) becomes one batch.  A lone call
// pays `gap`.  JFS_GATHER_US=<decompress gap>,<compress gap> overrides the
// gaps (max = 16 x gap).
struct Gather {
    int64_t gap_us, max_us;
};
// Decode batches of the coalescer run in chunks of at most this many blocks
// (JFS_COALESCE_CHUNK, 0 = by staging bytes only): the first chunk's callers
// return while later chunks run, and chunk copies / kernels pipeline.
int coalesce_chunk_blocks() {
    static int v = [] {
        const char *e = getenv("JFS_COALESCE_CHUNK");
        return e ? std::max(0, atoi(e)) : 16;
    }();
    return v;
}

Gather gather_window(int dir) {
    static int64_t g[2] = {-1, -1};
    static std::once_flag once;
    std::call_once(once, [] {
        g[DECOMPRESS_DIR] = 300;  // a lone 4 MiB decode takes milliseconds
        g[COMPRESS_DIR] = 2000;   // an encode takes ~0.1-0.5 s: gather generously
        if (const char *e = getenv("JFS_GATHER_US")) {
            char *end = nullptr;
            g[DECOMPRESS_DIR] = std::max(0ll, strtoll(e, &end, 10));
            if (end && *end == ',') g[COMPRESS_DIR] = std::max(0ll, strtoll(end + 1, nullptr, 10));
        }
    });
    static const int64_t mx = [] {  // JFS_GATHER_MAX_X: max = gap x this (default 16)
        const char *e = getenv("JFS_GATHER_MAX_X");
        return e ? std::max(1ll, atoll(e)) : 16ll;
    }();
    const int64_t gap = g[dir == DECOMPRESS_DIR ? DECOMPRESS_DIR : COMPRESS_DIR];
    return {gap, gap * mx};
}

int64_t gather_probe_us() {
    static const int64_t v = [] {
        const char *e = getenv("JFS_GATHER_PROBE_US");
        return e ? std::max(0ll, atoll(e)) : 0ll;
    }();
    return v;
}

int64_t gather_probe_enc_us() {
    static const int64_t v = [] {
        const char *e = getenv("JFS_GATHER_PROBE_ENC_US");
        return e ? std::max(0ll, atoll(e)) : 300ll;
    }();
    return v;
}

// Work of one block for the dealer: the bytes it stages in and out.
int64_t block_cost(const jfs_iov &v) { return std::max<int64_t>(v.src_len, 0) + std::max<int64_t>(v.dst_cap, 0) + 4096; }

// Size-balanced deal (SURVEY.md 8e, config 4's mixed 64 KiB - 4 MiB blocks):
// longest-processing-time greedy -- blocks by decreasing cost (ties in block
// order), each to the device with the least cost so far (ties to the lowest
// device).  No device ends more than one block's cost above another.
void plan_deal(const int64_t *cost, int n, int ndev, int32_t *out_dev) {
    if (n <= 0) return;
    if (ndev <= 1) {
        for (int i = 0; i < n; i++) out_dev[i] = 0;
        return;
    }
    std::vector<int> ord(n);
    for (int i = 0; i < n; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    std::vector<int64_t> load(ndev, 0);
    for (int i : ord) {
        int best = 0;
        for (int d = 1; d < ndev; d++)
            if (load[d] < load[best]) best = d;
        out_dev[i] = best;
        load[best] += std::max<int64_t>(cost[i], 0);
    }
}

// A gathered burst is spread over other devices' idle lanes when it holds at
// least this many staged bytes (JFS_SPREAD_MIN_MB; default 8 MiB: two 4 MiB blocks).
int64_t spread_min_bytes() {
    static const int64_t v = [] {
        const char *e = getenv("JFS_SPREAD_MIN_MB");
        return e ? std::max(0ll, atoll(e)) << 20 : (int64_t)8 << 20;
    }();
    return v;
}

// The lanes a coalescer worker runs a gathered burst on: its own lane, and
// (spreading) one idle lane of each other device, at most
// `parts - 1` of them.  Lock order, so that no two workers can deadlock: the
// own lane is taken first and blocking, while the worker holds nothing else;
// other devices' lanes are only ever try-locked, so no thread ever waits while
// holding a lane that another thread waits for.  (Round 4 try-locked the
// foreign lanes first and then blocked on its own: two workers could each
// hold the other's lane.)  Host-only logic: jfs_test_spread_locking runs it on
// fake devices.
struct SpreadLanes {
    std::unique_lock<std::mutex> own;
    std::vector<DevCtx *> hdev;
    std::vector<Lane *> hlane;
    std::vector<std::unique_lock<std::mutex>> hlock;
    void release() {
        hlock.clear();
        hlane.clear();
        hdev.clear();
        if (own.owns_lock()) own.unlock();
    }
};

void spread_acquire(DevCtx *dev, Lane &ln, const std::vector<DevCtx *> &all, int parts, SpreadLanes &sl) {
    sl.own = std::unique_lock<std::mutex>(ln.mu);
    for (DevCtx *d : all) {
        if (d == dev || (int)sl.hdev.size() + 1 >= parts) continue;
        for (int k = 0; k < NLANE; k++) {
            std::unique_lock<std::mutex> t(d->lane[k].mu, std::try_to_lock);
            if (t.owns_lock()) {
                sl.hdev.push_back(d);
                sl.hlane.push_back(&d->lane[k]);
                sl.hlock.push_back(std::move(t));
                break;
            }
        }
    }
}

class Coalescer {
   public:
    static Coalescer &get() {
        static Coalescer *c = new Coalescer();  // never destroyed: worker threads outlive static dtors
        return *c;
    }
    int64_t submit(int algo, int dir, const jfs_iov &iov) {
        std::vector<DevCtx *> &ds = devices();
        if (ds.empty()) return JFS_ERR_NO_DEVICE;
        start(ds);
        int64_t res = 0;
        if (dir == DECOMPRESS && inline_lone() && run_inline(ds, algo, dir, iov, &res)) return res;
        Pending p{algo, dir, iov, 0, false, {}};
        std::unique_lock<std::mutex> lk(mu_);
        q_.push_back(&p);
        arrivals_++;
        cv_work_.notify_all();
        p.cv.wait(lk, [&] { return p.done; });
        return p.res;
    }

   private:
    // A batch holds every queued call of one codec and direction, up to a
    // decode launch's worth of resident blocks; run_batch cuts it into
    // pipelined chunks of at most chunk_limit() staging bytes.
    static constexpr int kMaxBlocks = 4096;
    std::mutex mu_;
    std::condition_variable cv_work_;
    std::deque<Pending *> q_;
    uint64_t arrivals_ = 0;
    bool gathering_ = false;  // one worker gathers at a time; the others run batches
    int waiting_batches_ = 0;  // batches running with callers not yet released (guarded by mu_)
    std::once_flag started_;

    void start(std::vector<DevCtx *> &ds) {
        std::call_once(started_, [&] {
            // NLANE workers per device: a device runs the next batch while the
            // previous one is still in flight (each worker owns one lane)
            for (DevCtx *d : ds)
                for (int k = 0; k < NLANE; k++) std::thread([this, d, k] { worker(d, d->lane[k]); }).detach();
        });
    }
    // A decode that finds nothing queued and no batch waiting on the devices
    // (a lone cache miss) runs on the calling thread when a lane is free: no
    // hand-off to a worker and back (JFS_INLINE_LONE=0: always hand off).  It
    // counts as a waiting batch, so calls arriving meanwhile gather.
    static bool inline_lone() {
        static const bool v = [] {
            const char *e = getenv("JFS_INLINE_LONE");
            return !e || atoi(e) != 0;
        }();
        return v;
    }
    bool run_inline(std::vector<DevCtx *> &ds, int algo, int dir, const jfs_iov &iov, int64_t *res) {
        DevCtx *dev = nullptr;
        Lane *ln = nullptr;
        std::unique_lock<std::mutex> lane_lk;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!q_.empty() || gathering_ || waiting_batches_ != 0) return false;
            for (DevCtx *d : ds) {  // (lanes are only ever try-locked here)
                for (int k = 0; k < NLANE && !ln; k++) {
                    std::unique_lock<std::mutex> t(d->lane[k].mu, std::try_to_lock);
                    if (t.owns_lock()) {
                        lane_lk = std::move(t);
                        dev = d;
                        ln = &d->lane[k];
                    }
                }
                if (ln) break;
            }
            if (!ln) return false;
            waiting_batches_++;
        }
        const double t0 = host_trace() ? now_ms() : 0.0;
        jfs_iov v = iov;
        int64_t out = 0;
        if (run_batch(dev, *ln, algo, dir, 1, &v, &out, nullptr, nullptr, 0, nullptr) != JFS_OK)
            run_isolated(dev, *ln, algo, dir, 1, &v, &out);
        lane_lk.unlock();
        if (host_trace())
            fprintf(stderr, "[jfs coalescer] t=%.2f dev %d lane %d algo %d dir %d: 1 call inline, ran %.2f ms\n",
                    now_ms(), dev->id, (int)(ln - dev->lane), algo, dir, now_ms() - t0);
        {
            std::lock_guard<std::mutex> lk(mu_);
            waiting_batches_--;
        }
        cv_work_.notify_all();  // calls that queued meanwhile
        *res = out;
        return true;
    }
    int queued_like(int algo, int dir) const {
        int n = 0;
        for (const Pending *p : q_) n += p->algo == algo && p->dir == dir;
        return n;
    }
    void worker(DevCtx *dev, Lane &ln) {
        std::vector<Pending *> batch;
        std::vector<jfs_iov> iov;
        std::vector<int64_t> out;
        std::vector<char> released;
        double t_gather = 0.0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_work_.wait(lk, [&] { return !q_.empty() && !gathering_; });
                gathering_ = true;
                t_gather = host_trace() ? now_ms() : 0.0;
                const int algo = q_.front()->algo, dir = q_.front()->dir;
                // Decode on an idle device: a lone call (a cache miss) goes at
                // once -- or, with JFS_GATHER_PROBE_US set, once no second call
                // has followed it within that probe; under load the calls that
                // arrive while a batch runs form the next one.  (A burst's first
                // call alone costs the burst little: the 200-way legs measured
                // the same with a 40 us probe and without.)  Encode probes
                // longer (JFS_GATHER_PROBE_ENC_US, default 300): an encode
                // batch lasts about one block's parse whatever its size, so a
                // burst's first call sent alone would put the rest behind a
                // whole extra batch -- a burst's second call comes within the
                // probe, and a lone upload skips the 2 ms gather.
                Gather gw = gather_window(dir);
                if (waiting_batches_ == 0 && queued_like(algo, dir) == 1) {
                    const uint64_t s0 = arrivals_;
                    const int64_t probe = dir == DECOMPRESS ? gather_probe_us() : gather_probe_enc_us();
                    if (probe > 0)
                        cv_work_.wait_until(lk, std::chrono::steady_clock::now() + std::chrono::microseconds(probe),
                                            [&] { return arrivals_ != s0; });
                    if (arrivals_ == s0) gw.gap_us = 0;
                }
                const auto t_end = std::chrono::steady_clock::now() + std::chrono::microseconds(gw.max_us);
                uint64_t seen = arrivals_;
                while (gw.gap_us > 0 && queued_like(algo, dir) < kMaxBlocks) {
                    const auto until = std::min(t_end, std::chrono::steady_clock::now() +
                                                           std::chrono::microseconds(gw.gap_us));
                    cv_work_.wait_until(lk, until, [&] { return arrivals_ != seen; });
                    if (arrivals_ == seen || std::chrono::steady_clock::now() >= t_end) break;
                    seen = arrivals_;
                }
                batch.clear();
                for (auto it = q_.begin(); it != q_.end() && (int)batch.size() < kMaxBlocks;) {
                    if ((*it)->algo == algo && (*it)->dir == dir) {
                        batch.push_back(*it);
                        it = q_.erase(it);
                    } else {
                        ++it;
                    }
                }
                gathering_ = false;
                waiting_batches_++;
            }
            cv_work_.notify_all();  // the next worker may start gathering
            size_t nrel = 0;  // callers released so far (under mu_)
            bool counted = true;  // this batch is in waiting_batches_
            auto released_one = [&]() {
                if (++nrel == batch.size() && counted) {
                    counted = false;
                    waiting_batches_--;
                }
            };
            iov.resize(batch.size());
            out.assign(batch.size(), 0);
            released.assign(batch.size(), 0);
            for (size_t i = 0; i < batch.size(); i++) iov[i] = batch[i]->iov;
            {
                const double t0 = host_trace() ? now_ms() : 0.0;
                const int algo = batch[0]->algo, dir = batch[0]->dir, n = (int)batch.size();
                // Other devices with an idle lane take a size-balanced share of
                // the gathered burst: their lanes are locked here
                // and released after their parts finish.
                std::vector<int64_t> cost(n);
                int64_t tot = 0;
                for (int i = 0; i < n; i++) tot += (cost[i] = block_cost(iov[i]));
                SpreadLanes sl;
                spread_acquire(dev, ln, devices(), n >= 2 && tot >= spread_min_bytes() ? n : 1, sl);
                std::vector<DevCtx *> &hdev = sl.hdev;
                std::vector<Lane *> &hlane = sl.hlane;
                const int G = 1 + (int)hdev.size();
                std::vector<int32_t> where(n, 0);
                plan_deal(cost.data(), n, G, where.data());
                std::vector<std::vector<int>> pidx(G);
                for (int i = 0; i < n; i++) pidx[where[i]].push_back(i);
                // chunks of a decode batch release their callers as they finish:
                // those callers' next calls gather while the rest of the batch runs
                const int cb = dir == DECOMPRESS ? coalesce_chunk_blocks() : 0;
                auto run_part = [&](DevCtx *d, Lane &L, const std::vector<int> &idx) {
                    const int np = (int)idx.size();
                    if (np == 0) return;
                    std::vector<jfs_iov> piov(np);
                    std::vector<int64_t> pout(np, 0);
                    std::vector<char> prel(np, 0);
                    for (int k = 0; k < np; k++) piov[k] = iov[idx[k]];
                    const std::function<void(int, int)> release = [&](int s, int e) {
                        std::lock_guard<std::mutex> lk(mu_);
                        for (int k = s; k < e; k++) {
                            batch[idx[k]]->res = pout[k];
                            batch[idx[k]]->done = true;
                            batch[idx[k]]->cv.notify_one();
                            released[idx[k]] = 1;
                            prel[k] = 1;
                            released_one();
                        }
                    };
                    if (run_batch(d, L, algo, dir, np, piov.data(), pout.data(), nullptr, nullptr, cb, &release) !=
                        JFS_OK) {
                        // what was not released yet goes through the error-isolating path
                        std::vector<int> rest;
                        for (int k = 0; k < np; k++)
                            if (!prel[k]) rest.push_back(k);
                        std::vector<jfs_iov> iv2(rest.size());
                        std::vector<int64_t> o2(rest.size(), 0);
                        for (size_t q = 0; q < rest.size(); q++) iv2[q] = piov[rest[q]];
                        run_isolated(d, L, algo, dir, (int)rest.size(), iv2.data(), o2.data());
                        for (size_t q = 0; q < rest.size(); q++) pout[rest[q]] = o2[q];
                    }
                    for (int k = 0; k < np; k++) out[idx[k]] = pout[k];
                };
                std::vector<std::thread> th;
                for (int g = 1; g < G; g++) th.emplace_back([&, g] { run_part(hdev[g - 1], *hlane[g - 1], pidx[g]); });
                run_part(dev, ln, pidx[0]);
                for (auto &t : th) t.join();
                sl.release();
                if (host_trace())
                    fprintf(stderr, "[jfs coalescer] t=%.2f dev %d lane %d algo %d dir %d: %zu calls on %d device(s), gathered %.2f ms, ran %.2f ms\n",
                            now_ms(), dev->id, (int)(&ln - dev->lane), algo, dir, batch.size(), G, t0 - t_gather,
                            now_ms() - t0);
            }
            {
                std::lock_guard<std::mutex> lk(mu_);
                for (size_t i = 0; i < batch.size(); i++) {
                    if (released[i]) continue;
                    batch[i]->res = out[i];
                    batch[i]->done = true;
                    batch[i]->cv.notify_one();
                }
                if (counted) {
                    counted = false;
                    waiting_batches_--;
                }
            }
        }
    }
};

bool pre_answer(int algo, int dir, const jfs_iov &v, int64_t *res) {
    // Results the Go adapters produce before reaching the C codec.
    if (algo == JFS_ALGO_NONE) {  // compress.go:55-68
        if (v.dst_cap < v.src_len) { *res = JFS_ERR_SHORT_BUFFER; return true; }
        if (v.src_len > 0) memmove(v.dst, v.src, (size_t)v.src_len);
        *res = v.src_len;
        return true;
    }
    if (v.src_len < 0 || v.dst_cap < 0) { *res = JFS_ERR_INVALID; return true; }
    if (dir == DECOMPRESS && v.src_len == 0) { *res = JFS_ERR_EMPTY_INPUT; return true; }  // compress.go:121, ErrEmptySlice
    if (algo == JFS_ALGO_LZ4 && dir == COMPRESS && v.src_len > LZ4_MAX_INPUT) { *res = JFS_ERR_COMPRESS_FAIL; return true; }
    if (algo == JFS_ALGO_ZSTD && dir == COMPRESS && v.dst_cap < jfs_compress_bound(JFS_ALGO_ZSTD, v.src_len)) {
        *res = JFS_ERR_SHORT_BUFFER;  // compress.go:86-89 (DataDog checks cap(dst) against CompressBound)
        return true;
    }
    return false;
}

// the devices a call may use: those of device_mask (0: all)
std::vector<DevCtx *> devices_in(uint32_t device_mask) {
    std::vector<DevCtx *> ds;
    for (DevCtx *d : devices())
        if (device_mask == 0 || (d->id < 32 && (device_mask >> d->id) & 1u)) ds.push_back(d);
    return ds;
}

// Deal the todo blocks over the selected devices, size-balanced
// (plan_deal) and run them; ae_all (optional) is parallel to iov2.
int64_t deal(int algo, int dir, const std::vector<int> &todo, const std::vector<jfs_iov> &iov2, int64_t *out_n,
             uint32_t mask, const Aead *ae_all, uint32_t *crc = nullptr, uint8_t *const *csum = nullptr) {
    const std::vector<DevCtx *> ds = devices_in(mask);
    if (ds.empty()) return JFS_ERR_NO_DEVICE;
    const size_t G = std::min(ds.size(), todo.size());
    struct Part {
        std::vector<jfs_iov> iov, orig;
        std::vector<const uint8_t *> key, nonce;
        std::vector<jfs_seal_param> sp;
        std::vector<int64_t> hdr, res;
        std::vector<uint32_t> crc;
        std::vector<uint8_t *> csum;
        std::vector<int> idx;
    };
    std::vector<Part> part(G);
    std::vector<int64_t> cost(todo.size());
    for (size_t k = 0; k < todo.size(); k++) cost[k] = block_cost(iov2[k]);
    std::vector<int32_t> where(todo.size(), 0);
    plan_deal(cost.data(), (int)todo.size(), (int)G, where.data());
    for (size_t k = 0; k < todo.size(); k++) {
        Part &p = part[where[k]];
        p.iov.push_back(iov2[k]);
        p.idx.push_back(todo[k]);
        if (csum) p.csum.push_back(csum[todo[k]]);
        if (ae_all) {
            p.orig.push_back(ae_all->orig[k]);
            p.key.push_back(ae_all->key[k]);
            p.nonce.push_back(ae_all->nonce[k]);
            if (ae_all->sp) p.sp.push_back(ae_all->sp[k]);
            if (ae_all->hdr) p.hdr.push_back(ae_all->hdr[k]);
        }
    }
    auto work = [&](size_t g) {
        Part &p = part[g];
        p.res.assign(p.iov.size(), 0);
        p.crc.assign(p.iov.size(), 0u);
        uint32_t *pc = crc ? p.crc.data() : nullptr;
        std::unique_lock<std::mutex> lk;
        Lane &ln = ds[g]->acquire_lane(lk, algo * 2 + dir);
        if (ae_all) {
            Aead a{ae_all->cipher, ae_all->seal, p.orig.data(), p.key.data(), p.nonce.data(),
                   ae_all->sp ? p.sp.data() : nullptr, ae_all->hdr ? p.hdr.data() : nullptr};
            run_isolated(ds[g], ln, algo, dir, (int)p.iov.size(), p.iov.data(), p.res.data(), &a, pc,
                         csum ? p.csum.data() : nullptr);
        } else {
            run_isolated(ds[g], ln, algo, dir, (int)p.iov.size(), p.iov.data(), p.res.data(), nullptr, pc,
                         csum ? p.csum.data() : nullptr);
        }
    };
    if (G == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (size_t g = 0; g < G; g++) th.emplace_back(work, g);
        for (auto &t : th) t.join();
    }
    for (size_t g = 0; g < G; g++)
        for (size_t k = 0; k < part[g].idx.size(); k++) {
            out_n[part[g].idx[k]] = part[g].res[k];
            if (crc) crc[part[g].idx[k]] = part[g].crc[k];
        }
    return JFS_OK;
}

// disk_cache_file.go checksum() of n bytes on the host (blocks answered
// without the GPU: the "none" codec)
void host_csum(const uint8_t *p, int64_t n, uint8_t *out) {
    const int64_t nw = n > 0 ? (n - 1) / CSUM_SEG + 1 : 1;
    for (int64_t w = 0; w < nw; w++) {
        const int64_t a = w * CSUM_SEG, e = std::min<int64_t>(n, a + CSUM_SEG);
        const uint32_t v = n > 0 ? host_crc32c(0, p + a, e - a) : 0u;
        out[4 * w] = (uint8_t)(v >> 24);
        out[4 * w + 1] = (uint8_t)(v >> 16);
        out[4 * w + 2] = (uint8_t)(v >> 8);
        out[4 * w + 3] = (uint8_t)v;
    }
}

int64_t batch_common(int algo, int dir, int nblk, const jfs_iov *iov, int64_t *out_n, uint32_t mask,
                     uint32_t *crc = nullptr, uint8_t *const *csum = nullptr) {
    if (nblk < 0 || (nblk > 0 && (!iov || !out_n))) return JFS_ERR_INVALID;
    if (algo != JFS_ALGO_NONE && algo != JFS_ALGO_LZ4 && algo != JFS_ALGO_ZSTD) return JFS_ERR_INVALID;
    std::vector<int> todo;
    for (int i = 0; i < nblk; i++) {
        if (!pre_answer(algo, dir, iov[i], &out_n[i])) {
            todo.push_back(i);
        } else {
            if (crc) crc[i] = out_n[i] >= 0 ? host_crc32c(0, iov[i].dst, out_n[i]) : 0u;  // "none": the payload is dst
            if (csum && csum[i] && out_n[i] >= 0) host_csum(iov[i].dst, out_n[i], csum[i]);
        }
    }
    if (todo.empty()) return JFS_OK;
    std::vector<jfs_iov> iov2(todo.size());
    for (size_t k = 0; k < todo.size(); k++) iov2[k] = iov[todo[k]];
    return deal(algo, dir, todo, iov2, out_n, mask, nullptr, crc, csum);
}

// ---------------------------------------------------------------------------
// the on-device chains, one device and one lane per call:
//   compaction     (open ->) decode -> gather -> encode (-> seal)
//                  jfs_compact_batch, jfs_compact_seal_batch
//   read assembly  verify -> (open ->) decode -> gather (-> the reads' checksums)
//                  jfs_read_batch, jfs_read_open_batch and their _csum forms
// cipher < 0: no envelopes.  The planning arithmetic is chain_plan.h's.
// ---------------------------------------------------------------------------
using jfs_plan::ChainFlags;
using jfs_plan::ChainLayout;
using jfs_plan::ChainOut;
using jfs_plan::ChainSrc;

// One call's staging on its lane (the caller holds ln.mu).  Staging comes from
// the lane's slots: slot 0's pinned/HBM pair (h / d, laid out by ChainLayout)
// for what crosses the link, slot 0's device scratch for the decoded sources
// and the gathered blocks, slots 1 and 2's for the small-batch encoder and
// decoder.  The whole chain is a single pass on the lane's kernel stream.
struct Chain {
    int algo, cipher, ns, n, no;  // ns decoded sources of n staged objects, no outputs
    bool codec, sealed, lz4;
    jfs_plan::ChainOffsets off;
    ChainLayout L;
    Slot *sl, *s1;
    uint8_t *h, *d;
    uint8_t *hin, *din;          // the stored bytes: h and d, or where an earlier pass left them opened
    int32_t *open_h, *open_d;    // the opens' results: L.open's, or that pass's
    bool opened;                 // the sources were staged and opened by an earlier pass (ChainOpened)
    hipStream_t ks;

    template <class T>
    T *host(int64_t o) const { return (T *)(h + o); }
    template <class T>
    T *dev(int64_t o) const { return (T *)(d + o); }
    uint8_t *d_in(int k) const { return din + off.in[k]; }
    uint8_t *d_out(int k) const { return d + L.out + off.out[k]; }
    uint8_t *h_out(int k) const { return h + L.out + off.out[k]; }
    // where output k is gathered: in front of an encoder in the scratch, else in place
    uint8_t *gat(int k) const { return off.gat.empty() ? d_out(k) : sl->sp + off.gat[k]; }
};

// Sources that a call staged and opened before it could lay itself out (the
// sealed spliced compaction, whose plan needs their tables): the pinned / HBM
// pair their payloads lie in, at ChainOffsets::in, and the opens' results.  The
// layout then has no stored bytes of its own.
struct ChainOpened {
    uint8_t *h, *d;
    int32_t *open_h, *open_d;
};

// What a call adds to the layout for itself: bytes of records in the H2D part
// (ChainLayout::xmeta), of results (xres), of mirrored area behind the outputs
// and of device scratch behind the decoded sources and gathered blocks.
struct ChainExtra {
    int64_t meta = 0, res = 0, out = 0, scratch = 0;
    const ChainOpened *opened = nullptr;  // the call's sources, where an earlier pass of it opened them
};

// Lays the call out and sizes slot 0 for it: JFS_OK or JFS_ERR_NO_MEMORY.
int64_t chain_open(Chain &c, Lane &ln, int algo, int cipher, const std::vector<ChainSrc> &st, int ns,
                   const std::vector<ChainOut> &oo, const int32_t *seg_first, bool encode, bool out_crc, bool src_crc,
                   bool prefix, int64_t npiece = 0, bool seek = false, int64_t nrange = -1, const ChainExtra &x = {}) {
    c.algo = algo;
    c.cipher = cipher;
    c.ns = ns;
    c.n = (int)st.size();
    c.no = (int)oo.size();
    c.codec = algo != JFS_ALGO_NONE;
    c.sealed = cipher >= 0;
    c.lz4 = algo == JFS_ALGO_LZ4;
    c.off = jfs_plan::chain_offsets(st, ns, oo, c.codec, encode);
    int64_t nseg = 0;
    for (const ChainOut &o : oo) nseg += seg_first[o.idx + 1] - seg_first[o.idx];
    c.L = ChainLayout(x.opened ? 0 : c.off.tin, ns, c.n, c.no, nseg,
                      ChainFlags{c.sealed, encode, out_crc, src_crc, prefix, npiece > 0, seek, nrange >= 0}, npiece,
                      std::max<int64_t>(nrange, 0), x.meta, x.res);
    c.sl = &ln.slot[0];
    c.s1 = &ln.slot[1];
    c.ks = ln.s_k;
    if (!c.sl->ensure(c.L.out + c.off.tout + x.out)) return JFS_ERR_NO_MEMORY;
    if (c.codec && !c.sl->ensure_split(std::max<int64_t>(c.off.scratch + x.scratch, 16))) return JFS_ERR_NO_MEMORY;
    c.h = c.sl->h;
    c.d = c.sl->d;
    c.opened = x.opened != nullptr;
    c.hin = c.opened ? x.opened->h : c.h;
    c.din = c.opened ? x.opened->d : c.d;
    c.open_h = c.opened ? x.opened->open_h : c.host<int32_t>(c.L.open);
    c.open_d = c.opened ? x.opened->open_d : c.dev<int32_t>(c.L.open);
    return JFS_OK;
}

// fills 64-byte key | nonce cell `slot`; returns its device address
uint8_t *chain_cell(const Chain &c, int slot, const uint8_t *key, const uint8_t *nonce) {
    uint8_t *cell = c.h + c.L.kn + 64 * (int64_t)slot;
    memcpy(cell, key, (size_t)jfs_cipher_key_size(c.cipher));
    memcpy(cell + 32, nonce, 12);
    return c.d + c.L.kn + 64 * (int64_t)slot;
}

// The source side's staging: the stored bytes of every staged object (copy
// jobs for the caller's par_copy), and for the ns decoded sources the open and
// decode descriptors, key cells and preset lengths.
void chain_stage_sources(const Chain &c, const jfs_iov *src, const uint8_t *const *src_keys,
                         const std::vector<ChainSrc> &st, std::vector<CopyJob> &jobs) {
    jfs_dev_block *h_sdesc = c.host<jfs_dev_block>(c.L.sdesc);
    int32_t *h_srcn = c.host<int32_t>(c.L.srcn);
    for (int k = 0; k < c.n; k++) {
        const ChainSrc &s = st[k];
        const jfs_iov &v = src[s.idx];
        if (s.pay > 0 && !c.opened) jobs.push_back({c.hin + c.off.in[k], v.src + s.off, s.pay});
        if (k >= c.ns) continue;  // staged for its checksum only
        const int64_t plain = c.sealed ? s.pay - 16 : s.pay;  // sealed: pay >= 16, the host answered shorter ones
        if (c.sealed && !c.opened) {
            uint8_t *d_cell = chain_cell(c, k, src_keys[s.idx], v.src + s.noff);
            // open in place over the staged payload; the codec reads the plaintext
            c.host<jfs_aead_block>(c.L.sad)[k] =
                jfs_aead_block{c.d_in(k), c.d_in(k), (int32_t)s.pay, (int32_t)s.pay, d_cell, d_cell + 32};
        }
        // "none": the stored (opened) object is the decoded block
        uint8_t *dec = c.codec ? c.sl->sp + c.off.dec[k] : c.d_in(k);
        h_sdesc[k] = jfs_dev_block{c.d_in(k), dec, (int32_t)plain, (int32_t)(c.codec ? s.cap : plain)};
        h_srcn[k] = c.codec ? -1 : (int32_t)plain;  // a decoder overwrites it
    }
    h_sdesc[c.ns] = jfs_dev_block{nullptr, nullptr, 0, 0};  // "a failed source"
    h_srcn[c.ns] = -1;
}

// the gather plan of the outputs the device works on, its segments remapped to the staged sources
void chain_stage_plan(const Chain &c, const std::vector<ChainOut> &oo, const std::vector<int> &src_map,
                      const int32_t *seg_first, const jfs_compact_seg *seg) {
    jfs_compact_out *h_plan = c.host<jfs_compact_out>(c.L.plan);
    jfs_compact_seg *h_seg = c.host<jfs_compact_seg>(c.L.seg);
    int64_t sg = 0;
    for (int k = 0; k < c.no; k++) {
        const int j = oo[k].idx;
        const int cnt = seg_first[j + 1] - seg_first[j];
        h_plan[k] = jfs_compact_out{c.gat(k), (int32_t)oo[k].total, (int32_t)sg, cnt, 0};
        for (int q = 0; q < cnt; q++) h_seg[sg + q] = jfs_plan::chain_remap(seg[seg_first[j] + q], src_map, c.ns);
        sg += cnt;
    }
}

// The small-batch LZ4 decoder and encoder (h_enc, or null) run one after the
// other on the stream: they share slot 1's scratch, sized for both before
// anything is queued.
bool chain_lz4_scratch(const Chain &c, const jfs_dev_block *h_enc, bool fast) {
    if (!c.lz4) return true;
    const jfs_dev_block *h_sdesc = c.host<jfs_dev_block>(c.L.sdesc);
    int64_t need = 0;
    if (c.ns > 0) need = lz4_decode_scratch(c.ns, desc_lens(h_sdesc, c.ns).data(), desc_caps(h_sdesc, c.ns).data());
    if (h_enc && c.no > 0) need = std::max(need, lz4_encode_scratch(c.no, desc_lens(h_enc, c.no).data(), fast));
    return need <= 0 || c.s1->ensure_split(need);
}

// Queues open -> decode -> the opens' verdicts merged into the source lengths.
// d_want (prefix modes: LZ4, and Zstd in JFS_READ_DECODE_PREFIX_ALL; else null): where each decode stops.
// d_from (Zstd with JFS_READ_SEEK on; else null): with d_want the range each source is decoded for.
// d_rf, d_rng (Zstd with JFS_READ_SEEK sparse; else null): the list of ranges each source is decoded for.
// nchase (LZ4 with JFS_READ_LZ4_CHASE on; else 0): sources [0, nchase) take the origin chase for their lists in
// d_rf, d_rng, which touch at most max_quads 4-byte groups; the rest are decoded as without the switch.
int chain_decode(const Chain &c, const int32_t *d_want, int64_t max_want, const int32_t *d_from = nullptr,
                 const int32_t *d_rf = nullptr, const jfs_range *d_rng = nullptr, int nchase = 0, int64_t max_quads = 0) {
    const jfs_dev_block *h_sdesc = c.host<jfs_dev_block>(c.L.sdesc), *d_sdesc = c.dev<jfs_dev_block>(c.L.sdesc);
    int32_t *d_srcn = c.dev<int32_t>(c.L.srcn), *d_open = c.open_d;
    const int ns = c.ns;
    int lk = 0;
    if (c.sealed && !c.opened && ns > 0) lk = jfs_launch_aead(c.cipher, c.dev<jfs_aead_block>(c.L.sad), ns, 1, d_open, nullptr, c.ks);
    if (lk == 0 && c.lz4 && ns > 0) {
        int64_t r = JFS_OK;
        const int rest = ns - nchase;
        // (the slot's scratch was sized for both launches before anything was queued: read_run)
        if (nchase > 0)
            r = launch_rc(jfs_launch_lz4_chase(d_sdesc, desc_lens(h_sdesc, nchase).data(), desc_caps(h_sdesc, nchase).data(),
                                               d_rf, d_rng, nchase, d_srcn, c.s1->sp, max_quads, c.ks));
        if (r == JFS_OK && rest > 0)
            r = d_want ? launch_lz4_decode_prefix(*c.s1, h_sdesc + nchase, d_sdesc + nchase, rest, d_srcn + nchase,
                                                  d_want + nchase, max_want, c.ks)
                       : launch_lz4_decode(*c.s1, h_sdesc + nchase, d_sdesc + nchase, rest, d_srcn + nchase, c.ks);
        lk = r == JFS_OK ? 0 : -1;
    } else if (lk == 0 && c.algo == JFS_ALGO_ZSTD && ns > 0) {
        // (with a cipher the frame headers are ciphertext on the host) it plans its own scratch
        lk = d_rf     ? jfs_launch_zstd_decode_ranges(d_sdesc, d_rf, d_rng, ns, d_srcn, c.ks)
             : d_from ? jfs_launch_zstd_decode_range(d_sdesc, d_from, d_want, ns, d_srcn, c.ks)
             : d_want ? jfs_launch_zstd_decode_prefix(d_sdesc, ns, d_srcn, d_want, c.ks)
                      : jfs_launch_zstd_decode(d_sdesc, ns, d_srcn, nullptr, c.ks);
    }
    // a failed open left zeros, which may decode (for "none" they are the block): its verdict replaces the length
    if (lk == 0 && c.sealed) lk = jfs_launch_chain_merge(d_open, ns, d_srcn, c.ks);
    return lk;
}

// One D2H of [results, end) once the launches (lk) are queued; the stream is
// drained either way.  false: JFS_ERR_HIP.
bool chain_results(const Chain &c, int lk, int64_t end) {
    const int64_t at = c.L.results;
    if (lk == 0 && hipMemcpyAsync(c.h + at, c.d + at, (size_t)(end - at), hipMemcpyDeviceToHost, c.ks) == hipSuccess &&
        hipStreamSynchronize(c.ks) == hipSuccess)
        return true;
    (void)hipStreamSynchronize(c.ks);
    return false;
}

// decoded source k's result: aead.Open first (encrypt.go:283), then the codec
int64_t chain_src_result(const Chain &c, int k) {
    if (c.sealed && c.open_h[k] < 0) return JFS_ERR_AUTH;
    const int32_t raw = c.host<int32_t>(c.L.srcn)[k];
    return c.codec ? finish_result(c.algo, DECOMPRESS, raw) : (int64_t)raw;
}

// output result `raw` of the gather (encoded: of the encoder behind it)
int64_t chain_out_result(int algo, bool encoded, int32_t raw) {
    if (raw == JFS_CHAIN_FAILED) return JFS_ERR_CORRUPT;
    if (encoded) return finish_result(algo, COMPRESS, raw);
    return raw >= 0 ? (int64_t)raw : JFS_ERR_INVALID;
}

// Compaction on one lane: stored sources (sealed payloads), keys and the plan
// H2D, open in place, decode, the opens' verdicts merged into the source
// lengths, gather, encode into the output's payload area, seal in place
// (lengths from the encoder on the device), checksums (seeded with the
// envelope header's), results D2H, then exactly the compressed / sealed bytes
// D2H; the host writes the envelope headers.  Returns JFS_OK with src_n /
// out_n / crc of these blocks filled, or JFS_ERR_NO_MEMORY / JFS_ERR_HIP with
// nothing filled.  Per-block results of sealed calls follow BatchRun::finish's
// rules for sealed batches, so they equal jfs_open_decompress_batch's and
// jfs_compress_seal_batch's.
int64_t compact_run(DevCtx *dev, Lane &ln, int algo, int cipher, const jfs_iov *src, const uint8_t *const *src_keys,
                    const std::vector<ChainSrc> &ss, const std::vector<int> &src_map, const jfs_iov *out,
                    const jfs_seal_param *out_p, const std::vector<ChainOut> &oo, const int32_t *seg_first,
                    const jfs_compact_seg *seg, int64_t *src_n, int64_t *out_n, uint32_t *crc) {
    LaneRun scope(dev, ln, algo * 2 + COMPRESS, (uint64_t)(ss.size() + oo.size()));
    Chain c;
    const int64_t rc = chain_open(c, ln, algo, cipher, ss, (int)ss.size(), oo, seg_first, true, crc != nullptr, false, false);
    if (rc != JFS_OK) return rc;
    const ChainLayout &L = c.L;
    const int ns = c.ns, no = c.no;
    const bool codec = c.codec, sealed = c.sealed;
    std::vector<CopyJob> jobs;
    chain_stage_sources(c, src, src_keys, ss, jobs);
    par_copy(jobs);
    chain_stage_plan(c, oo, src_map, seg_first, seg);
    jfs_dev_block *h_enc = c.host<jfs_dev_block>(L.enc);
    for (int k = 0; k < no; k++) {
        uint8_t *pay = c.d_out(k);  // the output's payload area: oo[k].area bytes
        h_enc[k] = jfs_dev_block{c.gat(k), pay, (int32_t)oo[k].total, (int32_t)oo[k].cap};
        if (crc) c.host<jfs_dev_block>(L.ocd)[k] = jfs_dev_block{pay, nullptr, 0, 0};
        if (!sealed) continue;
        const jfs_seal_param &p = out_p[oo[k].idx];
        uint8_t *d_cell = chain_cell(c, ns + k, p.key, p.nonce);
        // seal in place; with a codec the length comes from the encoder on the device
        c.host<jfs_aead_block>(L.oad)[k] =
            jfs_aead_block{pay, pay, (int32_t)oo[k].total, (int32_t)(oo[k].cap + 16), d_cell, d_cell + 32};
        if (crc) c.host<uint32_t>(L.oseed)[k] = seal_header_crc(p);
    }
    const bool fast = lz4_fast_mode();
    if (!chain_lz4_scratch(c, h_enc, fast)) return JFS_ERR_NO_MEMORY;
    hipStream_t ks = c.ks;
    // one H2D: stored sources, the plan, keys and the preset source lengths
    if (hipMemcpyAsync(c.d, c.h, (size_t)L.h2d, hipMemcpyHostToDevice, ks) != hipSuccess) return JFS_ERR_HIP;
    const jfs_dev_block *d_sdesc = c.dev<jfs_dev_block>(L.sdesc), *d_enc = c.dev<jfs_dev_block>(L.enc);
    int32_t *d_srcn = c.dev<int32_t>(L.srcn), *d_ret = c.dev<int32_t>(L.ret), *d_r2 = c.dev<int32_t>(L.r2);
    const int32_t max_total = jfs_plan::chain_max_total(oo);
    auto gather = [&](int pass) {
        return jfs_launch_gather(d_sdesc, d_srcn, ns + 1, c.dev<jfs_compact_out>(L.plan), no, c.dev<jfs_compact_seg>(L.seg),
                                 max_total, d_ret, pass, ks);
    };
    int lk = chain_decode(c, nullptr, 0);
    if (lk == 0) lk = gather(0);
    if (lk == 0 && codec && no > 0) {
        lk = c.lz4 ? (launch_lz4_encode(*c.s1, h_enc, d_enc, no, d_ret, ks, fast) == JFS_OK ? 0 : -1)
                   : launch_kernel(algo, COMPRESS, d_enc, no, d_ret, ks, zstd_encode_now());
        // the encoder ran on every block: a failed gather's verdict replaces its result
        if (lk == 0) lk = gather(1);
    }
    // "none": the length is the planned total; the seal also runs over a block
    // whose gather failed (its verdict in d_ret decides on the host)
    if (lk == 0 && sealed && no > 0)
        lk = jfs_launch_aead(cipher, c.dev<jfs_aead_block>(L.oad), no, 0, d_r2, codec ? d_ret : nullptr, ks);
    if (lk == 0 && crc && no > 0)
        lk = jfs_launch_crc32c_lens(c.dev<jfs_dev_block>(L.ocd), no, sealed ? d_r2 : d_ret,
                                    sealed ? c.dev<uint32_t>(L.oseed) : nullptr, c.dev<uint32_t>(L.ocrc), ks);
    if (!chain_results(c, lk, L.out)) return JFS_ERR_HIP;
    const int32_t *h_ret = c.host<int32_t>(L.ret), *h_r2 = c.host<int32_t>(L.r2);
    std::vector<int64_t> res(no), back(no);  // per output: its result, its bytes in the payload area
    for (int k = 0; k < no; k++) {
        int64_t r = chain_out_result(algo, codec, h_ret[k]);
        if (sealed && r >= 0 && h_r2[k] != r + 16) r = JFS_ERR_HIP;
        else if (sealed && r >= 0 && oo[k].hdr + r + 16 > out[oo[k].idx].dst_cap) r = JFS_ERR_SHORT_BUFFER;
        res[k] = r;
        back[k] = r < 0 ? 0 : sealed ? r + 16 : r;
        // exactly the compressed / sealed bytes come back
        if (back[k] > 0 &&
            hipMemcpyAsync(c.h_out(k), c.d_out(k), (size_t)back[k], hipMemcpyDeviceToHost, ks) != hipSuccess) {
            (void)hipStreamSynchronize(ks);
            return JFS_ERR_HIP;
        }
    }
    if (hipStreamSynchronize(ks) != hipSuccess) return JFS_ERR_HIP;
    for (int k = 0; k < ns; k++) src_n[ss[k].idx] = chain_src_result(c, k);
    jobs.clear();
    for (int k = 0; k < no; k++) {
        const int j = oo[k].idx;
        if (sealed && res[k] >= 0) seal_header_write(out[j].dst, out_p[j]);
        if (back[k] > 0) jobs.push_back({out[j].dst + oo[k].hdr, c.h_out(k), back[k]});
        out_n[j] = res[k] >= 0 ? oo[k].hdr + back[k] : res[k];
        if (crc) crc[j] = res[k] >= 0 ? c.host<uint32_t>(L.ocrc)[k] : 0u;
    }
    par_copy(jobs);
    return JFS_OK;
}

// jfs_compact_splice_counts: outputs spliced, frames passed, frames re-encoded inside them, bytes passed
std::atomic<uint64_t> g_splice_counts[4];

// The sealed spliced compaction's first pass (JFS_COMPACT_SPLICE all; DESIGN
// 11e), which brings the host what its plan needs of sources that are
// ciphertext there.  In slot 1's pinned / HBM pair, which no other chain uses:
// one H2D (the envelopes' payloads, AEAD descriptors, key cells, the slots),
// the open of every source in place, the seek tables out of the opened payloads
// into their slots (zstd_seek_tables.hip), one D2H of the opens' verdicts, the
// table lengths and the packed tables, and the wait.  The opened payloads stay
// where they are for the second pass (`at`).
struct OpenedTables {
    ChainOpened at;
    std::vector<int64_t> slot, len;  // per source of the call: its slot's place; its plaintext bytes, or < 0
    std::vector<int32_t> tlen;       // per source of the call: its table's bytes, 0 without one
    const uint8_t *tab = nullptr;    // the packed tables
};

int64_t splice_open_tables(Lane &ln, int cipher, const jfs_iov *src, const uint8_t *const *src_keys,
                           const std::vector<ChainSrc> &ss, int nsrc, OpenedTables &T) {
    const int ns = (int)ss.size();
    const jfs_plan::ChainOffsets off = jfs_plan::chain_offsets(ss, ns, std::vector<ChainOut>(), false, false);
    std::vector<int32_t> sf(ns + 1, 0);
    for (int k = 0; k < ns; k++) sf[k + 1] = sf[k] + (int32_t)jfs_plan::splice_slot_bytes(ss[k].cap);
    const int64_t blk = (int64_t)sizeof(jfs_dev_block), aead = (int64_t)sizeof(jfs_aead_block);
    // [payloads | descriptors | AEAD descriptors | key cells | slots' places || opens | table lengths | tables]
    const int64_t a_blk = align16(off.tin), a_sad = a_blk + align16(ns * blk), a_kn = a_sad + align16(ns * aead),
                  a_sf = a_kn + 64ll * ns, h2d = a_sf + align16((ns + 1) * 4ll), r_tlen = h2d + align16(ns * 4ll),
                  r_tab = r_tlen + align16(ns * 4ll), end = r_tab + sf[ns];
    Slot &sl = ln.slot[1];
    if (!sl.ensure(end)) return JFS_ERR_NO_MEMORY;
    std::vector<CopyJob> jobs;
    for (int k = 0; k < ns; k++) {
        const ChainSrc &s = ss[k];
        const jfs_iov &v = src[s.idx];
        jobs.push_back({sl.h + off.in[k], v.src + s.off, s.pay});
        uint8_t *cell = sl.h + a_kn + 64ll * k, *d_cell = sl.d + a_kn + 64ll * k, *d_pay = sl.d + off.in[k];
        memcpy(cell, src_keys[s.idx], (size_t)jfs_cipher_key_size(cipher));
        memcpy(cell + 32, v.src + s.noff, 12);
        ((jfs_aead_block *)(sl.h + a_sad))[k] = jfs_aead_block{d_pay, d_pay, (int32_t)s.pay, (int32_t)s.pay, d_cell, d_cell + 32};
        ((jfs_dev_block *)(sl.h + a_blk))[k] = jfs_dev_block{d_pay, nullptr, 0, 0};
    }
    par_copy(jobs);
    memcpy(sl.h + a_sf, sf.data(), (size_t)(ns + 1) * 4);
    hipStream_t ks = ln.s_k;
    int32_t *d_open = (int32_t *)(sl.d + h2d);
    if (hipMemcpyAsync(sl.d, sl.h, (size_t)h2d, hipMemcpyHostToDevice, ks) != hipSuccess) return JFS_ERR_HIP;
    int lk = jfs_launch_aead(cipher, (const jfs_aead_block *)(sl.d + a_sad), ns, 1, d_open, nullptr, ks);
    // the open's result is the plaintext length, or negative: a failed open has no table
    if (lk == 0)
        lk = jfs_launch_zstd_seek_tables((const jfs_dev_block *)(sl.d + a_blk), d_open, ns, (const int32_t *)(sl.d + a_sf),
                                         sl.d + r_tab, (int32_t *)(sl.d + r_tlen), ks);
    if (lk != 0 || hipMemcpyAsync(sl.h + h2d, sl.d + h2d, (size_t)(end - h2d), hipMemcpyDeviceToHost, ks) != hipSuccess ||
        hipStreamSynchronize(ks) != hipSuccess) {
        (void)hipStreamSynchronize(ks);
        return JFS_ERR_HIP;
    }
    T.at = ChainOpened{sl.h, sl.d, (int32_t *)(sl.h + h2d), d_open};
    T.tab = sl.h + r_tab;
    T.slot.assign(nsrc, 0);
    T.len.assign(nsrc, -1);  // a source the host answered: no table
    T.tlen.assign(nsrc, 0);
    for (int k = 0; k < ns; k++) {
        T.slot[ss[k].idx] = sf[k];
        T.len[ss[k].idx] = T.at.open_h[k];
        T.tlen[ss[k].idx] = T.at.open_h[k] < 0 ? 0 : ((const int32_t *)(sl.h + r_tlen))[k];
    }
    return JFS_OK;
}

// the sealed call's plan, once the tables are on the host
typedef std::function<jfs_plan::SplicePlan(const jfs_plan::PackedTables &)> SpliceReplan;

// Compaction with untouched frames spliced (Zstd in the seekable parse mode).
// Without a cipher (JFS_COMPACT_SPLICE on or all): P0, splice_plan.h's answer
// over the stored objects, splices at least one of oo.  With one (all): the
// sources are opened first (splice_open_tables), `replan` answers from their
// packed tables, and every output is sealed at the end; a plan that splices
// nothing is then the switch off, continued from the opened sources -- every
// output one whole unit, the sources decoded whole.  own, seg_first, seg: the
// sealed outputs the host already answered, and the caller's plan (see `lists`).
// The chain's outputs are the plan's encode units -- every unspliced output
// whole, every FRESH piece of a spliced one -- so staging, gather and encode are
// compact_run's over the derived plan; a spliced output's object is assembled
// behind them (zstd_splice.hip) in an area of its own behind the units'.  On the
// lane's stream: one H2D (stored sources unless opened, the derived plan, the
// lists of ranges, the splice and seal records), the ranges decode of what the
// derived plan still reads, gather, seekable encode of all units (csum: with the
// 12-byte table for the whole outputs, and XXH64 of the FRESH pieces), the
// gather's verdicts merged, scan and copy, every output's payload length picked
// from the units' results or the scan's, the seal in place, CRC-32C of the
// finished objects, results D2H, then exactly the object bytes.  Results as
// compact_run's; src_n of a source with a valid table is the table's content
// size (the header has the contract).
int64_t compact_splice_run(DevCtx *dev, Lane &ln, int cipher, const jfs_iov *src, const uint8_t *const *src_keys,
                           const std::vector<ChainSrc> &ss, const std::vector<int> &src_map, int nsrc, const jfs_iov *out,
                           const jfs_seal_param *out_p, const std::vector<ChainOut> &oo, const jfs_plan::SplicePlan *P0,
                           const SpliceReplan &replan, const std::vector<int> &own, const int32_t *seg_first,
                           const jfs_compact_seg *seg, bool csum, int64_t *src_n, int64_t *out_n, uint32_t *crc) {
    const int algo = JFS_ALGO_ZSTD;
    const bool sealed = cipher >= 0;
    LaneRun scope(dev, ln, algo * 2 + COMPRESS, (uint64_t)(ss.size() + oo.size()));
    OpenedTables T;
    jfs_plan::SplicePlan replanned;
    if (sealed) {
        const int64_t rc = splice_open_tables(ln, cipher, src, src_keys, ss, nsrc, T);
        if (rc != JFS_OK) return rc;
        replanned = replan(jfs_plan::PackedTables{T.tab, T.slot.data(), T.tlen.data(), T.len.data(), nullptr});
    }
    const jfs_plan::SplicePlan &P = sealed ? replanned : *P0;
    const bool whole = P.outs == 0;  // nothing passes: the switch off
    const int ns = (int)ss.size(), no = (int)oo.size(), nu = (int)P.units.size(), nfr = (int)P.frames.size();
    const int nout = (int)P.frame_first.size() - 1;
    // output j: its place in oo; its whole unit, or its place among the spliced ones
    std::vector<int> oo_of(nout, -1), unit_of(nout, -1), sp_of(nout, -1), sp;
    for (int k = 0; k < no; k++) {
        oo_of[oo[k].idx] = k;
        if (P.spliced(oo[k].idx)) {
            sp_of[oo[k].idx] = (int)sp.size();
            sp.push_back(k);
        }
    }
    const int nsp = (int)sp.size();
    std::vector<ChainOut> uu(nu);
    for (int u = 0; u < nu; u++) {
        const jfs_plan::SpliceUnit &q = P.units[u];
        const int64_t cap = q.piece < 0 ? oo[oo_of[q.out]].cap : jfs_compress_bound(JFS_ALGO_ZSTD, q.total);
        // a whole output is sealed where it is encoded: its area also holds the tag
        uu[u] = ChainOut{u, q.total, q.piece < 0 ? oo[oo_of[q.out]].area : cap, cap, 0};
        if (q.piece < 0) unit_of[q.out] = u;
    }
    std::vector<int64_t> xo(nsp + 1, 0);  // the spliced objects' places behind the units' area
    for (int s = 0; s < nsp; s++) xo[s + 1] = xo[s] + align16(oo[sp[s]].area);
    // What is decoded: what the derived plan reads, and what the sealed outputs with an error of their own (`own`,
    // which are no units) would have read -- "a failed or short source wins" over that error, so src_n must tell.
    std::vector<int32_t> rd_first = P.seg_first;
    std::vector<jfs_compact_seg> rd_seg = P.seg;
    for (int j : own) {
        rd_seg.insert(rd_seg.end(), seg + seg_first[j], seg + seg_first[j + 1]);
        rd_first.push_back((int32_t)rd_seg.size());
    }
    const jfs_plan::ChainRanges lists =
        jfs_plan::chain_ranges(nsrc, (int)rd_first.size() - 1, rd_first.data(), rd_seg.data(), ss, ns);
    const int64_t blk = (int64_t)sizeof(jfs_dev_block), aead = (int64_t)sizeof(jfs_aead_block);
    // records: splice outputs | frames | XXH64 descriptors of the units (csum) | where every output's length is picked
    // from | checksum descriptors (crc) | the seals' descriptors, key cells and checksum seeds (sealed)
    const int64_t m_fr = align16(nsp * (int64_t)sizeof(jfs_splice_out)),
                  m_xd = m_fr + align16(nfr * (int64_t)sizeof(jfs_splice_frame)), m_pk = m_xd + (csum ? align16(nu * blk) : 0),
                  m_cd = m_pk + align16(no * 4ll), m_ad = m_cd + (crc ? align16(no * blk) : 0),
                  m_kn = m_ad + (sealed ? align16(no * aead) : 0), m_sd = m_kn + (sealed ? 64ll * no : 0);
    // results: the spliced outputs' verdicts | every output's payload length | the seals' results | the checksums;
    // scratch: frame offsets | unit hashes
    const int64_t r_len = align16(nsp * 4ll), r_r2 = r_len + align16(no * 4ll), r_crc = r_r2 + (sealed ? align16(no * 4ll) : 0),
                  s_hash = align16(nfr * 4ll);
    ChainExtra x;
    x.meta = m_sd + (sealed && crc ? align16(no * 4ll) : 0);
    x.res = r_crc + (crc ? align16(no * 4ll) : 0);
    x.out = xo[nsp];
    x.scratch = s_hash + align16(nu * 8ll);
    x.opened = sealed ? &T.at : nullptr;
    Chain c;
    // (the chain's own seal and checksum areas stay unused: the outputs are not its units)
    const int64_t rc = chain_open(c, ln, algo, cipher, ss, ns, uu, P.seg_first.data(), true, false, false, false, 0, false,
                                  whole ? -1 : (int64_t)lists.rng.size(), x);
    if (rc != JFS_OK) return rc;
    const ChainLayout &L = c.L;
    const int64_t xout = L.out + c.off.tout;  // the spliced objects' area, mirrored like the outputs'
    std::vector<CopyJob> jobs;
    chain_stage_sources(c, src, src_keys, ss, jobs);
    par_copy(jobs);
    chain_stage_plan(c, uu, src_map, P.seg_first.data(), P.seg.data());
    if (!whole) memcpy(c.h + L.rf, lists.first.data(), (size_t)(ns + 1) * 4);
    if (!whole && !lists.rng.empty()) memcpy(c.h + L.rng, lists.rng.data(), lists.rng.size() * sizeof(jfs_range));
    jfs_dev_block *h_enc = c.host<jfs_dev_block>(L.enc), *h_xd = c.host<jfs_dev_block>(L.xmeta + m_xd);
    for (int u = 0; u < nu; u++) {
        h_enc[u] = jfs_dev_block{c.gat(u), c.d_out(u), (int32_t)uu[u].total, (int32_t)uu[u].cap};
        // only a FRESH piece is hashed here: a whole output's table is the checksummed encoder's
        if (csum) h_xd[u] = P.units[u].piece < 0 ? jfs_dev_block{nullptr, nullptr, 0, 0}
                                                 : jfs_dev_block{c.gat(u), nullptr, (int32_t)uu[u].total, 0};
    }
    jfs_splice_out *h_so = c.host<jfs_splice_out>(L.xmeta);
    jfs_splice_frame *h_fr = c.host<jfs_splice_frame>(L.xmeta + m_fr);
    for (int s = 0; s < nsp; s++) {
        const int j = oo[sp[s]].idx;
        const int32_t f0 = P.frame_first[j], f1 = P.frame_first[j + 1];
        h_so[s] = jfs_splice_out{c.d + xout + xo[s], (int32_t)oo[sp[s]].cap, f0, f1 - f0, 0};
        for (int32_t f = f0; f < f1; f++) {
            const jfs_plan::SpliceFrame &q = P.frames[f];
            // a PASS frame lies in its staged (opened) source (a source with a table is never answered on the host)
            const uint8_t *from = q.src >= 0 ? c.d_in(src_map[q.src]) + q.coff : c.d_out(q.unit);
            h_fr[f] = jfs_splice_frame{from, (int32_t)q.c, (int32_t)q.d, q.x, q.unit, s, 0};
        }
    }
    // every output's finished object: its whole unit's payload area, or its spliced area
    auto d_obj = [&](int k) { return sp_of[oo[k].idx] >= 0 ? c.d + xout + xo[sp_of[oo[k].idx]] : c.d_out(unit_of[oo[k].idx]); };
    for (int k = 0; k < no; k++) {
        const int j = oo[k].idx, s = sp_of[j];
        c.host<int32_t>(L.xmeta + m_pk)[k] = s >= 0 ? ~s : unit_of[j];
        if (crc) c.host<jfs_dev_block>(L.xmeta + m_cd)[k] = jfs_dev_block{d_obj(k), nullptr, 0, 0};
        if (!sealed) continue;
        const jfs_seal_param &p = out_p[j];
        uint8_t *cell = c.h + L.xmeta + m_kn + 64ll * k, *d_cell = c.d + L.xmeta + m_kn + 64ll * k;
        memcpy(cell, p.key, (size_t)jfs_cipher_key_size(cipher));
        memcpy(cell + 32, p.nonce, 12);
        // seal in place; the length comes from the pick on the device
        c.host<jfs_aead_block>(L.xmeta + m_ad)[k] =
            jfs_aead_block{d_obj(k), d_obj(k), (int32_t)oo[k].total, (int32_t)(oo[k].cap + 16), d_cell, d_cell + 32};
        if (crc) c.host<uint32_t>(L.xmeta + m_sd)[k] = seal_header_crc(p);
    }
    hipStream_t ks = c.ks;
    if (hipMemcpyAsync(c.d, c.h, (size_t)L.h2d, hipMemcpyHostToDevice, ks) != hipSuccess) return JFS_ERR_HIP;
    const jfs_dev_block *d_sdesc = c.dev<jfs_dev_block>(L.sdesc), *d_enc = c.dev<jfs_dev_block>(L.enc);
    int32_t *d_srcn = c.dev<int32_t>(L.srcn), *d_ret = c.dev<int32_t>(L.ret), *d_sret = c.dev<int32_t>(L.xres);
    int32_t *d_len = c.dev<int32_t>(L.xres + r_len), *d_r2 = c.dev<int32_t>(L.xres + r_r2);
    uint32_t *d_off = (uint32_t *)(c.sl->sp + c.off.scratch);
    uint64_t *d_hash = (uint64_t *)(c.sl->sp + c.off.scratch + s_hash);
    const int32_t max_total = jfs_plan::chain_max_total(uu);
    auto gather = [&](int pass) {
        return jfs_launch_gather(d_sdesc, d_srcn, ns + 1, c.dev<jfs_compact_out>(L.plan), nu, c.dev<jfs_compact_seg>(L.seg),
                                 max_total, d_ret, pass, ks);
    };
    int lk = whole ? chain_decode(c, nullptr, 0)
                   : chain_decode(c, nullptr, 0, nullptr, c.dev<int32_t>(L.rf), c.dev<jfs_range>(L.rng));
    if (lk == 0) lk = gather(0);
    // a piece of at most 128 KiB comes back as one frame and no table in either layout
    if (lk == 0) lk = launch_kernel(algo, COMPRESS, d_enc, nu, d_ret, ks, csum ? ZSTD_ENCODE_SEEK_CSUM : JFS_ZSTD_PARSE_SEEKABLE);
    if (lk == 0 && csum) lk = jfs_launch_xxh64(c.dev<jfs_dev_block>(L.xmeta + m_xd), nu, d_hash, nullptr, ks);
    // the encoder ran on every unit: a failed gather's verdict replaces its result, and the scan reads it there
    if (lk == 0) lk = gather(1);
    if (lk == 0)
        lk = jfs_launch_zstd_splice(c.dev<jfs_splice_out>(L.xmeta), nsp, c.dev<jfs_splice_frame>(L.xmeta + m_fr), nfr, d_ret,
                                    csum ? d_hash : nullptr, d_off, d_sret, ks);
    // a seal also runs over an output whose gather failed (its verdict in d_len decides on the host)
    if (lk == 0) lk = jfs_launch_chain_pick(c.dev<int32_t>(L.xmeta + m_pk), no, d_ret, d_sret, d_len, ks);
    if (lk == 0 && sealed) lk = jfs_launch_aead(cipher, c.dev<jfs_aead_block>(L.xmeta + m_ad), no, 0, d_r2, d_len, ks);
    if (lk == 0 && crc)
        lk = jfs_launch_crc32c_lens(c.dev<jfs_dev_block>(L.xmeta + m_cd), no, sealed ? d_r2 : d_len,
                                    sealed ? c.dev<uint32_t>(L.xmeta + m_sd) : nullptr, c.dev<uint32_t>(L.xres + r_crc), ks);
    if (!chain_results(c, lk, L.out)) return JFS_ERR_HIP;
    const int32_t *h_len = c.host<int32_t>(L.xres + r_len), *h_r2 = c.host<int32_t>(L.xres + r_r2);
    std::vector<int64_t> res(no), back(no);  // per output: its result, its bytes behind the envelope header
    std::vector<uint8_t *> at(no);           // where output k's object lies in the pinned mirror
    for (int k = 0; k < no; k++) {
        const int j = oo[k].idx, s = sp_of[j];
        // (an object that outgrows its capacity: the bound keeps it out of reach)
        int64_t r = s >= 0 && h_len[k] == 0 ? JFS_ERR_SHORT_BUFFER : chain_out_result(algo, true, h_len[k]);
        if (sealed && r >= 0 && h_r2[k] != r + 16) r = JFS_ERR_HIP;
        else if (sealed && r >= 0 && oo[k].hdr + r + 16 > out[j].dst_cap) r = JFS_ERR_SHORT_BUFFER;
        res[k] = r;
        back[k] = r < 0 ? 0 : sealed ? r + 16 : r;
        at[k] = c.h + (d_obj(k) - c.d);
        if (back[k] > 0 && hipMemcpyAsync(at[k], d_obj(k), (size_t)back[k], hipMemcpyDeviceToHost, ks) != hipSuccess) {
            (void)hipStreamSynchronize(ks);
            return JFS_ERR_HIP;
        }
    }
    if (hipStreamSynchronize(ks) != hipSuccess) return JFS_ERR_HIP;
    for (int k = 0; k < ns; k++) {
        const int i = ss[k].idx;
        const int32_t raw = c.host<int32_t>(L.srcn)[k];
        // a table: its content size where every selected frame decoded and verified (none selected: 0)
        if (!whole && P.tab[i].valid && raw >= 0) src_n[i] = (int64_t)P.tab[i].total;
        else src_n[i] = !whole && raw == -4 ? JFS_ERR_CHECKSUM : chain_src_result(c, k);
    }
    jobs.clear();
    for (int k = 0; k < no; k++) {
        const int j = oo[k].idx;
        if (sealed && res[k] >= 0) seal_header_write(out[j].dst, out_p[j]);
        if (back[k] > 0) jobs.push_back({out[j].dst + oo[k].hdr, at[k], back[k]});
        out_n[j] = res[k] >= 0 ? oo[k].hdr + back[k] : res[k];
        if (crc) crc[j] = res[k] < 0 ? 0u : c.host<uint32_t>(L.xres + r_crc)[k];
    }
    par_copy(jobs);
    g_splice_counts[0].fetch_add(P.outs, std::memory_order_relaxed);
    g_splice_counts[1].fetch_add(P.passed, std::memory_order_relaxed);
    g_splice_counts[2].fetch_add(P.fresh, std::memory_order_relaxed);
    g_splice_counts[3].fetch_add(P.passed_bytes, std::memory_order_relaxed);
    return JFS_OK;
}

// The GET-side mirror of compact_run, its staging and decoder choice: stored
// bytes and the plan H2D, CRC-32C of every object that has an expected value
// (for an envelope the payload's, seeded on the host with the header's), open
// in place, decode, the opens' verdicts and then the checksums' verdicts
// merged into the source lengths, plan and flat gather into one packed area
// (16-byte aligned offsets), one D2H of the results and that area; the host
// copies the good reads out.  st[0, ns) are the decoded sources, the rest
// objects the host already answered, staged whole only for their checksum.
// Returns JFS_OK with src_n / out_n / crc_got of these objects filled, or
// JFS_ERR_NO_MEMORY / JFS_ERR_HIP.
// need (the prefix modes with a codec they cover, else null): per object of the call,
// the last byte a segment asks of it; the decode of source k stops there
// (clamped to its capacity, staged behind the expected checksums in the same
// H2D copy) unless every source is needed whole, which takes the full
// launchers.
// from (Zstd with JFS_READ_SEEK on, else null; `need` comes with it): per object
// of the call, the first byte a segment asks of it.  Every source then goes
// through the range launcher, [from, need) clamped to its capacity, also in a
// call that needs every source whole.
// sparse (Zstd with JFS_READ_SEEK sparse; need and from are then null): every
// source goes through the ranges launcher with the list chain_ranges makes of
// the segments that reference it, staged beside want and from in the same H2D
// copy; a source whose decoded frame fails its table checksum (-4) answers
// JFS_ERR_CHECKSUM.
// csum (the _csum calls, else null): per read of the call, where its
// disk-cache checksum goes (null: none).  The piece prefix of the reads that
// want one is staged with the plan, read_csum_flat_kernel runs behind the
// gather on the same stream, and the checksum area comes back in front of the
// reads in the same D2H copy.  A call without such a read is laid out and
// queued exactly like one without csum.
int64_t read_run(DevCtx *dev, Lane &ln, int algo, int cipher, const jfs_iov *src, const uint8_t *const *src_keys,
                 const std::vector<ChainSrc> &st, int ns, const std::vector<int> &src_map, const jfs_iov *out,
                 const std::vector<ChainOut> &oo, const int32_t *seg_first, const jfs_compact_seg *seg, int64_t *src_n,
                 int64_t *out_n, uint32_t *crc_got, const int64_t *need, const int64_t *from, uint8_t *const *csum,
                 int nsrc = 0, int nout = 0, bool sparse = false, int nchase = 0) {
    LaneRun scope(dev, ln, algo * 2 + DECOMPRESS, (uint64_t)st.size());
    const int n = (int)st.size(), no = (int)oo.size();
    bool any_check = false;
    for (const ChainSrc &s : st) any_check = any_check || s.check;
    std::vector<int32_t> tile_first(no + 1), want;
    int64_t ntiles = 0, max_want = 0;
    for (int k = 0; k < no; k++) {
        tile_first[k] = (int32_t)ntiles;
        ntiles += jfs_gather_tiles(oo[k].total);
        if (ntiles > INT32_MAX) return JFS_ERR_NO_MEMORY;
    }
    tile_first[no] = (int32_t)ntiles;
    const bool seek = need && from && algo == JFS_ALGO_ZSTD && ns > 0;
    if (need && (algo == JFS_ALGO_LZ4 || algo == JFS_ALGO_ZSTD)) want = jfs_plan::chain_want(need, st, ns, &max_want, seek);
    const bool prefix = !want.empty();
    sparse = sparse && algo == JFS_ALGO_ZSTD && ns > 0;
    jfs_plan::ChainRanges lists;
    // (LZ4 with JFS_READ_LZ4_CHASE on: read_call moved the nchase sources that take the chase to the front)
    nchase = algo == JFS_ALGO_LZ4 ? std::min(nchase, ns) : 0;
    const bool listed = sparse || nchase > 0;
    if (listed) lists = jfs_plan::chain_ranges(nsrc, nout, seg_first, seg, st, ns);
    std::vector<uint8_t> cs_want(no, 0);
    std::vector<int32_t> piece_first;
    std::vector<int64_t> cs_off;
    int64_t npiece = 0;
    if (csum) {
        for (int k = 0; k < no; k++) cs_want[k] = csum[oo[k].idx] != nullptr;
        npiece = jfs_plan::chain_csum_pieces(oo, cs_want, piece_first, cs_off);
        if (npiece < 0) return JFS_ERR_NO_MEMORY;
    }
    Chain c;
    const int64_t rc = chain_open(c, ln, algo, cipher, st, ns, oo, seg_first, false, false, any_check, prefix, npiece, seek,
                                  listed ? (int64_t)lists.rng.size() : -1);
    if (rc != JFS_OK) return rc;
    const ChainLayout &L = c.L;
    memcpy(c.h + L.tf, tile_first.data(), (size_t)(no + 1) * 4);
    if (npiece > 0) memcpy(c.h + L.pf, piece_first.data(), (size_t)(no + 1) * 4);
    if (prefix) memcpy(c.h + L.want, want.data(), (size_t)ns * 4);
    if (seek) memcpy(c.h + L.from, jfs_plan::chain_lo(from, st, ns).data(), (size_t)ns * 4);
    if (listed) {
        memcpy(c.h + L.rf, lists.first.data(), (size_t)(ns + 1) * 4);
        if (!lists.rng.empty()) memcpy(c.h + L.rng, lists.rng.data(), lists.rng.size() * sizeof(jfs_range));
    }
    std::vector<CopyJob> jobs;
    chain_stage_sources(c, src, src_keys, st, jobs);
    for (int k = 0; any_check && k < n; k++) {
        const ChainSrc &s = st[k];
        // the checksum covers the object as fetched: the staged bytes, behind the envelope header's on the host
        c.host<jfs_dev_block>(L.scd)[k] = jfs_dev_block{c.d_in(k), nullptr, (int32_t)s.pay, 0};
        c.host<uint32_t>(L.sseed)[k] = s.check && s.off > 0 ? host_crc32c(0, src[s.idx].src, s.off) : 0u;
        c.host<int32_t>(L.len)[k] = s.check && s.pay > 0 ? (int32_t)s.pay : -1;
        c.host<uint32_t>(L.exp)[k] = s.expect;
    }
    par_copy(jobs);
    chain_stage_plan(c, oo, src_map, seg_first, seg);
    if (nchase > 0) {
        // the chase and the decoders of the rest run one after the other on slot 1's scratch
        const jfs_dev_block *h_sdesc = c.host<jfs_dev_block>(L.sdesc);
        int64_t sneed = jfs_lz4_chase_scratch_bytes(nchase, desc_lens(h_sdesc, nchase).data());
        if (ns > nchase)
            sneed = std::max(sneed, lz4_decode_scratch(ns - nchase, desc_lens(h_sdesc + nchase, ns - nchase).data(),
                                                       desc_caps(h_sdesc + nchase, ns - nchase).data()));
        if (!c.s1->ensure_split(sneed)) return JFS_ERR_NO_MEMORY;
    } else if (!chain_lz4_scratch(c, nullptr, false)) {
        return JFS_ERR_NO_MEMORY;
    }
    hipStream_t ks = c.ks;
    // one H2D: stored bytes, the plan, keys, checksum inputs and the preset source lengths
    if (hipMemcpyAsync(c.d, c.h, (size_t)L.h2d, hipMemcpyHostToDevice, ks) != hipSuccess) return JFS_ERR_HIP;
    int32_t *d_srcn = c.dev<int32_t>(L.srcn);
    const int32_t *d_len = c.dev<int32_t>(L.len);
    int lk = 0;
    // verifyChecksum sits in front of Decrypt and Decompress: before the open rewrites the staged bytes
    if (any_check)
        lk = jfs_launch_crc32c_lens(c.dev<jfs_dev_block>(L.scd), n, d_len, c.dev<uint32_t>(L.sseed),
                                    c.dev<uint32_t>(L.scrc), ks);
    if (lk == 0)
        lk = chain_decode(c, prefix ? c.dev<int32_t>(L.want) : nullptr, max_want, seek ? c.dev<int32_t>(L.from) : nullptr,
                          listed ? c.dev<int32_t>(L.rf) : nullptr, listed ? c.dev<jfs_range>(L.rng) : nullptr, nchase,
                          nchase > 0 ? jfs_plan::chain_range_quads(lists, nchase) : 0);
    if (lk == 0 && any_check)
        lk = jfs_launch_verify_gate(c.dev<uint32_t>(L.scrc), d_len, c.dev<uint32_t>(L.exp), n, ns, d_srcn,
                                    c.dev<uint32_t>(L.got), ks);
    if (lk == 0)
        lk = jfs_launch_gather_flat(c.dev<jfs_dev_block>(L.sdesc), d_srcn, ns + 1, c.dev<jfs_compact_out>(L.plan), no,
                                    c.dev<jfs_compact_seg>(L.seg), c.dev<int32_t>(L.ret), c.dev<int32_t>(L.tf), ntiles,
                                    ks);
    if (lk == 0 && npiece > 0)
        lk = jfs_launch_read_csum_flat(c.dev<jfs_compact_out>(L.plan), no, c.dev<int32_t>(L.ret), c.dev<int32_t>(L.pf),
                                       npiece, c.dev<uint32_t>(L.csum), ks);
    // one D2H: the results, the checksums and every read, packed
    if (!chain_results(c, lk, L.out + c.off.tout)) return JFS_ERR_HIP;
    for (int k = 0; k < n; k++) {
        const ChainSrc &s = st[k];
        const uint32_t got = s.check && s.pay > 0 ? c.host<uint32_t>(L.got)[k] : 0u;  // an empty object's CRC is 0
        if (crc_got) crc_got[s.idx] = got;
        if (s.check && got != s.expect) src_n[s.idx] = JFS_ERR_CHECKSUM;  // before aead.Open and the codec
        else if (k < ns) src_n[s.idx] = chain_src_result(c, k);          // (else the host's answer stands)
        // a decoded frame that fails its table checksum (only the ranges launcher answers -4)
        if (sparse && k < ns && src_n[s.idx] == JFS_ERR_CORRUPT && c.host<int32_t>(L.srcn)[k] == -4)
            src_n[s.idx] = JFS_ERR_CHECKSUM;
    }
    jobs.clear();
    for (int k = 0; k < no; k++) {
        const int j = oo[k].idx;
        out_n[j] = chain_out_result(algo, false, c.host<int32_t>(L.ret)[k]);
        if (out_n[j] > 0) jobs.push_back({out[j].dst, c.h_out(k), out_n[j]});
        if (out_n[j] > 0 && cs_want[k]) jobs.push_back({csum[j], c.h + L.csum + cs_off[k], 4 * jfs_plan::csum_pieces(out_n[j])});
    }
    par_copy(jobs);
    return JFS_OK;
}

// The plan checks jfs_compact_batch and jfs_compact_seal_batch share (before
// any device is touched); total[j] = output j's gathered bytes.
bool compact_plan_ok(int algo, int nsrc, const jfs_iov *src, int nout, const jfs_iov *out, const int32_t *seg_first,
                     const jfs_compact_seg *seg, const int64_t *src_n, const int64_t *out_n,
                     std::vector<int64_t> &total) {
    if (algo != JFS_ALGO_NONE && algo != JFS_ALGO_LZ4 && algo != JFS_ALGO_ZSTD) return false;
    if (nsrc < 0 || nout < 0 || (nsrc > 0 && (!src || !src_n)) || (nout > 0 && (!out || !out_n || !seg_first)))
        return false;
    for (int i = 0; i < nsrc; i++) {
        const jfs_iov &v = src[i];
        if (v.src_len < 0 || v.dst_cap < 0 || v.src_len > INT32_MAX || v.dst_cap > INT32_MAX || (v.src_len > 0 && !v.src))
            return false;
    }
    total.assign(nout, 0);
    for (int j = 0; j < nout; j++) {
        if (out[j].dst_cap < 0 || (out[j].dst_cap > 0 && !out[j].dst)) return false;
        if (seg_first[j] < 0 || seg_first[j + 1] < seg_first[j] || (seg_first[j + 1] > seg_first[j] && !seg))
            return false;
        for (int k = seg_first[j]; k < seg_first[j + 1]; k++) {
            const jfs_compact_seg &s = seg[k];
            if (s.len <= 0 || (int64_t)s.dst_off != total[j] || s.src < -1 || s.src >= nsrc ||
                (s.src >= 0 && s.src_off < 0))
                return false;
            total[j] += s.len;
            if (total[j] > INT32_MAX) return false;
        }
    }
    return true;
}

// The sources of a chain call.  What the host answers before the device runs
// (chain_src_answer) goes to src_n; the sources the device decodes go to st,
// with src_map[i] = their position, and their count is returned.  Behind them
// st gets the answered objects that still need the device for their checksum
// (src_crc, reads only: verifyChecksum reads the whole object first).
int chain_sources(int algo, bool sealed, int nsrc, const jfs_iov *src, const int64_t *src_crc, int64_t *src_n,
                  uint32_t *crc_got, std::vector<ChainSrc> &st, std::vector<int> &src_map) {
    std::vector<ChainSrc> only_crc;
    src_map.assign(nsrc, -1);
    for (int i = 0; i < nsrc; i++) {
        const jfs_iov &v = src[i];
        const bool check = src_crc && src_crc[i] >= 0;
        ChainSrc r{i, 0, 0, 0, 0, check, check ? (uint32_t)src_crc[i] : 0u};
        if (crc_got) crc_got[i] = 0;
        src_n[i] = jfs_plan::chain_src_answer(algo, sealed, v, r);
        if (src_n[i] == JFS_OK) {
            // with a cipher dst_cap is staged for every codec: the Zstd frame
            // header is ciphertext on the host (see jfs_open_decompress_batch)
            r.cap = algo == JFS_ALGO_NONE ? (sealed ? r.pay - 16 : r.pay)
                    : sealed              ? std::min<int64_t>(v.dst_cap, INT32_MAX)
                                          : staged_cap(algo, DECOMPRESS, v);
            src_map[i] = (int)st.size();
            st.push_back(r);
        } else if (check && v.src_len == 0) {  // an empty object: CRC 0, no device needed
            if (r.expect != 0) src_n[i] = JFS_ERR_CHECKSUM;
        } else if (check) {
            only_crc.push_back(r);
        }
    }
    const int ns = (int)st.size();
    st.insert(st.end(), only_crc.begin(), only_crc.end());
    return ns;
}

std::atomic<unsigned> g_compact_turn{0};

// Runs a chain call's device part, run(dev, lane), on the next device in turn
// with one of its lanes held, if the call left the device anything to do.  A
// chain that did not run (JFS_ERR_NO_MEMORY / JFS_ERR_HIP, which is returned):
// every block it held reports why.
template <class Run>
int64_t chain_dispatch(const std::vector<DevCtx *> &ds, int algo, int dir, const std::vector<ChainSrc> &st,
                       const std::vector<ChainOut> &oo, int64_t *src_n, int64_t *out_n, Run run) {
    if (st.empty() && oo.empty()) return JFS_OK;
    DevCtx *dev = ds[g_compact_turn.fetch_add(1) % ds.size()];
    std::unique_lock<std::mutex> lk;
    Lane &ln = dev->acquire_lane(lk, algo * 2 + dir);
    const int64_t rc = run(dev, ln);
    if (rc == JFS_ERR_HIP) (void)lane_healthy(dev, ln);  // leave nothing in flight into the staging
    if (rc != JFS_OK) {
        for (const ChainSrc &s : st) src_n[s.idx] = rc;
        for (const ChainOut &o : oo) out_n[o.idx] = rc;
    }
    return rc;
}

// One direction's statistics of a chain call over its nblk blocks: len(i) =
// block i's input bytes, batch = the device worked on some, nanos = the call's
// time (< 0: it is counted on the other direction).
template <class Len>
void chain_stat(int algo, int dir, int nblk, Len len, const int64_t *res, bool batch, int64_t nanos) {
    OpStats *st = op_stats(algo, dir);
    if (!st) return;
    st->calls.fetch_add(1, std::memory_order_relaxed);
    if (batch) st->batches.fetch_add(1, std::memory_order_relaxed);
    for (int i = 0; i < nblk; i++) stat_block(st, len(i), res[i]);
    if (nanos >= 0) st->nanos.fetch_add((uint64_t)nanos, std::memory_order_relaxed);
}

// Small-batch device launches: per-device scratch shared by every caller,
// ordered across streams by an event (like the Zstd device decoder's).
struct SplitScratch {
    std::mutex mu;
    uint8_t *p = nullptr;
    int64_t cap = 0;
    hipEvent_t ev_done = nullptr;
};
SplitScratch g_split[64], g_eseg_scr[64], g_fast_scr[64], g_read_scr[64], g_splice_scr[64];

// One LZ4 small-batch launch (nblk > 0) on the caller's stream with `need`
// bytes of the current device's scratch in `tab`: launch(scratch, cap, stream)
template <class Launch>
int64_t scratch_launch(SplitScratch *tab, int dir, int nblk, int64_t need, void *stream, Launch launch) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return JFS_ERR_HIP;
    stat_launch(JFS_ALGO_LZ4, dir, nblk);
    SplitScratch &z = tab[dev];
    std::lock_guard<std::mutex> lk(z.mu);
    if (!z.ev_done && hipEventCreateWithFlags(&z.ev_done, hipEventDisableTiming) != hipSuccess) return JFS_ERR_HIP;
    if (need > z.cap) {
        if (hipEventSynchronize(z.ev_done) != hipSuccess) return JFS_ERR_HIP;  // earlier launches may still use it
        if (z.p) (void)hipFree(z.p);
        z.p = nullptr;
        z.cap = 0;
        int64_t want = 64ll << 20;
        while (want < need) want <<= 1;
        if (hipMalloc((void **)&z.p, (size_t)want) != hipSuccess) return JFS_ERR_NO_MEMORY;
        z.cap = want;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipStreamWaitEvent(st, z.ev_done, 0) != hipSuccess) return JFS_ERR_HIP;
    if (launch(z.p, z.cap, st) != 0) return JFS_ERR_HIP;
    return hipEventRecord(z.ev_done, st) == hipSuccess ? JFS_OK : JFS_ERR_HIP;
}

}  // namespace

extern "C" {

int jfs_codec_from_name(const char *name) {
    if (!name) return -1;
    std::string s(name);
    for (auto &ch : s) ch = (char)tolower((unsigned char)ch);
    if (s == "zstd") return JFS_ALGO_ZSTD;
    if (s == "lz4") return JFS_ALGO_LZ4;
    if (s == "none" || s.empty()) return JFS_ALGO_NONE;
    return -1;
}

const char *jfs_codec_name(int algo) {
    switch (algo) {
        case JFS_ALGO_NONE: return "Noop";
        case JFS_ALGO_LZ4: return "LZ4";
        case JFS_ALGO_ZSTD: return "Zstd";
        default: return nullptr;
    }
}

int64_t jfs_compress_bound(int algo, int64_t n) {
    switch (algo) {
        case JFS_ALGO_NONE: return n;
        case JFS_ALGO_LZ4:
            // LZ4_compressBound takes an int: (unsigned)n > LZ4_MAX_INPUT_SIZE -> 0
            if ((uint64_t)(uint32_t)n != (uint64_t)n && n >= 0) return 0;
            if ((uint32_t)n > (uint32_t)LZ4_MAX_INPUT) return 0;
            return n + n / 255 + 16;
        case JFS_ALGO_ZSTD: {
            int64_t low = 128 << 10;
            int64_t margin = n < low ? (low - n) >> 11 : 0;
            return n + (n >> 8) + margin;
        }
        default: return JFS_ERR_INVALID;
    }
}

static int64_t one_call(int algo, int dir, uint8_t *dst, int64_t dst_cap, const uint8_t *src, int64_t n) {
    if (algo != JFS_ALGO_NONE && algo != JFS_ALGO_LZ4 && algo != JFS_ALGO_ZSTD) return JFS_ERR_INVALID;
    const int64_t t0 = steady_ns();
    jfs_iov v{src, n, dst, dst_cap};
    int64_t r;
    if (!pre_answer(algo, dir, v, &r)) r = Coalescer::get().submit(algo, dir, v);
    OpStats *st = op_stats(algo, dir);
    st->calls.fetch_add(1, std::memory_order_relaxed);
    stat_block(st, n, r);
    st->nanos.fetch_add((uint64_t)(steady_ns() - t0), std::memory_order_relaxed);
    return r;
}

int64_t jfs_compress(int algo, uint8_t *dst, int64_t dst_cap, const uint8_t *src, int64_t n) {
    return one_call(algo, COMPRESS, dst, dst_cap, src, n);
}

int64_t jfs_decompress(int algo, uint8_t *dst, int64_t dst_cap, const uint8_t *src, int64_t n) {
    return one_call(algo, DECOMPRESS, dst, dst_cap, src, n);
}

static int64_t batch_call(int algo, int dir, int nblk, const jfs_iov *iov, int64_t *out_n, uint32_t device_mask,
                          uint32_t *crc = nullptr, uint8_t *const *csum = nullptr) {
    const int64_t t0 = steady_ns();
    const int64_t r = batch_common(algo, dir, nblk, iov, out_n, device_mask, crc, csum);
    stat_call(algo, dir, r, nblk, iov, out_n, t0);
    return r;
}

int64_t jfs_envelope_bound(int algo, int64_t n, int32_t wrapped_len) {
    if (n < 0 || wrapped_len < 0 || wrapped_len > 65535) return JFS_ERR_INVALID;
    const int64_t b = algo == JFS_ALGO_NONE ? n : jfs_compress_bound(algo, n);
    if (b < 0) return b;
    return 3 + wrapped_len + 12 + b + 16;
}

int64_t jfs_envelope_parse(const uint8_t *src, int64_t n, int64_t *wrapped_off, int64_t *wrapped_len,
                           int64_t *nonce_off, int64_t *nonce_len) {
    return envelope_parse(src, n, wrapped_off, wrapped_len, nonce_off, nonce_len);
}

int64_t jfs_compress_seal_batch(int algo, int cipher, int nblk, const jfs_iov *iov, const jfs_seal_param *p,
                                int64_t *out_n, uint32_t *crc, uint32_t device_mask) {
    if (nblk < 0 || (nblk > 0 && (!iov || !out_n || !p))) return JFS_ERR_INVALID;
    if (algo != JFS_ALGO_NONE && algo != JFS_ALGO_LZ4 && algo != JFS_ALGO_ZSTD) return JFS_ERR_INVALID;
    if (jfs_cipher_key_size(cipher) < 0) return JFS_ERR_INVALID;
    const int64_t t0 = steady_ns();
    std::vector<int> todo;
    std::vector<jfs_iov> iov2, orig;
    std::vector<const uint8_t *> key, nonce;
    std::vector<jfs_seal_param> sp;
    std::vector<int64_t> hdr;
    for (int i = 0; i < nblk; i++) {
        if (crc) crc[i] = 0;
        const jfs_iov &v = iov[i];
        const jfs_seal_param &q = p[i];
        const int64_t bound = jfs_envelope_bound(algo, v.src_len, q.wrapped_len);
        if (v.src_len < 0 || v.dst_cap < 0 || !q.key || !q.nonce || bound < 0 || (q.wrapped_len > 0 && !q.wrapped) ||
            (v.src_len > 0 && !v.src)) {
            out_n[i] = JFS_ERR_INVALID;
            continue;
        }
        if (algo == JFS_ALGO_LZ4 && v.src_len > LZ4_MAX_INPUT) {
            out_n[i] = JFS_ERR_COMPRESS_FAIL;
            continue;
        }
        if (v.dst_cap < bound) {
            out_n[i] = JFS_ERR_SHORT_BUFFER;
            continue;
        }
        todo.push_back(i);
        const int64_t pay = bound - (3 + q.wrapped_len + 12);  // codec bound + tag
        iov2.push_back(jfs_iov{v.src, v.src_len, nullptr, pay});
        orig.push_back(v);
        key.push_back(q.key);
        nonce.push_back(q.nonce);
        sp.push_back(q);
        hdr.push_back(3 + q.wrapped_len + 12);
    }
    int64_t rc = JFS_OK;
    if (!todo.empty()) {
        Aead ae{cipher, true, orig.data(), key.data(), nonce.data(), sp.data(), hdr.data()};
        rc = deal(algo, COMPRESS, todo, iov2, out_n, device_mask, &ae, crc);
    }
    stat_call(algo, COMPRESS, rc, nblk, iov, out_n, t0);
    return rc;
}

// jfs_open_decompress_batch (csum null) and jfs_open_decompress_batch_csum
static int64_t open_batch_call(int algo, int cipher, int nblk, const jfs_iov *iov, const uint8_t *const *keys,
                               int64_t *out_n, uint32_t device_mask, uint8_t *const *csum) {
    if (nblk < 0 || (nblk > 0 && (!iov || !out_n || !keys))) return JFS_ERR_INVALID;
    if (algo != JFS_ALGO_NONE && algo != JFS_ALGO_LZ4 && algo != JFS_ALGO_ZSTD) return JFS_ERR_INVALID;
    if (jfs_cipher_key_size(cipher) < 0) return JFS_ERR_INVALID;
    const int64_t t0 = steady_ns();
    std::vector<int> todo;
    std::vector<jfs_iov> iov2, orig;
    std::vector<const uint8_t *> key, nonce;
    for (int i = 0; i < nblk; i++) {
        const jfs_iov &v = iov[i];
        int64_t noff = 0, nlen = 0;
        const int64_t off = envelope_parse(v.src, v.src_len, nullptr, nullptr, &noff, &nlen);
        if (v.dst_cap < 0 || !keys[i]) {
            out_n[i] = JFS_ERR_INVALID;
            continue;
        }
        if (off < 0 || nlen != 12) {  // the AEADs here all take 12-byte nonces
            out_n[i] = JFS_ERR_CORRUPT;
            continue;
        }
        const int64_t pay = v.src_len - off;  // ciphertext || tag
        if (pay < 16) {
            out_n[i] = JFS_ERR_AUTH;  // aead.Open rejects a payload shorter than the tag
            continue;
        }
        if (algo != JFS_ALGO_NONE && pay == 16) {  // the codec would see an empty input
            out_n[i] = JFS_ERR_EMPTY_INPUT;
            continue;
        }
        int64_t cap;
        if (algo == JFS_ALGO_NONE) {
            if (v.dst_cap < pay - 16) {  // noOp.Decompress: "buffer too short" (compress.go:63-65)
                out_n[i] = JFS_ERR_SHORT_BUFFER;
                continue;
            }
            cap = pay - 16;
        } else if (algo == JFS_ALGO_ZSTD) {
            // DataDog's size hint reads the frame header, which is still
            // ciphertext here: stage dst_cap (frames from pkg/compress carry
            // their content size, for which both rules agree)
            cap = std::min<int64_t>(v.dst_cap, INT32_MAX);
        } else {
            jfs_iov pv{v.src + off, pay - 16, v.dst, v.dst_cap};
            cap = staged_cap(algo, DECOMPRESS, pv);
        }
        todo.push_back(i);
        iov2.push_back(jfs_iov{v.src + off, pay, nullptr, cap});
        orig.push_back(v);
        key.push_back(keys[i]);
        nonce.push_back(v.src + noff);
    }
    int64_t rc = JFS_OK;
    if (!todo.empty()) {
        Aead ae{cipher, false, orig.data(), key.data(), nonce.data(), nullptr, nullptr};
        rc = deal(algo, DECOMPRESS, todo, iov2, out_n, device_mask, &ae, nullptr, csum);
    }
    stat_call(algo, DECOMPRESS, rc, nblk, iov, out_n, t0);
    return rc;
}

int64_t jfs_open_decompress_batch(int algo, int cipher, int nblk, const jfs_iov *iov, const uint8_t *const *keys,
                                  int64_t *out_n, uint32_t device_mask) {
    return open_batch_call(algo, cipher, nblk, iov, keys, out_n, device_mask, nullptr);
}

int64_t jfs_open_decompress_batch_csum(int algo, int cipher, int nblk, const jfs_iov *iov, const uint8_t *const *keys,
                                       int64_t *out_n, uint8_t *const *csum, uint32_t device_mask) {
    if (nblk > 0 && !csum) return JFS_ERR_INVALID;
    return open_batch_call(algo, cipher, nblk, iov, keys, out_n, device_mask, csum);
}

int64_t jfs_compress_batch(int algo, int nblk, const jfs_iov *iov, int64_t *out_n, uint32_t device_mask) {
    return batch_call(algo, COMPRESS, nblk, iov, out_n, device_mask);
}

// Mixed-codec batches: the blocks of each codec form one batch call.  Decode
// calls run at once (a device has two lanes, so an LZ4 and a Zstd batch share
// every device instead of queueing one behind the other: config 4 decode
// 13.2 -> 21.9 GiB/s); encode calls run in turn (see below).
static int64_t batch_mixed(int dir, const int32_t *algo, int nblk, const jfs_iov *iov, int64_t *out_n,
                           uint32_t device_mask) {
    if (nblk < 0 || (nblk > 0 && (!algo || !iov || !out_n))) return JFS_ERR_INVALID;
    std::vector<int> idx[3];
    for (int i = 0; i < nblk; i++) {
        const int a = algo[i];
        if (a != JFS_ALGO_NONE && a != JFS_ALGO_LZ4 && a != JFS_ALGO_ZSTD) {
            out_n[i] = JFS_ERR_INVALID;
            continue;
        }
        idx[a].push_back(i);
    }
    struct Group {
        int algo;
        std::vector<jfs_iov> iov;
        std::vector<int64_t> out;
        int64_t rc = JFS_OK;
    };
    std::vector<Group> gs;
    for (int a = 0; a < 3; a++) {
        if (idx[a].empty()) continue;
        Group g;
        g.algo = a;
        for (int i : idx[a]) g.iov.push_back(iov[i]);
        g.out.assign(idx[a].size(), 0);
        gs.push_back(std::move(g));
    }
    auto run = [&](Group &g) {
        g.rc = batch_call(g.algo, dir, (int)g.iov.size(), g.iov.data(), g.out.data(), device_mask);
    };
    static const bool enc_together = [] {
        const char *e = getenv("JFS_MIXED_ENCODE_TOGETHER");
        return e && atoi(e) != 0;
    }();
    if (dir == DECOMPRESS || enc_together) {
        std::vector<std::thread> th;
        for (size_t k = 1; k < gs.size(); k++) th.emplace_back(run, std::ref(gs[k]));
        if (!gs.empty()) run(gs[0]);
        for (auto &t : th) t.join();
    } else {
        // encoders one codec after the other: measured on config 4's mix, the
        // LZ4 serial-parse kernels beside the Zstd encoder's host-synchronised
        // parse rounds ran 0.93 GiB/s against 1.47 in turn
        for (Group &g : gs) run(g);
    }
    // the first failing codec call's code is returned, and every block of a
    // failed call reports it in out_n (never a stale length)
    int64_t rc = JFS_OK;
    for (Group &g : gs) {
        const std::vector<int> &ix = idx[g.algo];
        if (g.rc != JFS_OK) {
            if (rc == JFS_OK) rc = g.rc;
            for (size_t k = 0; k < ix.size(); k++) out_n[ix[k]] = g.rc;
            continue;
        }
        for (size_t k = 0; k < ix.size(); k++) out_n[ix[k]] = g.out[k];
    }
    return rc;
}

int64_t jfs_compress_batch_mixed(const int32_t *algo, int nblk, const jfs_iov *iov, int64_t *out_n,
                                 uint32_t device_mask) {
    return batch_mixed(COMPRESS, algo, nblk, iov, out_n, device_mask);
}

int64_t jfs_decompress_batch_mixed(const int32_t *algo, int nblk, const jfs_iov *iov, int64_t *out_n,
                                   uint32_t device_mask) {
    return batch_mixed(DECOMPRESS, algo, nblk, iov, out_n, device_mask);
}

int64_t jfs_compress_batch_crc(int algo, int nblk, const jfs_iov *iov, int64_t *out_n, uint32_t *crc,
                               uint32_t device_mask) {
    if (nblk > 0 && !crc) return JFS_ERR_INVALID;
    return batch_call(algo, COMPRESS, nblk, iov, out_n, device_mask, crc);
}

int64_t jfs_decompress_batch(int algo, int nblk, const jfs_iov *iov, int64_t *out_n, uint32_t device_mask) {
    return batch_call(algo, DECOMPRESS, nblk, iov, out_n, device_mask);
}

int64_t jfs_decompress_batch_csum(int algo, int nblk, const jfs_iov *iov, int64_t *out_n, uint8_t *const *csum,
                                  uint32_t device_mask) {
    if (nblk > 0 && !csum) return JFS_ERR_INVALID;
    return batch_call(algo, DECOMPRESS, nblk, iov, out_n, device_mask, nullptr, csum);
}

void jfs_deal_plan(const int64_t *cost, int n, int ndev, int32_t *out_dev) {
    if (!cost || !out_dev || n <= 0) return;
    plan_deal(cost, n, ndev, out_dev);
}

int64_t jfs_test_spread_locking(int ndev, int iters, int timeout_ms) {
    if (ndev < 1 || ndev > 32 || iters < 1) return -2;
    // fake devices (no GPU state: only their lane mutexes are used)
    struct Run {
        std::vector<DevCtx *> devs;
        std::atomic<int> finished{0};
        std::atomic<int64_t> spread{0};
    };
    auto *r = new Run;  // leaked on a deadlock (the stuck threads still use it)
    for (int d = 0; d < ndev; d++) {
        r->devs.push_back(new DevCtx);
        r->devs.back()->id = d;
    }
    const int nthr = ndev * NLANE;
    for (int t = 0; t < nthr; t++) {
        std::thread([r, t, iters, ndev] {
            DevCtx *dev = r->devs[t / NLANE];
            Lane &ln = dev->lane[t % NLANE];
            for (int i = 0; i < iters; i++) {
                SpreadLanes sl;
                spread_acquire(dev, ln, r->devs, ndev + 1, sl);
                if (!sl.hdev.empty()) r->spread.fetch_add(1);
                std::this_thread::yield();
                sl.release();
            }
            r->finished.fetch_add(1);
        }).detach();
    }
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms);
    while (r->finished.load() < nthr) {
        if (std::chrono::steady_clock::now() > t_end) return -1;  // deadlocked
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
    const int64_t sp = r->spread.load();
    for (DevCtx *d : r->devs) delete d;
    delete r;
    return sp;
}

// The device-resident entry points launch on the caller's current device; it
// must be one the library selected (gfx950, in JFS_GPU_DEVICES).
static bool current_device_ok() {
    std::vector<DevCtx *> &ds = devices();
    int cur = -1;
    if (ds.empty() || hipGetDevice(&cur) != hipSuccess) return false;
    for (DevCtx *d : ds)
        if (d->id == cur) return true;
    return false;
}

int64_t jfs_lz4_decompress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_LZ4, DECOMPRESS, nblk);
    return jfs_launch_lz4_decode(d_blocks, nblk, d_ret, (hipStream_t)stream) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_lz4_decompress_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len, const int32_t *dst_cap,
                                        int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && (!src_len || !dst_cap))) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    const jfs_plan::Lz4SplitGeom g = jfs_plan::lz4_split_geom(nblk, src_len, dst_cap);
    return scratch_launch(g_split, DECOMPRESS, nblk, jfs_lz4_split_scratch_bytes(nblk, src_len, dst_cap), stream,
                          [&](uint8_t *p, int64_t, hipStream_t st) {
                              return jfs_launch_lz4_split(d_blocks, nblk, d_ret, p, g.nseg, g.max_cap, g.norg, st);
                          });
}

int64_t jfs_lz4_decompress_prefix_device(const jfs_dev_block *d_blocks, const int32_t *d_want, int nblk,
                                         int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk > 0 && !d_want) return JFS_ERR_INVALID;
    stat_launch(JFS_ALGO_LZ4, DECOMPRESS, nblk);
    return jfs_launch_lz4_decode_prefix(d_blocks, nblk, d_ret, d_want, nullptr, (hipStream_t)stream) == 0 ? JFS_OK
                                                                                                          : JFS_ERR_HIP;
}

int64_t jfs_lz4_decompress_prefix_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len,
                                               const int32_t *dst_cap, const int32_t *d_want, int nblk,
                                               int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && (!src_len || !dst_cap || !d_want))) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    const jfs_plan::Lz4SplitGeom g = jfs_plan::lz4_split_geom(nblk, src_len, dst_cap);
    // (want lives on the device only: the grids stay sized by the largest dst_cap)
    return scratch_launch(g_split, DECOMPRESS, nblk, jfs_lz4_split_scratch_bytes(nblk, src_len, dst_cap), stream,
                          [&](uint8_t *p, int64_t, hipStream_t st) {
                              return jfs_launch_lz4_split_prefix(d_blocks, nblk, d_ret, d_want, p, g.nseg, g.max_cap,
                                                                 g.norg, g.max_cap, st);
                          });
}

int64_t jfs_lz4_decompress_ranges_device(const jfs_dev_block *d_blocks, const int32_t *src_len, const int32_t *dst_cap,
                                         const int32_t *d_rng_first, const jfs_range *d_rng, int nblk, int32_t *d_ret,
                                         void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    // (d_rng: every list may be empty)
    if (nblk < 0 || (nblk > 0 && (!d_blocks || !src_len || !dst_cap || !d_rng_first || !d_ret))) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    // (the lists live on the device only: the capacities bound the chase's grid)
    return scratch_launch(g_split, DECOMPRESS, nblk, jfs_lz4_chase_scratch_bytes(nblk, src_len), stream,
                          [&](uint8_t *p, int64_t, hipStream_t st) {
                              return jfs_launch_lz4_chase(d_blocks, src_len, dst_cap, d_rng_first, d_rng, nblk, d_ret, p,
                                                          -1, st);
                          });
}

int jfs_read_lz4_chase_mode(void) { return read_lz4_chase().load(std::memory_order_relaxed); }

int jfs_set_read_lz4_chase_mode(int mode) {
    if (mode != JFS_READ_LZ4_CHASE_OFF && mode != JFS_READ_LZ4_CHASE_ON) return -1;
    return read_lz4_chase().exchange(mode);
}

int64_t jfs_lz4_chase_max(void) { return lz4_chase_max().load(std::memory_order_relaxed); }

int64_t jfs_set_lz4_chase_max(int64_t bytes) {
    if (bytes < 0 || bytes > INT32_MAX) return -1;
    return lz4_chase_max().exchange(bytes);
}

int64_t jfs_lz4_compress_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len, int nblk, int32_t *d_ret,
                                      void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && !src_len)) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    return scratch_launch(g_eseg_scr, COMPRESS, nblk, jfs_lz4_eseg_scratch_bytes(nblk, src_len), stream,
                          [&](uint8_t *p, int64_t cap, hipStream_t st) {
                              return jfs_launch_lz4_encode_seg(d_blocks, nblk, src_len, d_ret, p, cap, st);
                          });
}

int64_t jfs_lz4_compress_fast_device(const jfs_dev_block *d_blocks, const int32_t *src_len, int nblk, int32_t *d_ret,
                                     void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && !src_len)) return JFS_ERR_INVALID;
    if (nblk == 0) return JFS_OK;
    return scratch_launch(g_fast_scr, COMPRESS, nblk, jfs_lz4_fast_scratch_bytes(nblk, src_len), stream,
                          [&](uint8_t *p, int64_t cap, hipStream_t st) {
                              return jfs_launch_lz4_fast(d_blocks, nblk, src_len, d_ret, p, cap, st);
                          });
}

int jfs_lz4_parse_mode(void) { return lz4_parse().load(std::memory_order_relaxed); }

int jfs_set_lz4_parse_mode(int mode) {
    if (mode != JFS_LZ4_PARSE_EXACT && mode != JFS_LZ4_PARSE_FAST) return -1;
    return lz4_parse().exchange(mode);
}

int64_t jfs_lz4_compress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_LZ4, COMPRESS, nblk);
    return jfs_launch_lz4_encode(d_blocks, nblk, d_ret, (hipStream_t)stream) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_zstd_compress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_ZSTD, COMPRESS, nblk);
    return jfs_launch_zstd_encode(d_blocks, nblk, d_ret, (hipStream_t)stream, JFS_ZSTD_PARSE_EXACT) == 0 ? JFS_OK
                                                                                                         : JFS_ERR_HIP;
}

int64_t jfs_zstd_compress_fast_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_ZSTD, COMPRESS, nblk);
    return jfs_launch_zstd_encode(d_blocks, nblk, d_ret, (hipStream_t)stream, JFS_ZSTD_PARSE_FAST) == 0 ? JFS_OK
                                                                                                        : JFS_ERR_HIP;
}

int jfs_read_decode_mode(void) { return read_decode().load(std::memory_order_relaxed); }

int jfs_set_read_decode_mode(int mode) {
    if (mode != JFS_READ_DECODE_FULL && mode != JFS_READ_DECODE_PREFIX) return -1;
    return read_decode().exchange(mode);
}

int jfs_set_read_decode_mode_ext(int mode) {
    if (mode != JFS_READ_DECODE_FULL && mode != JFS_READ_DECODE_PREFIX && mode != JFS_READ_DECODE_PREFIX_ALL) return -1;
    return read_decode().exchange(mode);
}

int jfs_read_seek_mode(void) { return read_seek().load(std::memory_order_relaxed); }

int jfs_set_read_seek_mode(int mode) {
    if (mode != JFS_READ_SEEK_OFF && mode != JFS_READ_SEEK_ON) return -1;
    return read_seek().exchange(mode);
}

int jfs_set_read_seek_mode_ext(int mode) {
    if (mode != JFS_READ_SEEK_OFF && mode != JFS_READ_SEEK_ON && mode != JFS_READ_SEEK_SPARSE) return -1;
    return read_seek().exchange(mode);
}

int jfs_compact_splice_mode(void) { return compact_splice().load(std::memory_order_relaxed); }

int jfs_set_compact_splice_mode(int mode) {
    if (mode != JFS_COMPACT_SPLICE_OFF && mode != JFS_COMPACT_SPLICE_ON) return -1;
    return compact_splice().exchange(mode);
}

int jfs_set_compact_splice_mode_ext(int mode) {
    if (mode != JFS_COMPACT_SPLICE_OFF && mode != JFS_COMPACT_SPLICE_ON && mode != JFS_COMPACT_SPLICE_ALL) return -1;
    return compact_splice().exchange(mode);
}

int jfs_compact_splice_counts(uint64_t out[4], int reset) {
    if (!out) return -1;
    for (int k = 0; k < 4; k++)
        out[k] = reset ? g_splice_counts[k].exchange(0) : g_splice_counts[k].load(std::memory_order_relaxed);
    return 0;
}

int64_t jfs_zstd_splice_device(const jfs_splice_out *d_out, int nout, const jfs_splice_frame *d_frames, int nframes,
                               const int32_t *d_unit_len, const uint64_t *d_unit_hash, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nout < 0 || nframes < 0 || (nout > 0 && (!d_out || !d_ret)) || (nframes > 0 && !d_frames)) return JFS_ERR_INVALID;
    if (nout == 0) return JFS_OK;
    // the frames' places: the current device's shared scratch, ordered across streams by its event
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return JFS_ERR_HIP;
    SplitScratch &z = g_splice_scr[dev];
    std::lock_guard<std::mutex> lk(z.mu);
    if (!z.ev_done && hipEventCreateWithFlags(&z.ev_done, hipEventDisableTiming) != hipSuccess) return JFS_ERR_HIP;
    const int64_t need = ((int64_t)nframes + 1) * 4;
    if (need > z.cap) {
        if (hipEventSynchronize(z.ev_done) != hipSuccess) return JFS_ERR_HIP;  // earlier launches may still use it
        if (z.p) (void)hipFree(z.p);
        z.p = nullptr;
        z.cap = 0;
        int64_t want = 1ll << 20;
        while (want < need) want <<= 1;
        if (hipMalloc((void **)&z.p, (size_t)want) != hipSuccess) return JFS_ERR_NO_MEMORY;
        z.cap = want;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipStreamWaitEvent(st, z.ev_done, 0) != hipSuccess) return JFS_ERR_HIP;
    if (jfs_launch_zstd_splice(d_out, nout, d_frames, nframes, d_unit_len, d_unit_hash, (uint32_t *)z.p, d_ret, st) != 0)
        return JFS_ERR_HIP;
    return hipEventRecord(z.ev_done, st) == hipSuccess ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_zstd_seek_tables_device(const jfs_dev_block *d_blocks, const int32_t *d_len, int nblk,
                                    const int32_t *d_slot_first, uint8_t *d_tables, int32_t *d_table_len, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && (!d_blocks || !d_len || !d_slot_first || !d_tables || !d_table_len))) return JFS_ERR_INVALID;
    return jfs_launch_zstd_seek_tables(d_blocks, d_len, nblk, d_slot_first, d_tables, d_table_len, (hipStream_t)stream) == 0
               ? JFS_OK
               : JFS_ERR_HIP;
}

int jfs_get_zstd_split_frames(void) { return zstd_split_frames().load(std::memory_order_relaxed); }

int jfs_set_zstd_split_frames(int max_frames) {
    if (max_frames < 1 || max_frames > JFS_ZSTD_SPLIT_FRAMES_MAX) return -1;
    return zstd_split_frames().exchange(max_frames);
}

int jfs_zstd_parse_mode(void) { return zstd_parse_now(); }

int jfs_set_zstd_parse_mode_ext(int mode) {
    if (mode != JFS_ZSTD_PARSE_EXACT && mode != JFS_ZSTD_PARSE_FAST && mode != JFS_ZSTD_PARSE_SEEKABLE) return -1;
    return zstd_parse().exchange(mode);
}

int64_t jfs_zstd_compress_seekable_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_ZSTD, COMPRESS, nblk);
    return jfs_launch_zstd_encode(d_blocks, nblk, d_ret, (hipStream_t)stream, JFS_ZSTD_PARSE_SEEKABLE) == 0 ? JFS_OK
                                                                                                            : JFS_ERR_HIP;
}

int64_t jfs_zstd_decompress_range_device(const jfs_dev_block *d_blocks, const int32_t *d_lo, const int32_t *d_hi,
                                         int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk > 0 && (!d_lo || !d_hi)) return JFS_ERR_INVALID;
    stat_launch(JFS_ALGO_ZSTD, DECOMPRESS, nblk);
    return jfs_launch_zstd_decode_range(d_blocks, d_lo, d_hi, nblk, d_ret, (hipStream_t)stream) == 0 ? JFS_OK
                                                                                                     : JFS_ERR_HIP;
}

int64_t jfs_zstd_decompress_ranges_device(const jfs_dev_block *d_blocks, const int32_t *d_rng_first,
                                          const jfs_range *d_rng, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk > 0 && (!d_blocks || !d_rng_first || !d_ret)) return JFS_ERR_INVALID;  // (d_rng: every list may be empty)
    stat_launch(JFS_ALGO_ZSTD, DECOMPRESS, nblk);
    return jfs_launch_zstd_decode_ranges(d_blocks, d_rng_first, d_rng, nblk, d_ret, (hipStream_t)stream) == 0 ? JFS_OK
                                                                                                              : JFS_ERR_HIP;
}

int jfs_zstd_seek_csum_mode(void) { return zstd_seek_csum().load(std::memory_order_relaxed); }

int jfs_set_zstd_seek_csum_mode(int mode) {
    if (mode != JFS_ZSTD_SEEK_CSUM_OFF && mode != JFS_ZSTD_SEEK_CSUM_ON) return -1;
    return zstd_seek_csum().exchange(mode);
}

int64_t jfs_xxh64_device(const jfs_dev_block *d_blocks, int nblk, uint64_t *d_hash, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || (nblk > 0 && (!d_blocks || !d_hash))) return JFS_ERR_INVALID;
    return jfs_launch_xxh64(d_blocks, nblk, d_hash, d_ret, (hipStream_t)stream) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_zstd_compress_seekable_csum_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    // (the descriptors are copied back to the host from the pointer given)
    if (nblk < 0 || (nblk > 0 && (!d_blocks || !d_ret))) return JFS_ERR_INVALID;
    stat_launch(JFS_ALGO_ZSTD, COMPRESS, nblk);
    return jfs_launch_zstd_encode_seek_csum(d_blocks, nblk, d_ret, (hipStream_t)stream) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_zstd_decompress_frames_device(const jfs_seek_frag *d_frags, const int32_t *d_lo, const int32_t *d_hi,
                                          int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk > 0 && (!d_frags || !d_lo || !d_hi || !d_ret)) return JFS_ERR_INVALID;
    stat_launch(JFS_ALGO_ZSTD, DECOMPRESS, nblk);
    return jfs_launch_zstd_decode_frames(d_frags, d_lo, d_hi, nblk, d_ret, (hipStream_t)stream) == 0 ? JFS_OK
                                                                                                     : JFS_ERR_HIP;
}

int64_t jfs_zstd_seek_plan(const uint8_t *tail, int64_t tail_len, int64_t object_len, int64_t lo, int64_t hi,
                           jfs_seek_plan *out) {
    namespace zs = jfs::zseek;
    if (!out || tail_len < 0 || object_len < 0 || tail_len > object_len || object_len > 0x7FFFFFFFll ||
        (!tail && tail_len > 0))
        return JFS_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    out->status = JFS_SEEK_PLAN_NONE;
    if (tail_len < zs::FOOTER) return JFS_OK;
    // the footer: the frame count and the entry size place the table
    const uint8_t *f = tail + tail_len - zs::FOOTER;
    int32_t n = 0, entry = 0;
    if (!zs::footer_peek([f](int32_t p) { return (uint32_t)f[p]; }, zs::FOOTER, true, &n, &entry)) return JFS_OK;
    const int64_t table_len = (int64_t)entry * n + zs::TABLE_FIXED;
    if (table_len > object_len) return JFS_OK;
    if (tail_len < table_len) {
        out->status = JFS_SEEK_PLAN_MORE;
        out->checksums = entry == zs::ENTRY_CSUM;
        out->nf = n;
        out->table_off = object_len - table_len;
        out->table_len = table_len;
        return JFS_OK;
    }
    const uint8_t *t = tail + tail_len - table_len;
    const zs::TableSel s = zs::table_select([t](int32_t p) { return (uint32_t)t[p]; }, table_len, object_len, -1, lo, hi);
    if (!s.table) return JFS_OK;
    out->status = JFS_SEEK_PLAN_OK;
    out->checksums = s.checksums;
    out->nf = s.nf;
    out->first = s.first;
    out->count = s.count;
    out->table_off = object_len - table_len;
    out->table_len = table_len;
    out->get_off = (int64_t)s.coff;
    out->get_len = (int64_t)(s.cend - s.coff);
    out->content = (int64_t)s.total;
    out->first_off = (int64_t)s.doff;
    return JFS_OK;
}

int jfs_set_zstd_parse_mode(int mode) {
    if (mode != JFS_ZSTD_PARSE_EXACT && mode != JFS_ZSTD_PARSE_FAST) return -1;
    return zstd_parse().exchange(mode);
}

int64_t jfs_zstd_decompress_prefix_device(const jfs_dev_block *d_blocks, const int32_t *d_want, int nblk,
                                          int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk > 0 && !d_want) return JFS_ERR_INVALID;
    stat_launch(JFS_ALGO_ZSTD, DECOMPRESS, nblk);
    return jfs_launch_zstd_decode_prefix(d_blocks, nblk, d_ret, d_want, (hipStream_t)stream) == 0 ? JFS_OK
                                                                                                  : JFS_ERR_HIP;
}

int64_t jfs_zstd_decompress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    stat_launch(JFS_ALGO_ZSTD, DECOMPRESS, nblk);
    return jfs_launch_zstd_decode(d_blocks, nblk, d_ret, nullptr, (hipStream_t)stream) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_crc32c_device(const jfs_dev_block *d_blocks, int nblk, int32_t seg_bytes, uint32_t *d_crc,
                          int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || seg_bytes < 0 || (seg_bytes > 0 && seg_bytes % 4096 != 0)) return JFS_ERR_INVALID;
    return jfs_launch_crc32c(d_blocks, nblk, seg_bytes, d_crc, d_ret, (hipStream_t)stream) == 0 ? JFS_OK
                                                                                              : JFS_ERR_HIP;
}

int64_t jfs_aes256gcm_seal_device(const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0) return JFS_ERR_INVALID;
    return jfs_launch_aes256gcm(d_blocks, nblk, 0, d_ret, nullptr, (hipStream_t)stream) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_aes256gcm_open_device(const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0) return JFS_ERR_INVALID;
    return jfs_launch_aes256gcm(d_blocks, nblk, 1, d_ret, nullptr, (hipStream_t)stream) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int jfs_cipher_from_name(const char *name) {
    if (!name) return -1;
    std::string v(name);
    for (auto &ch : v) ch = (char)tolower((unsigned char)ch);
    if (v.empty() || v == "aes256gcm-rsa") return JFS_CIPHER_AES256GCM;  // encrypt.go:178
    if (v == "chacha20-rsa") return JFS_CIPHER_CHACHA20POLY1305;           // :190
    if (v == "sm4gcm") return JFS_CIPHER_SM4GCM;                            // :191
    return -1;
}

int jfs_cipher_key_size(int cipher) {
    switch (cipher) {
        case JFS_CIPHER_AES256GCM: return 32;
        case JFS_CIPHER_CHACHA20POLY1305: return 32;
        case JFS_CIPHER_SM4GCM: return 16;
        default: return -1;
    }
}

int64_t jfs_aead_seal_device(int cipher, const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || jfs_cipher_key_size(cipher) < 0) return JFS_ERR_INVALID;
    return jfs_launch_aead(cipher, d_blocks, nblk, 0, d_ret, nullptr, (hipStream_t)stream) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_aead_open_device(int cipher, const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0 || jfs_cipher_key_size(cipher) < 0) return JFS_ERR_INVALID;
    return jfs_launch_aead(cipher, d_blocks, nblk, 1, d_ret, nullptr, (hipStream_t)stream) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_lz4_compress_seal_device(const jfs_dev_block *d_comp, const jfs_aead_block *d_aead, int nblk,
                                     int32_t *d_ret_comp, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0) return JFS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (jfs_launch_lz4_encode(d_comp, nblk, d_ret_comp, st) != 0) return JFS_ERR_HIP;
    return jfs_launch_aes256gcm(d_aead, nblk, 0, d_ret, d_ret_comp, st) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_open_lz4_decompress_device(const jfs_aead_block *d_aead, const jfs_dev_block *d_dec, int nblk,
                                       int32_t *d_ret_open, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nblk < 0) return JFS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (jfs_launch_aes256gcm(d_aead, nblk, 1, d_ret_open, nullptr, st) != 0) return JFS_ERR_HIP;
    return jfs_launch_lz4_decode_lens(d_dec, nblk, d_ret, d_ret_open, st) == 0 ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_gather_device(const jfs_dev_block *d_src, const int32_t *d_src_n, int nsrc, const jfs_compact_out *d_out,
                          int nout, const jfs_compact_seg *d_seg, int32_t max_dst_cap, int32_t *d_ret, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nsrc < 0 || nout < 0 || (nout > 0 && (!d_out || !d_ret))) return JFS_ERR_INVALID;
    return jfs_launch_gather(d_src, d_src_n, nsrc, d_out, nout, d_seg, max_dst_cap, d_ret, 0, (hipStream_t)stream) == 0
               ? JFS_OK
               : JFS_ERR_HIP;
}

int64_t jfs_lz4_compact_device(const jfs_dev_block *d_src, int nsrc, int32_t *d_src_ret,
                               const jfs_compact_out *d_gather, const jfs_compact_seg *d_seg,
                               const jfs_dev_block *d_enc, int nout, int32_t max_dst_cap, int32_t *d_ret,
                               void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nsrc < 0 || nout < 0 || (nsrc > 0 && (!d_src || !d_src_ret)) || (nout > 0 && (!d_gather || !d_enc || !d_ret)))
        return JFS_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    stat_launch(JFS_ALGO_LZ4, DECOMPRESS, nsrc);
    stat_launch(JFS_ALGO_LZ4, COMPRESS, nout);
    if (nsrc > 0 && jfs_launch_lz4_decode(d_src, nsrc, d_src_ret, st) != 0) return JFS_ERR_HIP;
    if (jfs_launch_gather(d_src, d_src_ret, nsrc, d_gather, nout, d_seg, max_dst_cap, d_ret, 0, st) != 0)
        return JFS_ERR_HIP;
    if (nout > 0 && jfs_launch_lz4_encode(d_enc, nout, d_ret, st) != 0) return JFS_ERR_HIP;
    // the encoder ran on every block: a failed gather's verdict replaces its result
    return jfs_launch_gather(d_src, d_src_ret, nsrc, d_gather, nout, d_seg, max_dst_cap, d_ret, 1, st) == 0
               ? JFS_OK
               : JFS_ERR_HIP;
}

// jfs_compact_batch (cipher < 0) and jfs_compact_seal_batch
static int64_t compact_call(int algo, int cipher, int nsrc, const jfs_iov *src, const uint8_t *const *src_keys,
                            int nout, const jfs_iov *out, const jfs_seal_param *out_p, const int32_t *seg_first,
                            const jfs_compact_seg *seg, int64_t *src_n, int64_t *out_n, uint32_t *crc,
                            uint32_t device_mask) {
    const bool sealed = cipher >= 0;
    // the plan, the keys and the seal parameters are checked before any device is touched
    std::vector<int64_t> total;
    if (!compact_plan_ok(algo, nsrc, src, nout, out, seg_first, seg, src_n, out_n, total)) return JFS_ERR_INVALID;
    if (sealed) {
        if (jfs_cipher_key_size(cipher) < 0) return JFS_ERR_INVALID;
        if ((nsrc > 0 && !src_keys) || (nout > 0 && !out_p)) return JFS_ERR_INVALID;
        for (int i = 0; i < nsrc; i++)
            if (!src_keys[i]) return JFS_ERR_INVALID;
        for (int j = 0; j < nout; j++) {
            const jfs_seal_param &q = out_p[j];
            if (!q.key || !q.nonce || q.wrapped_len < 0 || q.wrapped_len > 65535 || (q.wrapped_len > 0 && !q.wrapped))
                return JFS_ERR_INVALID;
        }
    }
    const std::vector<DevCtx *> ds = devices_in(device_mask);
    if (ds.empty()) return JFS_ERR_NO_DEVICE;
    const int64_t t0 = steady_ns();
    std::vector<ChainSrc> ss;
    std::vector<int> src_map;
    chain_sources(algo, sealed, nsrc, src, nullptr, src_n, nullptr, ss, src_map);
    std::vector<ChainOut> oo;
    std::vector<int> own;  // sealed outputs with an error of their own: a failed source still wins (below)
    for (int j = 0; j < nout; j++) {
        if (crc) crc[j] = 0;
        if (jfs_plan::chain_dead(seg_first, seg, j, src_map)) {
            out_n[j] = JFS_ERR_CORRUPT;
            continue;
        }
        ChainOut o{j, total[j], 0, 0, 0};
        int64_t err = JFS_OK;
        if (sealed) {  // what jfs_compress_seal_batch answers for the gathered block
            const int64_t bound = jfs_envelope_bound(algo, total[j], out_p[j].wrapped_len);
            o.hdr = 3 + (int64_t)out_p[j].wrapped_len + 12;
            o.cap = bound - o.hdr - 16;  // the codec's bound of total; the payload area also holds the tag
            o.area = o.cap + 16;
            if (bound < 0) err = JFS_ERR_INVALID;
            else if (algo == JFS_ALGO_LZ4 && total[j] > LZ4_MAX_INPUT) err = JFS_ERR_COMPRESS_FAIL;
            else if (out[j].dst_cap < bound) err = JFS_ERR_SHORT_BUFFER;
        } else {  // pre_answer's rules for the gathered block as Compress sees it
            const jfs_iov g{nullptr, total[j], out[j].dst, out[j].dst_cap};
            if (algo == JFS_ALGO_NONE && g.dst_cap < g.src_len) err = JFS_ERR_SHORT_BUFFER;
            else if (algo == JFS_ALGO_LZ4 && g.src_len > LZ4_MAX_INPUT) err = JFS_ERR_COMPRESS_FAIL;
            else if (algo == JFS_ALGO_ZSTD && g.dst_cap < jfs_compress_bound(JFS_ALGO_ZSTD, g.src_len))
                err = JFS_ERR_SHORT_BUFFER;
            else o.area = o.cap = algo == JFS_ALGO_NONE ? total[j] : staged_cap(algo, COMPRESS, g);
        }
        if (err == JFS_OK) {
            oo.push_back(o);
        } else {
            out_n[j] = err;
            if (sealed) own.push_back(j);
        }
    }
    // JFS_COMPACT_SPLICE: the call takes the spliced path when the rule (splice_plan.h) passes at least one frame.
    // With a cipher (mode all) the rule runs inside the path, once the sources are opened and their tables back.
    jfs_plan::SplicePlan splice;
    const bool splice_csum = zstd_seek_csum().load(std::memory_order_relaxed) == JFS_ZSTD_SEEK_CSUM_ON;
    const int splice_mode = compact_splice().load(std::memory_order_relaxed);
    const bool splice_try = algo == JFS_ALGO_ZSTD && !oo.empty() && zstd_parse_now() == JFS_ZSTD_PARSE_SEEKABLE &&
                            (sealed ? splice_mode == JFS_COMPACT_SPLICE_ALL : splice_mode != JFS_COMPACT_SPLICE_OFF);
    std::vector<uint8_t> use(nout, 0);
    std::vector<int64_t> len(nsrc), cap(nsrc);
    for (const ChainOut &o : oo) use[o.idx] = 1;
    for (int i = 0; i < nsrc; i++) cap[i] = src_map[i] >= 0 ? ss[src_map[i]].cap : 0;
    auto plan_from = [&](auto fetch) {
        return jfs_plan::splice_plan(fetch, nsrc, len.data(), cap.data(), nout, seg_first, seg, total.data(), use.data(),
                                     splice_csum);
    };
    if (splice_try && !sealed) {
        for (int i = 0; i < nsrc; i++) len[i] = src[i].src_len;
        splice = plan_from([&](int i, int32_t p) { return src[i].src[p]; });
    }
    const SpliceReplan replan = [&](const jfs_plan::PackedTables &t) {
        for (int i = 0; i < nsrc; i++) len[i] = t.src_len(i);
        return plan_from(t);
    };
    const int64_t rc = chain_dispatch(ds, algo, COMPRESS, ss, oo, src_n, out_n, [&](DevCtx *dev, Lane &ln) {
        if (sealed ? splice_try : splice.outs > 0)
            return compact_splice_run(dev, ln, cipher, src, src_keys, ss, src_map, nsrc, out, out_p, oo, &splice, replan,
                                      own, seg_first, seg, splice_csum, src_n, out_n, crc);
        return compact_run(dev, ln, algo, cipher, src, src_keys, ss, src_map, out, out_p, oo, seg_first, seg, src_n, out_n,
                           crc);
    });
    if (rc == JFS_OK)
        for (int j : own)  // a source that failed on the device, or is too short, wins over the block's own error
            for (int k = seg_first[j]; k < seg_first[j + 1]; k++)
                if (seg[k].src >= 0 && (int64_t)seg[k].src_off + seg[k].len > src_n[seg[k].src]) out_n[j] = JFS_ERR_CORRUPT;
    const int64_t nanos = steady_ns() - t0;
    chain_stat(algo, DECOMPRESS, nsrc, [&](int i) { return src[i].src_len; }, src_n, !ss.empty(), -1);
    chain_stat(algo, COMPRESS, nout, [&](int j) { return total[j]; }, out_n, !oo.empty(), nanos);
    return JFS_OK;
}

int64_t jfs_compact_batch(int algo, int nsrc, const jfs_iov *src, int nout, const jfs_iov *out,
                          const int32_t *seg_first, const jfs_compact_seg *seg, int64_t *src_n, int64_t *out_n,
                          uint32_t *crc, uint32_t device_mask) {
    return compact_call(algo, -1, nsrc, src, nullptr, nout, out, nullptr, seg_first, seg, src_n, out_n, crc,
                        device_mask);
}

int64_t jfs_compact_seal_batch(int algo, int cipher, int nsrc, const jfs_iov *src, const uint8_t *const *src_keys,
                               int nout, const jfs_iov *out, const jfs_seal_param *out_p, const int32_t *seg_first,
                               const jfs_compact_seg *seg, int64_t *src_n, int64_t *out_n, uint32_t *crc,
                               uint32_t device_mask) {
    if (cipher < 0) return JFS_ERR_INVALID;
    return compact_call(algo, cipher, nsrc, src, src_keys, nout, out, out_p, seg_first, seg, src_n, out_n, crc,
                        device_mask);
}

int64_t jfs_read_gather_device(const jfs_dev_block *d_src, const int32_t *d_src_n, int nsrc, const jfs_compact_out *d_out,
                               const int32_t *dst_cap, int nout, const jfs_compact_seg *d_seg, int32_t *d_ret,
                               void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nsrc < 0 || nout < 0 || (nout > 0 && (!d_out || !d_ret || !dst_cap))) return JFS_ERR_INVALID;
    if (nout == 0) return JFS_OK;
    int64_t ntiles = 0;
    for (int j = 0; j < nout; j++) ntiles += jfs_gather_tiles(dst_cap[j]);
    if (ntiles > INT32_MAX) return JFS_ERR_INVALID;
    // the tile prefix is built on the device from d_out, in the current device's shared scratch
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return JFS_ERR_HIP;
    SplitScratch &z = g_read_scr[dev];
    std::lock_guard<std::mutex> lk(z.mu);
    if (!z.ev_done && hipEventCreateWithFlags(&z.ev_done, hipEventDisableTiming) != hipSuccess) return JFS_ERR_HIP;
    const int64_t need = ((int64_t)nout + 1) * 4;
    if (need > z.cap) {
        if (hipEventSynchronize(z.ev_done) != hipSuccess) return JFS_ERR_HIP;  // earlier launches may still use it
        if (z.p) (void)hipFree(z.p);
        z.p = nullptr;
        z.cap = 0;
        int64_t want = 1ll << 20;
        while (want < need) want <<= 1;
        if (hipMalloc((void **)&z.p, (size_t)want) != hipSuccess) return JFS_ERR_NO_MEMORY;
        z.cap = want;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipStreamWaitEvent(st, z.ev_done, 0) != hipSuccess) return JFS_ERR_HIP;
    int32_t *d_tf = (int32_t *)z.p;
    if (jfs_launch_gather_prefix(d_out, nout, d_tf, st) != 0 ||
        jfs_launch_gather_flat(d_src, d_src_n, nsrc, d_out, nout, d_seg, d_ret, d_tf, ntiles, st) != 0)
        return JFS_ERR_HIP;
    return hipEventRecord(z.ev_done, st) == hipSuccess ? JFS_OK : JFS_ERR_HIP;
}

int64_t jfs_read_csum_device(const jfs_compact_out *d_out, const int32_t *d_ret, int nout, const int32_t *d_piece_first,
                             int64_t npiece, uint8_t *d_csum, void *stream) {
    if (!current_device_ok()) return JFS_ERR_NO_DEVICE;
    if (nout < 0 || npiece < 0 || npiece > INT32_MAX || (nout > 0 && (!d_out || !d_ret || !d_piece_first)) ||
        (npiece > 0 && (!d_csum || ((uintptr_t)d_csum & 3u) != 0)))
        return JFS_ERR_INVALID;
    if (nout == 0 || npiece == 0) return JFS_OK;
    return launch_rc(
        jfs_launch_read_csum_flat(d_out, nout, d_ret, d_piece_first, npiece, (uint32_t *)d_csum, (hipStream_t)stream));
}

// jfs_read_batch (cipher < 0) and jfs_read_open_batch; csum: the _csum calls'
// array (nout entries), else null
static int64_t read_call(int algo, int cipher, int nsrc, const jfs_iov *src, const uint8_t *const *src_keys,
                         const int64_t *src_crc, int nout, const jfs_iov *out, const int32_t *seg_first,
                         const jfs_compact_seg *seg, int64_t *src_n, int64_t *out_n, uint32_t *crc_got,
                         uint32_t device_mask, uint8_t *const *csum = nullptr) {
    const bool sealed = cipher >= 0;
    // the plan, the keys and the checksums are checked before any device is touched
    std::vector<int64_t> total;
    if (!compact_plan_ok(algo, nsrc, src, nout, out, seg_first, seg, src_n, out_n, total)) return JFS_ERR_INVALID;
    for (int j = 0; j < nout; j++)
        if (total[j] > out[j].dst_cap) return JFS_ERR_INVALID;
    for (int i = 0; src_crc && i < nsrc; i++)
        if (src_crc[i] < -1 || src_crc[i] > 0xFFFFFFFFll) return JFS_ERR_INVALID;
    if (sealed) {
        if (jfs_cipher_key_size(cipher) < 0 || (nsrc > 0 && !src_keys)) return JFS_ERR_INVALID;
        for (int i = 0; i < nsrc; i++)
            if (!src_keys[i]) return JFS_ERR_INVALID;
    }
    const std::vector<DevCtx *> ds = devices_in(device_mask);
    if (ds.empty()) return JFS_ERR_NO_DEVICE;
    const int64_t t0 = steady_ns();
    std::vector<ChainSrc> st;
    std::vector<int> src_map;
    const int ns = chain_sources(algo, sealed, nsrc, src, src_crc, src_n, crc_got, st, src_map);
    std::vector<ChainOut> oo;
    for (int j = 0; j < nout; j++) {
        if (jfs_plan::chain_dead(seg_first, seg, j, src_map)) out_n[j] = JFS_ERR_CORRUPT;
        else if (total[j] == 0) out_n[j] = 0;
        else oo.push_back({j, total[j], total[j], 0, 0});
        // an empty read's checksum is checksum() of no bytes: one zero word, no device needed
        if (csum && csum[j] && out_n[j] == 0 && total[j] == 0) memset(csum[j], 0, 4);
    }
    // prefix modes (LZ4 in both, Zstd in prefix-all): the last byte the plan asks of every object
    std::vector<int64_t> need, from;
    const int dmode = read_decode().load(std::memory_order_relaxed);
    // JFS_READ_SEEK: every Zstd source is decoded for [from, need), whatever the decode mode
    const int smode = algo == JFS_ALGO_ZSTD ? read_seek().load(std::memory_order_relaxed) : JFS_READ_SEEK_OFF;
    const bool seek = smode == JFS_READ_SEEK_ON, sparse = smode == JFS_READ_SEEK_SPARSE;
    // (JFS_READ_SEEK sparse: the lists of ranges stand for both, read_run makes them)
    if ((algo == JFS_ALGO_LZ4 && dmode != JFS_READ_DECODE_FULL) ||
        (algo == JFS_ALGO_ZSTD && dmode == JFS_READ_DECODE_PREFIX_ALL && !sparse) || seek)
        need = jfs_plan::chain_need(nsrc, nout, seg_first, seg);
    if (seek) from = jfs_plan::chain_from(nsrc, nout, seg_first, seg);
    // JFS_READ_LZ4_CHASE: the LZ4 sources whose reads ask for little enough go first and take the chase
    int nchase = 0;
    if (algo == JFS_ALGO_LZ4 && ns > 0 && read_lz4_chase().load(std::memory_order_relaxed) == JFS_READ_LZ4_CHASE_ON)
        nchase = jfs_plan::chain_chase_front(nsrc, nout, seg_first, seg, st, ns, src_map,
                                             lz4_chase_max().load(std::memory_order_relaxed));
    chain_dispatch(ds, algo, DECOMPRESS, st, oo, src_n, out_n, [&](DevCtx *dev, Lane &ln) {
        return read_run(dev, ln, algo, cipher, src, src_keys, st, ns, src_map, out, oo, seg_first, seg, src_n, out_n,
                        crc_got, need.empty() ? nullptr : need.data(), from.empty() ? nullptr : from.data(), csum, nsrc, nout,
                        sparse, nchase);
    });
    chain_stat(algo, DECOMPRESS, nsrc, [&](int i) { return src[i].src_len; }, src_n, ns > 0, steady_ns() - t0);
    return JFS_OK;
}

int64_t jfs_read_batch(int algo, int nsrc, const jfs_iov *src, const int64_t *src_crc, int nout, const jfs_iov *out,
                       const int32_t *seg_first, const jfs_compact_seg *seg, int64_t *src_n, int64_t *out_n,
                       uint32_t *crc_got, uint32_t device_mask) {
    return read_call(algo, -1, nsrc, src, nullptr, src_crc, nout, out, seg_first, seg, src_n, out_n, crc_got,
                     device_mask);
}

int64_t jfs_read_open_batch(int algo, int cipher, int nsrc, const jfs_iov *src, const uint8_t *const *src_keys,
                            const int64_t *src_crc, int nout, const jfs_iov *out, const int32_t *seg_first,
                            const jfs_compact_seg *seg, int64_t *src_n, int64_t *out_n, uint32_t *crc_got,
                            uint32_t device_mask) {
    if (cipher < 0) return JFS_ERR_INVALID;
    return read_call(algo, cipher, nsrc, src, src_keys, src_crc, nout, out, seg_first, seg, src_n, out_n, crc_got,
                     device_mask);
}

int64_t jfs_read_batch_csum(int algo, int nsrc, const jfs_iov *src, const int64_t *src_crc, int nout, const jfs_iov *out,
                            const int32_t *seg_first, const jfs_compact_seg *seg, int64_t *src_n, int64_t *out_n,
                            uint32_t *crc_got, uint8_t *const *csum, uint32_t device_mask) {
    if (nout > 0 && !csum) return JFS_ERR_INVALID;
    return read_call(algo, -1, nsrc, src, nullptr, src_crc, nout, out, seg_first, seg, src_n, out_n, crc_got,
                     device_mask, csum);
}

int64_t jfs_read_open_batch_csum(int algo, int cipher, int nsrc, const jfs_iov *src, const uint8_t *const *src_keys,
                                 const int64_t *src_crc, int nout, const jfs_iov *out, const int32_t *seg_first,
                                 const jfs_compact_seg *seg, int64_t *src_n, int64_t *out_n, uint32_t *crc_got,
                                 uint8_t *const *csum, uint32_t device_mask) {
    if (cipher < 0 || (nout > 0 && !csum)) return JFS_ERR_INVALID;
    return read_call(algo, cipher, nsrc, src, src_keys, src_crc, nout, out, seg_first, seg, src_n, out_n, crc_got,
                     device_mask, csum);
}

// Ranged reads from host buffers: the host answers what the table
// alone decides; the rest run on one lane, on the read calls' staging -- slot
// 0's pinned and device buffers for what crosses the link (descriptors, tables,
// fragments up in one copy; results and the requested bytes down in one), its
// scratch for the decoded blocks.
int64_t jfs_zstd_load_range_batch(int n, const jfs_range_read *r, int64_t *out_n, uint32_t device_mask) {
    namespace zs = jfs::zseek;
    if (n < 0 || (n > 0 && (!r || !out_n))) return JFS_ERR_INVALID;
    for (int i = 0; i < n; i++) {
        const jfs_range_read &v = r[i];
        if (!v.table || v.table_len < 0 || v.object_len < 0 || v.frag_off < 0 || v.frag_len < 0 || v.block_size < 0 ||
            v.dst_cap < 0 || v.table_len > INT32_MAX || v.object_len > INT32_MAX || v.frag_off > INT32_MAX ||
            v.frag_len > INT32_MAX || v.block_size > INT32_MAX || (!v.frag && v.frag_len > 0) || (!v.dst && v.dst_cap > 0))
            return JFS_ERR_INVALID;
    }
    const std::vector<DevCtx *> ds = devices_in(device_mask);
    if (ds.empty()) return JFS_ERR_NO_DEVICE;
    const int64_t t0 = steady_ns();
    struct Job {
        int idx;
        int32_t lo, hi, len, expect;
        int64_t tab, frag, out, blk;  // offsets: staged table and fragment, packed output, decoded block
    };
    const auto up16 = [](int64_t x) { return (x + 15) & ~15ll; };
    std::vector<Job> jobs;
    std::vector<ChainOut> oo;
    std::vector<std::pair<std::pair<const uint8_t *, int64_t>, int64_t>> tabs;  // a table several reads share goes up once
    int64_t data = 0, outs = 0, blks = 0;
    int32_t max_len = 0;
    for (int i = 0; i < n; i++) {
        const jfs_range_read &v = r[i];
        const uint8_t *t = v.table;
        const zs::TableSel s =
            zs::table_select([t](int32_t p) { return (uint32_t)t[p]; }, v.table_len, v.object_len, v.block_size, v.lo, v.hi);
        const int64_t lo = std::max<int64_t>(v.lo, 0), hi = std::min(v.hi, v.block_size);
        const int64_t top = std::min<int64_t>((int64_t)s.total, hi), len = top > lo ? top - lo : 0;
        if (!s.table) out_n[i] = JFS_ERR_CORRUPT;
        else if (v.block_size == 0 || hi <= lo) out_n[i] = 0;
        else if ((int64_t)s.total > v.block_size || v.dst_cap < len) out_n[i] = JFS_ERR_SHORT_BUFFER;
        else if (len == 0) out_n[i] = 0;  // the range lies behind the content
        else {
            Job j{i, (int32_t)lo, (int32_t)hi, (int32_t)len, (int32_t)top, -1, 0, outs, blks};
            for (const auto &e : tabs)
                if (e.first.first == v.table && e.first.second == v.table_len) j.tab = e.second;
            if (j.tab < 0) {
                j.tab = data;
                tabs.push_back({{v.table, v.table_len}, data});
                data += up16(v.table_len);
            }
            j.frag = data;
            data += up16(v.frag_len);
            outs += up16(len);
            blks += (v.block_size + 255) & ~255ll;
            max_len = std::max(max_len, (int32_t)len);
            jobs.push_back(j);
            oo.push_back({i, len, len, 0, 0});
        }
    }
    const int m = (int)jobs.size();
    const int64_t o_lo = up16((int64_t)sizeof(jfs_seek_frag) * m), o_hi = o_lo + up16(4ll * m), o_pack = o_hi + up16(4ll * m),
                  o_data = o_pack + up16((int64_t)sizeof(jfs_range_pack) * m), o_ret = o_data + data,
                  o_out = o_ret + up16(4ll * m), end = o_out + outs;
    chain_dispatch(ds, JFS_ALGO_ZSTD, DECOMPRESS, std::vector<ChainSrc>(), oo, out_n, out_n, [&](DevCtx *dev, Lane &ln) {
        LaneRun scope(dev, ln, JFS_ALGO_ZSTD * 2 + DECOMPRESS, (uint64_t)m);
        Slot &sl = ln.slot[0];
        if (!sl.ensure(end) || !sl.ensure_split(std::max<int64_t>(blks, 16))) return (int64_t)JFS_ERR_NO_MEMORY;
        jfs_seek_frag *h_frag = (jfs_seek_frag *)sl.h;
        int32_t *h_lo = (int32_t *)(sl.h + o_lo), *h_hi = (int32_t *)(sl.h + o_hi);
        jfs_range_pack *h_pack = (jfs_range_pack *)(sl.h + o_pack);
        std::vector<CopyJob> cp;
        for (const auto &e : tabs) cp.push_back({sl.h + o_data + e.second, e.first.first, e.first.second});
        for (int k = 0; k < m; k++) {
            const Job &j = jobs[k];
            const jfs_range_read &v = r[j.idx];
            if (v.frag_len > 0) cp.push_back({sl.h + o_data + j.frag, v.frag, v.frag_len});
            // (an empty fragment still needs a pointer: its place in the staging)
            h_frag[k] = jfs_seek_frag{sl.d + o_data + j.tab,  (int32_t)v.table_len, (int32_t)v.object_len,
                                      sl.d + o_data + j.frag, (int32_t)v.frag_off,  (int32_t)v.frag_len,
                                      sl.sp + j.blk,          (int32_t)v.block_size, 0};
            h_lo[k] = j.lo;
            h_hi[k] = j.hi;
            h_pack[k] = jfs_range_pack{sl.sp + j.blk + j.lo, sl.d + o_out + j.out, j.len, j.expect};
        }
        par_copy(cp);
        hipStream_t ks = ln.s_k;
        int32_t *d_ret = (int32_t *)(sl.d + o_ret);
        int lk = hipMemcpyAsync(sl.d, sl.h, (size_t)o_ret, hipMemcpyHostToDevice, ks) == hipSuccess ? 0 : -1;
        if (lk == 0)
            lk = jfs_launch_zstd_decode_frames((const jfs_seek_frag *)sl.d, (const int32_t *)(sl.d + o_lo),
                                               (const int32_t *)(sl.d + o_hi), m, d_ret, ks);
        if (lk == 0) lk = jfs_launch_range_pack((const jfs_range_pack *)(sl.d + o_pack), m, max_len, d_ret, ks);
        if (lk == 0 && hipMemcpyAsync(sl.h + o_ret, sl.d + o_ret, (size_t)(end - o_ret), hipMemcpyDeviceToHost, ks) != hipSuccess)
            lk = -1;
        if (hipStreamSynchronize(ks) != hipSuccess || lk != 0) return (int64_t)JFS_ERR_HIP;
        const int32_t *h_ret = (const int32_t *)(sl.h + o_ret);
        cp.clear();
        for (int k = 0; k < m; k++) {
            const Job &j = jobs[k];
            const int32_t raw = h_ret[k];
            if (raw == j.expect) {
                out_n[j.idx] = j.len;
                cp.push_back({r[j.idx].dst, sl.h + o_out + j.out, (int64_t)j.len});
            } else {
                out_n[j.idx] = raw == -4 ? JFS_ERR_CHECKSUM : raw == -2 ? JFS_ERR_SHORT_BUFFER : JFS_ERR_CORRUPT;
            }
        }
        par_copy(cp);
        return (int64_t)JFS_OK;
    });
    chain_stat(JFS_ALGO_ZSTD, DECOMPRESS, n, [&](int i) { return r[i].table_len + r[i].frag_len; }, out_n, m > 0,
               steady_ns() - t0);
    return JFS_OK;
}

int jfs_device_count(void) { return (int)devices().size(); }

int jfs_gpu_mode(void) { return gpu_mode(); }

int jfs_stats(jfs_op_stats *out, int n) {
    for (int i = 0; out && i < n && i < JFS_STATS_N; i++) {
        const OpStats &g = g_stats[i];
        out[i].calls = g.calls.load(std::memory_order_relaxed);
        out[i].blocks = g.blocks.load(std::memory_order_relaxed);
        out[i].bytes_in = g.bytes_in.load(std::memory_order_relaxed);
        out[i].bytes_out = g.bytes_out.load(std::memory_order_relaxed);
        out[i].errors = g.errors.load(std::memory_order_relaxed);
        out[i].nanos = g.nanos.load(std::memory_order_relaxed);
        out[i].batches = g.batches.load(std::memory_order_relaxed);
    }
    return JFS_STATS_N;
}

void jfs_stats_reset(void) {
    for (OpStats &g : g_stats) {
        g.calls = 0;
        g.blocks = 0;
        g.bytes_in = 0;
        g.bytes_out = 0;
        g.errors = 0;
        g.nanos = 0;
        g.batches = 0;
    }
    for (DevCtx *d : devices()) {
        d->batches = 0;
        d->blocks = 0;
    }
}

int jfs_device_stats(jfs_device_stat *out, int n) {
    std::vector<DevCtx *> &ds = devices();
    for (int i = 0; out && i < n && i < (int)ds.size(); i++) {
        out[i].device = ds[i]->id;
        out[i].batches = ds[i]->batches.load(std::memory_order_relaxed);
        out[i].blocks = ds[i]->blocks.load(std::memory_order_relaxed);
    }
    return (int)ds.size();
}

void jfs_release_staging(void) {
    for (DevCtx *d : devices()) {
        DevGuard guard;
        for (Lane &ln : d->lane) {
            std::lock_guard<std::mutex> lk(ln.mu);
            release_lane_staging(d, ln);
        }
    }
}

const char *jfs_version(void) { return JFS_VERSION; }

int64_t jfs_gen_blocks_device(uint8_t *d_dst, int nblk, int64_t block_bytes, char cls, uint64_t seed_base,
                          void *stream) {
    std::vector<DevCtx *> &ds = devices();
    if (ds.empty()) return JFS_ERR_NO_DEVICE;
    int cur = 0;
    (void)hipGetDevice(&cur);
    DevCtx *dev = nullptr;
    for (DevCtx *d : ds)
        if (d->id == cur) dev = d;
    if (!dev) return JFS_ERR_NO_DEVICE;
    {
        std::lock_guard<std::mutex> lk(dev->vocab_mu);
        if (!dev->d_vocab) {
            std::vector<uint8_t> v(JFS_VOCAB_WORDS * 16);
            jfs_build_vocab(v.data());
            if (hipMalloc((void **)&dev->d_vocab, v.size()) != hipSuccess) return JFS_ERR_HIP;
            if (hipMemcpy(dev->d_vocab, v.data(), v.size(), hipMemcpyHostToDevice) != hipSuccess) return JFS_ERR_HIP;
        }
    }
    return jfs_launch_gen(d_dst, nblk, block_bytes, cls, seed_base, dev->d_vocab, (hipStream_t)stream) == 0
               ? JFS_OK
               : JFS_ERR_HIP;
}

void jfs_gen_block_host(uint8_t *dst, int64_t n, char cls, uint64_t seed) {
    static std::once_flag once;
    static std::vector<uint8_t> vocab(JFS_VOCAB_WORDS * 16);
    std::call_once(once, [] { jfs_build_vocab(vocab.data()); });
    struct E {
        uint8_t *p;
        void operator()(uint8_t b) { *p++ = b; }
    } e{dst};
    jfs_gen_stream(vocab.data(), cls, seed, n, e);
}

}  // extern "C"
