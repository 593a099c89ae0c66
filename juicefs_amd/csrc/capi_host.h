// What the three host files of the C ABI share: capi.hip (the host batch
// path, which also defines what is only declared here), capi_chain.hip (the
// on-device chains) and capi_device.hip (the device-resident entry points).
// Host code only; the namespace is hidden, so nothing of it reaches the
// library's dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <vector>

#include "../../include/jfs_gpucodec_test.h"
#include "chain_plan.h"
#include "host_modes.h"
#include "jfs_internal.h"

namespace jfs_host __attribute__((visibility("hidden"))) {

constexpr int64_t LZ4_MAX_INPUT = 0x7E000000;

using jfs_plan::align16;
using jfs_plan::envelope_parse;

// JFS_HOST_TRACE=1: per-chunk host timings on stderr (diagnostics)
inline bool host_trace() {
    static bool v = getenv("JFS_HOST_TRACE") != nullptr;
    return v;
}
inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// (trace) a staging or scratch allocation: hipFree waits for the whole device
inline void trace_alloc(const char *what, int64_t bytes, double t0) {
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
inline int64_t staging_max_bytes() {
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

// The switches themselves are host_modes.h's (Lz4Parse::get() and so on).
inline bool lz4_fast_mode() { return Lz4Parse::get() == JFS_LZ4_PARSE_FAST; }
inline int zstd_parse_now() { return ZstdParse::get(); }
// What a host-buffer compress call encodes with: the parse mode, or this value
// (no parse mode of the public switch) for seekable objects with checksums.
constexpr int ZSTD_ENCODE_SEEK_CSUM = 3;
inline int zstd_encode_now() {
    const int p = zstd_parse_now();
    return p == JFS_ZSTD_PARSE_SEEKABLE && ZstdSeekCsum::get() == JFS_ZSTD_SEEK_CSUM_ON ? ZSTD_ENCODE_SEEK_CSUM : p;
}

// per-(algo, dir) counters behind jfs_stats()
struct OpStats {
    std::atomic<uint64_t> calls{0}, blocks{0}, bytes_in{0}, bytes_out{0}, errors{0}, nanos{0}, batches{0};
};
extern OpStats g_stats[JFS_STATS_N];

inline OpStats *op_stats(int algo, int dir) {
    return (algo >= 0 && algo <= 2 && (dir == 0 || dir == 1)) ? &g_stats[algo * 2 + dir] : nullptr;
}

int64_t steady_ns();
int64_t steady_ms();

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

// the usable gfx950 devices, found once; those of device_mask (0: all)
std::vector<DevCtx *> &devices();
std::vector<DevCtx *> devices_in(uint32_t device_mask);
void start_janitor();
// false after a sticky HIP error: the lane's streams no longer synchronise
bool lane_healthy(DevCtx *dev, Lane &ln);

enum Dir { COMPRESS = 0, DECOMPRESS = 1 };
constexpr int COMPRESS_DIR = COMPRESS, DECOMPRESS_DIR = DECOMPRESS;

// a kernel's raw per-block value as the C ABI's; what the kernel may write of a block
int64_t finish_result(int algo, int dir, int32_t raw);
int64_t staged_cap(int algo, int dir, const jfs_iov &v);

// memcpy jobs spread over host threads (pageable <-> pinned is CPU-bound)
struct CopyJob {
    uint8_t *dst;
    const uint8_t *src;
    int64_t n;
};
void par_copy(std::vector<CopyJob> &jobs);

// CRC-32C on the host; an envelope header's checksum and bytes
uint32_t host_crc32c(uint32_t crc, const uint8_t *p, int64_t n);
uint32_t seal_header_crc(const jfs_seal_param &p);
void seal_header_write(uint8_t *dst, const jfs_seal_param &p);

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

// The launchers of staged blocks (capi.hip): the codec kernel of (algo, dir),
// and the LZ4 ones that choose between the small-batch and the per-block
// kernels and take their scratch from a slot.
int launch_kernel(int algo, int dir, const jfs_dev_block *d_desc, int nblk, int32_t *d_ret, hipStream_t st, int zparse);
std::vector<int32_t> desc_lens(const jfs_dev_block *h_desc, int n);
std::vector<int32_t> desc_caps(const jfs_dev_block *h_desc, int n);
int64_t lz4_encode_scratch(int n, const int32_t *lens, bool fast);
int64_t launch_lz4_encode(Slot &sl, const jfs_dev_block *h_desc, const jfs_dev_block *d_desc, int n, int32_t *d_ret,
                          hipStream_t st, bool fast);
int64_t lz4_decode_scratch(int n, const int32_t *lens, const int32_t *caps);
int64_t launch_lz4_decode(Slot &sl, const jfs_dev_block *h_desc, const jfs_dev_block *d_desc, int n, int32_t *d_ret,
                          hipStream_t st);
int64_t launch_lz4_decode_prefix(Slot &sl, const jfs_dev_block *h_desc, const jfs_dev_block *d_desc, int n,
                                 int32_t *d_ret, const int32_t *d_want, int64_t max_want, hipStream_t st);
// the window decode of a batch the small-batch path takes, and whether it takes n blocks (JFS_LZ4_SPLIT_MAX)
int64_t launch_lz4_decode_window(Slot &sl, const jfs_dev_block *h_desc, const jfs_dev_block *d_desc, int n,
                                 int32_t *d_ret, const int32_t *d_lo, const int32_t *d_hi, int64_t max_want,
                                 hipStream_t st);
bool lz4_decode_is_small(int n);

// Small-batch device launches: per-device scratch shared by every caller,
// ordered across streams by an event (like the Zstd device decoder's).
struct SplitScratch {
    std::mutex mu;
    uint8_t *p = nullptr;
    int64_t cap = 0;
    hipEvent_t ev_done = nullptr;

    // `need` bytes for launches on `stream` (the caller holds mu): grows the
    // block to a power of two, at least `floor`, once earlier launches are done
    // with it, and orders the stream behind them.  JFS_OK, JFS_ERR_NO_MEMORY or
    // JFS_ERR_HIP; after JFS_OK the caller launches, then release(stream).
    int64_t acquire(int64_t need, int64_t floor, hipStream_t stream) {
        if (!ev_done && hipEventCreateWithFlags(&ev_done, hipEventDisableTiming) != hipSuccess) return JFS_ERR_HIP;
        if (need > cap) {
            if (hipEventSynchronize(ev_done) != hipSuccess) return JFS_ERR_HIP;  // earlier launches may still use it
            if (p) (void)hipFree(p);
            p = nullptr;
            cap = 0;
            int64_t want = floor;
            while (want < need) want <<= 1;
            if (hipMalloc((void **)&p, (size_t)want) != hipSuccess) return JFS_ERR_NO_MEMORY;
            cap = want;
        }
        return hipStreamWaitEvent(stream, ev_done, 0) == hipSuccess ? JFS_OK : JFS_ERR_HIP;
    }
    int64_t release(hipStream_t stream) { return hipEventRecord(ev_done, stream) == hipSuccess ? JFS_OK : JFS_ERR_HIP; }
};

}  // namespace jfs_host
