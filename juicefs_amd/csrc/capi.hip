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
//
// This file: device discovery, staging and its janitor, the host batch path
// and its entry points, the switches' getters and setters, the statistics.
// The on-device chains are capi_chain.hip's, the device-resident entry points
// capi_device.hip's; capi_host.h holds what the three share.
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
#include "capi_host.h"
#include "chain_plan.h"
#include "jfs_internal.h"

#define JFS_VERSION "jfs-gpucodec 0.1.0 (gfx950)"

using namespace jfs_host;

// this file's own
namespace {

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

}  // namespace

// what capi_host.h declares and this file defines
namespace jfs_host __attribute__((visibility("hidden"))) {

OpStats g_stats[JFS_STATS_N];

int64_t steady_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

std::vector<DevCtx *> &devices() {
    std::call_once(g_once, init_devices);
    return g_devs;
}

int64_t steady_ms() {
    return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
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

bool lz4_decode_is_small(int n) { return n <= split_max(); }
// The window decode of n <= split_max() staged blocks: block k for [d_lo[k], d_hi[k]) (max_want: the largest
// hi, known on the host).  The scratch is lz4_decode_scratch's.
int64_t launch_lz4_decode_window(Slot &sl, const jfs_dev_block *h_desc, const jfs_dev_block *d_desc, int n,
                                 int32_t *d_ret, const int32_t *d_lo, const int32_t *d_hi, int64_t max_want,
                                 hipStream_t st) {
    if (n > split_max()) return JFS_ERR_INVALID;
    const std::vector<int32_t> lens = desc_lens(h_desc, n), caps = desc_caps(h_desc, n);
    if (!sl.ensure_split(lz4_decode_scratch(n, lens.data(), caps.data()))) return JFS_ERR_NO_MEMORY;
    const jfs_plan::Lz4SplitGeom g = jfs_plan::lz4_split_geom(n, lens.data(), caps.data());
    return launch_rc(
        jfs_launch_lz4_split_window(d_desc, n, d_ret, d_lo, d_hi, sl.sp, g.nseg, g.max_cap, g.norg, max_want, st));
}

bool lane_healthy(DevCtx *dev, Lane &ln) {
    DevGuard guard;
    (void)hipSetDevice(dev->id);
    return hipStreamSynchronize(dev->s_in) == hipSuccess && hipStreamSynchronize(ln.s_k) == hipSuccess &&
           hipStreamSynchronize(dev->s_out) == hipSuccess;
}

// the devices a call may use: those of device_mask (0: all)
std::vector<DevCtx *> devices_in(uint32_t device_mask) {
    std::vector<DevCtx *> ds;
    for (DevCtx *d : devices())
        if (device_mask == 0 || (d->id < 32 && (device_mask >> d->id) & 1u)) ds.push_back(d);
    return ds;
}

}  // namespace jfs_host

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

int jfs_device_count(void) { return (int)devices().size(); }

int jfs_gpu_mode(void) { return gpu_mode(); }

// The run-time switches (host_modes.h has the table): a setter answers the
// previous value, or -1 for a value it does not take; the plain setters keep
// to the values they were introduced with, the _ext ones take every value.
int jfs_lz4_parse_mode(void) { return Lz4Parse::get(); }
int jfs_set_lz4_parse_mode(int mode) { return Lz4Parse::set(mode); }
int jfs_zstd_parse_mode(void) { return ZstdParse::get(); }
int jfs_set_zstd_parse_mode(int mode) { return ZstdParse::set(mode); }
int jfs_set_zstd_parse_mode_ext(int mode) { return ZstdParse::set_ext(mode); }
int jfs_zstd_seek_csum_mode(void) { return ZstdSeekCsum::get(); }
int jfs_set_zstd_seek_csum_mode(int mode) { return ZstdSeekCsum::set(mode); }
int jfs_get_zstd_split_frames(void) { return (int)ZstdSplitFrames::get(); }
int jfs_set_zstd_split_frames(int max_frames) { return (int)ZstdSplitFrames::set(max_frames); }
int jfs_read_decode_mode(void) { return ReadDecode::get(); }
int jfs_set_read_decode_mode(int mode) { return ReadDecode::set(mode); }
int jfs_set_read_decode_mode_ext(int mode) { return ReadDecode::set_ext(mode); }
int jfs_read_seek_mode(void) { return ReadSeek::get(); }
int jfs_set_read_seek_mode(int mode) { return ReadSeek::set(mode); }
int jfs_set_read_seek_mode_ext(int mode) { return ReadSeek::set_ext(mode); }
int jfs_read_lz4_chase_mode(void) { return ReadLz4Chase::get(); }
int jfs_set_read_lz4_chase_mode(int mode) { return ReadLz4Chase::set(mode); }
int jfs_read_lz4_window_mode(void) { return ReadLz4Window::get(); }
int jfs_set_read_lz4_window_mode(int mode) { return ReadLz4Window::set(mode); }
int64_t jfs_lz4_chase_max(void) { return Lz4ChaseMax::get(); }
int64_t jfs_set_lz4_chase_max(int64_t bytes) { return Lz4ChaseMax::set(bytes); }
int jfs_compact_splice_mode(void) { return CompactSplice::get(); }
int jfs_set_compact_splice_mode(int mode) { return CompactSplice::set(mode); }
int jfs_set_compact_splice_mode_ext(int mode) { return CompactSplice::set_ext(mode); }
int jfs_compact_lz4_lift_mode(void) { return CompactLz4Lift::get(); }
int jfs_set_compact_lz4_lift_mode(int mode) { return CompactLz4Lift::set(mode); }

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
    return launch_rc(jfs_launch_gen(d_dst, nblk, block_bytes, cls, seed_base, dev->d_vocab, (hipStream_t)stream));
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
