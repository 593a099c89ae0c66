// Decode of seekable Zstd objects through their seek table (zstd_seek.h), read
// on the device.  Three calls, one sequence (the contracts are
// those of jfs_zstd_decompress_range_device, _frames_device and _ranges_device
// in the header): scan finds, per input, the frames that are asked for, and
// leaves a Rounds record of them; zseek_offsets gives every input its slice of
// one expanded list; expand writes that list, one independent decoder input per
// selected frame; the prefix launcher of zstd_decode_prefix.hip decodes it as
// it decodes any batch; XXH64 is taken of the pieces whose table carries
// checksums; fold turns the frames' results into the inputs'.  An input that is
// passed through is one entry of the list, itself.  What differs between the
// calls is a policy type each (RangeCall, FramesCall, RangesCall below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "jfs_internal.h"
#include "wave.cuh"
#include "zstd_seek.h"

namespace jfs {
namespace zseek {

enum : int32_t {
    M_PASS = 0,   // no table (or an early answer of the decoder's): the input itself
    M_TABLE = 1,  // the selected frames
    M_EMPTY = 2,  // nothing is asked for: 0
    M_BIG = 3,    // a table whose content exceeds dst_cap: -2
    M_BAD = 4,    // a bad descriptor, a bad list, or no valid table where one must be: -1
    M_FRAG = 5,   // a selected frame lies outside the fragment: -3
};

// per input, scan's answer
struct In {
    int32_t mode;
    int32_t answer;       // M_TABLE: min(D, hi'); M_PASS: the prefix decode's want
    int32_t nf, entry;    // the table's frames and its entry size
    int32_t tpos;         // where it starts in the bytes it is read from
    int32_t count;        // selected frames
    int32_t slot0;        // zseek_offsets: the input's first entry of the expanded list
};

__device__ __forceinline__ int32_t slots_of(const In &z) { return z.mode == M_TABLE && z.count > 0 ? z.count : 1; }

struct Fetch {
    const gc_u8 *s;
    __device__ __forceinline__ uint32_t operator()(int32_t p) const { return s[p]; }
};

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o, 64);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int l) {
    return (uint64_t)lane_read((uint32_t)(v >> 32), l) << 32 | lane_read((uint32_t)v, l);
}
__device__ __forceinline__ uint64_t wave_scan_incl64(uint64_t v) {
    const int l = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = shfl_up64(v, o);
        if (l >= o) v += y;
    }
    return v;
}

// ---- the three calls ----------------------------------------------------------
// One input as its call describes it.
struct Src {
    const uint8_t *table;   // the table is parsed from the end of table[0, end)
    int32_t end;
    int32_t body;           // a stand-alone table: the bytes its frames must take
    const uint8_t *frames;  // byte 0 of the object's frames
    uint8_t *dst;
    int32_t dst_cap;
};

// What is asked of an input: the selection predicate and h, the end of it (the
// answer is min(D, h)).  One range, or a list of them.
struct Run {
    int32_t l, h;
    __device__ __forceinline__ bool operator()(uint64_t d0, uint32_t d) const { return frame_in_run(d0, d, l, h); }
};
struct List {
    const jfs_range *rg;
    int32_t nr, cap, h;
    __device__ __forceinline__ bool operator()(uint64_t d0, uint32_t d) const { return frame_in_ranges(rg, nr, cap, d0, d); }
};

// A policy says: CSUM, whether 12-byte tables are taken (and their checksums
// compared); ALONE, whether the table stands alone beside a fragment of the
// frames; NO_TABLE, the mode of an input without a valid table; TABLE_FIRST,
// whether the table is judged before emptiness; COUNTS, whether
// g_sparse_counts move; src(i); and open(), the mode the input ends in before
// its table is looked at (M_TABLE: go on), with what is asked of it and the
// want of a passed-through input.  open() is called by the whole wave.
struct RangeCall {
    const jfs_dev_block *blocks;
    const int32_t *lo, *hi;
    using Ask = Run;
    static constexpr bool CSUM = false, ALONE = false, TABLE_FIRST = false, COUNTS = false;
    static constexpr int32_t NO_TABLE = M_PASS;
    __device__ __forceinline__ Src src(int i) const {
        const jfs_dev_block b = blocks[i];
        return Src{b.src, b.src_len, 0, b.src, b.dst, b.dst_cap};
    }
    __device__ __forceinline__ int32_t open(int i, const Src &s, Ask *a, int32_t *want) const {
        *a = Run{range_lo(lo[i]), range_hi(hi[i], s.dst_cap)};
        *want = hi[i];  // as given, not clamped
        if (s.table == nullptr || s.end <= 0 || s.dst_cap <= 0) return M_PASS;  // the decoder's own early answers
        return a->h <= a->l ? M_EMPTY : M_TABLE;
    }
};

struct FramesCall {
    const jfs_seek_frag *frags;
    const int32_t *lo, *hi;
    using Ask = Run;
    static constexpr bool CSUM = true, ALONE = true, TABLE_FIRST = true, COUNTS = false;
    static constexpr int32_t NO_TABLE = M_BAD;
    __device__ __forceinline__ Src src(int i) const {
        const jfs_seek_frag b = frags[i];
        return Src{b.table, b.table_len, (int32_t)((uint32_t)b.object_len - (uint32_t)b.table_len), b.frag - b.frag_off, b.dst,
                   b.dst_cap};
    }
    __device__ __forceinline__ int32_t open(int i, const Src &s, Ask *a, int32_t *want) const {
        const jfs_seek_frag b = frags[i];
        *a = Run{range_lo(lo[i]), range_hi(hi[i], b.dst_cap)};
        *want = 0;
        if (b.table == nullptr || b.frag == nullptr || b.dst == nullptr || b.table_len < 0 || b.object_len < 0 ||
            b.frag_off < 0 || b.frag_len < 0 || b.dst_cap < 0 || b.table_len > b.object_len)
            return M_BAD;
        return b.dst_cap == 0 || a->h <= a->l ? M_EMPTY : M_TABLE;
    }
    // the selected frames' bytes [c0, cend) of the object lie in the fragment
    __device__ __forceinline__ bool holds(int i, uint64_t c0, uint64_t cend) const {
        const jfs_seek_frag b = frags[i];
        return c0 >= (uint64_t)(uint32_t)b.frag_off && cend <= (uint64_t)(uint32_t)b.frag_off + (uint32_t)b.frag_len;
    }
};

struct RangesCall {
    const jfs_dev_block *blocks;
    const int32_t *rng_first;
    const jfs_range *rng;
    using Ask = List;
    static constexpr bool CSUM = true, ALONE = false, TABLE_FIRST = false, COUNTS = true;
    static constexpr int32_t NO_TABLE = M_PASS;
    __device__ __forceinline__ Src src(int i) const {
        const jfs_dev_block b = blocks[i];
        return Src{b.src, b.src_len, 0, b.src, b.dst, b.dst_cap};
    }
    // The list, one lane per range against its neighbour.
    __device__ __forceinline__ int32_t open(int i, const Src &s, Ask *a, int32_t *want) const {
        *a = List{rng, 0, s.dst_cap, 0};
        *want = s.dst_cap;
        if (s.table == nullptr || s.end <= 0 || s.dst_cap <= 0) return M_PASS;  // in front of the list's answers
        const int32_t r0 = rng_first[i], r1 = rng_first[i + 1];
        bool bad = r0 < 0 || r1 < r0, live = false;
        const jfs_range *rg = rng + (bad ? 0 : r0);
        const int32_t nr = bad ? 0 : r1 - r0;
        uint32_t top = 0;
        for (int32_t q = lane_id(); q < nr; q += 64) {
            const jfs_range c = rg[q];
            bad = bad || !range_follows(q > 0 ? &rg[q - 1] : (const jfs_range *)nullptr, c);
            if (range_live(c, s.dst_cap)) {
                live = true;
                top = umax32(top, (uint32_t)range_hi(c.hi, s.dst_cap));
            }
        }
        bad = __ballot(bad) != 0ull;
        live = __ballot(live) != 0ull;
        *a = List{rg, nr, s.dst_cap, (int32_t)wave_max(top)};
        *want = a->h;
        return bad ? M_BAD : !live ? M_EMPTY : M_TABLE;
    }
};

// inputs decoded through a table, frames selected, frames whose checksum was
// compared: of the ranges call alone
__device__ unsigned long long g_sparse_counts[3];

// One wave per input: 64 table entries a round, the two running sums by a wave
// scan, each lane asking about its own frame.
template <class P>
__global__ __launch_bounds__(64) void scan(const P p, int nblk, In *__restrict__ out, Rounds *__restrict__ rounds) {
    const int i = blockIdx.x, lane = lane_id();
    if (i >= nblk) return;
    const Src s = p.src(i);
    typename P::Ask ask;
    In z;
    z.nf = 0; z.entry = 0; z.tpos = 0; z.count = 0; z.slot0 = 0;
    z.mode = p.open(i, s, &ask, &z.answer);
    const Fetch f{(const gc_u8 *)s.table};
    int32_t nf = 0, tpos = 0, entry = 0;
    if (z.mode == M_TABLE || (P::TABLE_FIRST && z.mode == M_EMPTY)) {
        const bool empty = z.mode == M_EMPTY;
        z.mode = P::NO_TABLE;
        if (seek_table(f, s.end, P::CSUM, P::ALONE, &nf, &tpos, &entry)) {
            Rounds &R = rounds[i];
            uint64_t cs = 0, ds = 0;  // the sums in front of this round
            uint64_t c0 = 0, cend = 0;  // the selected frames' bytes, first to last
            int32_t cnt = 0;
            bool zero = false;
            for (int32_t k0 = 0; k0 < nf; k0 += 64) {
                const int32_t k = k0 + lane;
                const bool has = k < nf;
                uint32_t c = 0, d = 0, x = 0;
                if (has) seek_entry(f, tpos, entry, k, &c, &d, &x);
                const uint64_t ic = wave_scan_incl64(c), id = wave_scan_incl64(d);
                zero = zero || __ballot(has && c == 0u) != 0ull;
                const uint64_t m = __ballot(has && ask(ds + id - d, d));
                if (lane == 0) {
                    R.word[k0 >> 6] = m;
                    R.coff[k0 >> 6] = (uint32_t)cs;
                    R.doff[k0 >> 6] = (uint32_t)ds;
                    R.before[k0 >> 6] = cnt;
                }
                if (P::ALONE && m) {
                    if (cnt == 0) c0 = cs + shfl64(ic - c, __builtin_ctzll(m));
                    cend = cs + shfl64(ic, 63 - __builtin_clzll(m));
                }
                cnt += __popcll(m);
                cs += shfl64(ic, 63);
                ds += shfl64(id, 63);
            }
            if (seek_sums_ok(cs, ds, zero ? 1u : 0u, P::ALONE ? s.body : tpos)) {
                if (empty) {
                    z.mode = M_EMPTY;
                } else if (ds > (uint64_t)(uint32_t)s.dst_cap) {
                    z.mode = M_BIG;
                } else {
                    z.mode = M_TABLE;
                    z.nf = nf;
                    z.entry = entry;
                    z.tpos = tpos;
                    z.count = cnt;
                    z.answer = (int32_t)(ds < (uint64_t)(uint32_t)ask.h ? ds : (uint64_t)(uint32_t)ask.h);
                    if constexpr (P::ALONE) {
                        if (cnt > 0 && !p.holds(i, c0, cend)) z.mode = M_FRAG;
                    }
                }
            }
        }
    }
    if (lane == 0) out[i] = z;
}

// slot0 of every input and the length of the expanded list (one wave)
__global__ __launch_bounds__(64) void zseek_offsets(In *__restrict__ in, int nblk, uint64_t *__restrict__ total) {
    const int lane = lane_id();
    uint64_t base = 0;
    for (int i0 = 0; i0 < nblk; i0 += 64) {
        const int i = i0 + lane;
        const uint32_t n = i < nblk ? (uint32_t)slots_of(in[i]) : 0u;
        uint32_t sum = 0;
        const uint32_t ex = wave_scan_excl(n, &sum);
        // (an input takes MAX_FRAMES slots at most, so a round's 32-bit sum cannot wrap; a list
        // beyond int32 is refused on the host: the value only has to stay in range)
        if (i < nblk) in[i].slot0 = (int32_t)(base + ex < 0x7FFFFFFFull ? base + ex : 0x7FFFFFFFull);
        base += sum;
    }
    if (lane == 0) *total = base;
}

// One thread per entry of the expanded list: its input by binary search over
// slot0, its frame by place_frame (zstd_seek.h) from the input's Rounds.  With
// checksums, entry e also gets the piece XXH64 is taken of (its decoded
// content; nothing for a table without them) and the word to expect.
template <class P>
__global__ __launch_bounds__(64) void expand(const P p, int nblk, const In *__restrict__ in,
                                             const Rounds *__restrict__ rounds, int32_t total,
                                             jfs_dev_block *__restrict__ xdesc, int32_t *__restrict__ xwant,
                                             jfs_dev_block *__restrict__ hdesc, uint32_t *__restrict__ expect) {
    const int32_t e = (int32_t)(blockIdx.x * 64u + threadIdx.x);
    if (e >= total) return;
    int a = 0, z = nblk - 1;  // the last input with slot0 <= e
    while (a < z) {
        const int m = (a + z + 1) >> 1;
        if (in[m].slot0 <= e) a = m;
        else z = m - 1;
    }
    const In s = in[a];
    const Src b = p.src(a);
    jfs_dev_block x{b.table, b.dst, 0, 0};  // nothing to decode: an empty input
    jfs_dev_block hd{nullptr, nullptr, 0, 0};
    int32_t want = 0, k = 0;
    uint32_t coff = 0, doff = 0, c = 0, d = 0, sum = 0;
    const Fetch f{(const gc_u8 *)b.table};
    if (s.mode == M_PASS) {
        x = jfs_dev_block{b.table, b.dst, b.end, b.dst_cap};
        want = s.answer;
    } else if (s.mode == M_TABLE && s.count > 0 &&
               place_frame(f, s.tpos, s.entry, s.nf, rounds[a], e - s.slot0, &k, &coff, &doff)) {
        seek_entry(f, s.tpos, s.entry, k, &c, &d, &sum);
        if (d > 0u) {  // (a frame without content inside a run has nothing to write)
            x = jfs_dev_block{b.frames + coff, b.dst + doff, (int32_t)c, (int32_t)d};
            want = (int32_t)d;
        }
        if (s.entry == ENTRY_CSUM) hd = jfs_dev_block{b.dst + doff, nullptr, (int32_t)d, 0};
    }
    xdesc[e] = x;
    xwant[e] = want;
    if constexpr (P::CSUM) {
        hdesc[e] = hd;
        expect[e] = sum;
    }
}

// One wave per input: its result from its entries' results.  -1 (a frame that
// did not return its table size) wins over -4 (a frame whose content's XXH64
// low word is not its entry's), which wins over the answer.
template <class P>
__global__ __launch_bounds__(64) void fold(const In *__restrict__ in, int nblk, const jfs_dev_block *__restrict__ xdesc,
                                           const int32_t *__restrict__ xret, const jfs_dev_block *__restrict__ hdesc,
                                           const uint64_t *__restrict__ hash, const uint32_t *__restrict__ expect,
                                           int32_t *__restrict__ ret) {
    const int i = blockIdx.x, lane = lane_id();
    if (i >= nblk) return;
    const In s = in[i];
    int32_t r;
    if (s.mode == M_PASS) {
        r = xret[s.slot0];
    } else if (s.mode == M_BAD) {
        r = -1;
    } else if (s.mode == M_EMPTY) {
        r = 0;
    } else if (s.mode == M_BIG) {
        r = -2;
    } else if (s.mode == M_FRAG) {
        r = -3;
    } else {
        bool bad = false, differ = false;
        uint32_t compared = 0;
        for (int32_t j = lane; j < s.count; j += 64) {
            const int32_t d = xdesc[s.slot0 + j].dst_cap;
            bad = bad || (d > 0 && xret[s.slot0 + j] != d);
            if constexpr (P::CSUM) {
                if (hdesc[s.slot0 + j].src != nullptr) {
                    compared++;
                    differ = differ || (uint32_t)hash[s.slot0 + j] != expect[s.slot0 + j];
                }
            }
        }
        r = __ballot(bad) ? -1 : __ballot(differ) ? -4 : s.answer;
        if constexpr (P::COUNTS) {
            compared = wave_sum(compared);
            if (lane == 0) {
                atomicAdd(&g_sparse_counts[0], 1ull);
                if (s.count > 0) atomicAdd(&g_sparse_counts[1], (unsigned long long)s.count);
                if (compared > 0u) atomicAdd(&g_sparse_counts[2], (unsigned long long)compared);
            }
        }
    }
    if (lane == 0) ret[i] = r;
}

// jfs_zstd_load_range_batch: read i's requested bytes, block[lo, lo + len) of
// its decoded block, go to its place in the area that crosses the link -- only
// where the decode answered the length the host expects (anything else is a
// failed read: nothing of it comes down).  grid (tiles of 16 KiB, reads).
constexpr int32_t PACK_TILE = 16 << 10;
__global__ __launch_bounds__(256) void zframes_pack(const jfs_range_pack *__restrict__ pk, int n,
                                                    const int32_t *__restrict__ ret) {
    const int i = blockIdx.y;
    if (i >= n) return;
    const jfs_range_pack p = pk[i];
    if (p.len <= 0 || ret[i] != p.expect) return;
    const int64_t t0 = (int64_t)blockIdx.x * PACK_TILE;
    if (t0 >= p.len) return;
    const int32_t m = (int32_t)(p.len - t0 < PACK_TILE ? p.len - t0 : PACK_TILE);
    gc_u8 *s = (gc_u8 *)p.src + t0;
    g_u8 *d = (g_u8 *)p.dst + t0;
    if ((((uintptr_t)s | (uintptr_t)d) & 15u) == 0) {
        const int32_t q = m >> 4;
        for (int32_t k = threadIdx.x; k < q; k += 256) ((g_u4 *)d)[k] = ((gc_u4 *)s)[k];
        for (int32_t k = (q << 4) + threadIdx.x; k < m; k += 256) d[k] = s[k];
    } else {
        for (int32_t k = threadIdx.x; k < m; k += 256) d[k] = s[k];
    }
}

namespace {
struct Scratch {
    std::mutex mu;
    bool ready = false;  // the four below exist
    uint64_t *d_total = nullptr, *h_total = nullptr;
    hipEvent_t ev_total = nullptr, ev_done = nullptr;
    In *d_in = nullptr;
    size_t in_cap = 0;
    uint8_t *d_r = nullptr;  // per input: its Rounds
    size_t r_cap = 0;
    uint8_t *d_x = nullptr;  // per entry: descriptor, want, result
    size_t x_cap = 0;
    uint8_t *d_h = nullptr;  // per entry of a call that compares checksums: hash descriptor, hash, expected word
    size_t h_cap = 0;
};
Scratch g_scr[16];

// all four or none: a scratch that is not ready is set up again by the next call
bool init(Scratch &z) {
    uint64_t *d = nullptr, *h = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipMalloc((void **)&d, sizeof(uint64_t)) == hipSuccess &&
        hipHostMalloc((void **)&h, sizeof(uint64_t), hipHostMallocDefault) == hipSuccess &&
        hipEventCreateWithFlags(&e0, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&e1, hipEventDisableTiming) == hipSuccess) {
        z.d_total = d; z.h_total = h; z.ev_total = e0; z.ev_done = e1;
        return z.ready = true;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
    return false;
}

template <class T>
bool grow(T **p, size_t *cap, size_t want) {
    if (*cap >= want) return true;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    size_t n = 1024;
    while (n < want) n <<= 1;
    if (hipMalloc((void **)p, n * sizeof(T)) != hipSuccess) return false;
    *cap = n;
    return true;
}
constexpr size_t X_ENTRY = sizeof(jfs_dev_block) + 8;
constexpr size_t H_ENTRY = sizeof(jfs_dev_block) + 8 + 8;  // (the expected word's 4 bytes, padded)

// scan -> offsets -> (one host wait for the list's length, as the decoder waits
// for its header scan) -> expand -> prefix decode of the list -> XXH64 of the
// decoded pieces (where the call compares checksums) -> fold
template <class P>
int launch(const P &p, int nblk, int32_t *d_ret, hipStream_t stream) {
    if (nblk <= 0) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return -1;
    Scratch &z = g_scr[dev];
    std::lock_guard<std::mutex> lk(z.mu);
    if (!z.ready && !init(z)) return -1;
    if ((size_t)nblk > z.in_cap || (size_t)nblk * sizeof(Rounds) > z.r_cap) {
        // earlier launches (any stream) may still read the old scratch
        if (hipEventSynchronize(z.ev_done) != hipSuccess) return -1;
        if (!grow(&z.d_in, &z.in_cap, (size_t)nblk)) return -1;
        if (!grow(&z.d_r, &z.r_cap, (size_t)nblk * sizeof(Rounds))) return -1;
    }
    // launches that share the scratch run in call order across streams
    if (hipStreamWaitEvent(stream, z.ev_done, 0) != hipSuccess) return -1;
    hipLaunchKernelGGL(scan<P>, dim3((unsigned)nblk), dim3(64), 0, stream, p, nblk, z.d_in, (Rounds *)z.d_r);
    hipLaunchKernelGGL(zseek_offsets, dim3(1), dim3(64), 0, stream, z.d_in, nblk, z.d_total);
    if (hipGetLastError() != hipSuccess) return -1;
    if (hipMemcpyAsync(z.h_total, z.d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, stream) != hipSuccess) return -1;
    if (hipEventRecord(z.ev_total, stream) != hipSuccess) return -1;
    if (hipEventSynchronize(z.ev_total) != hipSuccess) return -1;
    const uint64_t total = *z.h_total;
    if (total < (uint64_t)nblk || total > 0x7FFFFFF0ull / (P::CSUM ? H_ENTRY : X_ENTRY)) return -1;
    // every earlier launch on the scratch is done: ev_done was waited for on
    // `stream` ahead of ev_total
    if (!grow(&z.d_x, &z.x_cap, (size_t)total * X_ENTRY)) return -1;
    if (P::CSUM && !grow(&z.d_h, &z.h_cap, (size_t)total * H_ENTRY)) return -1;
    jfs_dev_block *xdesc = (jfs_dev_block *)z.d_x, *hdesc = P::CSUM ? (jfs_dev_block *)z.d_h : nullptr;
    int32_t *xwant = (int32_t *)(xdesc + total), *xret = xwant + total;
    uint64_t *hash = P::CSUM ? (uint64_t *)(hdesc + total) : nullptr;
    uint32_t *expect = P::CSUM ? (uint32_t *)(hash + total) : nullptr;
    hipLaunchKernelGGL(expand<P>, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, stream, p, nblk, (const In *)z.d_in,
                       (const Rounds *)z.d_r, (int32_t)total, xdesc, xwant, hdesc, expect);
    if (hipGetLastError() != hipSuccess) return -1;
    if (jfs_launch_zstd_decode_prefix(xdesc, (int)total, xret, xwant, stream) != 0) return -1;
    if (P::CSUM && jfs_launch_xxh64(hdesc, (int)total, hash, nullptr, stream) != 0) return -1;
    hipLaunchKernelGGL(fold<P>, dim3((unsigned)nblk), dim3(64), 0, stream, (const In *)z.d_in, nblk,
                       (const jfs_dev_block *)xdesc, (const int32_t *)xret, (const jfs_dev_block *)hdesc,
                       (const uint64_t *)hash, (const uint32_t *)expect, d_ret);
    if (hipGetLastError() != hipSuccess) return -1;
    return hipEventRecord(z.ev_done, stream) == hipSuccess ? 0 : -1;
}
}  // namespace

}  // namespace zseek
}  // namespace jfs

extern "C" int jfs_launch_zstd_decode_range(const jfs_dev_block *d_blocks, const int32_t *d_lo, const int32_t *d_hi,
                                            int nblk, int32_t *d_ret, hipStream_t stream) {
    return jfs::zseek::launch(jfs::zseek::RangeCall{d_blocks, d_lo, d_hi}, nblk, d_ret, stream);
}

extern "C" int jfs_launch_zstd_decode_frames(const jfs_seek_frag *d_frags, const int32_t *d_lo, const int32_t *d_hi,
                                             int nblk, int32_t *d_ret, hipStream_t stream) {
    return jfs::zseek::launch(jfs::zseek::FramesCall{d_frags, d_lo, d_hi}, nblk, d_ret, stream);
}

extern "C" int jfs_launch_zstd_decode_ranges(const jfs_dev_block *d_blocks, const int32_t *d_rng_first,
                                             const jfs_range *d_rng, int nblk, int32_t *d_ret, hipStream_t stream) {
    return jfs::zseek::launch(jfs::zseek::RangesCall{d_blocks, d_rng_first, d_rng}, nblk, d_ret, stream);
}

// Diagnostics of the ranges call (and of the reads in JFS_READ_SEEK=sparse) on
// the current device since the last reset; synchronous.
extern "C" int jfs_zstd_sparse_counts(uint64_t out[3], int reset) {
    unsigned long long v[3] = {0, 0, 0};
    if (!out) return -1;
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(jfs::zseek::g_sparse_counts), sizeof(v)) != hipSuccess) return -1;
    for (int i = 0; i < 3; i++) out[i] = v[i];
    if (reset) {
        unsigned long long z[3] = {0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(jfs::zseek::g_sparse_counts), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}

extern "C" int jfs_launch_range_pack(const jfs_range_pack *d_pack, int n, int32_t max_len, const int32_t *d_ret,
                                     hipStream_t stream) {
    using namespace jfs::zseek;
    if (n <= 0 || max_len <= 0) return 0;
    for (int a = 0; a < n; a += 65535) {  // (the grid's y extent)
        const int m = n - a < 65535 ? n - a : 65535;
        hipLaunchKernelGGL(zframes_pack, dim3((unsigned)((max_len + PACK_TILE - 1) / PACK_TILE), (unsigned)m), dim3(256),
                           0, stream, d_pack + a, m, d_ret + a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
