// Range decode of seekable Zstd objects (the contract is
// jfs_zstd_decompress_range_device's in the header).  The seek table
// (zstd_seek.h) is read on the device: zseek_scan finds, per input, the frames
// a byte range touches; zseek_offsets gives every input its slice of one
// expanded list; zseek_expand writes that list, one independent decoder input
// per selected frame; the prefix launcher of zstd_decode_prefix.hip decodes it
// as it decodes any batch; zseek_fold turns the frames' results into the
// inputs'.  An input without a valid table is one entry of the list, itself.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "jfs_internal.h"
#include "wave.cuh"
#include "zstd_seek.h"

namespace jfs {
namespace zseek {

enum : int32_t {
    M_PASS = 0,   // no table (or an early answer of the decoder's): the input itself, want = hi
    M_TABLE = 1,  // the selected frames
    M_EMPTY = 2,  // hi' <= lo': 0
    M_BIG = 3,    // a table whose content exceeds dst_cap: -2
};

// per input, zseek_scan's answer
struct In {
    int32_t mode;
    int32_t answer;  // M_TABLE: min(D, hi')
    int32_t nf;
    int32_t first, count;  // selected frames
    uint32_t coff, doff;   // where frame `first` starts: compressed, content
    int32_t slot0;         // zseek_offsets: the input's first entry of the expanded list
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

// One wave per input: 64 table entries a round, the two running sums by a wave
// scan.  The frames in front of the range are a prefix of the table and those
// behind it a suffix, so a round's ballots place the selection.
__global__ __launch_bounds__(64) void zseek_scan(const jfs_dev_block *__restrict__ blocks, const int32_t *__restrict__ lo,
                                                 const int32_t *__restrict__ hi, int nblk, In *__restrict__ out) {
    const int i = blockIdx.x, lane = lane_id();
    if (i >= nblk) return;
    const jfs_dev_block b = blocks[i];
    In z;
    z.mode = M_PASS; z.answer = 0; z.nf = 0; z.first = 0; z.count = 0; z.coff = 0; z.doff = 0; z.slot0 = 0;
    const int32_t l = range_lo(lo[i]), h = range_hi(hi[i], b.dst_cap);
    const Fetch f{(const gc_u8 *)b.src};
    int32_t nf = 0, tpos = 0;
    if (b.src == nullptr || b.src_len <= 0 || b.dst_cap <= 0) {
        // the decoder's own early answers
    } else if (h <= l) {
        z.mode = M_EMPTY;
    } else if (seek_footer(f, b.src_len, &nf, &tpos)) {
        uint64_t cs = 0, ds = 0;  // the sums in front of this round
        int32_t before = 0, end = 0;
        uint64_t coff = 0, doff = 0;
        bool zero = false;
        for (int32_t k0 = 0; k0 < nf; k0 += 64) {
            const int32_t k = k0 + lane;
            const bool has = k < nf;
            uint32_t c = 0, d = 0;
            if (has) seek_entry(f, tpos, k, &c, &d);
            const uint64_t ic = wave_scan_incl64(c), id = wave_scan_incl64(d);
            const uint64_t d0 = ds + id - d;
            const bool bef = has && frame_before(d0, d, l);
            const bool sel = has && !bef && !frame_from(d0, h);
            zero = zero || __ballot(has && c == 0u) != 0ull;
            const int nbef = __popcll(__ballot(bef));
            if (nbef > 0) {
                before = k0 + nbef;
                coff = cs + shfl64(ic, nbef - 1);
                doff = ds + shfl64(id, nbef - 1);
            }
            const uint64_t m = __ballot(sel);
            if (m) end = k0 + 64 - __builtin_clzll(m);
            cs += shfl64(ic, 63);
            ds += shfl64(id, 63);
        }
        if (seek_sums_ok(cs, ds, zero ? 1u : 0u, tpos)) {
            if (ds > (uint64_t)(uint32_t)b.dst_cap) {
                z.mode = M_BIG;
            } else {
                z.mode = M_TABLE;
                z.nf = nf;
                z.answer = (int32_t)(ds < (uint64_t)(uint32_t)h ? ds : (uint64_t)(uint32_t)h);
                if (end > before) {
                    z.first = before;
                    z.count = end - before;
                    z.coff = (uint32_t)coff;
                    z.doff = (uint32_t)doff;
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
// slot0, its frame by walking the table on from the first selected one.
__global__ __launch_bounds__(64) void zseek_expand(const jfs_dev_block *__restrict__ blocks, const int32_t *__restrict__ hi,
                                                   int nblk, const In *__restrict__ in, int32_t total,
                                                   jfs_dev_block *__restrict__ xdesc, int32_t *__restrict__ xwant) {
    const int32_t e = (int32_t)(blockIdx.x * 64u + threadIdx.x);
    if (e >= total) return;
    int a = 0, z = nblk - 1;  // the last input with slot0 <= e
    while (a < z) {
        const int m = (a + z + 1) >> 1;
        if (in[m].slot0 <= e) a = m;
        else z = m - 1;
    }
    const In s = in[a];
    const jfs_dev_block b = blocks[a];
    jfs_dev_block x{b.src, b.dst, 0, 0};  // nothing to decode: an empty input
    int32_t want = 0;
    if (s.mode == M_PASS) {
        x = b;
        want = hi[a];
    } else if (s.mode == M_TABLE && s.count > 0) {
        const Fetch f{(const gc_u8 *)b.src};
        const int32_t tpos = b.src_len - (int32_t)table_bytes(s.nf), j = e - s.slot0;
        uint32_t coff = s.coff, doff = s.doff, c = 0, d = 0;
        for (int32_t k = s.first; k < s.first + j; k++) {
            seek_entry(f, tpos, k, &c, &d);
            coff += c;
            doff += d;
        }
        seek_entry(f, tpos, s.first + j, &c, &d);
        if (d > 0u) {  // (a frame without content inside the selection has nothing to write)
            x = jfs_dev_block{b.src + coff, b.dst + doff, (int32_t)c, (int32_t)d};
            want = (int32_t)d;
        }
    }
    xdesc[e] = x;
    xwant[e] = want;
}

// One wave per input: its result from its entries' results.
__global__ __launch_bounds__(64) void zseek_fold(const In *__restrict__ in, int nblk, const jfs_dev_block *__restrict__ xdesc,
                                                 const int32_t *__restrict__ xret, int32_t *__restrict__ ret) {
    const int i = blockIdx.x, lane = lane_id();
    if (i >= nblk) return;
    const In s = in[i];
    int32_t r;
    if (s.mode == M_PASS) {
        r = xret[s.slot0];
    } else if (s.mode == M_EMPTY) {
        r = 0;
    } else if (s.mode == M_BIG) {
        r = -2;
    } else {
        bool bad = false;
        for (int32_t j = lane; j < s.count; j += 64) {
            const int32_t d = xdesc[s.slot0 + j].dst_cap;
            bad = bad || (d > 0 && xret[s.slot0 + j] != d);
        }
        r = __ballot(bad) ? -1 : s.answer;
    }
    if (lane == 0) ret[i] = r;
}

// ---- fragments (jfs_zstd_decompress_frames_device) --------------
// The same four steps over a table that stands alone (zstd_seek.h, second
// part) and a fragment of the object's frames: sibling kernels, so the range
// call keeps its own.  zseek_offsets serves both.
enum : int32_t {
    M_BAD = 4,   // a bad descriptor or no valid table: -1
    M_FRAG = 5,  // a selected frame lies outside the fragment: -3
};

__global__ __launch_bounds__(64) void zframes_scan(const jfs_seek_frag *__restrict__ frags, const int32_t *__restrict__ lo,
                                                   const int32_t *__restrict__ hi, int nblk, In *__restrict__ out) {
    const int i = blockIdx.x, lane = lane_id();
    if (i >= nblk) return;
    const jfs_seek_frag b = frags[i];
    In z;
    z.mode = M_BAD; z.answer = 0; z.nf = 0; z.first = 0; z.count = 0; z.coff = 0; z.doff = 0; z.slot0 = 0;
    const int32_t l = range_lo(lo[i]), h = range_hi(hi[i], b.dst_cap);
    const Fetch f{(const gc_u8 *)b.table};
    int32_t nf = 0, entry = 0;
    if (b.table == nullptr || b.frag == nullptr || b.dst == nullptr || b.table_len < 0 || b.object_len < 0 ||
        b.frag_off < 0 || b.frag_len < 0 || b.dst_cap < 0) {
        // -1
    } else if (table_header(f, b.table_len, b.object_len, &nf, &entry)) {
        uint64_t cs = 0, ds = 0;  // the sums in front of this round
        int32_t before = 0, end = 0;
        uint64_t coff = 0, doff = 0, cend = 0;
        bool zero = false;
        for (int32_t k0 = 0; k0 < nf; k0 += 64) {
            const int32_t k = k0 + lane;
            const bool has = k < nf;
            uint32_t c = 0, d = 0, x = 0;
            if (has) table_entry(f, entry, k, &c, &d, &x);
            const uint64_t ic = wave_scan_incl64(c), id = wave_scan_incl64(d);
            const uint64_t d0 = ds + id - d;
            const bool bef = has && frame_before(d0, d, l);
            const bool sel = has && !bef && !frame_from(d0, h);
            zero = zero || __ballot(has && c == 0u) != 0ull;
            const int nbef = __popcll(__ballot(bef));
            if (nbef > 0) {
                before = k0 + nbef;
                coff = cs + shfl64(ic, nbef - 1);
                doff = ds + shfl64(id, nbef - 1);
            }
            const uint64_t m = __ballot(sel);
            if (m) {
                end = k0 + 64 - __builtin_clzll(m);
                cend = cs + shfl64(ic, 63 - __builtin_clzll(m));
            }
            cs += shfl64(ic, 63);
            ds += shfl64(id, 63);
        }
        if (zero || cs != (uint64_t)(uint32_t)(b.object_len - b.table_len) || ds > 0xFFFFFFFFull) {
            // -1
        } else if (b.dst_cap == 0 || h <= l) {
            z.mode = M_EMPTY;
        } else if (ds > (uint64_t)(uint32_t)b.dst_cap) {
            z.mode = M_BIG;
        } else {
            z.mode = M_TABLE;
            z.nf = nf;
            z.answer = (int32_t)(ds < (uint64_t)(uint32_t)h ? ds : (uint64_t)(uint32_t)h);
            if (end > before) {
                if (coff < (uint64_t)(uint32_t)b.frag_off || cend > (uint64_t)(uint32_t)b.frag_off + (uint32_t)b.frag_len) {
                    z.mode = M_FRAG;
                } else {
                    z.first = before;
                    z.count = end - before;
                    z.coff = (uint32_t)coff;
                    z.doff = (uint32_t)doff;
                }
            }
        }
    }
    if (lane == 0) out[i] = z;
}

// As zseek_expand; entry e also gets the piece XXH64 is taken of (its decoded
// content; nothing for a table without checksums) and the word to expect.
__global__ __launch_bounds__(64) void zframes_expand(const jfs_seek_frag *__restrict__ frags, int nblk,
                                                     const In *__restrict__ in, int32_t total,
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
    const jfs_seek_frag b = frags[a];
    jfs_dev_block x{b.frag, b.dst, 0, 0};  // nothing to decode: an empty input
    jfs_dev_block hd{nullptr, nullptr, 0, 0};
    int32_t want = 0;
    uint32_t sum = 0;
    if (s.mode == M_TABLE && s.count > 0) {
        const Fetch f{(const gc_u8 *)b.table};
        const int32_t entry = f(b.table_len - 5) ? ENTRY_CSUM : ENTRY, j = e - s.slot0;
        uint32_t coff = s.coff, doff = s.doff, c = 0, d = 0;
        for (int32_t k = s.first; k < s.first + j; k++) {
            table_entry(f, entry, k, &c, &d, &sum);
            coff += c;
            doff += d;
        }
        table_entry(f, entry, s.first + j, &c, &d, &sum);
        if (d > 0u) {  // (a frame without content inside the selection has nothing to write)
            x = jfs_dev_block{b.frag + (coff - (uint32_t)b.frag_off), b.dst + doff, (int32_t)c, (int32_t)d};
            want = (int32_t)d;
        }
        if (entry == ENTRY_CSUM) hd = jfs_dev_block{b.dst + doff, nullptr, (int32_t)d, 0};
    }
    xdesc[e] = x;
    xwant[e] = want;
    hdesc[e] = hd;
    expect[e] = sum;
}

// As zseek_fold, with the two new answers and the checksum verdict: -1 (a frame
// that did not return its table size) wins over -4 (a frame whose content's
// XXH64 low word is not its entry's).
__global__ __launch_bounds__(64) void zframes_fold(const In *__restrict__ in, int nblk, const jfs_dev_block *__restrict__ xdesc,
                                                   const int32_t *__restrict__ xret, const jfs_dev_block *__restrict__ hdesc,
                                                   const uint64_t *__restrict__ hash, const uint32_t *__restrict__ expect,
                                                   int32_t *__restrict__ ret) {
    const int i = blockIdx.x, lane = lane_id();
    if (i >= nblk) return;
    const In s = in[i];
    int32_t r;
    if (s.mode == M_BAD) {
        r = -1;
    } else if (s.mode == M_EMPTY) {
        r = 0;
    } else if (s.mode == M_BIG) {
        r = -2;
    } else if (s.mode == M_FRAG) {
        r = -3;
    } else {
        bool bad = false, differ = false;
        for (int32_t j = lane; j < s.count; j += 64) {
            const int32_t d = xdesc[s.slot0 + j].dst_cap;
            bad = bad || (d > 0 && xret[s.slot0 + j] != d);
            differ = differ || (hdesc[s.slot0 + j].src != nullptr && (uint32_t)hash[s.slot0 + j] != expect[s.slot0 + j]);
        }
        r = __ballot(bad) ? -1 : __ballot(differ) ? -4 : s.answer;
    }
    if (lane == 0) ret[i] = r;
}

// ---- several ranges per input (jfs_zstd_decompress_ranges_device) --
// The same sequence once more for a whole object and a list of ranges: the
// table of either layout is found from the object's end, the selection is a
// set of frames (frame_in_ranges of zstd_seek.h), no longer a run of them, and a
// 12-byte table's checksums are compared.  What zsparse_scan leaves per input:
// In with first = the entry size and coff = the table's position, and per round
// of 64 entries its selection word and what lies in front of it, so that
// zsparse_expand places an entry without walking the table from its start.
constexpr int32_t ROUNDS = MAX_FRAMES / 64;
struct Rounds {
    uint64_t word[ROUNDS];   // the round's selected frames, bit = lane
    uint32_t coff[ROUNDS];   // compressed bytes in front of the round
    uint32_t doff[ROUNDS];   // content in front of it
    int32_t before[ROUNDS];  // selected frames in front of it
};

// inputs decoded through a table, frames selected, frames whose checksum was compared
__device__ unsigned long long g_sparse_counts[3];

// One wave per input.  The list first, one lane per range against its
// neighbour; then 64 table entries a round, each lane asking the list about its
// own frame.
__global__ __launch_bounds__(64) void zsparse_scan(const jfs_dev_block *__restrict__ blocks,
                                                   const int32_t *__restrict__ rng_first,
                                                   const jfs_range *__restrict__ rng, int nblk, In *__restrict__ out,
                                                   Rounds *__restrict__ rounds) {
    const int i = blockIdx.x, lane = lane_id();
    if (i >= nblk) return;
    const jfs_dev_block b = blocks[i];
    In z;
    z.mode = M_PASS; z.answer = b.dst_cap; z.nf = 0; z.first = 0; z.count = 0; z.coff = 0; z.doff = 0; z.slot0 = 0;
    if (b.src == nullptr || b.src_len <= 0 || b.dst_cap <= 0) {
        // the decoder's own early answers, in front of the list's
    } else {
        const int32_t r0 = rng_first[i], r1 = rng_first[i + 1];
        bool bad = r0 < 0 || r1 < r0, live = false;
        const jfs_range *rg = rng + (bad ? 0 : r0);
        const int32_t nr = bad ? 0 : r1 - r0;
        uint32_t top = 0;
        for (int32_t q = lane; q < nr; q += 64) {
            const jfs_range c = rg[q];
            bad = bad || !range_follows(q > 0 ? &rg[q - 1] : (const jfs_range *)nullptr, c);
            if (range_live(c, b.dst_cap)) {
                live = true;
                top = umax32(top, (uint32_t)range_hi(c.hi, b.dst_cap));
            }
        }
        bad = __ballot(bad) != 0ull;
        live = __ballot(live) != 0ull;
        const int32_t H = (int32_t)wave_max(top);
        const Fetch f{(const gc_u8 *)b.src};
        int32_t nf = 0, tpos = 0, entry = 0;
        z.answer = H;  // M_PASS: the prefix decode's want
        if (bad) {
            z.mode = M_BAD;
        } else if (!live) {
            z.mode = M_EMPTY;
        } else if (seek_footer_any(f, b.src_len, &nf, &tpos, &entry)) {
            Rounds &R = rounds[i];
            uint64_t cs = 0, ds = 0;  // the sums in front of this round
            int32_t cnt = 0;
            bool zero = false;
            for (int32_t k0 = 0; k0 < nf; k0 += 64) {
                const int32_t k = k0 + lane;
                const bool has = k < nf;
                uint32_t c = 0, d = 0, x = 0;
                if (has) seek_entry_any(f, tpos, entry, k, &c, &d, &x);
                const uint64_t ic = wave_scan_incl64(c), id = wave_scan_incl64(d);
                const bool sel = has && frame_in_ranges(rg, nr, b.dst_cap, ds + id - d, d);
                zero = zero || __ballot(has && c == 0u) != 0ull;
                const uint64_t m = __ballot(sel);
                if (lane == 0) {
                    R.word[k0 >> 6] = m;
                    R.coff[k0 >> 6] = (uint32_t)cs;
                    R.doff[k0 >> 6] = (uint32_t)ds;
                    R.before[k0 >> 6] = cnt;
                }
                cnt += __popcll(m);
                cs += shfl64(ic, 63);
                ds += shfl64(id, 63);
            }
            if (seek_sums_ok(cs, ds, zero ? 1u : 0u, tpos)) {
                if (ds > (uint64_t)(uint32_t)b.dst_cap) {
                    z.mode = M_BIG;
                } else {
                    z.mode = M_TABLE;
                    z.nf = nf;
                    z.first = entry;
                    z.coff = (uint32_t)tpos;
                    z.count = cnt;
                    z.answer = (int32_t)(ds < (uint64_t)(uint32_t)H ? ds : (uint64_t)(uint32_t)H);
                }
            }
        }
    }
    if (lane == 0) out[i] = z;
}

// One thread per entry of the expanded list: its input by binary search over
// slot0, its round by binary search over the rounds' counts, its frame the j-th
// set bit of the round's word, its offsets the round's plus at most 63 entries.
__global__ __launch_bounds__(64) void zsparse_expand(const jfs_dev_block *__restrict__ blocks, int nblk,
                                                     const In *__restrict__ in, const Rounds *__restrict__ rounds,
                                                     int32_t total, jfs_dev_block *__restrict__ xdesc,
                                                     int32_t *__restrict__ xwant, jfs_dev_block *__restrict__ hdesc,
                                                     uint32_t *__restrict__ expect) {
    const int32_t e = (int32_t)(blockIdx.x * 64u + threadIdx.x);
    if (e >= total) return;
    int a = 0, z = nblk - 1;  // the last input with slot0 <= e
    while (a < z) {
        const int m = (a + z + 1) >> 1;
        if (in[m].slot0 <= e) a = m;
        else z = m - 1;
    }
    const In s = in[a];
    const jfs_dev_block b = blocks[a];
    jfs_dev_block x{b.src, b.dst, 0, 0};  // nothing to decode: an empty input
    jfs_dev_block hd{nullptr, nullptr, 0, 0};
    int32_t want = 0;
    uint32_t sum = 0;
    if (s.mode == M_PASS) {
        x = b;
        want = s.answer;
    } else if (s.mode == M_TABLE && s.count > 0) {
        const Rounds &R = rounds[a];
        const int32_t j = e - s.slot0;
        int32_t r = 0, rz = ((s.nf + 63) >> 6) - 1;  // the last round with before <= j: the one that holds entry j
        while (r < rz) {
            const int32_t m = (r + rz + 1) >> 1;
            if (R.before[m] <= j) r = m;
            else rz = m - 1;
        }
        uint64_t w = R.word[r];
        for (int32_t t = j - R.before[r]; t > 0; t--) w &= w - 1;
        if (w != 0ull) {  // (always: the round holds more than j - before selected frames)
            const Fetch f{(const gc_u8 *)b.src};
            const int32_t tpos = (int32_t)s.coff, entry = s.first, k = r * 64 + __builtin_ctzll(w);
            uint32_t coff = R.coff[r], doff = R.doff[r], c = 0, d = 0;
            for (int32_t q = r * 64; q < k; q++) {
                seek_entry_any(f, tpos, entry, q, &c, &d, &sum);
                coff += c;
                doff += d;
            }
            seek_entry_any(f, tpos, entry, k, &c, &d, &sum);
            x = jfs_dev_block{b.src + coff, b.dst + doff, (int32_t)c, (int32_t)d};  // d > 0: the frame was selected
            want = (int32_t)d;
            if (entry == ENTRY_CSUM) hd = jfs_dev_block{b.dst + doff, nullptr, (int32_t)d, 0};
        }
    }
    xdesc[e] = x;
    xwant[e] = want;
    hdesc[e] = hd;
    expect[e] = sum;
}

// zframes_fold's precedence with the bad list's answer, and the three counters.
__global__ __launch_bounds__(64) void zsparse_fold(const In *__restrict__ in, int nblk, const jfs_dev_block *__restrict__ xdesc,
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
    } else {
        bool bad = false, differ = false;
        uint32_t compared = 0;
        for (int32_t j = lane; j < s.count; j += 64) {
            const int32_t d = xdesc[s.slot0 + j].dst_cap;
            bad = bad || (d > 0 && xret[s.slot0 + j] != d);
            if (hdesc[s.slot0 + j].src != nullptr) {
                compared++;
                differ = differ || (uint32_t)hash[s.slot0 + j] != expect[s.slot0 + j];
            }
        }
        r = __ballot(bad) ? -1 : __ballot(differ) ? -4 : s.answer;
        compared = wave_sum(compared);
        if (lane == 0) {
            atomicAdd(&g_sparse_counts[0], 1ull);
            if (s.count > 0) atomicAdd(&g_sparse_counts[1], (unsigned long long)s.count);
            if (compared > 0u) atomicAdd(&g_sparse_counts[2], (unsigned long long)compared);
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
    In *d_in = nullptr;
    size_t in_cap = 0;
    uint8_t *d_x = nullptr;  // per entry: descriptor, want, result
    size_t x_cap = 0;
    uint8_t *d_h = nullptr;  // per entry of a fragment or ranges decode: hash descriptor, hash, expected word
    size_t h_cap = 0;
    uint8_t *d_r = nullptr;  // per input of a ranges decode: its Rounds
    size_t r_cap = 0;
    uint64_t *d_total = nullptr, *h_total = nullptr;
    hipEvent_t ev_total = nullptr, ev_done = nullptr;
};
Scratch g_scr[16];

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
}  // namespace

}  // namespace zseek
}  // namespace jfs

// scan -> offsets -> (one host wait for the list's length, as the decoder waits
// for its header scan) -> expand -> prefix decode of the list -> fold
extern "C" int jfs_launch_zstd_decode_range(const jfs_dev_block *d_blocks, const int32_t *d_lo, const int32_t *d_hi,
                                            int nblk, int32_t *d_ret, hipStream_t stream) {
    using namespace jfs::zseek;
    if (nblk <= 0) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return -1;
    Scratch &z = g_scr[dev];
    std::lock_guard<std::mutex> lk(z.mu);
    if (!z.d_total) {
        if (hipMalloc((void **)&z.d_total, sizeof(uint64_t)) != hipSuccess) return -1;
        if (hipHostMalloc((void **)&z.h_total, sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) return -1;
        if (hipEventCreateWithFlags(&z.ev_total, hipEventDisableTiming) != hipSuccess) return -1;
        if (hipEventCreateWithFlags(&z.ev_done, hipEventDisableTiming) != hipSuccess) return -1;
    }
    if ((size_t)nblk > z.in_cap) {
        // earlier launches (any stream) may still read the old scratch
        if (hipEventSynchronize(z.ev_done) != hipSuccess) return -1;
        if (!grow(&z.d_in, &z.in_cap, (size_t)nblk)) return -1;
    }
    // launches that share the scratch run in call order across streams
    if (hipStreamWaitEvent(stream, z.ev_done, 0) != hipSuccess) return -1;
    hipLaunchKernelGGL(zseek_scan, dim3((unsigned)nblk), dim3(64), 0, stream, d_blocks, d_lo, d_hi, nblk, z.d_in);
    hipLaunchKernelGGL(zseek_offsets, dim3(1), dim3(64), 0, stream, z.d_in, nblk, z.d_total);
    if (hipGetLastError() != hipSuccess) return -1;
    if (hipMemcpyAsync(z.h_total, z.d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, stream) != hipSuccess) return -1;
    if (hipEventRecord(z.ev_total, stream) != hipSuccess) return -1;
    if (hipEventSynchronize(z.ev_total) != hipSuccess) return -1;
    const uint64_t total = *z.h_total;
    if (total < (uint64_t)nblk || total > 0x7FFFFFF0ull / X_ENTRY) return -1;
    // every earlier launch on the scratch is done: ev_done was waited for on
    // `stream` ahead of ev_total
    if (!grow(&z.d_x, &z.x_cap, (size_t)total * X_ENTRY)) return -1;
    jfs_dev_block *xdesc = (jfs_dev_block *)z.d_x;
    int32_t *xwant = (int32_t *)(xdesc + total), *xret = xwant + total;
    hipLaunchKernelGGL(zseek_expand, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, stream, d_blocks, d_hi, nblk,
                       (const In *)z.d_in, (int32_t)total, xdesc, xwant);
    if (hipGetLastError() != hipSuccess) return -1;
    if (jfs_launch_zstd_decode_prefix(xdesc, (int)total, xret, xwant, stream) != 0) return -1;
    hipLaunchKernelGGL(zseek_fold, dim3((unsigned)nblk), dim3(64), 0, stream, (const In *)z.d_in, nblk,
                       (const jfs_dev_block *)xdesc, (const int32_t *)xret, d_ret);
    if (hipGetLastError() != hipSuccess) return -1;
    return hipEventRecord(z.ev_done, stream) == hipSuccess ? 0 : -1;
}

// The same sequence for fragments: scan -> offsets -> (the host wait) -> expand
// -> prefix decode of the list -> XXH64 of the decoded pieces -> fold
extern "C" int jfs_launch_zstd_decode_frames(const jfs_seek_frag *d_frags, const int32_t *d_lo, const int32_t *d_hi,
                                             int nblk, int32_t *d_ret, hipStream_t stream) {
    using namespace jfs::zseek;
    if (nblk <= 0) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return -1;
    Scratch &z = g_scr[dev];
    std::lock_guard<std::mutex> lk(z.mu);
    if (!z.d_total) {
        if (hipMalloc((void **)&z.d_total, sizeof(uint64_t)) != hipSuccess) return -1;
        if (hipHostMalloc((void **)&z.h_total, sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) return -1;
        if (hipEventCreateWithFlags(&z.ev_total, hipEventDisableTiming) != hipSuccess) return -1;
        if (hipEventCreateWithFlags(&z.ev_done, hipEventDisableTiming) != hipSuccess) return -1;
    }
    if ((size_t)nblk > z.in_cap) {
        if (hipEventSynchronize(z.ev_done) != hipSuccess) return -1;
        if (!grow(&z.d_in, &z.in_cap, (size_t)nblk)) return -1;
    }
    if (hipStreamWaitEvent(stream, z.ev_done, 0) != hipSuccess) return -1;
    hipLaunchKernelGGL(zframes_scan, dim3((unsigned)nblk), dim3(64), 0, stream, d_frags, d_lo, d_hi, nblk, z.d_in);
    hipLaunchKernelGGL(zseek_offsets, dim3(1), dim3(64), 0, stream, z.d_in, nblk, z.d_total);
    if (hipGetLastError() != hipSuccess) return -1;
    if (hipMemcpyAsync(z.h_total, z.d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, stream) != hipSuccess) return -1;
    if (hipEventRecord(z.ev_total, stream) != hipSuccess) return -1;
    if (hipEventSynchronize(z.ev_total) != hipSuccess) return -1;
    const uint64_t total = *z.h_total;
    if (total < (uint64_t)nblk || total > 0x7FFFFFF0ull / H_ENTRY) return -1;
    if (!grow(&z.d_x, &z.x_cap, (size_t)total * X_ENTRY)) return -1;
    if (!grow(&z.d_h, &z.h_cap, (size_t)total * H_ENTRY)) return -1;
    jfs_dev_block *xdesc = (jfs_dev_block *)z.d_x, *hdesc = (jfs_dev_block *)z.d_h;
    int32_t *xwant = (int32_t *)(xdesc + total), *xret = xwant + total;
    uint64_t *hash = (uint64_t *)(hdesc + total);
    uint32_t *expect = (uint32_t *)(hash + total);
    hipLaunchKernelGGL(zframes_expand, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, stream, d_frags, nblk,
                       (const In *)z.d_in, (int32_t)total, xdesc, xwant, hdesc, expect);
    if (hipGetLastError() != hipSuccess) return -1;
    if (jfs_launch_zstd_decode_prefix(xdesc, (int)total, xret, xwant, stream) != 0) return -1;
    if (jfs_launch_xxh64(hdesc, (int)total, hash, nullptr, stream) != 0) return -1;
    hipLaunchKernelGGL(zframes_fold, dim3((unsigned)nblk), dim3(64), 0, stream, (const In *)z.d_in, nblk,
                       (const jfs_dev_block *)xdesc, (const int32_t *)xret, (const jfs_dev_block *)hdesc,
                       (const uint64_t *)hash, (const uint32_t *)expect, d_ret);
    if (hipGetLastError() != hipSuccess) return -1;
    return hipEventRecord(z.ev_done, stream) == hipSuccess ? 0 : -1;
}

// And for lists of ranges: the sparse scan -> offsets -> (the host wait) ->
// sparse expand -> prefix decode of the list -> XXH64 of the decoded pieces
// (those of 12-byte tables) -> fold.  The scratch, its lock and ev_done are the
// two calls' above.
extern "C" int jfs_launch_zstd_decode_ranges(const jfs_dev_block *d_blocks, const int32_t *d_rng_first,
                                             const jfs_range *d_rng, int nblk, int32_t *d_ret, hipStream_t stream) {
    using namespace jfs::zseek;
    if (nblk <= 0) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return -1;
    Scratch &z = g_scr[dev];
    std::lock_guard<std::mutex> lk(z.mu);
    if (!z.d_total) {
        if (hipMalloc((void **)&z.d_total, sizeof(uint64_t)) != hipSuccess) return -1;
        if (hipHostMalloc((void **)&z.h_total, sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) return -1;
        if (hipEventCreateWithFlags(&z.ev_total, hipEventDisableTiming) != hipSuccess) return -1;
        if (hipEventCreateWithFlags(&z.ev_done, hipEventDisableTiming) != hipSuccess) return -1;
    }
    if ((size_t)nblk > z.in_cap || (size_t)nblk * sizeof(Rounds) > z.r_cap) {
        if (hipEventSynchronize(z.ev_done) != hipSuccess) return -1;
        if (!grow(&z.d_in, &z.in_cap, (size_t)nblk)) return -1;
        if (!grow(&z.d_r, &z.r_cap, (size_t)nblk * sizeof(Rounds))) return -1;
    }
    if (hipStreamWaitEvent(stream, z.ev_done, 0) != hipSuccess) return -1;
    hipLaunchKernelGGL(zsparse_scan, dim3((unsigned)nblk), dim3(64), 0, stream, d_blocks, d_rng_first, d_rng, nblk, z.d_in,
                       (Rounds *)z.d_r);
    hipLaunchKernelGGL(zseek_offsets, dim3(1), dim3(64), 0, stream, z.d_in, nblk, z.d_total);
    if (hipGetLastError() != hipSuccess) return -1;
    if (hipMemcpyAsync(z.h_total, z.d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, stream) != hipSuccess) return -1;
    if (hipEventRecord(z.ev_total, stream) != hipSuccess) return -1;
    if (hipEventSynchronize(z.ev_total) != hipSuccess) return -1;
    const uint64_t total = *z.h_total;
    if (total < (uint64_t)nblk || total > 0x7FFFFFF0ull / H_ENTRY) return -1;
    if (!grow(&z.d_x, &z.x_cap, (size_t)total * X_ENTRY)) return -1;
    if (!grow(&z.d_h, &z.h_cap, (size_t)total * H_ENTRY)) return -1;
    jfs_dev_block *xdesc = (jfs_dev_block *)z.d_x, *hdesc = (jfs_dev_block *)z.d_h;
    int32_t *xwant = (int32_t *)(xdesc + total), *xret = xwant + total;
    uint64_t *hash = (uint64_t *)(hdesc + total);
    uint32_t *expect = (uint32_t *)(hash + total);
    hipLaunchKernelGGL(zsparse_expand, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, stream, d_blocks, nblk,
                       (const In *)z.d_in, (const Rounds *)z.d_r, (int32_t)total, xdesc, xwant, hdesc, expect);
    if (hipGetLastError() != hipSuccess) return -1;
    if (jfs_launch_zstd_decode_prefix(xdesc, (int)total, xret, xwant, stream) != 0) return -1;
    if (jfs_launch_xxh64(hdesc, (int)total, hash, nullptr, stream) != 0) return -1;
    hipLaunchKernelGGL(zsparse_fold, dim3((unsigned)nblk), dim3(64), 0, stream, (const In *)z.d_in, nblk,
                       (const jfs_dev_block *)xdesc, (const int32_t *)xret, (const jfs_dev_block *)hdesc,
                       (const uint64_t *)hash, (const uint32_t *)expect, d_ret);
    if (hipGetLastError() != hipSuccess) return -1;
    return hipEventRecord(z.ev_done, stream) == hipSuccess ? 0 : -1;
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
