// The Zstd decoder's frame / block walk (RFC 8878; ZSTD_decompressMultiFrame +
// ZSTD_decompressFrame order) and the header scan that sizes an input's
// scratch.  Every stage of zstd_decode.hip walks its input through this one
// Walk, so they all stop at the same block without talking to each other.
// Host and device; also compiles with a plain C++ compiler (tests/zstd_walk_check.cc).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "jfs_internal.h"
#define JFS_ZW_FN __host__ __device__ __forceinline__
#define JFS_ZW_INLINE __host__ __device__ inline
#else
typedef const uint8_t gc_u8;
#define JFS_ZW_FN inline
#define JFS_ZW_INLINE inline
#endif

namespace jfs {
namespace zstdd {

enum { E_CORRUPT = -1, E_DSTSMALL = -2, E_SRCSIZE = -3, E_SCRATCH = -4, E_BUG = -100 };
enum { FE_FCS = 1, FE_CHECK = 2, FE_MISSING = 4 };
constexpr uint32_t ZSTD_MAGIC = 0xFD2FB528u;
constexpr int32_t BLOCK_MAX = 128 << 10;

// per-input bookkeeping
struct ZInfo {
    uint64_t item_off;      // first item (host scan)
    uint64_t lit_off;       // first literal byte (host scan)
    uint64_t tab_off;       // first FSE table cell (host scan)
    uint32_t n_items;       // zscan: capacity; zseq: items written
    uint32_t lit_bytes;     // zscan: capacity
    uint32_t n_cblk;        // zscan: compressed blocks (TAB_CELLS table cells each)
    uint32_t lit_err_blk;   // zlit: ordinal of the block whose literals failed
    int32_t lit_err_code;
    uint32_t ovf;           // zplan: the scratch cannot hold this input (ret = E_SCRATCH)
    uint32_t n_sblk;        // zseqa: compressed blocks described (ZDesc after each table area)
    uint32_t n_blk;         // zscan: blocks of every type (small-batch path: one record each)
    int32_t cap;            // zscan: the input's dst_cap
    uint32_t want_st;       // zscan (prefix decode, host plans): want, 0 .. INT32_MAX | the walk stopped << 31
};
static_assert(sizeof(ZInfo) == 64, "ZInfo is 64 bytes (jfs_zstd_info_bytes)");
JFS_ZW_FN int32_t zinfo_want(const ZInfo &z) { return (int32_t)(z.want_st & 0x7FFFFFFFu); }
JFS_ZW_FN int zinfo_stopped(const ZInfo &z) { return (int)(z.want_st >> 31); }

// where a prefix decode of an input stops: want <= 0 stops in front of the
// first block, want above dst_cap acts as dst_cap
JFS_ZW_FN int32_t want_clamp(int32_t want, int32_t cap) {
    const int32_t w = want < cap ? want : cap;
    return w > 0 ? w : 0;
}

JFS_ZW_FN uint32_t rd8(const gc_u8 *s, int32_t p) { return s[p]; }
JFS_ZW_FN uint32_t rd16(const gc_u8 *s, int32_t p) { return s[p] | (s[p + 1] << 8); }
JFS_ZW_FN uint32_t rd24(const gc_u8 *s, int32_t p) { return rd16(s, p) | (s[p + 2] << 16); }
JFS_ZW_FN uint32_t rd32(const gc_u8 *s, int32_t p) { return rd16(s, p) | (rd16(s, p + 2) << 16); }

// ---------------------------------------------------------------------------
// frame / block walk (ZSTD_decompressMultiFrame + ZSTD_decompressFrame order)
// ---------------------------------------------------------------------------
enum { EV_DONE = 0, EV_ERROR, EV_FSTART, EV_FEND, EV_BLOCK };

struct Walk {
    const gc_u8 *s;
    int32_t n, p;
    int32_t cap;       // dst capacity (stop rule)
    int32_t want;      // output bytes that are enough (stop rule; INT32_MAX: all)
    int64_t lb;        // lower bound of the output produced so far
    int32_t phase;     // 0 between frames, 1 in a frame, 2 finished
    int32_t frames_done, after_last;
    int32_t check, has_fcs;
    int32_t stopped;   // the walk ended at lb >= want, in front of a block header
    uint64_t fcs;
    uint32_t ordinal;  // blocks seen
    // current block
    int32_t btype, bsize, bpos;
};

JFS_ZW_FN void walk_init(Walk &w, const gc_u8 *s, int32_t n, int32_t cap, int32_t want) {
    w.s = s; w.n = n; w.p = 0; w.cap = cap; w.lb = 0; w.phase = 0; w.frames_done = 0; w.after_last = 0;
    w.check = 0; w.has_fcs = 0; w.fcs = 0; w.ordinal = 0; w.btype = 0; w.bsize = 0; w.bpos = 0;
    w.want = want; w.stopped = 0;
}

// Next event.  *err for EV_ERROR; for EV_FEND *flags/*chk describe the frame end.
// STOP = false compiles the `want` rule out: the full decoder's kernels pass
// INT32_MAX, which the rule could only meet where `lb > cap` ends the walk too.
template <bool STOP = true>
JFS_ZW_FN int walk_next(Walk &w, int32_t *err, uint32_t *flags, uint32_t *chk) {
    const gc_u8 *s = w.s;
    if (w.phase == 2) return EV_DONE;
    if (w.phase == 1 && w.after_last) {
        w.after_last = 0;
        uint32_t f = (w.has_fcs ? FE_FCS : 0) | (w.check ? FE_CHECK : 0);
        *chk = 0;
        if (w.check) {
            if (w.n - w.p < 4) { f |= FE_MISSING; w.phase = 2; }
            else { *chk = rd32(s, w.p); w.p += 4; w.phase = 0; }
        } else {
            w.phase = 0;
        }
        w.frames_done = 1;
        *flags = f;
        return EV_FEND;
    }
    if (w.phase == 1) {
        // enough output lies behind: the blocks from here on are not decoded
        if (STOP && w.lb >= (int64_t)w.want) { w.stopped = 1; w.phase = 2; return EV_DONE; }
        if (w.lb > (int64_t)w.cap) { w.phase = 2; return EV_DONE; }  // zexec fails inside the last block
        if (w.n - w.p < 3) { *err = E_SRCSIZE; w.phase = 2; return EV_ERROR; }
        uint32_t bh = rd24(s, w.p);
        w.p += 3;
        int32_t btype = (bh >> 1) & 3, bsize = (int32_t)(bh >> 3);
        if (btype == 3) { *err = E_CORRUPT; w.phase = 2; return EV_ERROR; }
        int32_t csize = btype == 1 ? 1 : bsize;
        if (csize > w.n - w.p) { *err = E_SRCSIZE; w.phase = 2; return EV_ERROR; }
        if (btype == 2 && bsize >= BLOCK_MAX) { *err = E_SRCSIZE; w.phase = 2; return EV_ERROR; }
        w.btype = btype; w.bsize = bsize; w.bpos = w.p;
        w.p += csize;
        w.after_last = bh & 1;
        w.ordinal++;
        return EV_BLOCK;
    }
    // between frames
    for (;;) {
        int32_t rem = w.n - w.p;
        if (rem < 5) {
            w.phase = 2;
            if (rem > 0) { *err = E_SRCSIZE; return EV_ERROR; }
            return EV_DONE;
        }
        uint32_t magic = rd32(s, w.p);
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
            if (rem < 8) { *err = E_SRCSIZE; w.phase = 2; return EV_ERROR; }
            uint32_t sz = rd32(s, w.p + 4);
            if ((uint32_t)(rem - 8) < sz) { *err = E_SRCSIZE; w.phase = 2; return EV_ERROR; }
            w.p += 8 + (int32_t)sz;
            continue;
        }
        if (rem < 9) { *err = E_SRCSIZE; w.phase = 2; return EV_ERROR; }
        uint32_t fhd = rd8(s, w.p + 4);
        int32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, did = fhd & 3;
        int32_t did_size = did == 0 ? 0 : did == 1 ? 1 : did == 2 ? 2 : 4;
        int32_t fcs_size = fcs_flag == 0 ? (single ? 1 : 0) : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8;
        int32_t fhs = 5 + (single ? 0 : 1) + did_size + fcs_size;
        if (rem < fhs + 3) { *err = E_SRCSIZE; w.phase = 2; return EV_ERROR; }
        if (magic != ZSTD_MAGIC) { *err = w.frames_done ? E_SRCSIZE : E_CORRUPT; w.phase = 2; return EV_ERROR; }
        if (fhd & 8) { *err = E_CORRUPT; w.phase = 2; return EV_ERROR; }
        int32_t q = w.p + 5;
        if (!single) {
            if ((rd8(s, q) >> 3) + 10 > 31) { *err = E_CORRUPT; w.phase = 2; return EV_ERROR; }
            q++;
        }
        if (did) {
            uint32_t id = 0;
            for (int i = 0; i < did_size; i++) id |= rd8(s, q + i) << (8 * i);
            q += did_size;
            if (id != 0) { *err = E_CORRUPT; w.phase = 2; return EV_ERROR; }
        }
        w.has_fcs = fcs_size != 0;
        uint64_t v = 0;
        for (int i = 0; i < fcs_size; i++) v |= (uint64_t)rd8(s, q + i) << (8 * i);
        if (fcs_size == 2) v += 256;
        w.fcs = v;
        q += fcs_size;
        w.check = (fhd >> 2) & 1;
        w.p = q;
        w.phase = 1;
        w.after_last = 0;
        return EV_FSTART;
    }
}

// Literal section header (ZSTD_decodeLiteralsBlock size logic).  Returns 0 or
// an error; *sec = total bytes of the literal section.
struct LitHdr {
    int32_t type, regen, csize, hsz, streams, sec;
};
JFS_ZW_FN int32_t lit_header(const gc_u8 *s, int32_t bpos, int32_t bsize, LitHdr &h) {
    if (bsize < 3) return E_CORRUPT;  // MIN_CBLOCK_SIZE
    uint32_t b0 = rd8(s, bpos);
    h.type = b0 & 3;
    int32_t sf = (b0 >> 2) & 3;
    h.streams = 1;
    h.csize = 0;
    if (h.type <= 1) {
        if (sf == 0 || sf == 2) { h.regen = b0 >> 3; h.hsz = 1; }
        else if (sf == 1) { h.regen = rd16(s, bpos) >> 4; h.hsz = 2; }
        else { h.regen = rd24(s, bpos) >> 4; h.hsz = 3; }
        if (h.type == 0) {
            if (h.hsz + h.regen > bsize) return E_CORRUPT;
            h.sec = h.hsz + h.regen;
        } else {
            if (h.hsz + 1 > bsize) return E_CORRUPT;
            if (h.regen > BLOCK_MAX) return E_CORRUPT;
            h.sec = h.hsz + 1;
        }
        return 0;
    }
    if (bsize < 5) return E_CORRUPT;
    uint32_t lhc = rd32(s, bpos);
    if (sf <= 1) {
        h.hsz = 3; h.streams = sf == 0 ? 1 : 4;
        h.regen = (lhc >> 4) & 0x3FF; h.csize = (lhc >> 14) & 0x3FF;
    } else if (sf == 2) {
        h.hsz = 4; h.streams = 4;
        h.regen = (lhc >> 4) & 0x3FFF; h.csize = lhc >> 18;
    } else {
        h.hsz = 5; h.streams = 4;
        h.regen = (lhc >> 4) & 0x3FFFF; h.csize = (lhc >> 22) + (rd8(s, bpos + 4) << 10);
    }
    if (h.regen > BLOCK_MAX) return E_CORRUPT;
    if (h.csize + h.hsz > bsize) return E_CORRUPT;
    h.sec = h.hsz + h.csize;
    return 0;
}

// nbSeq field (ZSTD_decodeSeqHeaders prefix).  Returns 0 or error; *nseq, *used.
JFS_ZW_FN int32_t nbseq_header(const gc_u8 *s, int32_t ip, int32_t end, int32_t *nseq, int32_t *used) {
    if (ip >= end) return E_SRCSIZE;
    int32_t v = (int32_t)rd8(s, ip);
    int32_t u = 1;
    if (v >= 128) {
        if (v == 255) {
            if (ip + 3 > end) return E_SRCSIZE;
            v = (int32_t)rd16(s, ip + 1) + 0x7F00;
            u = 3;
        } else {
            if (ip + 2 > end) return E_SRCSIZE;
            v = ((v - 128) << 8) + (int32_t)rd8(s, ip + 1);
            u = 2;
        }
    }
    *nseq = v;
    *used = u;
    if (v == 0 && ip + u != end) return E_SRCSIZE;
    return 0;
}

// ---------------------------------------------------------------------------
// header scan -> scratch sizes
// ---------------------------------------------------------------------------
// Scratch one input needs (exact): items, literal bytes, compressed blocks.
// Host and device: run_batch plans from the host copy of its inputs.
// STOP: the scan ends where a decode that needs `want` output bytes ends, and
// records want and whether the rule fired (else `want` is not looked at).
template <bool STOP = true>
JFS_ZW_INLINE void zscan_one(const gc_u8 *src, int32_t n, int32_t cap, int32_t want, ZInfo &out) {
    Walk w;
    walk_init(w, src, n, cap, want);
    uint64_t items = 0, lits = 0;
    uint32_t cblk = 0;
    for (;;) {
        int32_t err = 0;
        uint32_t fl = 0, chk = 0;
        int ev = walk_next<STOP>(w, &err, &fl, &chk);
        if (ev == EV_DONE) break;
        items++;  // FSTART / FEND / ERROR / BSTART
        if (ev == EV_ERROR) break;
        if (ev == EV_FEND && (fl & FE_MISSING)) break;
        if (ev != EV_BLOCK) continue;
        items++;  // BEND or ERR
        if (w.btype != 2) {
            items++;  // one literal-only item
            int64_t room = (int64_t)w.cap - w.lb;
            if ((int64_t)w.bsize <= room) lits += w.bsize;  // bytes past cap are never read
            w.lb += w.bsize;
            continue;
        }
        LitHdr h;
        if (lit_header(w.s, w.bpos, w.bsize, h)) break;
        lits += (uint64_t)h.regen + (h.type >= 2 ? 4 : 0);  // 4-stream segments may overhang by <= 3
        int32_t nseq = 0, used = 0;
        if (nbseq_header(w.s, w.bpos + h.sec, w.bpos + w.bsize, &nseq, &used)) break;
        items += (uint64_t)nseq + 1;  // sequences + BREP
        cblk++;
        w.lb += (int64_t)h.regen + 3 * (int64_t)nseq;
    }
    out.n_items = (uint32_t)(items + 1);
    out.lit_bytes = (uint32_t)(lits + 16);
    out.n_cblk = cblk;
    out.n_blk = w.ordinal;
    out.cap = cap;
    if (STOP) out.want_st = ((uint32_t)want & 0x7FFFFFFFu) | ((uint32_t)w.stopped << 31);
}

}  // namespace zstdd
}  // namespace jfs
