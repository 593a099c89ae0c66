// Host-only planning arithmetic of the batch pipeline (capi.hip run_batch):
// how a batch is cut into chunks, where each area of a chunk's staging lies,
// how a chunk's copies are cut into pieces, and the LZ4 small-batch grid sizes.
// Plain C++17 integer code -- no HIP, no environment, no globals -- so that
// tests/batch_plan_check.cc checks it on a CPU under ASan + UBSan.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/jfs_gpucodec.h"

namespace jfs_plan {

inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

// ---------------------------------------------------------------------------
// chunk planner
// ---------------------------------------------------------------------------
struct Block {
    int64_t in;   // staged input bytes (src_len)
    int64_t cap;  // staged output capacity
};

// blocks [s, e) on staging slot `slot`: tin / tout staged input / output bytes
struct Chunk {
    int s, e, slot;
    int64_t tin, tout;
};

struct PlanParams {
    int64_t limit;         // staging bytes (input + output) of a chunk
    int max_chunk_blocks;  // > 0: also caps a chunk's block count
    bool ramp_ok;          // the caller allows the decode ramp
    int ramp_len;          // number of small first chunks (0 = no ramp)
    int first_big;         // blocks in the first full chunk after the ramp (0: no cap)
    int nslot;             // chunk k uses slot k % nslot
};

struct Plan {
    std::vector<Chunk> ch;
    std::vector<int64_t> in_off, out_off;  // per block, from the start of its chunk's input / output area
};

// append block i (= c.e) to the chunk
inline void place(const Block *b, Chunk &c, Plan &pl) {
    pl.in_off[c.e] = c.tin;
    pl.out_off[c.e] = c.tout;
    c.tin += align16(b[c.e].in);
    c.tout += align16(b[c.e].cap);
    c.e++;
}

// Cut blocks [0, n) into chunks, in order.  A chunk takes blocks while it
// stays within `limit` staging bytes and its block cap; a block larger than
// the limit rides alone.
// Decode ramp (ramp_ok, for batches of more than two chunks' bytes): the first
// output cannot leave before chunk 0's H2D and kernel are done, and the
// one-workgroup-per-block kernels take a block's whole latency (~20 ms)
// whatever the chunk size; so a long decode starts with chunks of 32, 64 and
// 128 blocks (the small-batch kernels) that put the D2H stream to work while
// the first full chunk is staged and decoded, and ends with a chunk of at most
// 128 blocks so that little copy-out is left after the last D2H.  Measured on
// 2,048 x 4 MiB LZ4 (scripts/hostpath.py): no ramp 34.9-36.5 GiB/s,
// 3 ramp chunks 39.7-40.0, 5: 37.5, 7: 36.5.
inline Plan plan_chunks(const Block *b, int n, const PlanParams &p) {
    Plan pl;
    pl.in_off.resize(n > 0 ? n : 0);
    pl.out_off.resize(n > 0 ? n : 0);
    int64_t total = 0;
    for (int i = 0; i < n; i++) total += align16(b[i].in) + align16(b[i].cap);
    const bool ramp = p.ramp_ok && p.ramp_len > 0 && total > 2 * p.limit;
    auto next_chunk = [&](int s) { return Chunk{s, s, (int)(pl.ch.size() % p.nslot), 0, 0}; };
    for (int s = 0; s < n;) {
        Chunk c = next_chunk(s);
        const int k = (int)pl.ch.size();
        // (the first full chunk's H2D and one-block kernel latency are on
        // the critical path: a smaller one reaches the D2H stream sooner)
        int cap_blocks = ramp && k < p.ramp_len ? std::min(32 << k, 128) : p.max_chunk_blocks;
        if (p.first_big > 0 && ramp && k == p.ramp_len) cap_blocks = p.first_big;
        while (c.e < n) {
            const int64_t add = align16(b[c.e].in) + align16(b[c.e].cap);
            if (c.e > s && (c.tin + c.tout + add > p.limit || (cap_blocks > 0 && c.e - s >= cap_blocks))) break;
            place(b, c, pl);
        }
        pl.ch.push_back(c);
        s = c.e;
    }
    if (ramp && pl.ch.size() > 4 && pl.ch.back().e - pl.ch.back().s > 128) {  // ramp down: split the last chunk
        const Chunk last = pl.ch.back();
        pl.ch.pop_back();
        auto lay_out = [&](int s, int e) {
            Chunk c = next_chunk(s);
            while (c.e < e) place(b, c, pl);
            pl.ch.push_back(c);
        };
        lay_out(last.s, last.e - 128);
        lay_out(last.e - 128, last.e);
    }
    return pl;
}

// ---------------------------------------------------------------------------
// staging layout of one chunk
// ---------------------------------------------------------------------------
// in | out | desc | ret | zinfo | aead (descriptors, results, key+nonce slots)
// | crc (descriptors, seeds, results) | csum (descriptors, checksum bytes):
// byte offsets from the slot's base, the same in the pinned and the HBM copy.
// An absent area has no bytes and sits where the next one starts.
struct ChunkLayout {
    int64_t in, out, desc, ret, zinfo;
    int64_t aead_desc, aead_ret, aead_kn;
    int64_t crc_desc, crc_seed, crc;
    int64_t csum_desc, csum;
    int64_t aead_bytes, csum_bytes;  // the whole aead area; the checksum bytes
    int64_t total;

    // nb blocks; zib: Zstd plan bytes per block (0: none); csum_area_bytes:
    // the chunk's checksum bytes (has_csum)
    ChunkLayout(int64_t nb, int64_t tin, int64_t tout, int64_t zib, bool has_aead, bool has_crc, bool has_csum,
                int64_t csum_area_bytes) {
        int64_t o = 0;
        auto take = [&o](bool present, int64_t bytes) {
            const int64_t at = o;
            if (present) o += align16(bytes);
            return at;
        };
        const int64_t nd = nb * (int64_t)sizeof(jfs_dev_block);
        in = take(true, tin);
        out = take(true, tout);
        desc = take(true, nd);
        ret = take(true, nb * 4);
        zinfo = take(true, nb * zib);
        aead_desc = take(has_aead, nb * (int64_t)sizeof(jfs_aead_block));
        aead_ret = take(has_aead, nb * 4);
        aead_kn = take(has_aead, nb * 64);  // 64 bytes per block: key (32) + nonce (12)
        aead_bytes = o - aead_desc;
        crc_desc = take(has_crc, nd);
        crc_seed = take(has_crc, nb * 4);
        crc = take(has_crc, nb * 4);
        csum_desc = take(has_csum, nd);
        csum = take(has_csum, csum_area_bytes);
        csum_bytes = o - csum;
        total = o;
    }
    // the area at byte offset `off` of a slot's pinned (sl.h) or HBM (sl.d) copy
    template <class T = uint8_t>
    static T *at(uint8_t *base, int64_t off) {
        return (T *)(base + off);
    }
};

// ---------------------------------------------------------------------------
// copy pieces of a chunk
// ---------------------------------------------------------------------------
// Output pieces: large chunks go in block ranges [piece_b(c, p), piece_b(c, p + 1));
// a one-block chunk (a lone cache miss) in byte ranges of the output area
// (byte_npiece), so that the copy-out of one piece overlaps the D2H of the
// next; other small chunks (the coalescer's 16-block ones) stay whole: a
// piece's host copy is a thread-pool round of its own.  piece_o(c, p) = the
// piece's first byte.  Input staging pieces: block ranges of large chunks only.
struct Pieces {
    int max_npiece;   // NPIECE
    int byte_npiece;  // pieces of a one-block chunk's output (0 or 1: whole)

    bool byte_pieces(const Chunk &c) const { return byte_npiece > 1 && c.e - c.s == 1; }
    int in_npiece(const Chunk &c) const { return c.e - c.s >= 64 ? std::min(max_npiece, c.e - c.s) : 1; }
    int in_piece_b(const Chunk &c, int p) const { return c.s + (int)((int64_t)(c.e - c.s) * p / in_npiece(c)); }
    int npiece(const Chunk &c) const { return byte_pieces(c) ? byte_npiece : in_npiece(c); }
    int piece_b(const Chunk &c, int p) const {
        return byte_pieces(c) ? c.s : c.s + (int)((int64_t)(c.e - c.s) * p / npiece(c));
    }
    int64_t piece_o(const Chunk &c, int p, const int64_t *out_off) const {
        const int np = npiece(c);
        if (p >= np) return c.tout;
        if (byte_pieces(c)) return (c.tout * p / np) & ~(int64_t)15;
        const int b = piece_b(c, p);
        return b < c.e ? out_off[b] : c.tout;
    }
};

// ---------------------------------------------------------------------------
// LZ4 small-batch decode (lz4_split.hip) grid sizes
// ---------------------------------------------------------------------------
constexpr int LZ4_SPLIT_SEG = 256;  // = JFS_LZ4_SPLIT_SEG (jfs_internal.h)

struct Lz4SplitGeom {
    int64_t nseg;     // input segments of all blocks
    int64_t max_cap;  // largest dst_cap
    int64_t norg;     // origin entries: every capacity rounded up to 4
};

inline Lz4SplitGeom lz4_split_geom(int n, const int32_t *lens, const int32_t *caps) {
    Lz4SplitGeom g{0, 0, 0};
    for (int k = 0; k < n; k++) {
        g.nseg += (std::max<int64_t>(lens[k], 0) + LZ4_SPLIT_SEG - 1) / LZ4_SPLIT_SEG;
        g.max_cap = std::max<int64_t>(g.max_cap, caps[k]);
        g.norg += (std::max<int64_t>(caps[k], 0) + 3) & ~3ll;
    }
    return g;
}

}  // namespace jfs_plan
