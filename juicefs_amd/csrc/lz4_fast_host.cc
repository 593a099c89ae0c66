// Host twin of the fast LZ4 encoder: plain C++, no GPU.  It restates
// the kernels of lz4_fast.hip tile by tile and produces the same bytes, so the
// parse can be tested without a device and the kernels can be pinned byte for
// byte with one.  Test infrastructure only: no product entry point calls it.
#include <string.h>

#include <vector>

#include "../../include/jfs_gpucodec_lz4_fast_test.h"
#include "lz4_fast.h"
#include "lz4_lift.h"

namespace {
using namespace jfs::lz4f;

struct Rec {
    int64_t lit;  // literals before the match (carry from earlier chunks included)
    int32_t mlen, off;
};

inline uint32_t ld32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

// One chunk: c[0, clen) at block position cbase of an n-byte block.  Appends its
// sequences to out (the first one takes `carry` literals more) and returns the
// count of trailing literals.
int64_t parse_chunk(const uint8_t *c, int64_t n, int64_t cbase, int64_t clen, int64_t carry, std::vector<Rec> &out) {
    std::vector<uint16_t> tab((size_t)1 << kHashLog, 0);
    // block end rules, in chunk coordinates: matches end at or before mend and
    // start at or before slim (4 readable bytes inside the chunk, too)
    const int64_t mend = clen < n - kLastLits - cbase ? clen : n - kLastLits - cbase;
    const int64_t slim = clen - kMinMatch < n - kMfLimit - cbase ? clen - kMinMatch : n - kMfLimit - cbase;
    int64_t anchor = 0, cur = 0;
    for (int64_t t0 = 0; t0 <= slim;) {
        uint32_t h[kTile];
        int64_t cand[kTile];
        bool act[kTile];
        // every position of the tile looks up the table as the tiles before it left it
        for (int l = 0; l < kTile; ++l) {
            const int64_t p = t0 + l;
            act[l] = p <= slim;
            cand[l] = -1;
            if (!act[l]) continue;
            const uint32_t v = ld32(c + p);
            h[l] = hash4(v);
            if (p >= kNear)
                for (int k = 1; k <= kNear && cand[l] < 0; ++k)
                    if (ld32(c + p - k) == v) cand[l] = p - k;
            if (cand[l] < 0) {
                const int64_t e = tab[h[l]];
                if (e < p && ld32(c + e) == v) cand[l] = e;
            }
        }
        // greedy choice in position order
        for (int l = 0; l < kTile; ++l) {
            const int64_t p = t0 + l;
            if (!act[l] || cand[l] < 0 || p < cur) continue;
            int64_t len = kMinMatch;
            while (p + len < mend && c[cand[l] + len] == c[p + len]) ++len;
            out.push_back({p - anchor + carry, (int32_t)len, (int32_t)(p - cand[l])});
            carry = 0;
            anchor = cur = p + len;
        }
        // insert: the highest position of the tile wins a table entry
        for (int l = 0; l < kTile; ++l)
            if (act[l]) tab[h[l]] = (uint16_t)(t0 + l);
        t0 = t0 + kTile > cur ? t0 + kTile : cur;
    }
    return clen - anchor + carry;
}

uint8_t *put_len(uint8_t *o, int64_t v) {  // v = length - 15 already checked >= 0
    for (; v >= 255; v -= 255) *o++ = 255;
    *o++ = (uint8_t)v;
    return o;
}

// The block of the sequences recs over src and `carry` trailing literals (stitch
// and emit): its size, or 0 and not a byte when it does not fit dst_cap.
// (the records may be lifted ones: jfs_test_lz4_fast_lift_host below.)
int64_t emit_block(uint8_t *dst, int64_t dst_cap, const uint8_t *src, const std::vector<Rec> &recs, int64_t carry) {
    int64_t total = 1 + len_bytes(carry) + carry;
    for (const Rec &r : recs) total += 1 + len_bytes(r.lit) + r.lit + 2 + len_bytes(r.mlen - kMinMatch);
    if (total > dst_cap) return 0;
    uint8_t *o = dst;
    const uint8_t *ip = src;
    for (const Rec &r : recs) {
        const int32_t ml = r.mlen - kMinMatch;
        *o++ = (uint8_t)((r.lit >= 15 ? 15 : (int)r.lit) << 4 | (ml >= 15 ? 15 : ml));
        if (r.lit >= 15) o = put_len(o, r.lit - 15);
        memcpy(o, ip, (size_t)r.lit);
        o += r.lit;
        ip += r.lit + r.mlen;
        *o++ = (uint8_t)(r.off & 255);
        *o++ = (uint8_t)(r.off >> 8);
        if (ml >= 15) o = put_len(o, ml - 15);
    }
    *o++ = (uint8_t)((carry >= 15 ? 15 : (int)carry) << 4);
    if (carry >= 15) o = put_len(o, carry - 15);
    if (carry) memcpy(o, ip, (size_t)carry);
    o += carry;
    return o - dst == total ? total : 0;
}
}  // namespace

extern "C" int64_t jfs_test_lz4_fast_host(uint8_t *dst, int64_t dst_cap, const uint8_t *src, int64_t n) {
    if (n < 0 || n > kMaxInput || dst_cap < 0) return 0;
    std::vector<Rec> recs;
    int64_t carry = 0;
    for (int64_t cbase = 0; cbase < n; cbase += kChunk) {
        const int64_t clen = n - cbase < kChunk ? n - cbase : kChunk;
        carry = parse_chunk(src + cbase, n, cbase, clen, carry, recs);
    }
    return emit_block(dst, dst_cap, src, recs, carry);
}

// The lift form (lz4_lift.h): a chunk the lift takes contributes the
// records lift_host reads from its source's stored stream, as stitch joins them
// to the chunks around it; every other chunk is parsed.
extern "C" int64_t jfs_test_lz4_fast_lift_host(uint8_t *dst, int64_t dst_cap, const uint8_t *src, int64_t n,
                                               const int32_t *lift, int nsrc, const uint8_t *const *stream,
                                               const int32_t *stream_len, const int32_t *src_cap, int32_t *lifted,
                                               int32_t *chunk_nrec) {
    namespace lz4l = jfs::lz4l;
    if (lifted) *lifted = 0;
    if (n < 0 || n > kMaxInput || dst_cap < 0) return 0;
    std::vector<Rec> recs;
    int64_t carry = 0;
    int32_t count = 0;
    for (int64_t cbase = 0; cbase < n; cbase += kChunk) {
        const int64_t clen = n - cbase < kChunk ? n - cbase : kChunk, j = cbase >> kChunkLog;
        const int32_t s = lift[2 * j], i = lift[2 * j + 1];
        bool take = lz4l::interior(j, n) && s >= 0 && s < nsrc && lz4l::interior(i, src_cap[s]) && stream_len[s] >= 0;
        if (take) {
            const lz4l::Lifted r = lz4l::lift_host(stream[s], stream_len[s], i);
            take = r.ok && r.total <= src_cap[s];
            // what stitch does with a chunk's results
            for (int32_t k = 0; take && k < r.nrec; k++)
                recs.push_back({(int64_t)(r.y[k] >> 16) + (k ? 0 : carry), (int32_t)(r.x[k] >> 16), (int32_t)(r.y[k] & 0xffff)});
            if (take) carry = r.nrec ? r.tail : carry + r.tail;
            if (take && chunk_nrec) chunk_nrec[j] = r.nrec;
            count += take;
        }
        if (!take) {
            carry = parse_chunk(src + cbase, n, cbase, clen, carry, recs);
            if (chunk_nrec) chunk_nrec[j] = -1;
        }
    }
    if (lifted) *lifted = count;
    return emit_block(dst, dst_cap, src, recs, carry);
}
