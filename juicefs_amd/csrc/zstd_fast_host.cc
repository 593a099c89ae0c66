// Host twin of the fast Zstd parse: plain C++, no GPU.  It restates
// zfast_parse and zfast_seq of zstd_fast.hip tile by tile and produces the same
// sequence records, so the parse can be tested without a device and the kernels
// can be pinned record for record with one.  Test infrastructure only: no
// product entry point calls it.
#include <string.h>

#include <vector>

#include "../../include/jfs_gpucodec_zstd_fast_test.h"
#include "zstd_fast.h"

namespace {
using namespace jfs::zfast;

struct Rec {
    uint32_t lit, mlen, off;  // literals since the chunk's previous match
};

inline uint32_t ld32(const uint8_t *p) {
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

inline int64_t match_len(const uint8_t *c, int64_t p, int64_t cand, int64_t lim) {
    int64_t len = kMinMatch;
    while (p + len < lim && c[cand + len] == c[p + len]) ++len;
    return len;
}

// One chunk c[0, clen): appends its matches and returns the trailing literals.
// A match starts at or after the chunk's first byte and may end at its last.
int32_t parse_chunk(const uint8_t *c, int32_t clen, std::vector<Rec> &out) {
    std::vector<uint16_t> tab((size_t)1 << kHashLog, 0);
    const int64_t slim = (int64_t)clen - kMinMatch;  // last position with 4 readable bytes
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
            const int64_t len = match_len(c, p, cand[l], clen);
            out.push_back({(uint32_t)(p - anchor), (uint32_t)len, (uint32_t)(p - cand[l])});
            anchor = cur = p + len;
        }
        // insert: the highest position of the tile wins a table entry
        for (int l = 0; l < kTile; ++l)
            if (act[l]) tab[h[l]] = (uint16_t)(t0 + l);
        t0 = t0 + kTile > cur ? t0 + kTile : cur;
    }
    return (int32_t)(clen - anchor);
}
}  // namespace

extern "C" int64_t jfs_test_zstd_fast_host_seqs(const uint8_t *src, int64_t n, uint64_t *out_u64, int64_t cap,
                                                int32_t *ns_per_block, int32_t *nl_per_block) {
    if (n < 0 || n > 0x7FFFFF00ll || cap < 0) return -1;
    std::vector<uint64_t> seqs;
    std::vector<int32_t> ns, nl;
    for (int64_t bs = 0; bs < n; bs += kBlock) {
        const int32_t bsz = (int32_t)(n - bs < kBlock ? n - bs : kBlock);
        if (bsz < kNoCompBelow) {  // F_NOCOMP
            ns.push_back(0);
            nl.push_back(bsz);
            continue;
        }
        RepHist hist;
        hist.start(bs == 0);
        uint32_t carry = 0, lits = 0;
        int32_t count = 0;
        for (int32_t cb = 0; cb < bsz; cb += kChunk) {
            std::vector<Rec> recs;
            const int32_t tail = parse_chunk(src + bs + cb, bsz - cb < kChunk ? bsz - cb : kChunk, recs);
            for (const Rec &r : recs) {
                // the literals a chunk leaves over join the next chunk's first sequence
                const uint32_t ll = r.lit + carry;
                carry = 0;
                seqs.push_back(seq_rec(ll, r.mlen, hist.code(ll, r.off)));
                lits += ll;
                ++count;
            }
            carry += (uint32_t)tail;
        }
        ns.push_back(count);
        nl.push_back((int32_t)(lits + carry));  // a block's trailing literals stay in the block
    }
    if ((int64_t)seqs.size() > cap) return -1;
    if (!seqs.empty()) memcpy(out_u64, seqs.data(), seqs.size() * sizeof(uint64_t));
    if (!ns.empty()) {
        memcpy(ns_per_block, ns.data(), ns.size() * sizeof(int32_t));
        memcpy(nl_per_block, nl.data(), nl.size() * sizeof(int32_t));
    }
    return (int64_t)seqs.size();
}
