// Host-only planning of the on-device chain calls (capi_chain.hip compact_run and
// read_run): which sources the host answers, where each area of a call's
// staging lies, and what the plan asks of every source.  Plain C++17 integer
// code -- no HIP, no environment, no globals -- so that
// tests/chain_plan_check.cc checks it on a CPU under ASan + UBSan.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/jfs_gpucodec.h"
#include "batch_plan.h"

namespace jfs_plan {

// One stored object the device works on (the others were answered on the
// host); idx = its position in the caller's arrays.  Bytes [off, off + pay) of
// it are staged: the whole object, or the sealed payload (ciphertext || tag)
// of an envelope whose 12-byte nonce lies at noff; off = noff = 0 without a
// cipher.  check: an expected CRC-32C came with it (reads only).
struct ChainSrc {
    int idx;
    int64_t off, noff, pay;
    int64_t cap;  // staged decode capacity
    bool check;
    uint32_t expect;
};

// One output the device works on.  total = gathered bytes; area = bytes of its
// part of the output area (a read: total; a compacted block: the encoder's
// capacity, + 16 for the tag of a sealed one); cap = encoder capacity; hdr =
// envelope header bytes, which the host writes.
struct ChainOut {
    int idx;
    int64_t total, area, cap, hdr;
};

// encrypt.go Decrypt's header checks: [klen:2 | nlen:1 | wrapped key | nonce |
// payload].  Returns the payload's offset, or JFS_ERR_CORRUPT.
inline int64_t envelope_parse(const uint8_t *src, int64_t n, int64_t *woff, int64_t *wlen, int64_t *noff,
                              int64_t *nlen) {
    if (!src || n < 3) return JFS_ERR_CORRUPT;  // "received encrypted text length is less than 3"
    const int64_t kl = ((int64_t)src[0] << 8) + src[1], nl = src[2];
    if (3 + kl + nl >= n) return JFS_ERR_CORRUPT;  // "malformed ciphertext"
    if (woff) *woff = 3;
    if (wlen) *wlen = kl;
    if (noff) *noff = 3 + kl;
    if (nlen) *nlen = nl;
    return 3 + kl + nl;
}

// What the Go adapters answer for stored object v before a codec or a cipher
// runs: pre_answer's rules without a cipher ("none" decodes by copying, here
// without the copy), jfs_open_decompress_batch's with one.  Returns JFS_OK with
// r.off / r.noff / r.pay set when the device has to run, else the answer with
// r describing the whole object (as staged for a checksum).  r.cap is the
// caller's to set.
inline int64_t chain_src_answer(int algo, bool sealed, const jfs_iov &v, ChainSrc &r) {
    r.off = r.noff = 0;
    r.pay = v.src_len;
    if (!sealed) {
        if (algo == JFS_ALGO_NONE) return v.dst_cap < v.src_len ? JFS_ERR_SHORT_BUFFER : JFS_OK;
        return v.src_len == 0 ? JFS_ERR_EMPTY_INPUT : JFS_OK;
    }
    int64_t noff = 0, nlen = 0;
    const int64_t off = envelope_parse(v.src, v.src_len, nullptr, nullptr, &noff, &nlen);
    const int64_t pay = v.src_len - off;  // ciphertext || tag
    if (off < 0 || nlen != 12) return JFS_ERR_CORRUPT;  // the AEADs here all take 12-byte nonces
    if (pay < 16) return JFS_ERR_AUTH;  // aead.Open rejects a payload shorter than the tag
    if (algo != JFS_ALGO_NONE && pay == 16) return JFS_ERR_EMPTY_INPUT;  // the codec would see an empty input
    if (algo == JFS_ALGO_NONE && v.dst_cap < pay - 16) return JFS_ERR_SHORT_BUFFER;  // noOp.Decompress (compress.go:63-65)
    r.off = off;
    r.noff = noff;
    r.pay = pay;
    return JFS_OK;
}

// ---------------------------------------------------------------------------
// the plan: jfs_compact_seg lists, src_map[i] = source i's position among the
// sources the device decodes, or -1 (answered on the host: it counts as failed)
// ---------------------------------------------------------------------------
// a source answered on the host feeds output j
inline bool chain_dead(const int32_t *seg_first, const jfs_compact_seg *seg, int j, const std::vector<int> &src_map) {
    for (int k = seg_first[j]; k < seg_first[j + 1]; k++)
        if (seg[k].src >= 0 && src_map[seg[k].src] < 0) return true;
    return false;
}

// segment s as the device sees it: its source's staged position, ns ("a failed
// source") for one the host answered; a hole (src = -1) stays
inline jfs_compact_seg chain_remap(jfs_compact_seg s, const std::vector<int> &src_map, int ns) {
    if (s.src >= 0) s.src = src_map[s.src] >= 0 ? src_map[s.src] : ns;
    return s;
}

inline int32_t chain_max_total(const std::vector<ChainOut> &oo) {
    int64_t m = 0;
    for (const ChainOut &o : oo) m = std::max(m, o.total);
    return (int32_t)m;
}

// per object of the call, the last byte a segment asks of it (0: unused)
inline std::vector<int64_t> chain_need(int nsrc, int nout, const int32_t *seg_first, const jfs_compact_seg *seg) {
    std::vector<int64_t> need(nsrc > 0 ? nsrc : 0, 0);
    for (int j = 0; j < nout; j++)
        for (int k = seg_first[j]; k < seg_first[j + 1]; k++)
            if (seg[k].src >= 0) need[seg[k].src] = std::max(need[seg[k].src], (int64_t)seg[k].src_off + seg[k].len);
    return need;
}

// per object of the call, the first byte a segment asks of it (0: unused, as
// chain_need): the lower end of the range a seekable source is decoded for
inline std::vector<int64_t> chain_from(int nsrc, int nout, const int32_t *seg_first, const jfs_compact_seg *seg) {
    std::vector<int64_t> from(nsrc > 0 ? nsrc : 0, -1);
    for (int j = 0; j < nout; j++)
        for (int k = seg_first[j]; k < seg_first[j + 1]; k++) {
            if (seg[k].src < 0) continue;
            int64_t &f = from[seg[k].src];
            f = f < 0 ? (int64_t)seg[k].src_off : std::min(f, (int64_t)seg[k].src_off);
        }
    for (int64_t &f : from) f = std::max<int64_t>(f, 0);
    return from;
}

// Prefix mode: want[k] = where the decode of source k stops, `need` clamped to
// its capacity.  Empty when every source is needed whole, which takes the full
// launchers -- unless keep_whole (the range launcher takes every call).
// *max_want = the largest entry.
inline std::vector<int32_t> chain_want(const int64_t *need, const std::vector<ChainSrc> &st, int ns, int64_t *max_want,
                                       bool keep_whole = false) {
    std::vector<int32_t> want(ns);
    bool whole = true;
    *max_want = 0;
    for (int k = 0; k < ns; k++) {
        want[k] = (int32_t)std::min<int64_t>(need[st[k].idx], st[k].cap);
        *max_want = std::max<int64_t>(*max_want, want[k]);
        whole = whole && want[k] >= st[k].cap;
    }
    if (whole && !keep_whole) want.clear();
    return want;
}

// Seek mode: lo[k] = where the range of source k starts, `from` clamped as want is
inline std::vector<int32_t> chain_lo(const int64_t *from, const std::vector<ChainSrc> &st, int ns) {
    std::vector<int32_t> lo(ns);
    for (int k = 0; k < ns; k++) lo[k] = (int32_t)std::min<int64_t>(from[st[k].idx], st[k].cap);
    return lo;
}

// Sparse mode (JFS_READ_SEEK_SPARSE): per decoded source k, the ranges [src_off,
// src_off + len) of the segments that reference it, clamped to its capacity
// (what is left empty is dropped), sorted by lo, the ones that overlap or touch
// merged: an ascending, disjoint list of live ranges.  Source k owns rng[first[k]
// .. first[k + 1]); first has ns + 1 entries.  Holes are no one's; a source
// nothing references has no range.
struct ChainRanges {
    std::vector<int32_t> first;
    std::vector<jfs_range> rng;
};

inline ChainRanges chain_ranges(int nsrc, int nout, const int32_t *seg_first, const jfs_compact_seg *seg,
                                const std::vector<ChainSrc> &st, int ns) {
    std::vector<std::vector<jfs_range>> per(nsrc > 0 ? nsrc : 0);
    std::vector<int64_t> cap(nsrc > 0 ? nsrc : 0, 0);
    for (int k = 0; k < ns; k++) cap[st[k].idx] = std::min<int64_t>(st[k].cap, INT32_MAX);
    for (int j = 0; j < nout; j++)
        for (int k = seg_first[j]; k < seg_first[j + 1]; k++) {
            const jfs_compact_seg &g = seg[k];
            if (g.src < 0) continue;
            const int64_t lo = std::min<int64_t>(std::max<int64_t>(g.src_off, 0), cap[g.src]);
            const int64_t hi = std::min<int64_t>((int64_t)g.src_off + g.len, cap[g.src]);
            if (hi > lo) per[g.src].push_back(jfs_range{(int32_t)lo, (int32_t)hi});
        }
    ChainRanges r;
    r.first.assign(ns + 1, 0);
    for (int k = 0; k < ns; k++) {
        std::vector<jfs_range> &v = per[st[k].idx];
        std::sort(v.begin(), v.end(), [](const jfs_range &a, const jfs_range &b) { return a.lo < b.lo; });
        r.first[k] = (int32_t)r.rng.size();
        size_t base = r.rng.size();
        for (const jfs_range &x : v) {
            if (r.rng.size() > base && x.lo <= r.rng.back().hi) r.rng.back().hi = std::max(r.rng.back().hi, x.hi);
            else r.rng.push_back(x);
        }
    }
    r.first[ns] = (int32_t)r.rng.size();
    return r;
}

// LZ4 chase (JFS_READ_LZ4_CHASE_ON): the decoded sources whose lists ask for at
// least one and at most max_bytes bytes are moved, in their order, to the
// front of st[0, ns) and src_map follows; their count is returned.  The chase
// then takes st[0, count) and the decoders of the switch being off the rest,
// each a run of the staged descriptors.
inline int chain_chase_front(int nsrc, int nout, const int32_t *seg_first, const jfs_compact_seg *seg,
                             std::vector<ChainSrc> &st, int ns, std::vector<int> &src_map, int64_t max_bytes) {
    const ChainRanges r = chain_ranges(nsrc, nout, seg_first, seg, st, ns);
    std::vector<ChainSrc> front, back;
    for (int k = 0; k < ns; k++) {
        int64_t bytes = 0;
        for (int32_t q = r.first[k]; q < r.first[k + 1]; q++) bytes += (int64_t)r.rng[q].hi - r.rng[q].lo;
        (bytes > 0 && bytes <= max_bytes ? front : back).push_back(st[k]);
    }
    const int nf = (int)front.size();
    std::copy(front.begin(), front.end(), st.begin());
    std::copy(back.begin(), back.end(), st.begin() + nf);
    for (int k = 0; k < ns; k++) src_map[st[k].idx] = k;
    return nf;
}

// the 4-aligned groups of output positions the lists of sources [0, n) touch (the chase's grid)
inline int64_t chain_range_quads(const ChainRanges &r, int n) {
    int64_t quads = 0;
    for (int32_t q = r.first[0]; q < r.first[n]; q++) quads += ((r.rng[q].hi + 3) >> 2) - (r.rng[q].lo >> 2);
    return quads;
}

// ---------------------------------------------------------------------------
// the reads' disk-cache checksums (disk_cache_file.go checksum()): the
// big-endian CRC-32C of every 32 KiB piece of a read's gathered bytes
// ---------------------------------------------------------------------------
constexpr int64_t CSUM_PIECE = 32 << 10;  // csBlock

// Go's ((n-1)/csBlock+1): one piece for n = 0
inline int64_t csum_pieces(int64_t n) { return n > 0 ? (n - 1) / CSUM_PIECE + 1 : 1; }

// piece_first[k] = the first piece of output k among all pieces of the call
// (no + 1 entries, the last one their count); an output with want[k] == 0 has
// none.  Piece p of the call has its 4 bytes at 4 p of the checksum area, so
// output k's checksum starts at off[k] = 4 piece_first[k].  Returns the piece
// count, or -1 when it does not fit an int32.
inline int64_t chain_csum_pieces(const std::vector<ChainOut> &oo, const std::vector<uint8_t> &want,
                                 std::vector<int32_t> &piece_first, std::vector<int64_t> &off) {
    const size_t no = oo.size();
    piece_first.assign(no + 1, 0);
    off.assign(no, 0);
    int64_t np = 0;
    for (size_t k = 0; k < no; k++) {
        piece_first[k] = (int32_t)np;
        off[k] = 4 * np;
        if (k < want.size() && want[k]) np += csum_pieces(oo[k].total);
        if (np > INT32_MAX) return -1;
    }
    piece_first[no] = (int32_t)np;
    return np;
}

// ---------------------------------------------------------------------------
// staging of one call
// ---------------------------------------------------------------------------
// Where each object lies in its area: in[k] in the stored bytes (every staged
// object: the ns decoded sources, then those staged for a checksum only),
// out[k] in the output area; with a codec, dec[k] (decoded source k) and, in
// front of an encoder, gat[k] (gathered block k) in the lane's device scratch,
// the sources first.  tin / tout / scratch = the three areas' bytes.
struct ChainOffsets {
    std::vector<int64_t> in, dec, out, gat;
    int64_t tin = 0, tout = 0, scratch = 0;
};

inline ChainOffsets chain_offsets(const std::vector<ChainSrc> &st, int ns, const std::vector<ChainOut> &oo, bool codec,
                                  bool encode) {
    ChainOffsets f;
    auto take = [](int64_t &o, int64_t bytes) {
        const int64_t at = o;
        o += align16(bytes);
        return at;
    };
    for (size_t k = 0; k < st.size(); k++) {
        f.in.push_back(take(f.tin, st[k].pay));
        if (codec && (int)k < ns) f.dec.push_back(take(f.scratch, st[k].cap));
    }
    for (const ChainOut &o : oo) {
        f.out.push_back(take(f.tout, o.area));
        if (codec && encode) f.gat.push_back(take(f.scratch, o.total));
    }
    return f;
}

// what a call uses of the layout
struct ChainFlags {
    bool sealed;   // envelopes: AEAD descriptors, key | nonce cells, the opens' results
    bool encode;   // compaction: encoder (and seal) descriptors; else the flat gather's tile prefix
    bool out_crc;  // CRC-32C of every output
    bool src_crc;  // expected CRC-32C of stored objects
    bool prefix;   // per-source decode limits
    bool read_csum = false;  // disk-cache checksums of the reads (last: the initialisers above leave it off)
    bool seek = false;       // per-source lower ends of the decoded ranges (JFS_READ_SEEK)
    bool sparse = false;     // per-source lists of ranges (JFS_READ_SEEK_SPARSE)
};

// The staged area, mirrored pinned / HBM: [stored bytes | meta | results |
// outputs], byte offsets from the slot's base.  ns decoded sources, n staged
// objects (n - ns of them only for their checksum), no outputs, nseg segments,
// npiece 32 KiB pieces of the reads that asked for their checksums, nrange
// ranges of the sparse lists, xmeta_bytes / xres_bytes of records and results
// that only the call itself knows.
// An area the call does not use has no bytes and sits where the next one
// starts.  The host writes [0, h2d), which goes to the device in one copy;
// [results, out) comes back in one copy.  srcn, the source lengths, lies in
// both: the host presets it and a decoder overwrites it.
struct ChainLayout {
    // meta, host-written:
    int64_t sdesc;  // source descriptors, ns + 1: the last one is "a failed source"
    int64_t plan, seg;  // gather plan and its segments
    int64_t tf;         // tile prefix of the flat gather, no + 1
    int64_t enc, ocd;   // encoder descriptors; checksum descriptors of the outputs
    int64_t sad, oad;   // AEAD descriptors: opens, seals
    int64_t kn;         // one 64-byte key | nonce cell per opened source, then per sealed output
    int64_t oseed;      // checksum seeds of sealed outputs (the envelope header's CRC)
    int64_t scd, sseed, len, exp;  // stored objects' checksums: descriptors, seeds, lengths (-1: none), expected
    int64_t want;                  // prefix mode's decode limits
    int64_t pf;                    // piece prefix of the reads' checksums, no + 1
    int64_t from;                  // seek mode's lower ends, beside want
    int64_t rf, rng;               // sparse mode's lists: their running sums, ns + 1, and the nrange ranges
    int64_t xmeta;                 // a call's own records (the spliced compaction's), xmeta_bytes of them
    int64_t srcn;                  // source lengths, ns + 1, preset
    // results, which only the device writes:
    int64_t open;        // the opens'
    int64_t ret, r2;     // the outputs': gather / encoder, seal
    int64_t ocrc;        // output checksums
    int64_t scrc, got;   // stored objects' checksums: raw, checked
    int64_t csum;        // the reads' checksums, 4 bytes per piece
    int64_t xres;        // a call's own results, xres_bytes of them
    int64_t out;         // the output area
    int64_t h2d, results;

    ChainLayout() = default;
    ChainLayout(int64_t tin, int64_t ns, int64_t n, int64_t no, int64_t nseg, const ChainFlags &f,
                int64_t npiece = 0, int64_t nrange = 0, int64_t xmeta_bytes = 0, int64_t xres_bytes = 0) {
        int64_t o = align16(tin);
        auto take = [&o](bool used, int64_t count, int64_t size) {
            const int64_t at = o;
            if (used) o += align16(count * size);
            return at;
        };
        const int64_t blk = (int64_t)sizeof(jfs_dev_block), aead = (int64_t)sizeof(jfs_aead_block);
        sdesc = take(true, ns + 1, blk);
        plan = take(true, no, (int64_t)sizeof(jfs_compact_out));
        seg = take(true, nseg, (int64_t)sizeof(jfs_compact_seg));
        tf = take(!f.encode, no + 1, 4);
        enc = take(f.encode, no, blk);
        ocd = take(f.out_crc, no, blk);
        sad = take(f.sealed, ns, aead);
        oad = take(f.sealed && f.encode, no, aead);
        kn = take(f.sealed, ns + (f.encode ? no : 0), 64);
        oseed = take(f.sealed && f.out_crc, no, 4);
        scd = take(f.src_crc, n, blk);
        sseed = take(f.src_crc, n, 4);
        len = take(f.src_crc, n, 4);
        exp = take(f.src_crc, n, 4);
        want = take(f.prefix, ns, 4);
        pf = take(f.read_csum, no + 1, 4);
        from = take(f.seek, ns, 4);
        rf = take(f.sparse, ns + 1, 4);
        rng = take(f.sparse, nrange, (int64_t)sizeof(jfs_range));
        xmeta = take(xmeta_bytes > 0, xmeta_bytes, 1);
        results = srcn = take(true, ns + 1, 4);
        h2d = o;
        open = take(f.sealed, ns, 4);
        ret = take(true, no, 4);
        r2 = take(f.sealed && f.encode, no, 4);
        ocrc = take(f.out_crc, no, 4);
        scrc = take(f.src_crc, n, 4);
        got = take(f.src_crc, n, 4);
        csum = take(f.read_csum, npiece, 4);
        xres = take(xres_bytes > 0, xres_bytes, 1);
        out = o;
    }
};

}  // namespace jfs_plan
