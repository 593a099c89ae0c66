// libjfsgpu.so host side: the on-device chains of the C ABI
// (include/jfs_gpucodec.h), one device and one lane per call:
//   compaction     (open ->) decode -> gather -> encode (-> seal)
//                  jfs_compact_batch, jfs_compact_seal_batch
//   read assembly  verify -> (open ->) decode -> gather (-> the reads' checksums)
//                  jfs_read_batch, jfs_read_open_batch and their _csum forms
//   ranged loads   jfs_zstd_load_range_batch
// cipher < 0: no envelopes.  The planning arithmetic is chain_plan.h's and
// splice_plan.h's; no kernel lives here.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <mutex>
#include <utility>
#include <vector>

#include "capi_host.h"
#include "chain_plan.h"
#include "jfs_internal.h"
#include "lz4_lift.h"
#include "lz4_window.h"
#include "splice_plan.h"
#include "zstd_seek.h"

using namespace jfs_host;

namespace {

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
// and of device scratch behind the decoded sources and gathered blocks; the
// 32 KiB pieces of the reads' checksums (ChainFlags::read_csum) and the ranges
// of the sources' lists (ChainFlags::sparse).
struct ChainExtra {
    int64_t meta = 0, res = 0, out = 0, scratch = 0;
    int64_t npiece = 0, nrange = 0;
    const ChainOpened *opened = nullptr;  // the call's sources, where an earlier pass of it opened them
};

// One chain call as its entry point received and sorted it (compact_call,
// read_call), the same for every runner: the caller's arrays, and the sources
// and outputs the host left to the device.
struct ChainCall {
    int algo, cipher;
    int nsrc;
    const jfs_iov *src;
    const uint8_t *const *src_keys;
    int nout;
    const jfs_iov *out;
    const int32_t *seg_first;
    const jfs_compact_seg *seg;
    int64_t *src_n, *out_n;
    std::vector<ChainSrc> st;  // [0, ns): the decoded sources; behind them what is staged for its checksum only
    int ns;
    std::vector<int> src_map;  // per source of the call: its place in st, or -1
    std::vector<ChainOut> oo;
};

// Lays the call out over the outputs oo (seg_first: their segments' places)
// and sizes slot 0 for it: JFS_OK or JFS_ERR_NO_MEMORY.
int64_t chain_open(Chain &c, Lane &ln, const ChainCall &cc, const std::vector<ChainOut> &oo, const int32_t *seg_first,
                   ChainFlags f, const ChainExtra &x) {
    const std::vector<ChainSrc> &st = cc.st;
    const int algo = cc.algo, ns = cc.ns;
    c.algo = algo;
    c.cipher = cc.cipher;
    c.ns = ns;
    c.n = (int)st.size();
    c.no = (int)oo.size();
    c.codec = algo != JFS_ALGO_NONE;
    c.sealed = f.sealed = cc.cipher >= 0;  // (the one place that says so: callers leave the flag alone)
    c.lz4 = algo == JFS_ALGO_LZ4;
    c.off = jfs_plan::chain_offsets(st, ns, oo, c.codec, f.encode);
    int64_t nseg = 0;
    for (const ChainOut &o : oo) nseg += seg_first[o.idx + 1] - seg_first[o.idx];
    c.L = ChainLayout(x.opened ? 0 : c.off.tin, ns, c.n, c.no, nseg, f, x.npiece, x.nrange, x.meta, x.res);
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
void chain_stage_sources(const Chain &c, const ChainCall &cc, std::vector<CopyJob> &jobs) {
    const uint8_t *const *src_keys = cc.src_keys;
    jfs_dev_block *h_sdesc = c.host<jfs_dev_block>(c.L.sdesc);
    int32_t *h_srcn = c.host<int32_t>(c.L.srcn);
    for (int k = 0; k < c.n; k++) {
        const ChainSrc &s = cc.st[k];
        const jfs_iov &v = cc.src[s.idx];
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
// anything is queued.  lift_need (> 0: the encode step is the lift launcher's): its scratch instead of the encoder's.
bool chain_lz4_scratch(const Chain &c, const jfs_dev_block *h_enc, bool fast, int64_t lift_need = 0) {
    if (!c.lz4) return true;
    const jfs_dev_block *h_sdesc = c.host<jfs_dev_block>(c.L.sdesc);
    int64_t need = 0;
    if (c.ns > 0) need = lz4_decode_scratch(c.ns, desc_lens(h_sdesc, c.ns).data(), desc_caps(h_sdesc, c.ns).data());
    if (h_enc && c.no > 0)
        need = std::max(need, lift_need > 0 ? lift_need : lz4_encode_scratch(c.no, desc_lens(h_enc, c.no).data(), fast));
    return need <= 0 || c.s1->ensure_split(need);
}

// What the decodes of a call are limited to (nothing set: every source whole).
// d_want (prefix modes: LZ4, and Zstd in JFS_READ_DECODE_PREFIX_ALL; else null): where each decode stops.
// d_from (Zstd with JFS_READ_SEEK on; else null): with d_want the range each source is decoded for.
// d_rf, d_rng (Zstd with JFS_READ_SEEK sparse; else null): the list of ranges each source is decoded for.
// nchase (LZ4 with JFS_READ_LZ4_CHASE on; else 0): sources [0, nchase) take the origin chase for their lists in
// d_rf, d_rng, which touch at most max_quads 4-byte groups; the rest are decoded as without the switch.
// window (LZ4 with JFS_READ_LZ4_WINDOW on, where read_run takes it): the sources the chase leaves are decoded by
// the window launcher for [d_from, d_want).
struct ChainDecode {
    const int32_t *d_want = nullptr;
    int64_t max_want = 0;
    const int32_t *d_from = nullptr, *d_rf = nullptr;
    const jfs_range *d_rng = nullptr;
    int nchase = 0;
    int64_t max_quads = 0;
    bool window = false;
};

// Queues open -> decode -> the opens' verdicts merged into the source lengths.
int chain_decode(const Chain &c, const ChainDecode &q) {
    const jfs_dev_block *h_sdesc = c.host<jfs_dev_block>(c.L.sdesc), *d_sdesc = c.dev<jfs_dev_block>(c.L.sdesc);
    int32_t *d_srcn = c.dev<int32_t>(c.L.srcn), *d_open = c.open_d;
    const int ns = c.ns;
    int lk = 0;
    if (c.sealed && !c.opened && ns > 0) lk = jfs_launch_aead(c.cipher, c.dev<jfs_aead_block>(c.L.sad), ns, 1, d_open, nullptr, c.ks);
    if (lk == 0 && c.lz4 && ns > 0) {
        int64_t r = JFS_OK;
        const int rest = ns - q.nchase;
        // (the slot's scratch was sized for both launches before anything was queued: read_run)
        if (q.nchase > 0)
            r = launch_rc(jfs_launch_lz4_chase(d_sdesc, desc_lens(h_sdesc, q.nchase).data(), desc_caps(h_sdesc, q.nchase).data(),
                                               q.d_rf, q.d_rng, q.nchase, d_srcn, c.s1->sp, q.max_quads, c.ks));
        if (r == JFS_OK && rest > 0)
            r = q.window ? launch_lz4_decode_window(*c.s1, h_sdesc + q.nchase, d_sdesc + q.nchase, rest, d_srcn + q.nchase,
                                                    q.d_from + q.nchase, q.d_want + q.nchase, q.max_want, c.ks)
                : q.d_want ? launch_lz4_decode_prefix(*c.s1, h_sdesc + q.nchase, d_sdesc + q.nchase, rest, d_srcn + q.nchase,
                                                  q.d_want + q.nchase, q.max_want, c.ks)
                       : launch_lz4_decode(*c.s1, h_sdesc + q.nchase, d_sdesc + q.nchase, rest, d_srcn + q.nchase, c.ks);
        lk = r == JFS_OK ? 0 : -1;
    } else if (lk == 0 && c.algo == JFS_ALGO_ZSTD && ns > 0) {
        // (with a cipher the frame headers are ciphertext on the host) it plans its own scratch
        lk = q.d_rf     ? jfs_launch_zstd_decode_ranges(d_sdesc, q.d_rf, q.d_rng, ns, d_srcn, c.ks)
             : q.d_from ? jfs_launch_zstd_decode_range(d_sdesc, q.d_from, q.d_want, ns, d_srcn, c.ks)
             : q.d_want ? jfs_launch_zstd_decode_prefix(d_sdesc, ns, d_srcn, q.d_want, c.ks)
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

// What the compaction runners get beside the call: the outputs' seal
// parameters (sealed calls) and where their CRC-32C goes (or null).
struct CompactOpts {
    const jfs_seal_param *out_p;
    uint32_t *crc;
};

// jfs_compact_lz4_lift_counts: calls that took the lift launcher, candidate chunks planned, chunks lifted, candidates
// the device refused and parsed
std::atomic<uint64_t> g_lift_counts[4];

// The lift plan of a compaction call (lz4_lift.h) over the outputs and sources the device works on: empty unless
// the call is LZ4 in the fast parse mode with JFS_COMPACT_LZ4_LIFT on.  The segments are the staged ones
// (chain_remap), so a source the host answered is no candidate.
jfs::lz4l::LiftPlan compact_lift_plan(const ChainCall &cc, bool fast) {
    jfs::lz4l::LiftPlan lp;
    if (cc.algo != JFS_ALGO_LZ4 || !fast || CompactLz4Lift::get() != JFS_COMPACT_LZ4_LIFT_ON || cc.ns <= 0 || cc.oo.empty())
        return lp;
    std::vector<int32_t> first(1, 0), total, cap;
    std::vector<jfs_compact_seg> sg;
    for (const ChainOut &o : cc.oo) {
        for (int q = cc.seg_first[o.idx]; q < cc.seg_first[o.idx + 1]; q++)
            sg.push_back(jfs_plan::chain_remap(cc.seg[q], cc.src_map, cc.ns));
        first.push_back((int32_t)sg.size());
        total.push_back((int32_t)o.total);
    }
    for (int k = 0; k < cc.ns; k++) cap.push_back((int32_t)cc.st[k].cap);
    return jfs::lz4l::lift_plan((int)cc.oo.size(), first.data(), sg.data(), total.data(), cc.ns, cap.data());
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
// LZ4 in the fast parse mode with JFS_COMPACT_LZ4_LIFT on, where the plan has a
// candidate chunk: the candidates and the sources to index ride in
// the H2D copy, the encode step is the lift launcher's over the stored (opened)
// streams, and the chunks lifted per output come back with the results.  Any
// other call is laid out and queued exactly as without the switch.
int64_t compact_run(DevCtx *dev, Lane &ln, const ChainCall &cc, const CompactOpts &opt) {
    const int algo = cc.algo, cipher = cc.cipher;
    const std::vector<ChainSrc> &ss = cc.st;
    const std::vector<ChainOut> &oo = cc.oo;
    const jfs_iov *out = cc.out;
    const jfs_seal_param *out_p = opt.out_p;
    int64_t *src_n = cc.src_n, *out_n = cc.out_n;
    uint32_t *crc = opt.crc;
    LaneRun scope(dev, ln, algo * 2 + COMPRESS, (uint64_t)(ss.size() + oo.size()));
    Chain c;
    ChainFlags flags{};
    flags.encode = true;
    flags.out_crc = crc != nullptr;
    const bool fast = lz4_fast_mode();
    const jfs::lz4l::LiftPlan lp = compact_lift_plan(cc, fast);
    const bool lift = lp.candidates > 0;
    const int nsel = (int)lp.srcs.size();
    const int64_t m_sel = align16((int64_t)lp.chunk.size() * (int64_t)sizeof(jfs_lz4_lift));
    ChainExtra x;
    if (lift) {
        x.meta = m_sel + align16(nsel * 4ll);
        x.res = align16((int64_t)oo.size() * 4);
    }
    const int64_t rc = chain_open(c, ln, cc, oo, cc.seg_first, flags, x);
    if (rc != JFS_OK) return rc;
    const ChainLayout &L = c.L;
    const int ns = c.ns, no = c.no;
    const bool codec = c.codec, sealed = c.sealed;
    std::vector<CopyJob> jobs;
    chain_stage_sources(c, cc, jobs);
    par_copy(jobs);
    chain_stage_plan(c, oo, cc.src_map, cc.seg_first, cc.seg);
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
    std::vector<int32_t> sel_len(nsel), sel_cap(nsel);
    int64_t lift_need = 0;
    if (lift) {
        memcpy(c.h + L.xmeta, lp.chunk.data(), lp.chunk.size() * sizeof(jfs_lz4_lift));
        memcpy(c.h + L.xmeta + m_sel, lp.srcs.data(), (size_t)nsel * 4);
        const jfs_dev_block *h_sdesc = c.host<jfs_dev_block>(L.sdesc);
        for (int q = 0; q < nsel; q++) {
            sel_len[q] = h_sdesc[lp.srcs[q]].src_len;
            sel_cap[q] = h_sdesc[lp.srcs[q]].dst_cap;
        }
        lift_need = jfs_lz4_fast_lift_scratch_bytes(no, desc_lens(h_enc, no).data(), ns, nsel, sel_len.data());
    }
    if (!chain_lz4_scratch(c, h_enc, fast, lift_need)) return JFS_ERR_NO_MEMORY;
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
    int lk = chain_decode(c, {});
    if (lk == 0) lk = gather(0);
    if (lk == 0 && codec && no > 0) {
        if (lift) {
            const jfs_lz4_lift_srcs S{d_sdesc, d_srcn, ns, c.dev<int32_t>(L.xmeta + m_sel), nsel, sel_len.data(), sel_cap.data()};
            lk = jfs_launch_lz4_fast_lift(d_enc, no, desc_lens(h_enc, no).data(), c.dev<jfs_lz4_lift>(L.xmeta), &S, d_ret,
                                          c.dev<int32_t>(L.xres), c.s1->sp, c.s1->sp_cap, ks);
        } else {
            lk = c.lz4 ? (launch_lz4_encode(*c.s1, h_enc, d_enc, no, d_ret, ks, fast) == JFS_OK ? 0 : -1)
                       : launch_kernel(algo, COMPRESS, d_enc, no, d_ret, ks, zstd_encode_now());
        }
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
    if (lift) {
        uint64_t lifted = 0;
        for (int k = 0; k < no; k++) lifted += (uint64_t)std::max(c.host<int32_t>(L.xres)[k], 0);
        const uint64_t planned = (uint64_t)lp.candidates;
        g_lift_counts[0].fetch_add(1, std::memory_order_relaxed);
        g_lift_counts[1].fetch_add(planned, std::memory_order_relaxed);
        g_lift_counts[2].fetch_add(lifted, std::memory_order_relaxed);
        g_lift_counts[3].fetch_add(planned > lifted ? planned - lifted : 0, std::memory_order_relaxed);
    }
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

int64_t splice_open_tables(Lane &ln, const ChainCall &cc, OpenedTables &T) {
    const int cipher = cc.cipher, nsrc = cc.nsrc;
    const jfs_iov *src = cc.src;
    const uint8_t *const *src_keys = cc.src_keys;
    const std::vector<ChainSrc> &ss = cc.st;
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

// What the spliced compaction gets beside compact_run's: the plan over the
// stored objects (calls without a cipher), `replan` (calls with one), the
// sealed outputs the host already answered, and whether the objects it writes
// carry checksums (JFS_ZSTD_SEEK_CSUM).
struct SpliceOpts {
    const jfs_plan::SplicePlan &plan;
    const SpliceReplan &replan;
    const std::vector<int> &own;
    bool csum;
};

// Compaction with untouched frames spliced (Zstd in the seekable parse mode).
// Without a cipher (JFS_COMPACT_SPLICE on or all): sopt.plan, splice_plan.h's answer
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
int64_t compact_splice_run(DevCtx *dev, Lane &ln, const ChainCall &cc, const CompactOpts &opt, const SpliceOpts &sopt) {
    const int algo = JFS_ALGO_ZSTD, cipher = cc.cipher, nsrc = cc.nsrc;
    const std::vector<ChainSrc> &ss = cc.st;
    const std::vector<ChainOut> &oo = cc.oo;
    const std::vector<int> &src_map = cc.src_map, &own = sopt.own;
    const jfs_iov *out = cc.out;
    const jfs_seal_param *out_p = opt.out_p;
    const int32_t *seg_first = cc.seg_first;
    const jfs_compact_seg *seg = cc.seg;
    int64_t *src_n = cc.src_n, *out_n = cc.out_n;
    uint32_t *crc = opt.crc;
    const bool csum = sopt.csum;
    const bool sealed = cipher >= 0;
    LaneRun scope(dev, ln, algo * 2 + COMPRESS, (uint64_t)(ss.size() + oo.size()));
    OpenedTables T;
    jfs_plan::SplicePlan replanned;
    if (sealed) {
        const int64_t rc = splice_open_tables(ln, cc, T);
        if (rc != JFS_OK) return rc;
        replanned = sopt.replan(jfs_plan::PackedTables{T.tab, T.slot.data(), T.tlen.data(), T.len.data(), nullptr});
    }
    const jfs_plan::SplicePlan &P = sealed ? replanned : sopt.plan;
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
    x.nrange = whole ? 0 : (int64_t)lists.rng.size();
    x.opened = sealed ? &T.at : nullptr;
    ChainFlags flags{};
    flags.encode = true;
    flags.sparse = !whole;
    Chain c;
    // (the chain's own seal and checksum areas stay unused: the outputs are not its units)
    const int64_t rc = chain_open(c, ln, cc, uu, P.seg_first.data(), flags, x);
    if (rc != JFS_OK) return rc;
    const ChainLayout &L = c.L;
    const int64_t xout = L.out + c.off.tout;  // the spliced objects' area, mirrored like the outputs'
    std::vector<CopyJob> jobs;
    chain_stage_sources(c, cc, jobs);
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
    ChainDecode dec;
    if (!whole) {
        dec.d_rf = c.dev<int32_t>(L.rf);
        dec.d_rng = c.dev<jfs_range>(L.rng);
    }
    int lk = chain_decode(c, dec);
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
// wneed, wfrom (LZ4 with JFS_READ_LZ4_WINDOW on, else null): chain_need and
// chain_from of the call, whatever the decode mode.  Where the sources the
// chase leaves fit the small-batch decoder and one of them has a read that starts
// at or above its first 64 KiB chunk boundary (Fc(from) > 0, lz4_window.h),
// those sources are decoded by the window launcher for [from, need), staged as
// the seek mode's; any other call is laid out and queued exactly as without them.
struct ReadOpts {
    uint32_t *crc_got;
    const int64_t *need, *from;
    uint8_t *const *csum;
    bool sparse;
    int nchase;  // LZ4 with JFS_READ_LZ4_CHASE on: the sources at the front that take the chase
    const int64_t *wneed = nullptr, *wfrom = nullptr;
};

int64_t read_run(DevCtx *dev, Lane &ln, const ChainCall &cc, const ReadOpts &opt) {
    const int algo = cc.algo, ns = cc.ns, nsrc = cc.nsrc, nout = cc.nout;
    const std::vector<ChainSrc> &st = cc.st;
    const std::vector<ChainOut> &oo = cc.oo;
    const jfs_iov *src = cc.src, *out = cc.out;
    const int32_t *seg_first = cc.seg_first;
    const jfs_compact_seg *seg = cc.seg;
    int64_t *src_n = cc.src_n, *out_n = cc.out_n;
    uint32_t *crc_got = opt.crc_got;
    const int64_t *need = opt.need, *from = opt.from;
    uint8_t *const *csum = opt.csum;
    bool sparse = opt.sparse;
    int nchase = opt.nchase;
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
    // (LZ4 with JFS_READ_LZ4_CHASE on: read_call moved the nchase sources that take the chase to the front)
    nchase = algo == JFS_ALGO_LZ4 ? std::min(nchase, ns) : 0;
    bool window = false;
    if (algo == JFS_ALGO_LZ4 && opt.wneed && opt.wfrom && ns > nchase && lz4_decode_is_small(ns - nchase))
        for (int k = nchase; k < ns && !window; k++)
            window = jfs::lz4w::floor_of((int32_t)std::min<int64_t>(opt.wfrom[st[k].idx], st[k].cap)) > 0;
    if (window) {
        need = opt.wneed;
        from = opt.wfrom;
    }
    const bool seek = need && from && ((algo == JFS_ALGO_ZSTD && ns > 0) || window);
    if (need && (algo == JFS_ALGO_LZ4 || algo == JFS_ALGO_ZSTD)) want = jfs_plan::chain_want(need, st, ns, &max_want, seek);
    const bool prefix = !want.empty();
    sparse = sparse && algo == JFS_ALGO_ZSTD && ns > 0;
    jfs_plan::ChainRanges lists;
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
    ChainFlags flags{};
    flags.src_crc = any_check;
    flags.prefix = prefix;
    flags.read_csum = npiece > 0;
    flags.seek = seek;
    flags.sparse = listed;
    ChainExtra x;
    x.npiece = npiece;
    x.nrange = listed ? (int64_t)lists.rng.size() : 0;
    Chain c;
    const int64_t rc = chain_open(c, ln, cc, oo, seg_first, flags, x);
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
    chain_stage_sources(c, cc, jobs);
    for (int k = 0; any_check && k < n; k++) {
        const ChainSrc &s = st[k];
        // the checksum covers the object as fetched: the staged bytes, behind the envelope header's on the host
        c.host<jfs_dev_block>(L.scd)[k] = jfs_dev_block{c.d_in(k), nullptr, (int32_t)s.pay, 0};
        c.host<uint32_t>(L.sseed)[k] = s.check && s.off > 0 ? host_crc32c(0, src[s.idx].src, s.off) : 0u;
        c.host<int32_t>(L.len)[k] = s.check && s.pay > 0 ? (int32_t)s.pay : -1;
        c.host<uint32_t>(L.exp)[k] = s.expect;
    }
    par_copy(jobs);
    chain_stage_plan(c, oo, cc.src_map, seg_first, seg);
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
    ChainDecode dec;
    dec.d_want = prefix ? c.dev<int32_t>(L.want) : nullptr;
    dec.max_want = max_want;
    dec.d_from = seek ? c.dev<int32_t>(L.from) : nullptr;
    dec.d_rf = listed ? c.dev<int32_t>(L.rf) : nullptr;
    dec.d_rng = listed ? c.dev<jfs_range>(L.rng) : nullptr;
    dec.nchase = nchase;
    dec.max_quads = nchase > 0 ? jfs_plan::chain_range_quads(lists, nchase) : 0;
    dec.window = window;
    if (lk == 0) lk = chain_decode(c, dec);
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

}  // namespace

extern "C" {

int jfs_compact_splice_counts(uint64_t out[4], int reset) {
    if (!out) return -1;
    for (int k = 0; k < 4; k++)
        out[k] = reset ? g_splice_counts[k].exchange(0) : g_splice_counts[k].load(std::memory_order_relaxed);
    return 0;
}

int jfs_compact_lz4_lift_counts(uint64_t out[4], int reset) {
    if (!out) return -1;
    for (int k = 0; k < 4; k++)
        out[k] = reset ? g_lift_counts[k].exchange(0) : g_lift_counts[k].load(std::memory_order_relaxed);
    return 0;
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
    ChainCall cc{algo, cipher, nsrc, src, src_keys, nout, out, seg_first, seg, src_n, out_n, {}, 0, {}, {}};
    std::vector<ChainSrc> &ss = cc.st;
    std::vector<int> &src_map = cc.src_map;
    cc.ns = chain_sources(algo, sealed, nsrc, src, nullptr, src_n, nullptr, ss, src_map);
    std::vector<ChainOut> &oo = cc.oo;
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
    const bool splice_csum = ZstdSeekCsum::get() == JFS_ZSTD_SEEK_CSUM_ON;
    const int splice_mode = CompactSplice::get();
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
    const CompactOpts opt{out_p, crc};
    const int64_t rc = chain_dispatch(ds, algo, COMPRESS, ss, oo, src_n, out_n, [&](DevCtx *dev, Lane &ln) {
        if (sealed ? splice_try : splice.outs > 0)
            return compact_splice_run(dev, ln, cc, opt, SpliceOpts{splice, replan, own, splice_csum});
        return compact_run(dev, ln, cc, opt);
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
    ChainCall cc{algo, cipher, nsrc, src, src_keys, nout, out, seg_first, seg, src_n, out_n, {}, 0, {}, {}};
    std::vector<ChainSrc> &st = cc.st;
    std::vector<int> &src_map = cc.src_map;
    const int ns = cc.ns = chain_sources(algo, sealed, nsrc, src, src_crc, src_n, crc_got, st, src_map);
    std::vector<ChainOut> &oo = cc.oo;
    for (int j = 0; j < nout; j++) {
        if (jfs_plan::chain_dead(seg_first, seg, j, src_map)) out_n[j] = JFS_ERR_CORRUPT;
        else if (total[j] == 0) out_n[j] = 0;
        else oo.push_back({j, total[j], total[j], 0, 0});
        // an empty read's checksum is checksum() of no bytes: one zero word, no device needed
        if (csum && csum[j] && out_n[j] == 0 && total[j] == 0) memset(csum[j], 0, 4);
    }
    // prefix modes (LZ4 in both, Zstd in prefix-all): the last byte the plan asks of every object
    std::vector<int64_t> need, from;
    const int dmode = ReadDecode::get();
    // JFS_READ_SEEK: every Zstd source is decoded for [from, need), whatever the decode mode
    const int smode = algo == JFS_ALGO_ZSTD ? ReadSeek::get() : JFS_READ_SEEK_OFF;
    const bool seek = smode == JFS_READ_SEEK_ON, sparse = smode == JFS_READ_SEEK_SPARSE;
    // (JFS_READ_SEEK sparse: the lists of ranges stand for both, read_run makes them)
    if ((algo == JFS_ALGO_LZ4 && dmode != JFS_READ_DECODE_FULL) ||
        (algo == JFS_ALGO_ZSTD && dmode == JFS_READ_DECODE_PREFIX_ALL && !sparse) || seek)
        need = jfs_plan::chain_need(nsrc, nout, seg_first, seg);
    if (seek) from = jfs_plan::chain_from(nsrc, nout, seg_first, seg);
    // JFS_READ_LZ4_CHASE: the LZ4 sources whose reads ask for little enough go first and take the chase
    int nchase = 0;
    if (algo == JFS_ALGO_LZ4 && ns > 0 && ReadLz4Chase::get() == JFS_READ_LZ4_CHASE_ON)
        nchase = jfs_plan::chain_chase_front(nsrc, nout, seg_first, seg, st, ns, src_map, Lz4ChaseMax::get());
    // JFS_READ_LZ4_WINDOW: the range every LZ4 source is asked for, in every decode mode (read_run decides)
    std::vector<int64_t> wneed, wfrom;
    if (algo == JFS_ALGO_LZ4 && ns > 0 && ReadLz4Window::get() == JFS_READ_LZ4_WINDOW_ON) {
        wneed = jfs_plan::chain_need(nsrc, nout, seg_first, seg);
        wfrom = jfs_plan::chain_from(nsrc, nout, seg_first, seg);
    }
    const ReadOpts opt{crc_got, need.empty() ? nullptr : need.data(), from.empty() ? nullptr : from.data(), csum, sparse,
                       nchase, wneed.empty() ? nullptr : wneed.data(), wfrom.empty() ? nullptr : wfrom.data()};
    chain_dispatch(ds, algo, DECOMPRESS, st, oo, src_n, out_n,
                   [&](DevCtx *dev, Lane &ln) { return read_run(dev, ln, cc, opt); });
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

}  // extern "C"
