// Checks juicefs_amd/csrc/chain_plan.h (the planning of the on-device chain
// calls: compaction and read assembly) on a CPU: the staging layout over every
// flag combination and against the offset chains the three runners derived by
// hand before they shared it, the plan functions, and the table of what the
// host answers for a source.  Built and run by tests/test_chain_plan.py under
// ASan + UBSan.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../juicefs_amd/csrc/chain_plan.h"

using namespace jfs_plan;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            g_fail++;                                      \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
            if (g_fail > 20) exit(1);                      \
        }                                                  \
    } while (0)

static const int64_t BLK = sizeof(jfs_dev_block), AEAD = sizeof(jfs_aead_block), PLAN = sizeof(jfs_compact_out),
                     SEG = sizeof(jfs_compact_seg);

// ---------------------------------------------------------------------------
// layout
// ---------------------------------------------------------------------------
struct Area {
    const char *name;
    int64_t off;
    bool used;
    int64_t bytes;  // when used
    bool host;      // host-written (else only the device writes it)
};

// every area in order, with the size this test expects of it
static std::vector<Area> areas(const ChainLayout &L, int64_t ns, int64_t n, int64_t no, int64_t nseg, const ChainFlags &f) {
    const bool seal = f.sealed && f.encode;
    return {
        {"sdesc", L.sdesc, true, (ns + 1) * BLK, true},
        {"plan", L.plan, true, no * PLAN, true},
        {"seg", L.seg, true, nseg * SEG, true},
        {"tf", L.tf, !f.encode, (no + 1) * 4, true},
        {"enc", L.enc, f.encode, no * BLK, true},
        {"ocd", L.ocd, f.out_crc, no * BLK, true},
        {"sad", L.sad, f.sealed, ns * AEAD, true},
        {"oad", L.oad, seal, no * AEAD, true},
        {"kn", L.kn, f.sealed, 64 * (ns + (f.encode ? no : 0)), true},
        {"oseed", L.oseed, f.sealed && f.out_crc, no * 4, true},
        {"scd", L.scd, f.src_crc, n * BLK, true},
        {"sseed", L.sseed, f.src_crc, n * 4, true},
        {"len", L.len, f.src_crc, n * 4, true},
        {"exp", L.exp, f.src_crc, n * 4, true},
        {"want", L.want, f.prefix, ns * 4, true},
        {"srcn", L.srcn, true, (ns + 1) * 4, true},
        {"open", L.open, f.sealed, ns * 4, false},
        {"ret", L.ret, true, no * 4, false},
        {"r2", L.r2, seal, no * 4, false},
        {"ocrc", L.ocrc, f.out_crc, no * 4, false},
        {"scrc", L.scrc, f.src_crc, n * 4, false},
        {"got", L.got, f.src_crc, n * 4, false},
    };
}

static void layout_invariants() {
    const int64_t nss[] = {0, 1, 3}, nos[] = {0, 1, 4}, nsegs[] = {0, 1, 7}, tins[] = {0, 48};
    for (int bits = 0; bits < 32; bits++)
        for (int64_t ns : nss)
            for (int64_t n : {ns, ns + 2})
                for (int64_t no : nos)
                    for (int64_t nseg : nsegs)
                        for (int64_t tin : tins) {
                            const ChainFlags f{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0,
                                               (bits & 16) != 0};
                            const ChainLayout L(tin, ns, n, no, nseg, f);
                            const std::vector<Area> a = areas(L, ns, n, no, nseg, f);
                            CHECK(a[0].off == tin, "flags %d: the meta starts behind the stored bytes", bits);
                            for (size_t k = 0; k < a.size(); k++) {
                                const int64_t next = k + 1 < a.size() ? a[k + 1].off : L.out;
                                const int64_t size = next - a[k].off;
                                CHECK(a[k].off % 16 == 0, "flags %d %s: offset %lld", bits, a[k].name, (long long)a[k].off);
                                // in order, disjoint, nothing between two areas; an unused one has no bytes
                                CHECK(size == (a[k].used ? align16(a[k].bytes) : 0), "flags %d %s: %lld bytes, want %lld", bits,
                                      a[k].name, (long long)size, (long long)(a[k].used ? align16(a[k].bytes) : 0));
                                if (a[k].host) CHECK(next <= L.h2d, "flags %d %s: host-written, but ends behind the H2D copy", bits, a[k].name);
                                else CHECK(a[k].off >= L.h2d, "flags %d %s: device-only, but inside the H2D copy", bits, a[k].name);
                                if (!a[k].host) CHECK(a[k].off >= L.results && next <= L.out, "flags %d %s: a result outside the D2H copy", bits, a[k].name);
                            }
                            // the preset source lengths go down and come back
                            CHECK(L.results == L.srcn && L.srcn + align16((ns + 1) * 4) == L.h2d && L.h2d <= L.out,
                                  "flags %d: srcn %lld, results %lld, h2d %lld", bits, (long long)L.srcn, (long long)L.results,
                                  (long long)L.h2d);
                        }
}

// The offset chains of compact_run, compact_seal_run and read_run as each
// derived them by hand before ChainLayout.  (read_run always laid out the
// opens' and the checksums' areas: it corresponds to sealed + src_crc.)
static void layout_tables() {
    const int64_t nss[] = {0, 1, 3}, nos[] = {0, 1, 4}, nsegs[] = {0, 1, 7};
    for (int64_t ns : nss)
        for (int64_t no : nos)
            for (int64_t nseg : nsegs) {
                const int64_t tin = 4096 + 16 * ns;
                {
                    const int64_t o_sdesc = tin;
                    const int64_t o_plan = o_sdesc + align16((ns + 1) * BLK);
                    const int64_t o_seg = o_plan + align16(no * PLAN);
                    const int64_t o_enc = o_seg + align16(nseg * SEG);
                    const int64_t o_cd = o_enc + align16(no * BLK);
                    const int64_t o_srcn = o_cd + align16(no * BLK);
                    const int64_t o_ret = o_srcn + align16((ns + 1) * 4);
                    const int64_t o_crc = o_ret + align16(no * 4);
                    const int64_t o_out = o_crc + align16(no * 4);
                    const ChainLayout L(tin, ns, ns, no, nseg, ChainFlags{false, true, true, false, false});
                    CHECK(L.sdesc == o_sdesc && L.plan == o_plan && L.seg == o_seg && L.enc == o_enc && L.ocd == o_cd &&
                              L.srcn == o_srcn && L.ret == o_ret && L.ocrc == o_crc && L.out == o_out,
                          "compaction layout %lld %lld %lld", (long long)ns, (long long)no, (long long)nseg);
                    CHECK(L.h2d == o_ret && L.results == o_srcn, "compaction copies %lld %lld", (long long)ns, (long long)no);
                }
                {
                    const int64_t o_sdesc = tin;
                    const int64_t o_plan = o_sdesc + align16((ns + 1) * BLK);
                    const int64_t o_seg = o_plan + align16(no * PLAN);
                    const int64_t o_enc = o_seg + align16(nseg * SEG);
                    const int64_t o_cd = o_enc + align16(no * BLK);
                    const int64_t o_sad = o_cd + align16(no * BLK);
                    const int64_t o_oad = o_sad + align16(ns * AEAD);
                    const int64_t o_kn = o_oad + align16(no * AEAD);
                    const int64_t o_seed = o_kn + 64 * (ns + no);
                    const int64_t o_srcn = o_seed + align16(no * 4);
                    const int64_t o_open = o_srcn + align16((ns + 1) * 4);
                    const int64_t o_ret = o_open + align16(ns * 4);
                    const int64_t o_r2 = o_ret + align16(no * 4);
                    const int64_t o_crc = o_r2 + align16(no * 4);
                    const int64_t o_out = o_crc + align16(no * 4);
                    const ChainLayout L(tin, ns, ns, no, nseg, ChainFlags{true, true, true, false, false});
                    CHECK(L.sdesc == o_sdesc && L.plan == o_plan && L.seg == o_seg && L.enc == o_enc && L.ocd == o_cd &&
                              L.sad == o_sad && L.oad == o_oad && L.kn == o_kn && L.oseed == o_seed && L.srcn == o_srcn &&
                              L.open == o_open && L.ret == o_ret && L.r2 == o_r2 && L.ocrc == o_crc && L.out == o_out,
                          "sealed compaction layout %lld %lld %lld", (long long)ns, (long long)no, (long long)nseg);
                    CHECK(L.h2d == o_open && L.results == o_srcn, "sealed compaction copies %lld %lld", (long long)ns,
                          (long long)no);
                }
                for (int64_t n : {ns, ns + 2})
                    for (bool prefix : {false, true}) {
                        const int64_t o_sdesc = tin;
                        const int64_t o_plan = o_sdesc + align16((ns + 1) * BLK);
                        const int64_t o_seg = o_plan + align16(no * PLAN);
                        const int64_t o_tf = o_seg + align16(nseg * SEG);
                        const int64_t o_sad = o_tf + align16((no + 1) * 4);
                        const int64_t o_kn = o_sad + align16(ns * AEAD);
                        const int64_t o_cd = o_kn + 64 * ns;
                        const int64_t o_seed = o_cd + align16(n * BLK);
                        const int64_t o_len = o_seed + align16(n * 4);
                        const int64_t o_exp = o_len + align16(n * 4);
                        const int64_t o_want = o_exp + align16(n * 4);
                        const int64_t o_srcn = o_want + (prefix ? align16(ns * 4) : 0);
                        const int64_t o_open = o_srcn + align16((ns + 1) * 4);
                        const int64_t o_ret = o_open + align16(ns * 4);
                        const int64_t o_crc = o_ret + align16(no * 4);
                        const int64_t o_got = o_crc + align16(n * 4);
                        const int64_t o_out = o_got + align16(n * 4);
                        const ChainLayout L(tin, ns, n, no, nseg, ChainFlags{true, false, false, true, prefix});
                        CHECK(L.sdesc == o_sdesc && L.plan == o_plan && L.seg == o_seg && L.tf == o_tf && L.sad == o_sad &&
                                  L.kn == o_kn && L.scd == o_cd && L.sseed == o_seed && L.len == o_len && L.exp == o_exp &&
                                  L.want == o_want && L.srcn == o_srcn && L.open == o_open && L.ret == o_ret &&
                                  L.scrc == o_crc && L.got == o_got && L.out == o_out,
                              "read layout %lld %lld %lld %lld %d", (long long)ns, (long long)n, (long long)no,
                              (long long)nseg, (int)prefix);
                        CHECK(L.h2d == o_open && L.results == o_srcn, "read copies %lld %lld", (long long)ns, (long long)no);
                    }
            }
}

static void offsets() {
    // three staged objects, two of them decoded; two outputs
    const std::vector<ChainSrc> st = {{0, 0, 0, 100, 1000, false, 0}, {2, 31, 19, 33, 4096, false, 0}, {1, 0, 0, 7, 0, true, 5}};
    const std::vector<ChainOut> oo = {{0, 500, 700, 684, 31}, {1, 17, 48, 32, 31}};
    const ChainOffsets a = chain_offsets(st, 2, oo, true, true);
    CHECK((a.in == std::vector<int64_t>{0, 112, 160}) && a.tin == 176, "staged inputs");
    CHECK((a.dec == std::vector<int64_t>{0, 1008}), "decoded sources");
    CHECK((a.out == std::vector<int64_t>{0, 704}) && a.tout == 752, "output areas");
    CHECK((a.gat == std::vector<int64_t>{5104, 5616}) && a.scratch == 5648, "gathered blocks behind the decoded sources");
    const ChainOffsets b = chain_offsets(st, 2, oo, true, false);  // a read: gathered in place
    CHECK(b.in == a.in && b.dec == a.dec && b.out == a.out && b.gat.empty() && b.scratch == 5104, "read offsets");
    const ChainOffsets c = chain_offsets(st, 2, oo, false, true);  // "none": the staged bytes are the decoded blocks
    CHECK(c.in == a.in && c.out == a.out && c.dec.empty() && c.gat.empty() && c.scratch == 0, "offsets without a codec");
    CHECK(chain_max_total(oo) == 500 && chain_max_total({}) == 0, "max_total");
}

// ---------------------------------------------------------------------------
// plan functions
// ---------------------------------------------------------------------------
static void plan_functions() {
    // four sources; 1 was answered on the host, 3 is unused.  Outputs: 0 reads
    // 0 and 2 around a hole, 1 reads 1 (dead), 2 is a hole only, 3 is empty.
    const std::vector<int> src_map = {0, -1, 1, 2};
    const int ns = 3;
    const jfs_compact_seg seg[] = {{0, 10, 0, 50}, {-1, 0, 50, 6}, {2, 0, 56, 300}, {0, 40, 356, 30},
                                   {2, 100, 0, 8},  {1, 0, 8, 1},   {-1, 0, 0, 9}};
    const int32_t seg_first[] = {0, 4, 6, 7, 7};
    const bool dead[] = {false, true, false, false};
    for (int j = 0; j < 4; j++) CHECK(chain_dead(seg_first, seg, j, src_map) == dead[j], "dead %d", j);
    const int want_src[] = {0, -1, 1, 0, 1, ns, -1};
    for (int k = 0; k < 7; k++) {
        const jfs_compact_seg s = chain_remap(seg[k], src_map, ns);
        CHECK(s.src == want_src[k] && s.src_off == seg[k].src_off && s.dst_off == seg[k].dst_off && s.len == seg[k].len,
              "remap of segment %d: src %d", k, s.src);
    }
    const std::vector<int64_t> need = chain_need(4, 4, seg_first, seg);
    CHECK((need == std::vector<int64_t>{70, 1, 300, 0}), "need %lld %lld %lld %lld", (long long)need[0], (long long)need[1],
          (long long)need[2], (long long)need[3]);
    CHECK(chain_need(0, 0, seg_first, seg).empty(), "need of an empty call");

    // prefix mode: staged sources are 0, 2, 3 (the caller's indices)
    std::vector<ChainSrc> st = {{0, 0, 0, 40, 100, false, 0}, {2, 0, 0, 90, 300, false, 0}, {3, 0, 0, 5, 64, false, 0}};
    int64_t max_want = -1;
    std::vector<int32_t> want = chain_want(need.data(), st, 3, &max_want);
    CHECK((want == std::vector<int32_t>{70, 300, 0}) && max_want == 300, "want: a prefix of source 0, none of source 3");
    // every source needed up to (or past) its capacity: prefix mode is off
    st[0].cap = 70;
    st[2].cap = 0;
    want = chain_want(need.data(), st, 3, &max_want);
    CHECK(want.empty() && max_want == 300, "whole sources take the full launchers");
    st[0].cap = 60;  // need past the capacity is clamped, still whole
    CHECK(chain_want(need.data(), st, 3, &max_want).empty(), "need past the capacity");
    st[0].cap = 71;
    want = chain_want(need.data(), st, 3, &max_want);
    CHECK((want == std::vector<int32_t>{70, 300, 0}), "one byte short of whole");
    CHECK(chain_want(need.data(), st, 0, &max_want).empty() && max_want == 0, "no sources");
}

// ---------------------------------------------------------------------------
// what the host answers for a source
// ---------------------------------------------------------------------------
// [klen:2 | nlen:1 | wrapped key | nonce | payload]
static std::vector<uint8_t> envelope(int klen, int nlen, int pay) {
    std::vector<uint8_t> e(3 + klen + nlen + pay, 0xA5);
    e[0] = (uint8_t)(klen >> 8);
    e[1] = (uint8_t)klen;
    e[2] = (uint8_t)nlen;
    return e;
}

static void expect_answer(const char *what, int algo, bool sealed, const std::vector<uint8_t> &obj, int64_t dst_cap,
                          int64_t want, int64_t off = 0, int64_t noff = 0, int64_t pay = -1) {
    const jfs_iov v{obj.empty() ? nullptr : obj.data(), (int64_t)obj.size(), nullptr, dst_cap};
    ChainSrc r{7, -5, -5, -5, 123, true, 9};
    const int64_t got = chain_src_answer(algo, sealed, v, r);
    if (pay < 0) pay = (int64_t)obj.size();  // answered: the whole object, as staged for a checksum
    CHECK(got == want, "%s: answer %lld, want %lld", what, (long long)got, (long long)want);
    CHECK(r.off == off && r.noff == noff && r.pay == pay, "%s: off %lld noff %lld pay %lld", what, (long long)r.off,
          (long long)r.noff, (long long)r.pay);
    CHECK(r.idx == 7 && r.cap == 123 && r.check && r.expect == 9, "%s: the other fields are the caller's", what);
}

static void answers() {
    const int L = JFS_ALGO_LZ4, Z = JFS_ALGO_ZSTD, N = JFS_ALGO_NONE;
    for (int algo : {N, L, Z}) {
        // malformed headers
        expect_answer("no bytes", algo, true, {}, 100, JFS_ERR_CORRUPT);
        expect_answer("two bytes", algo, true, {0, 0}, 100, JFS_ERR_CORRUPT);
        expect_answer("key longer than the object", algo, true, {1, 0, 12, 1, 2, 3}, 100, JFS_ERR_CORRUPT);
        expect_answer("no payload", algo, true, envelope(256, 12, 0), 100, JFS_ERR_CORRUPT);
        // the AEADs take 12-byte nonces
        expect_answer("nonce of 11", algo, true, envelope(256, 11, 64), 100, JFS_ERR_CORRUPT);
        expect_answer("nonce of 16", algo, true, envelope(256, 16, 64), 100, JFS_ERR_CORRUPT);
        // payloads around the tag's 16 bytes
        expect_answer("payload 15", algo, true, envelope(256, 12, 15), 100, JFS_ERR_AUTH);
        if (algo == N) expect_answer("payload 16, none", algo, true, envelope(256, 12, 16), 0, JFS_OK, 271, 259, 16);
        else expect_answer("payload 16, codec", algo, true, envelope(256, 12, 16), 100, JFS_ERR_EMPTY_INPUT);
        expect_answer("payload 17", algo, true, envelope(256, 12, 17), 100, JFS_OK, 271, 259, 17);
        expect_answer("payload 17, no wrapped key", algo, true, envelope(0, 12, 17), 100, JFS_OK, 15, 3, 17);
        // the plain calls: pre_answer's rules
        expect_answer("plain, empty", algo, false, {}, 100, algo == N ? (int64_t)JFS_OK : JFS_ERR_EMPTY_INPUT);
        expect_answer("plain", algo, false, std::vector<uint8_t>(40, 1), 40, JFS_OK);
        expect_answer("plain, dst_cap one short", algo, false, std::vector<uint8_t>(40, 1), 39,
                      algo == N ? JFS_ERR_SHORT_BUFFER : (int64_t)JFS_OK);
        // an envelope is just bytes to a plain call
        expect_answer("plain, envelope bytes", algo, false, envelope(256, 11, 3), 1000, JFS_OK);
    }
    // "none" copies the opened payload: dst_cap against payload - 16
    expect_answer("none, dst_cap one short", N, true, envelope(256, 12, 116), 99, JFS_ERR_SHORT_BUFFER);
    expect_answer("none, dst_cap exact", N, true, envelope(256, 12, 116), 100, JFS_OK, 271, 259, 116);
    // a codec's capacity is the caller's business
    expect_answer("lz4, dst_cap 0", L, true, envelope(256, 12, 116), 0, JFS_OK, 271, 259, 116);
    expect_answer("zstd, dst_cap 0", Z, true, envelope(256, 12, 116), 0, JFS_OK, 271, 259, 116);

    int64_t woff = 0, wlen = 0, noff = 0, nlen = 0;
    const std::vector<uint8_t> e = envelope(300, 12, 20);
    CHECK(envelope_parse(e.data(), (int64_t)e.size(), &woff, &wlen, &noff, &nlen) == 315 && woff == 3 && wlen == 300 &&
              noff == 303 && nlen == 12,
          "envelope_parse");
}

int main() {
    layout_invariants();
    layout_tables();
    offsets();
    plan_functions();
    answers();
    if (g_fail) {
        fprintf(stderr, "%d chain plan checks FAILED\n", g_fail);
        return 1;
    }
    printf("chain plan check OK\n");
    return 0;
}
