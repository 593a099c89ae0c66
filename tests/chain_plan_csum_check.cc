// Checks the read calls' disk-cache checksum planning in
// juicefs_amd/csrc/chain_plan.h on a CPU: the piece prefix and the checksum
// offsets (chain_csum_pieces), that a call which does not ask for checksums is
// laid out byte for byte as before the "reads' checksums" flag existed, and
// that with the flag on every area keeps to itself.  Built and run by
// tests/test_chain_plan_csum.py under ASan + UBSan.
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
// piece prefix and checksum offsets
// ---------------------------------------------------------------------------
static std::vector<ChainOut> outs_of(const std::vector<int64_t> &totals) {
    std::vector<ChainOut> oo;
    for (size_t k = 0; k < totals.size(); k++) oo.push_back({(int)k, totals[k], totals[k], 0, 0});
    return oo;
}

static void pieces() {
    // Go's ((n-1)/csBlock+1) words: 1 for n = 0
    const std::vector<int64_t> totals = {0, 1, 32767, 32768, 32769, 3 * 32768 + 5};
    const int64_t words[] = {1, 1, 1, 1, 2, 4};
    for (size_t k = 0; k < totals.size(); k++)
        CHECK(csum_pieces(totals[k]) == words[k], "total %lld: %lld pieces", (long long)totals[k],
              (long long)csum_pieces(totals[k]));
    CHECK(CSUM_PIECE == 32768, "piece size");
    const std::vector<ChainOut> oo = outs_of(totals);
    std::vector<int32_t> pf;
    std::vector<int64_t> off;
    {  // every read wants one
        const int64_t np = chain_csum_pieces(oo, std::vector<uint8_t>(6, 1), pf, off);
        CHECK(np == 10, "all wanted: %lld pieces", (long long)np);
        CHECK((pf == std::vector<int32_t>{0, 1, 2, 3, 4, 6, 10}), "all wanted: prefix");
        CHECK((off == std::vector<int64_t>{0, 4, 8, 12, 16, 24}), "all wanted: offsets");
    }
    {  // none does: no pieces, and a prefix of zeros
        const int64_t np = chain_csum_pieces(oo, std::vector<uint8_t>(6, 0), pf, off);
        CHECK(np == 0 && pf == std::vector<int32_t>(7, 0) && off == std::vector<int64_t>(6, 0), "none wanted");
        const int64_t np2 = chain_csum_pieces(oo, {}, pf, off);  // a short mask reads as "not wanted"
        CHECK(np2 == 0 && pf == std::vector<int32_t>(7, 0), "empty mask");
    }
    // every mask over the six totals: a read that is not wanted has no pieces
    // and shares its start with the next one; a wanted one starts at 4 x its
    // first piece and is followed by its own piece count
    for (int bits = 0; bits < 64; bits++) {
        std::vector<uint8_t> want(6);
        for (int k = 0; k < 6; k++) want[k] = (bits >> k) & 1;
        const int64_t np = chain_csum_pieces(oo, want, pf, off);
        int64_t run = 0;
        CHECK(pf.size() == 7 && off.size() == 6, "mask %d: sizes", bits);
        for (int k = 0; k < 6; k++) {
            CHECK(pf[k] == run && off[k] == 4 * run, "mask %d read %d: first piece %d, offset %lld, want %lld", bits, k,
                  (int)pf[k], (long long)off[k], (long long)run);
            if (want[k]) run += words[k];
        }
        CHECK(pf[6] == run && np == run, "mask %d: %lld pieces, want %lld", bits, (long long)np, (long long)run);
    }
    {  // first, last and interior entries of a longer batch; no outputs at all
        std::vector<int64_t> t;
        std::vector<uint8_t> want;
        for (int k = 0; k < 40; k++) {
            t.push_back(4096 + 9000 * k);
            want.push_back(k % 3 != 0);
        }
        const int64_t np = chain_csum_pieces(outs_of(t), want, pf, off);
        int64_t run = 0;
        for (int k = 0; k < 40; k++) {
            CHECK(pf[k] == run, "batch read %d", k);
            if (want[k]) run += (t[k] - 1) / 32768 + 1;
        }
        CHECK(np == run && pf[40] == run, "batch total");
        CHECK(chain_csum_pieces({}, {}, pf, off) == 0 && pf == std::vector<int32_t>{0} && off.empty(), "no outputs");
    }
    {  // more pieces than an int32 holds: refused
        std::vector<int64_t> t(3, (int64_t)INT32_MAX);
        std::vector<ChainOut> big = outs_of(t);
        for (ChainOut &o : big) o.total = (int64_t)INT32_MAX * 32768;
        CHECK(chain_csum_pieces(big, std::vector<uint8_t>(3, 1), pf, off) == -1, "piece count overflow");
    }
}

// ---------------------------------------------------------------------------
// layout
// ---------------------------------------------------------------------------
// The layout as ChainLayout computed it before the reads' checksums: the same
// chain of areas, written out again here.
struct Before {
    int64_t sdesc, plan, seg, tf, enc, ocd, sad, oad, kn, oseed, scd, sseed, len, exp, want, srcn, open, ret, r2, ocrc, scrc,
        got, out, h2d, results;
};

static Before before(int64_t tin, int64_t ns, int64_t n, int64_t no, int64_t nseg, bool sealed, bool encode, bool out_crc,
                     bool src_crc, bool prefix) {
    Before b;
    int64_t o = align16(tin);
    auto take = [&o](bool used, int64_t count, int64_t size) {
        const int64_t at = o;
        if (used) o += align16(count * size);
        return at;
    };
    b.sdesc = take(true, ns + 1, BLK);
    b.plan = take(true, no, PLAN);
    b.seg = take(true, nseg, SEG);
    b.tf = take(!encode, no + 1, 4);
    b.enc = take(encode, no, BLK);
    b.ocd = take(out_crc, no, BLK);
    b.sad = take(sealed, ns, AEAD);
    b.oad = take(sealed && encode, no, AEAD);
    b.kn = take(sealed, ns + (encode ? no : 0), 64);
    b.oseed = take(sealed && out_crc, no, 4);
    b.scd = take(src_crc, n, BLK);
    b.sseed = take(src_crc, n, 4);
    b.len = take(src_crc, n, 4);
    b.exp = take(src_crc, n, 4);
    b.want = take(prefix, ns, 4);
    b.results = b.srcn = take(true, ns + 1, 4);
    b.h2d = o;
    b.open = take(sealed, ns, 4);
    b.ret = take(true, no, 4);
    b.r2 = take(sealed && encode, no, 4);
    b.ocrc = take(out_crc, no, 4);
    b.scrc = take(src_crc, n, 4);
    b.got = take(src_crc, n, 4);
    b.out = o;
    return b;
}

static bool same(const ChainLayout &L, const Before &b) {
    return L.sdesc == b.sdesc && L.plan == b.plan && L.seg == b.seg && L.tf == b.tf && L.enc == b.enc && L.ocd == b.ocd &&
           L.sad == b.sad && L.oad == b.oad && L.kn == b.kn && L.oseed == b.oseed && L.scd == b.scd && L.sseed == b.sseed &&
           L.len == b.len && L.exp == b.exp && L.want == b.want && L.srcn == b.srcn && L.open == b.open && L.ret == b.ret &&
           L.r2 == b.r2 && L.ocrc == b.ocrc && L.scrc == b.scrc && L.got == b.got && L.out == b.out && L.h2d == b.h2d &&
           L.results == b.results;
}

// what the calls pass today: compaction plain and sealed (with the outputs'
// CRC), reads plain and sealed (with the sources' CRC); prefix mode rides on
// the reads
struct Combo {
    const char *name;
    bool sealed, encode, out_crc, src_crc;
};
static const Combo COMBOS[] = {{"jfs_compact_batch", false, true, true, false},
                               {"jfs_compact_seal_batch", true, true, true, false},
                               {"jfs_read_batch", false, false, false, true},
                               {"jfs_read_open_batch", true, false, false, true}};

static void layout_off_is_unchanged() {
    const int64_t nss[] = {0, 1, 3}, nos[] = {0, 1, 4}, nsegs[] = {0, 1, 7}, tins[] = {0, 48, 4099};
    for (const Combo &c : COMBOS)
        for (bool prefix : {false, true})
            for (int64_t ns : nss)
                for (int64_t n : {ns, ns + 2})
                    for (int64_t no : nos)
                        for (int64_t nseg : nsegs)
                            for (int64_t tin : tins) {
                                const Before b = before(tin, ns, n, no, nseg, c.sealed, c.encode, c.out_crc, c.src_crc, prefix);
                                // the initialiser the runners use today leaves the new flag off
                                const ChainFlags f5{c.sealed, c.encode, c.out_crc, c.src_crc, prefix};
                                CHECK(!f5.read_csum, "%s: five initialisers switch the flag on", c.name);
                                const ChainLayout L5(tin, ns, n, no, nseg, f5);
                                CHECK(same(L5, b), "%s prefix %d (%lld %lld %lld %lld %lld): layout moved", c.name, (int)prefix,
                                      (long long)tin, (long long)ns, (long long)n, (long long)no, (long long)nseg);
                                // ... and so does the flag spelled out, whatever piece count comes with it
                                const ChainFlags f6{c.sealed, c.encode, c.out_crc, c.src_crc, prefix, false};
                                const ChainLayout L6(tin, ns, n, no, nseg, f6, 77);
                                CHECK(same(L6, b), "%s prefix %d: layout moved with the flag off", c.name, (int)prefix);
                                // the two new areas have no bytes and sit where the next one starts
                                CHECK(L5.pf == L5.srcn && L5.csum == L5.out && L6.pf == L6.srcn && L6.csum == L6.out,
                                      "%s: an unused area has bytes", c.name);
                            }
}

struct Area {
    const char *name;
    int64_t off, bytes;
    bool host;
};

static void layout_on() {
    const int64_t nss[] = {0, 1, 3}, nos[] = {1, 4, 40}, nsegs[] = {1, 7}, tins[] = {0, 48}, nps[] = {1, 3, 4, 131};
    for (int bits = 0; bits < 32; bits++)
        for (int64_t ns : nss)
            for (int64_t n : {ns, ns + 2})
                for (int64_t no : nos)
                    for (int64_t nseg : nsegs)
                        for (int64_t tin : tins)
                            for (int64_t np : nps) {
                                const bool sealed = bits & 1, encode = bits & 2, out_crc = bits & 4, src_crc = bits & 8,
                                           prefix = bits & 16, seal = sealed && encode;
                                const ChainFlags f{sealed, encode, out_crc, src_crc, prefix, true};
                                const ChainLayout L(tin, ns, n, no, nseg, f, np);
                                const std::vector<Area> a = {
                                    {"sdesc", L.sdesc, (ns + 1) * BLK, true},
                                    {"plan", L.plan, no * PLAN, true},
                                    {"seg", L.seg, nseg * SEG, true},
                                    {"tf", L.tf, encode ? 0 : (no + 1) * 4, true},
                                    {"enc", L.enc, encode ? no * BLK : 0, true},
                                    {"ocd", L.ocd, out_crc ? no * BLK : 0, true},
                                    {"sad", L.sad, sealed ? ns * AEAD : 0, true},
                                    {"oad", L.oad, seal ? no * AEAD : 0, true},
                                    {"kn", L.kn, sealed ? 64 * (ns + (encode ? no : 0)) : 0, true},
                                    {"oseed", L.oseed, sealed && out_crc ? no * 4 : 0, true},
                                    {"scd", L.scd, src_crc ? n * BLK : 0, true},
                                    {"sseed", L.sseed, src_crc ? n * 4 : 0, true},
                                    {"len", L.len, src_crc ? n * 4 : 0, true},
                                    {"exp", L.exp, src_crc ? n * 4 : 0, true},
                                    {"want", L.want, prefix ? ns * 4 : 0, true},
                                    {"pf", L.pf, (no + 1) * 4, true},
                                    {"srcn", L.srcn, (ns + 1) * 4, true},
                                    {"open", L.open, sealed ? ns * 4 : 0, false},
                                    {"ret", L.ret, no * 4, false},
                                    {"r2", L.r2, seal ? no * 4 : 0, false},
                                    {"ocrc", L.ocrc, out_crc ? no * 4 : 0, false},
                                    {"scrc", L.scrc, src_crc ? n * 4 : 0, false},
                                    {"got", L.got, src_crc ? n * 4 : 0, false},
                                    {"csum", L.csum, np * 4, false},
                                };
                                CHECK(a[0].off == tin, "flags %d: the meta starts behind the stored bytes", bits);
                                for (size_t k = 0; k < a.size(); k++) {
                                    const int64_t end = a[k].off + a[k].bytes;
                                    CHECK(a[k].off % 16 == 0, "flags %d %s: offset %lld", bits, a[k].name, (long long)a[k].off);
                                    // no two areas overlap: each one ends where a later one starts, or before
                                    for (size_t q = k + 1; q < a.size(); q++)
                                        CHECK(end <= a[q].off, "flags %d: %s [%lld, %lld) runs into %s at %lld", bits, a[k].name,
                                              (long long)a[k].off, (long long)end, a[q].name, (long long)a[q].off);
                                    CHECK(end <= L.out, "flags %d %s: runs into the output area", bits, a[k].name);
                                    // host-written areas go down in the one H2D copy; the device's come back in the one D2H copy
                                    if (a[k].host) CHECK(end <= L.h2d, "flags %d %s: host-written, but behind the H2D copy", bits, a[k].name);
                                    else CHECK(a[k].off >= L.h2d && a[k].off >= L.results, "flags %d %s: a result outside the D2H copy", bits, a[k].name);
                                }
                                // [0, h2d) goes down, [results, out + reads) comes back; the preset
                                // source lengths lie in both, the checksums directly in front of the reads
                                CHECK(L.results == L.srcn && L.results <= L.h2d && L.h2d <= L.out, "flags %d: results %lld h2d %lld out %lld",
                                      bits, (long long)L.results, (long long)L.h2d, (long long)L.out);
                                CHECK(L.pf + align16((no + 1) * 4) == L.srcn, "flags %d: the prefix is the last staged area before srcn", bits);
                                CHECK(L.csum + align16(np * 4) == L.out, "flags %d: the checksums end where the reads start", bits);
                                // the flag adds exactly its two areas
                                const ChainLayout L0(tin, ns, n, no, nseg, ChainFlags{sealed, encode, out_crc, src_crc, prefix});
                                CHECK(L.out - L0.out == align16((no + 1) * 4) + align16(np * 4), "flags %d: the flag costs %lld bytes", bits,
                                      (long long)(L.out - L0.out));
                            }
}

int main() {
    pieces();
    layout_off_is_unchanged();
    layout_on();
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("chain plan csum check OK\n");
    return 0;
}
