// Host driver of the seek-table parser (juicefs_amd/csrc/zstd_seek.h), built by
// tests/test_zstd_seek_table.py with AddressSanitizer and UBSan.  Every object
// lies in a heap buffer of exactly its length, and the fetch counts an index
// outside [0, n) instead of reading it.
//
//   zstd_seek_main cases FILE      FILE: records u32 len | i32 cap | i32 lo | i32 hi | bytes.
//                                  One line per record: table nf total first count coff doff
//   zstd_seek_main fuzz FILE N     FILE: one valid object.  Parses every prefix of it, N seeded
//                                  random byte strings of 25..600 bytes and N strings that carry a
//                                  table with one field damaged at random, and checks every
//                                  accepted table against the validity list, written out again here.
//   zstd_seek_main plan -          chain_from / chain_want / chain_lo of chain_plan.h on plans with
//                                  holes, unused sources and repeated sources; the seek area of
//                                  ChainLayout moves nothing when unused.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "chain_plan.h"
#include "zstd_seek.h"

using namespace jfs::zseek;

static long g_oob = 0;

struct Buf {
    uint8_t *p;
    int32_t n;
    explicit Buf(const uint8_t *s, int32_t len) : p((uint8_t *)malloc(len > 0 ? (size_t)len : 1)), n(len) {
        if (len > 0) memcpy(p, s, (size_t)len);
    }
    ~Buf() { free(p); }
    Buf(const Buf &) = delete;
};

static Sel parse(const Buf &b, int32_t cap, int32_t lo, int32_t hi) {
    auto fetch = [&](int32_t i) -> uint32_t {
        if (i < 0 || i >= b.n) {
            g_oob++;
            return 0u;
        }
        return b.p[i];
    };
    return seek_select(fetch, b.n, cap, lo, hi);
}

static uint32_t rd32(const uint8_t *p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

// the validity list of jfs_zstd_decompress_range_device, from the bytes
static bool valid(const uint8_t *p, int64_t n, uint64_t *total) {
    if (n < 17 + 8) return false;
    if (rd32(p + n - 4) != 0x8F92EAB1u || p[n - 5] != 0) return false;
    const int64_t nf = rd32(p + n - 9);
    if (nf < 1 || nf > 16384 || 8 * nf + 17 > n) return false;
    const int64_t t = n - (8 * nf + 17);
    if (rd32(p + t) != 0x184D2A5Eu || rd32(p + t + 4) != (uint32_t)(8 * nf + 9)) return false;
    uint64_t cs = 0, ds = 0;
    for (int64_t k = 0; k < nf; k++) {
        const uint32_t c = rd32(p + t + 8 + 8 * k);
        if (c < 1) return false;
        cs += c;
        ds += rd32(p + t + 12 + 8 * k);
    }
    *total = ds;
    return cs == (uint64_t)t && ds <= 0xFFFFFFFFull;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

static std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint8_t tmp[65536];
    size_t k;
    while ((k = fread(tmp, 1, sizeof(tmp), f)) > 0) v.insert(v.end(), tmp, tmp + k);
    fclose(f);
    return v;
}

static int plan_checks() {
    using namespace jfs_plan;
    int bad = 0;
    auto expect = [&](bool ok, const char *what) {
        if (!ok) {
            printf("FAIL %s\n", what);
            bad++;
        }
    };
    // 4 sources: 0 read twice (a repeated source), 1 once from its middle, 2 unused, 3 from byte 0; two holes
    const jfs_compact_seg seg[] = {{0, 5000, 0, 100}, {-1, 0, 100, 50}, {1, 300000, 150, 4096},
                                   {0, 200, 0, 10},   {3, 0, 10, 7},    {-1, 0, 17, 3}};
    const int32_t first[] = {0, 3, 3, 6};  // read 1 is empty
    const std::vector<int64_t> from = chain_from(4, 3, first, seg), need = chain_need(4, 3, first, seg);
    expect(from == std::vector<int64_t>({200, 300000, 0, 0}), "chain_from");
    expect(need == std::vector<int64_t>({5100, 304096, 0, 7}), "chain_need");
    expect(chain_from(0, 0, first, seg).empty() && chain_from(2, 0, first, seg) == std::vector<int64_t>({0, 0}),
           "chain_from of no reads");
    // staged: sources 3, 1, 0 (2 was answered on the host); 1's capacity is below its range
    const std::vector<ChainSrc> st = {{3, 0, 0, 10, 7, false, 0}, {1, 0, 0, 10, 262144, false, 0}, {0, 0, 0, 10, 1 << 22, false, 0}};
    int64_t mw = 0;
    expect(chain_want(need.data(), st, 3, &mw, true) == std::vector<int32_t>({7, 262144, 5100}) && mw == 262144, "want");
    expect(chain_lo(from.data(), st, 3) == std::vector<int32_t>({0, 262144, 200}), "chain_lo");
    // every source needed whole: the prefix modes take the full launchers, seek mode keeps the list
    const std::vector<ChainSrc> one = {{3, 0, 0, 10, 7, false, 0}};
    expect(chain_want(need.data(), one, 1, &mw).empty() && chain_want(need.data(), one, 1, &mw, true).size() == 1, "whole");
    const ChainLayout a(1000, 3, 4, 2, 5, ChainFlags{true, false, false, true, true, true}, 9),
        b(1000, 3, 4, 2, 5, ChainFlags{true, false, false, true, true, true, true}, 9);
    expect(a.from == a.srcn && a.pf + 16 == a.from, "unused seek area has no bytes");
    expect(b.from == a.from && b.srcn == a.srcn + 16 && b.out == a.out + 16 && b.want == a.want && b.h2d == a.h2d + 16,
           "seek area: 3 x 4 bytes rounded to 16, in front of srcn");
    printf("plan bad=%d\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "plan")) return plan_checks();
    const std::vector<uint8_t> file = read_file(argv[2]);
    if (!strcmp(argv[1], "cases")) {
        size_t at = 0;
        while (at + 16 <= file.size()) {
            const uint32_t len = rd32(&file[at]);
            const int32_t cap = (int32_t)rd32(&file[at + 4]), lo = (int32_t)rd32(&file[at + 8]),
                          hi = (int32_t)rd32(&file[at + 12]);
            at += 16;
            if (at + len > file.size()) return 2;
            const Buf b(file.data() + at, (int32_t)len);
            at += len;
            const Sel s = parse(b, cap, lo, hi);
            printf("%d %d %u %d %d %u %u\n", s.table, s.nf, s.total, s.first, s.count, s.coff, s.doff);
        }
        printf("oob=%ld\n", g_oob);
        return g_oob ? 1 : 0;
    }
    if (strcmp(argv[1], "fuzz") || argc < 4) return 2;
    const int N = atoi(argv[3]);
    long accepted = 0, bad = 0, prefixes = 0;
    auto check = [&](const uint8_t *p, int32_t n) {
        const Buf b(p, n);
        const Sel s = parse(b, INT32_MAX, (int32_t)(rnd() % 700) - 50, (int32_t)(rnd() % 700));
        uint64_t total = 0;
        const bool v = valid(b.p, n, &total);
        if ((s.table != 0) != v || (v && s.total != (uint32_t)total)) bad++;
        accepted += s.table;
    };
    for (size_t n = 0; n <= file.size(); n++, prefixes++) check(file.data(), (int32_t)n);
    std::vector<uint8_t> s;
    for (int i = 0; i < N; i++) {
        s.resize(25 + rnd() % 576);
        for (auto &c : s) c = (uint8_t)rnd();
        check(s.data(), (int32_t)s.size());
    }
    // a table that is valid for the bytes in front of it, then one byte of the table changed (half of them)
    for (int i = 0; i < N; i++) {
        const uint32_t nf = 1 + rnd() % 40;
        std::vector<uint32_t> c(nf), d(nf);
        uint32_t body = 0;
        for (uint32_t k = 0; k < nf; k++) {
            c[k] = 1 + rnd() % 6;
            d[k] = rnd() % 9;
            body += c[k];
        }
        s.assign(body, 0);
        for (auto &x : s) x = (uint8_t)rnd();
        auto put = [&](uint32_t v) { for (int j = 0; j < 4; j++) s.push_back((uint8_t)(v >> (8 * j))); };
        put(0x184D2A5Eu);
        put(8 * nf + 9);
        for (uint32_t k = 0; k < nf; k++) { put(c[k]); put(d[k]); }
        put(nf);
        s.push_back(0);
        put(0x8F92EAB1u);
        if (rnd() & 1) s[body + rnd() % (s.size() - body)] ^= (uint8_t)(1u << (rnd() % 8));
        check(s.data(), (int32_t)s.size());
    }
    printf("prefixes=%ld random=%d planted=%d accepted=%ld oob=%ld bad=%ld\n", prefixes, N, N, accepted, g_oob, bad);
    return (g_oob || bad) ? 1 : 0;
}
