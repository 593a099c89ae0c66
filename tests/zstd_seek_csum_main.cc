// Stand-alone driver of the stand-alone seek-table parser of
// juicefs_amd/csrc/zstd_seek.h (table_header / table_entry / table_select; both
// layouts), built with AddressSanitizer + UBSan by
// tests/test_zstd_seek_csum.py.  The fetch it hands the parser counts every
// index outside [0, table_len).
//   cases FILE   records of (u32 table_len, i64 object_len, i64 cap, i64 lo, i64 hi, table bytes);
//                one line per record, then "oob=N"
//   fuzz FILE N  FILE = a valid table: every prefix and suffix of it, N random strings, N copies
//                with one bit flipped (object_len kept), each selected over a random range
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "zstd_seek.h"

namespace zs = jfs::zseek;

static long g_oob = 0;
struct CountingFetch {
    const uint8_t *p;
    int64_t n;
    uint32_t operator()(int32_t i) const {
        if (i < 0 || i >= n) {
            g_oob++;
            return 0;
        }
        return p[i];
    }
};

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

static std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

// what a selection must satisfy whatever the bytes were
static bool sane(const zs::TableSel &s, int64_t table_len, int64_t object_len) {
    if (!s.table) return s.count == 0 && s.nf == 0;
    if (s.nf < 1 || s.nf > zs::MAX_FRAMES || s.first < 0 || s.count < 0 || s.first + s.count > s.nf) return false;
    if (s.total > 0xFFFFFFFFull) return false;
    if (s.count == 0) return s.coff == 0 && s.cend == 0;
    return s.coff <= s.cend && s.cend <= (uint64_t)(object_len - table_len) && s.doff <= s.dend && s.dend <= s.total;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "cases")) {
        const std::vector<uint8_t> all = slurp(argv[2]);
        size_t at = 0;
        while (at + 36 <= all.size()) {
            uint32_t tl;
            int64_t q[4];
            memcpy(&tl, &all[at], 4);
            memcpy(q, &all[at + 4], 32);
            at += 36;
            if (at + tl > all.size()) return 3;
            // a copy of exactly table_len bytes: AddressSanitizer sees a read past it
            std::vector<uint8_t> t(all.begin() + (long)at, all.begin() + (long)(at + tl));
            at += tl;
            const zs::TableSel s = zs::table_select(CountingFetch{t.data(), (int64_t)tl}, (int64_t)tl, q[0], q[1], q[2], q[3]);
            if (!sane(s, tl, q[0])) return 4;
            printf("%d %d %d %llu %d %d %llu %llu %llu %llu\n", s.table, s.checksums, s.nf, (unsigned long long)s.total,
                   s.first, s.count, (unsigned long long)s.coff, (unsigned long long)s.cend, (unsigned long long)s.doff,
                   (unsigned long long)s.dend);
        }
        printf("oob=%ld\n", g_oob);
        return 0;
    }
    if (!strcmp(argv[1], "fuzz") && argc >= 4) {
        const std::vector<uint8_t> good = slurp(argv[2]);
        const long n = atol(argv[3]);
        const int64_t tl = (int64_t)good.size();
        int nf = 0, entry = 0;
        if (!zs::table_header(CountingFetch{good.data(), tl}, tl, tl + 1, &nf, &entry)) return 3;
        uint64_t cs = 0;
        for (int k = 0; k < nf; k++) {
            uint32_t c, d, x;
            zs::table_entry(CountingFetch{good.data(), tl}, entry, k, &c, &d, &x);
            cs += c;
        }
        const int64_t object_len = (int64_t)cs + tl;
        long accepted = 0, bad = 0, cuts = 0;
        auto one = [&](const std::vector<uint8_t> &t, int64_t olen) {
            const int64_t lo = (int64_t)(rnd() % 300000) - 1000, hi = lo + (int64_t)(rnd() % 300000) - 100;
            const zs::TableSel s = zs::table_select(CountingFetch{t.data(), (int64_t)t.size()}, (int64_t)t.size(), olen,
                                                    (rnd() & 1) ? -1 : (int64_t)(rnd() % 400000), lo, hi);
            accepted += s.table;
            bad += !sane(s, (int64_t)t.size(), olen);
        };
        for (int64_t k = 0; k <= tl; k++) {  // every prefix and every suffix
            one(std::vector<uint8_t>(good.begin(), good.begin() + k), object_len - (tl - k));
            one(std::vector<uint8_t>(good.begin() + k, good.end()), object_len - k);
            cuts += 2;
        }
        for (long i = 0; i < n; i++) {
            std::vector<uint8_t> r((size_t)(rnd() % 600));
            for (auto &b : r) b = (uint8_t)rnd();
            if (r.size() >= 9 && (i & 1)) {  // a random string under a footer that is one
                const uint32_t m = zs::SEEK_MAGIC;
                memcpy(&r[r.size() - 4], &m, 4);
                r[r.size() - 5] = (i & 2) ? 0x80 : 0;
            }
            one(r, (int64_t)r.size() + (int64_t)(rnd() % 100000));
        }
        for (long i = 0; i < n; i++) {
            std::vector<uint8_t> t = good;
            if (i % 4) t[(size_t)(rnd() % t.size())] ^= (uint8_t)(1u << (rnd() % 8));
            one(t, object_len);
        }
        printf("oob=%ld bad=%ld cuts=%ld random=%ld accepted=%ld\n", g_oob, bad, cuts, n, accepted);
        return 0;
    }
    return 2;
}
