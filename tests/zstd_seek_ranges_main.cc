// Stand-alone driver of the several-ranges selection of
// juicefs_amd/csrc/zstd_seek.h (seek_table / ranges_ok / frame_in_ranges /
// ranges_select), built with AddressSanitizer + UBSan by
// tests/test_zstd_seek_ranges.py.  The fetch it hands the parser counts every
// index outside [0, src_len).
//   cases FILE   records of (u32 src_len, i32 dst_cap, u32 nr, nr x (i32 lo, i32 hi), object bytes);
//                one line per record: "bad live top table checksums nf total count" and then
//                " k:coff:doff:c:d:x" per selected frame; at the end "oob=N"
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

struct Range {
    int32_t lo, hi;
};

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

int main(int argc, char **argv) {
    if (argc < 3 || strcmp(argv[1], "cases")) return 2;
    const std::vector<uint8_t> all = slurp(argv[2]);
    size_t at = 0;
    while (at + 12 <= all.size()) {
        uint32_t len, nr;
        int32_t cap;
        memcpy(&len, &all[at], 4);
        memcpy(&cap, &all[at + 4], 4);
        memcpy(&nr, &all[at + 8], 4);
        at += 12;
        if (at + 8ull * nr + len > all.size()) return 3;
        // copies of exactly the list's and the object's bytes: AddressSanitizer sees a read past either
        std::vector<Range> rng(nr);
        if (nr) memcpy(rng.data(), &all[at], 8ull * nr);
        at += 8ull * nr;
        std::vector<uint8_t> obj(all.begin() + (long)at, all.begin() + (long)(at + len));
        at += len;
        std::vector<unsigned long long> picked;
        int32_t last = -1;
        bool ascending = true;
        const zs::RangesSel s = zs::ranges_select(
            CountingFetch{obj.data(), (int64_t)len}, (int32_t)len, cap, rng.data(), (int32_t)nr,
            [&](int32_t k, uint32_t coff, uint32_t doff, uint32_t c, uint32_t d, uint32_t x) {
                ascending = ascending && k > last;
                last = k;
                picked.insert(picked.end(), {(unsigned long long)k, coff, doff, c, d, x});
            });
        // what an answer must satisfy whatever the bytes were
        if (!ascending || (size_t)s.count * 6 != picked.size() || (s.bad && (s.table || s.count || s.live))) return 4;
        if (s.table && (s.nf < 1 || s.nf > zs::MAX_FRAMES || s.count > s.nf)) return 4;
        if (!s.table && (s.count || s.nf)) return 4;
        printf("%d %d %d %d %d %d %u %d", s.bad, s.live, s.top, s.table, s.checksums, s.nf, s.total, s.count);
        for (size_t q = 0; q < picked.size(); q += 6)
            printf(" %llu:%llu:%llu:%llu:%llu:%llu", picked[q], picked[q + 1], picked[q + 2], picked[q + 3], picked[q + 4],
                   picked[q + 5]);
        printf("\n");
    }
    if (at != all.size()) return 3;
    printf("oob=%ld\n", g_oob);
    return 0;
}
