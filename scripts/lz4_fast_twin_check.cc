// Stand-alone check of the fast LZ4 encoder's host twin, meant to be built with
// sanitizers (host code only, no GPU, no Python):
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/lz4_fast_twin_check.cc juicefs_amd/csrc/lz4_fast_host.cc -o /tmp/lz4_fast_twin_check
//   /tmp/lz4_fast_twin_check
//
// Every source and destination is an exact-size heap allocation, so one byte
// read or written outside them is reported.  Each block is decoded again by a
// small LZ4 block decoder written here.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/jfs_gpucodec_lz4_fast_test.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// strict decoder: -1 on any malformed input or a size other than n
static int64_t decode(const uint8_t *s, int64_t sn, uint8_t *d, int64_t n) {
    int64_t i = 0, o = 0;
    for (;;) {
        if (i >= sn) return -1;
        const int tok = s[i++];
        int64_t lit = tok >> 4;
        if (lit == 15) {
            int b;
            do {
                if (i >= sn) return -1;
                b = s[i++];
                lit += b;
            } while (b == 255);
        }
        if (i + lit > sn || o + lit > n) return -1;
        memcpy(d + o, s + i, (size_t)lit);
        i += lit;
        o += lit;
        if (i == sn) return (tok & 15) == 0 && o == n ? o : -1;
        if (i + 2 > sn) return -1;
        const int64_t off = s[i] | s[i + 1] << 8;
        i += 2;
        int64_t ml = tok & 15;
        if (ml == 15) {
            int b;
            do {
                if (i >= sn) return -1;
                b = s[i++];
                ml += b;
            } while (b == 255);
        }
        ml += 4;
        if (off < 1 || off > o || o + ml > n - 5 || o > n - 12) return -1;  // the end rules, too
        for (int64_t k = 0; k < ml; ++k, ++o) d[o] = d[o - off];
    }
}

static int64_t bound(int64_t n) { return n + n / 255 + 16; }

static int check(const std::vector<uint8_t> &src, const char *what) {
    const int64_t n = (int64_t)src.size();
    uint8_t *in = (uint8_t *)malloc((size_t)(n ? n : 1));
    if (n) memcpy(in, src.data(), (size_t)n);
    uint8_t *out = (uint8_t *)malloc((size_t)bound(n));
    const int64_t r = jfs_test_lz4_fast_host(out, bound(n), in, n);
    int bad = 0;
    if (r <= 0 || r > bound(n)) bad = 1;
    if (!bad) {
        uint8_t *back = (uint8_t *)malloc((size_t)(n ? n : 1));
        if (decode(out, r, back, n) != n || (n && memcmp(back, in, (size_t)n))) bad = 2;
        free(back);
        // exactly enough room, then one byte short, in exact-size buffers
        uint8_t *fit = (uint8_t *)malloc((size_t)r);
        if (jfs_test_lz4_fast_host(fit, r, in, n) != r || memcmp(fit, out, (size_t)r)) bad = 3;
        free(fit);
        uint8_t *shorter = (uint8_t *)malloc((size_t)(r > 1 ? r - 1 : 1));
        if (jfs_test_lz4_fast_host(shorter, r - 1, in, n) != 0) bad = 4;
        free(shorter);
    }
    free(out);
    free(in);
    if (bad) fprintf(stderr, "FAIL %s (n = %lld): step %d\n", what, (long long)n, bad);
    return bad != 0;
}

int main() {
    const int64_t lengths[] = {0,  1,     4,     5,     11,    12,    13,     14,     63,
                               64, 65,    65535, 65536, 65537, 65548, 131071, 131072, 200003};
    const int periods[] = {1, 2, 3, 4, 63, 64, 65};
    int fails = 0, runs = 0;
    for (int64_t n : lengths) {
        std::vector<uint8_t> v((size_t)n, 0);
        fails += check(v, "zeros"), ++runs;
        for (int p : periods) {
            for (int64_t i = 0; i < n; ++i) v[(size_t)i] = (uint8_t)(37 * (i % p) + 11 * p);
            fails += check(v, "period"), ++runs;
        }
        for (int64_t i = 0; i < n; ++i) v[(size_t)i] = (uint8_t)rnd();
        fails += check(v, "random"), ++runs;
        // text-like: words from a small vocabulary
        for (int64_t i = 0; i < n;) {
            const uint32_t w = rnd() % 97, len = 2 + w % 9;
            for (uint32_t k = 0; k < len && i < n; ++k) v[(size_t)i++] = (uint8_t)('a' + (w * 7 + k * 3) % 26);
            if (i < n) v[(size_t)i++] = ' ';
        }
        fails += check(v, "words"), ++runs;
    }
    // a few thousand random short inputs over small alphabets (many matches near both ends)
    for (int it = 0; it < 4000; ++it) {
        const int64_t n = rnd() % 700;
        const uint32_t alpha = 1 + rnd() % 6;
        std::vector<uint8_t> v((size_t)n);
        for (auto &b : v) b = (uint8_t)(rnd() % alpha);
        fails += check(v, "short"), ++runs;
    }
    // inputs around the chunk cut with repeats across it
    for (int it = 0; it < 40; ++it) {
        const int64_t n = 65536 - 40 + rnd() % 80 + (it & 1) * 65536;
        std::vector<uint8_t> v((size_t)n);
        const uint32_t per = 1 + rnd() % 300;
        for (int64_t i = 0; i < n; ++i) v[(size_t)i] = (uint8_t)((i % per) * 31 + (i / 9000));
        fails += check(v, "cut"), ++runs;
    }
    printf("%d inputs, %d failures\n", runs, fails);
    return fails ? 1 : 0;
}
