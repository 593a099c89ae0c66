// Host driver of the LZ4 origin chase (juicefs_amd/csrc/lz4_chase.h), built
// with AddressSanitizer and UBSan by tests/test_lz4_chase.py.
//
//   lz4_chase_main CASES
//
// CASES: little-endian records [u32 n][u32 stride][n bytes], one LZ4 block each
// (stride 1: every output position; k: every k-th position and quad, for a
// block whose chains are thousands of steps deep).  Per block
// the driver builds the index (entry[], cnt[] per 256-byte segment) with a
// serial token walk over the header's parse, decodes the block with a serial LZ
// interpreter as far as it is well-formed, runs the header's rule for every
// output position -- chase_one, and chase_quad for every aligned quad and, in
// the first 8 KiB, for two ragged masks -- and prints one line:
//   case I n N total T ok A bad B deep C wrong W maxhops H unseen U
// ok / bad / deep: positions answered with a literal index, BAD, DEEP; wrong: a
// literal index whose byte differs from the interpreter's, or a chase_quad
// answer that differs from chase_one's; unseen: literal indexes for positions
// behind the first fault, where the interpreter stopped (the chase sees the
// sequences it visits, so literals behind a faulty match still resolve).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "lz4_chase.h"

namespace lz4s = jfs::lz4s;
namespace lz4c = jfs::lz4c;

// the interpreter: plain LZ4 block decoding with every bound checked; returns the bytes it could define
static std::vector<uint8_t> interpret(const uint8_t *s, int32_t n) {
    std::vector<uint8_t> out;
    int64_t i = 0;
    while (i < n) {
        const uint32_t tok = s[i++];
        int64_t ll = tok >> 4;
        if (ll == 15) {
            uint32_t b;
            do {
                if (i >= n) return out;
                b = s[i++];
                ll += b;
            } while (b == 255);
        }
        if (i + ll > n) return out;
        out.insert(out.end(), s + i, s + i + ll);
        i += ll;
        if (i >= n) return out;
        if (i + 2 > n) return out;
        const int64_t off = s[i] | (s[i + 1] << 8);
        i += 2;
        int64_t ml = tok & 15;
        if (ml == 15) {
            uint32_t b;
            do {
                if (i >= n) return out;
                b = s[i++];
                ml += b;
            } while (b == 255);
        }
        ml += 4;
        if (off < 1 || off > (int64_t)out.size()) return out;
        for (int64_t k = 0; k < ml; k++) out.push_back(out[out.size() - off]);
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int cases = 0;
    for (;; cases++) {
        uint32_t n = 0;
        uint32_t stride = 1;
        if (fread(&n, 4, 1, f) != 1) break;
        if (fread(&stride, 4, 1, f) != 1 || stride < 1) return 2;
        std::vector<uint8_t> src(n);
        if (n && fread(src.data(), 1, n, f) != n) return 2;
        const uint8_t *s = src.data();
        const std::vector<uint8_t> want = interpret(s, (int32_t)n);
        // the index, by a serial walk: a segment's entry is the first token at or behind its first byte
        const int32_t nseg = ((int32_t)n + lz4c::SEG - 1) / lz4c::SEG;
        std::vector<int32_t> entry(nseg, (int32_t)n), cnt(nseg, 0);
        int64_t total = 0;
        {
            int32_t p = 0, k = 0;
            while (p < (int32_t)n) {
                for (; k < nseg && k * lz4c::SEG <= p; k++) {
                    entry[k] = p;
                    cnt[k] = (int32_t)total;
                }
                const lz4s::Tok t = lz4s::parse_rd(s, (int32_t)n, p, false);
                total += (int64_t)t.ll + t.ml;
                if (total > (1 << 28)) return 2;  // (no case is that large)
                p = t.next;
            }
            for (; k < nseg; k++) cnt[k] = (int32_t)total;
        }
        const int32_t cap = (int32_t)total;
        int64_t ok = 0, bad = 0, deep = 0, wrong = 0, unseen = 0;
        uint32_t maxhops = 0;
        std::vector<int32_t> one((size_t)total, 0);
        int64_t asked = 0;
        for (int32_t x = 0; x < (int32_t)total; x += (int32_t)stride, asked++) {
            uint32_t hops = 0;
            const int32_t r = lz4c::chase_one(s, (int32_t)n, cap, entry.data(), cnt.data(), nseg, x, hops);
            one[x] = r;
            maxhops = hops > maxhops ? hops : maxhops;
            if (r == lz4c::BAD) bad++;
            else if (r == lz4c::DEEP) deep++;
            else {
                ok++;
                if (r < 0 || r >= (int32_t)n) wrong++;
                else if (x >= (int32_t)want.size()) unseen++;  // behind a fault that no visited sequence holds
                else if (s[r] != want[x]) wrong++;
            }
        }
        // quads: whole ones, and two ragged masks that open a quad in its middle
        const uint32_t masks[3] = {15u, 6u, 9u};
        for (int32_t x0 = 0; stride == 1 && x0 < (int32_t)total; x0 += 4)
            for (uint32_t m0 : masks) {
                if (m0 != 15u && x0 >= 8192) break;  // (the ragged masks: the block's first 8 KiB)
                uint32_t m = 0;
                for (int i = 0; i < 4; i++)
                    if (((m0 >> i) & 1u) && x0 + i < (int32_t)total) m |= 1u << i;
                if (!m) continue;
                int32_t idx[4];
                uint32_t hops = 0;
                const int32_t rc = lz4c::chase_quad(s, (int32_t)n, cap, entry.data(), cnt.data(), nseg, x0, m, idx, hops);
                bool any_bad = false, any_deep = false;
                for (int i = 0; i < 4; i++)
                    if ((m >> i) & 1u) {
                        any_bad = any_bad || one[x0 + i] == lz4c::BAD;
                        any_deep = any_deep || one[x0 + i] == lz4c::DEEP;
                    }
                if (rc == 0) {
                    for (int i = 0; i < 4; i++)
                        if (((m >> i) & 1u) && idx[i] != one[x0 + i]) wrong++;
                } else if ((rc == lz4c::BAD && !any_bad) || (rc == lz4c::DEEP && !any_deep) ||
                           (rc != lz4c::BAD && rc != lz4c::DEEP)) {
                    wrong++;
                }
            }
        if (stride > 1) total = asked;  // (the line's total: the positions asked)
        printf("case %d n %u total %lld ok %lld bad %lld deep %lld wrong %lld maxhops %u unseen %lld\n", cases, n,
               (long long)total, (long long)ok, (long long)bad, (long long)deep, (long long)wrong, maxhops, (long long)unseen);
    }
    fclose(f);
    printf("cases=%d\n", cases);
    return 0;
}
