// Host driver of the LZ4 window decode's rules (juicefs_amd/csrc/lz4_window.h),
// built with AddressSanitizer and UBSan by tests/test_lz4_window.py.
//
//   lz4_window_main CASES
//
// CASES: little-endian records [u32 n][i32 lo][i32 hi][n bytes], one LZ4 block
// and one window each.  Per record the driver decodes the block with a serial
// LZ interpreter, walks its tokens with the shared parse (lz4_chase.h parse_rd),
// and applies the header's rules as the kernels do:
//   Fc = floor_of(lo), H = min(max(hi, 0), total);
//   below = some sequence reaches_below(Fc, H, ...); F = below ? 0 : Fc;
//   the origin entries of the visited sequences, clipped to [F, E) by clip(),
//   E = min(total, H); every entry of [F, E) resolved by following its pointers.
// and prints one line:
//   case I n N total T fc X below B floor Y wrong W escape E forced G reach R
// wrong: bytes of [F, E) that differ from the interpreter's, or an entry of
// [F, E) no visited sequence wrote; escape: pointers met that leave [F, E) or
// do not go backwards (the floor rule says there are none); forced: the same
// count with the floor held at Fc whatever the probe says (what the probe
// protects against: > 0 exactly where a sequence reaches below); reach: over
// EVERY chunk floor k * CHUNK below total with H = total, the sequences that
// reach below it (the property a fast-parse block has: 0).
// The last line checks the switch's row of host_modes.h.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "host_modes.h"
#include "lz4_window.h"

namespace lz4s = jfs::lz4s;
namespace lz4w = jfs::lz4w;

struct Seq {
    int32_t op, ll, lit, ml, off;  // output position, literals (input position lit), match
};

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

constexpr int32_t UNWRITTEN = 0x7fffffff;

// the windowed decode from floor F: wrong bytes and escaping pointers
static void decode_from(const std::vector<Seq> &seqs, const uint8_t *s, const std::vector<uint8_t> &want, int32_t F,
                        int32_t H, int32_t total, int64_t &wrong, int64_t &escape) {
    const int32_t E = total < H ? total : H;
    std::vector<int32_t> org((size_t)total + 1, UNWRITTEN);  // >= 0: a pointer; < 0: -(input position) - 1
    for (const Seq &q : seqs) {
        if (!lz4w::visited(F, H, q.op, q.ll + q.ml)) continue;
        const lz4w::Clip a = lz4w::clip(q.op, q.ll, F, E);
        for (int32_t i = a.i0; i < a.i1; i++) org[q.op + i] = -(q.lit + i) - 1;
        const int32_t m = q.op + q.ll;
        const lz4w::Clip b = lz4w::clip(m, q.ml, F, E);
        for (int32_t i = b.i0; i < b.i1; i++) org[m + i] = m - q.off + (q.off > 0 ? i % q.off : 0);
    }
    for (int32_t x = F; x < E; x++) {
        int32_t p = x;
        bool lost = false;
        while (true) {
            const int32_t e = org[p];
            if (e == UNWRITTEN) {
                wrong++;
                lost = true;
                break;
            }
            if (e < 0) break;
            if (e < F || e >= p) {
                escape++;
                lost = true;
                break;
            }
            p = e;
        }
        if (lost) continue;
        const int32_t at = -org[p] - 1;
        if (x >= (int32_t)want.size() || s[at] != want[x]) wrong++;
    }
}

static int check_mode_row() {
    using namespace jfs_host;
    const ModeDesc &d = MODE_READ_LZ4_WINDOW;
    int bad = 0;
    bad += strcmp(d.env, "JFS_READ_LZ4_WINDOW") != 0;
    bad += d.def != JFS_READ_LZ4_WINDOW_OFF || d.set_max != JFS_READ_LZ4_WINDOW_ON || d.ext_max != JFS_READ_LZ4_WINDOW_ON;
    const struct {
        const char *s;
        int v;
    } rows[] = {{nullptr, 0}, {"", 0}, {"on", 1}, {"ON", 1}, {"oN", 1}, {"off", 0}, {"OFF", 0}, {"oFf", 0},
                {"onx", 0},   {" on", 0}, {"on ", 0}, {"1", 0}, {"bogus", 0}, {"o", 0}};
    for (const auto &r : rows) bad += mode_parse(d, r.s) != r.v;
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int cases = 0;
    for (;; cases++) {
        uint32_t n = 0;
        int32_t lo = 0, hi = 0;
        if (fread(&n, 4, 1, f) != 1) break;
        if (fread(&lo, 4, 1, f) != 1 || fread(&hi, 4, 1, f) != 1) return 2;
        std::vector<uint8_t> src(n);
        if (n && fread(src.data(), 1, n, f) != n) return 2;
        const uint8_t *s = src.data();
        const std::vector<uint8_t> want = interpret(s, (int32_t)n);
        std::vector<Seq> seqs;
        int64_t total = 0;
        for (int32_t p = 0; p < (int32_t)n;) {
            const lz4s::Tok t = lz4s::parse_rd(s, (int32_t)n, p, true);
            seqs.push_back(Seq{(int32_t)total, t.ll, t.lenip, t.ml, t.off});
            total += (int64_t)t.ll + t.ml;
            if (total > (1 << 28)) return 2;  // (no case is that large)
            p = t.next;
        }
        const int32_t T = (int32_t)total;
        const int32_t H = hi < 0 ? 0 : hi < T ? hi : T;  // (dst_cap = total)
        const int32_t Fc = lz4w::floor_of(lo);
        bool below = false;
        for (const Seq &q : seqs) below = below || (q.ml > 0 && lz4w::reaches_below(Fc, H, q.op + q.ll, q.ml, q.off));
        const int32_t F = below ? 0 : Fc;
        int64_t wrong = 0, escape = 0, w2 = 0, forced = 0, reach = 0;
        decode_from(seqs, s, want, F, H, T, wrong, escape);
        decode_from(seqs, s, want, Fc, H, T, w2, forced);
        for (int32_t fk = lz4w::CHUNK; fk < T; fk += lz4w::CHUNK)
            for (const Seq &q : seqs) reach += q.ml > 0 && lz4w::reaches_below(fk, T, q.op + q.ll, q.ml, q.off);
        printf("case %d n %u total %d fc %d below %d floor %d wrong %lld escape %lld forced %lld reach %lld\n", cases, n, T,
               Fc, (int)below, F, (long long)wrong, (long long)escape, (long long)forced, (long long)reach);
    }
    fclose(f);
    printf("cases=%d modes_bad=%d\n", cases, check_mode_row());
    return 0;
}
