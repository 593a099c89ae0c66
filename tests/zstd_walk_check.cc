// Stand-alone check of juicefs_amd/csrc/zstd_walk.h (the Zstd decoder's shared
// frame / block walk and its stop rule) on a CPU: tests/test_zstd_walk.py
// builds it with g++ (ASan + UBSan where available), dumps frames made by
// tests/zstd_frames.py and the golden frames into a file and passes its name.
//
// File: u32 ncases, then per case
//   u32 n; i32 cap; i32 want; i32 blocks; i32 stopped; i32 fends; u32 has_totals;
//   u32 n_items, lit_bytes, n_cblk, n_blk;  n source bytes
// blocks / stopped / fends: what a walk with `want` must see (blocks walked,
// whether the rule fired, frame ends run); -1 = not checked.  has_totals: the
// four values are zscan_one's for want = INT32_MAX, recorded before the rule
// existed.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../juicefs_amd/csrc/zstd_walk.h"

using namespace jfs::zstdd;

static int g_fail = 0;
#define CHECK(c, ...)                                 \
    do {                                              \
        if (!(c)) {                                   \
            g_fail++;                                 \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                      \
            printf("\n");                             \
        }                                             \
    } while (0)

struct Seen {
    int blocks, stopped, fends, errors;
    int64_t lb;
};

// the walk as every stage drives it: lb advanced as zscan_one does
template <bool STOP>
static Seen drive(const uint8_t *s, int32_t n, int32_t cap, int32_t want) {
    Walk w;
    walk_init(w, s, n, cap, want);
    Seen r = {0, 0, 0, 0, 0};
    for (;;) {
        int32_t err = 0;
        uint32_t fl = 0, chk = 0;
        const int ev = walk_next<STOP>(w, &err, &fl, &chk);
        if (ev == EV_DONE) break;
        if (ev == EV_ERROR) { r.errors++; break; }
        if (ev == EV_FEND) {
            r.fends++;
            if (fl & FE_MISSING) break;
            continue;
        }
        if (ev != EV_BLOCK) continue;
        r.blocks++;
        if (w.btype != 2) { w.lb += w.bsize; continue; }
        LitHdr h;
        if (lit_header(w.s, w.bpos, w.bsize, h)) break;
        int32_t nseq = 0, used = 0;
        if (nbseq_header(w.s, w.bpos + h.sec, w.bpos + w.bsize, &nseq, &used)) break;
        w.lb += (int64_t)h.regen + 3 * (int64_t)nseq;
    }
    r.stopped = w.stopped;
    r.lb = w.lb;
    // a finished walk stays finished
    int32_t err = 0;
    uint32_t fl = 0, chk = 0;
    if (w.phase == 2) CHECK(walk_next<STOP>(w, &err, &fl, &chk) == EV_DONE, "a finished walk gave an event");
    return r;
}

static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) { printf("usage: zstd_walk_check CASES\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    uint32_t ncases = 0;
    if (!rd(f, &ncases, 4)) return 2;
    int checked_totals = 0, checked_stops = 0;
    for (uint32_t c = 0; c < ncases; c++) {
        uint32_t n = 0, has_totals = 0, tot[4];
        int32_t cap = 0, want = 0, blocks = 0, stopped = 0, fends = 0;
        if (!rd(f, &n, 4) || !rd(f, &cap, 4) || !rd(f, &want, 4) || !rd(f, &blocks, 4) || !rd(f, &stopped, 4) ||
            !rd(f, &fends, 4) || !rd(f, &has_totals, 4) || !rd(f, tot, 16)) {
            printf("case %u: short file\n", c);
            return 2;
        }
        // exactly n bytes on the heap: a read past the input is ASan's to find
        std::vector<uint8_t> src(n);
        if (n && !rd(f, src.data(), n)) { printf("case %u: short file\n", c); return 2; }
        const uint8_t *s = src.data();

        const int32_t w = want_clamp(want, cap);
        CHECK(w >= 0 && w <= (cap > 0 ? cap : 0) && (want < 0 || want > cap || w == want), "case %u: want_clamp(%d, %d) = %d", c,
              want, cap, w);
        const Seen a = drive<true>(s, (int32_t)n, cap, w);
        if (blocks >= 0) CHECK(a.blocks == blocks, "case %u want %d: walked %d blocks, expected %d", c, want, a.blocks, blocks);
        if (stopped >= 0) CHECK(a.stopped == stopped, "case %u want %d: stopped %d, expected %d", c, want, a.stopped, stopped);
        if (fends >= 0) CHECK(a.fends == fends, "case %u want %d: %d frame ends, expected %d", c, want, a.fends, fends);
        if (a.stopped) CHECK(a.lb >= w, "case %u: stopped at lb %lld < want %d", c, (long long)a.lb, w);
        if (blocks >= 0) checked_stops++;

        ZInfo zi;
        memset(&zi, 0, sizeof zi);
        zscan_one<true>(s, (int32_t)n, cap, w, zi);
        CHECK((int)zi.n_blk == a.blocks, "case %u: zscan_one walked %u blocks, the walk %d", c, zi.n_blk, a.blocks);
        CHECK(zinfo_want(zi) == w && zinfo_stopped(zi) == a.stopped, "case %u: ZInfo want %d stopped %d", c, zinfo_want(zi),
              zinfo_stopped(zi));
        CHECK(zi.cap == cap, "case %u: cap", c);

        // want = INT32_MAX: the scan of the full decoder, with or without the rule compiled in
        ZInfo zf, zn;
        memset(&zf, 0, sizeof zf);
        memset(&zn, 0xEE, sizeof zn);
        zscan_one<true>(s, (int32_t)n, cap, INT32_MAX, zf);
        zscan_one<false>(s, (int32_t)n, cap, INT32_MAX, zn);
        CHECK(zf.n_items == zn.n_items && zf.lit_bytes == zn.lit_bytes && zf.n_cblk == zn.n_cblk && zf.n_blk == zn.n_blk,
              "case %u: the scan with the rule at INT32_MAX differs from the scan without it", c);
        CHECK(zn.want_st == 0xEEEEEEEEu, "case %u: the scan without the rule wrote want_st", c);
        CHECK(!zinfo_stopped(zf) || (int64_t)cap == INT32_MAX, "case %u: stopped at INT32_MAX", c);
        // a prefix scan never needs more scratch than the full one
        CHECK(zi.n_items <= zf.n_items && zi.lit_bytes <= zf.lit_bytes && zi.n_cblk <= zf.n_cblk && zi.n_blk <= zf.n_blk,
              "case %u: the prefix scan is larger than the full scan", c);
        if (has_totals) {
            CHECK(zf.n_items == tot[0] && zf.lit_bytes == tot[1] && zf.n_cblk == tot[2] && zf.n_blk == tot[3],
                  "case %u: totals %u %u %u %u, recorded %u %u %u %u", c, zf.n_items, zf.lit_bytes, zf.n_cblk, zf.n_blk,
                  tot[0], tot[1], tot[2], tot[3]);
            checked_totals++;
        }
    }
    fclose(f);
    if (g_fail) { printf("%d checks FAILED\n", g_fail); return 1; }
    printf("zstd walk check OK: %u cases, %d stops, %d recorded totals\n", ncases, checked_stops, checked_totals);
    return 0;
}
