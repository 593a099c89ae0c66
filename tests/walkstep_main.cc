// Host driver for juicefs_amd/csrc/lz4_walkstep.h (tests/test_lz4_walkstep.py):
// the deferred-check walks the kernel's SegWalk runs (ws_spec_iter,
// ws_fix_iter) against plain walks that ask ws_next_exact at every position,
// over the same bytes, from every entry of a 32-byte pre-roll + 128-byte
// segment.  Compared: the visited positions (bit sets), the exit, STOP
// results; every fetch index must lie in [0, n).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lz4_walkstep.h"

using namespace jfs::lz4d;

static constexpr int SEG = 128, SPRE = 32;
static long g_oob = 0, g_bad = 0, g_walks = 0, g_redone = 0, g_arrived = 0, g_fix = 0;

struct Fetch {
    const uint8_t *b;
    int32_t n;
    uint32_t operator()(uint32_t i) const {
        if (i >= (uint32_t)n) {
            g_oob++;
            return 0;
        }
        return b[i];
    }
};

struct Lane {  // the fields of SegWalk the iterations use
    int32_t plo, phi, q;
    uint32_t sx, ex, pe2;
    uint64_t vs0, vs1, vt0, vt1, vp0, vp1;
    bool mv, pend;
};

struct Res {
    uint64_t v0, v1;
    uint32_t exit;
    bool operator==(const Res &o) const { return v0 == o.v0 && v1 == o.v1 && exit == o.exit; }
};

static void fail(const char *what, int32_t n, int32_t plo, int32_t e, const Res &a, const Res &b) {
    if (g_bad++ < 10)
        printf("MISMATCH %s n=%d plo=%d entry=%d: deferred %016llx %016llx exit %08x, plain %016llx %016llx exit %08x\n", what, n,
               plo, e, (unsigned long long)a.v0, (unsigned long long)a.v1, a.exit, (unsigned long long)b.v0,
               (unsigned long long)b.v1, b.exit);
}

// speculative walk from entry e: plain
static Res spec_plain(const Fetch &f, int32_t plo, int32_t e) {
    Res r = {0, 0, 0};
    const int32_t phi = plo + SEG;
    int32_t q = e;
    for (;;) {
        const uint32_t x = ws_next_exact(f, f.n, q);
        const bool stop = (x & WS_STOP) != 0;
        if (!stop && q >= plo) sbit2(r.v0, r.v1, (uint32_t)(q - plo));
        if (stop || (int32_t)x >= phi) {
            r.exit = x;
            return r;
        }
        q = (int32_t)x;
    }
}

static void count(int kind) {
    g_redone += kind == WS_REDONE;
    g_arrived += kind == WS_ARRIVED;
}

static Res spec_deferred(const Fetch &f, int32_t plo, int32_t e, Lane *keep) {
    Lane w;
    memset(&w, 0, sizeof(w));
    w.plo = plo;
    w.phi = plo + SEG;
    w.q = e;
    w.mv = true;
    const auto exact = [&](int32_t p) { return ws_next_exact(f, f.n, p); };
    int it = 0;
    while (w.mv) {
        count(ws_spec_iter(w, f, exact, f.n));
        if (++it > 2 * (SEG + SPRE)) {
            g_bad++;
            printf("speculative walk does not end: n=%d plo=%d entry=%d\n", f.n, plo, e);
            break;
        }
    }
    if (w.pend) {
        g_bad++;
        printf("a finished lane still owes a test: n=%d plo=%d entry=%d\n", f.n, plo, e);
    }
    if (keep) *keep = w;
    return Res{w.vs0, w.vs1, w.sx};
}

// fix-up walk from the true entry in (in [plo, phi), off the chain vs): plain
static Res fix_plain(const Fetch &f, int32_t plo, uint64_t vs0, uint64_t vs1, uint32_t sx, int32_t in) {
    const int32_t phi = plo + SEG;
    uint64_t p0 = 0, p1 = 0;
    int32_t q = in;
    for (;;) {
        const uint32_t d = (uint32_t)(q - plo);
        if (tbit2(vs0, vs1, d)) return Res{p0 | (vs0 & from_lo(d)), p1 | (vs1 & from_hi(d)), sx};
        const uint32_t x = ws_next_exact(f, f.n, q);
        const bool stop = (x & WS_STOP) != 0;
        if (!stop) sbit2(p0, p1, d);
        if (stop || (int32_t)x >= phi) return Res{p0, p1, x};
        q = (int32_t)x;
    }
}

static Res fix_deferred(const Fetch &f, Lane w, int32_t in) {
    // the state SegWalk::advance sets up for a lane whose entry changed to `in`
    w.q = in;
    w.vp0 = w.vp1 = 0;
    w.mv = true;
    const auto exact = [&](int32_t p) { return ws_next_exact(f, f.n, p); };
    int it = 0;
    while (w.mv) {
        count(ws_fix_iter(w, f, exact, f.n));
        if (++it > 2 * SEG) {
            g_bad++;
            printf("fix-up walk does not end: n=%d plo=%d entry=%d\n", f.n, w.plo, in);
            break;
        }
    }
    if (w.pend) {
        g_bad++;
        printf("a finished fix-up lane still owes a test: n=%d plo=%d entry=%d\n", f.n, w.plo, in);
    }
    return Res{w.vt0, w.vt1, w.ex};
}

// every entry of the pre-roll + segment at plo; the fix-up walks against the
// chain the kernel's lane would hold (entry plo - SPRE, or plo for lane 0)
static void check_segment(const uint8_t *b, int32_t n, int32_t plo) {
    const Fetch f{b, n};
    const int32_t lo = plo - SPRE < 0 ? 0 : plo - SPRE;
    for (int32_t e = lo; e < plo + SEG; ++e) {
        const Res a = spec_deferred(f, plo, e, nullptr), p = spec_plain(f, plo, e);
        g_walks++;
        if (!(a == p)) fail("speculative", n, plo, e, a, p);
    }
    for (int lane0 = 0; lane0 < 2; ++lane0) {
        Lane w;
        const Res sp = spec_deferred(f, plo, lane0 ? plo : lo, &w);
        for (int32_t in = plo; in < plo + SEG; ++in) {
            if (tbit2(sp.v0, sp.v1, (uint32_t)(in - plo))) continue;
            const Res a = fix_deferred(f, w, in), p = fix_plain(f, plo, sp.v0, sp.v1, sp.exit, in);
            g_walks++;
            g_fix++;
            if (!(a == p)) fail("fix-up", n, plo, in, a, p);
        }
    }
}

static void check_stream(const std::vector<uint8_t> &s, int32_t n, int stride) {
    // exactly n bytes on the heap: a read past them is the sanitizer's to report
    uint8_t *b = (uint8_t *)malloc((size_t)n);
    memcpy(b, s.data(), (size_t)n);
    for (int32_t plo = 0; plo < n; plo += stride) check_segment(b, n, plo);
    free(b);
}

// ---- streams --------------------------------------------------------------
static uint64_t g_rng;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 11);
}

// one token: ll literals (bytes from lit()), offset bytes, match-length code
// mlc (match length - 4) with explicit extension bytes when mext is given
static void token(std::vector<uint8_t> &s, uint32_t ll, uint32_t mlc, const std::vector<uint8_t> *mext, int litmode) {
    const uint32_t mn = mext ? 15u : (mlc < 15u ? mlc : 15u);
    s.push_back((uint8_t)(((ll < 15u ? ll : 15u) << 4) | mn));
    if (ll >= 15u) {
        uint32_t r = ll - 15u;
        for (; r >= 255u; r -= 255u) s.push_back(255);
        s.push_back((uint8_t)r);
    }
    for (uint32_t i = 0; i < ll; ++i) s.push_back(litmode == 1 ? 255 : litmode == 2 ? (uint8_t)(rnd() % 3 ? 255 : rnd()) : (uint8_t)rnd());
    s.push_back(litmode ? 255 : (uint8_t)rnd());
    s.push_back((uint8_t)rnd());
    if (mext) {
        for (uint8_t v : *mext) s.push_back(v);
    } else if (mlc >= 15u) {
        uint32_t r = mlc - 15u;
        for (; r >= 255u; r -= 255u) s.push_back(255);
        s.push_back((uint8_t)r);
    }
}

static void filler(std::vector<uint8_t> &s, size_t upto, int litmode) {
    while (s.size() < upto) token(s, rnd() % 9, rnd() % 14, nullptr, litmode);
}

static void random_stream(std::vector<uint8_t> &s, uint32_t len) {
    s.clear();
    const uint32_t flavour = rnd() % 4;  // how common the long forms are
    while (s.size() < len) {
        const uint32_t r = rnd() % 100;
        uint32_t ll = rnd() % 12, mlc = rnd() % 15;
        const uint32_t longp = flavour == 0 ? 2 : flavour == 1 ? 8 : flavour == 2 ? 20 : 40;
        if (r < longp) mlc = 15 + rnd() % 700;            // extended match, often >= 270 (a 255 byte)
        else if (r < 2 * longp) mlc = 15 + 255 * (1 + rnd() % 3) + (rnd() % 4 ? rnd() % 255 : 0);
        if (rnd() % 100 < longp / 2) ll = 15 + rnd() % 600;  // extended literal run
        else if (rnd() % 40 == 0) ll = 15 + 255;
        token(s, ll, mlc, nullptr, rnd() % 5 == 0 ? 2 : 0);
    }
    s.resize(len);
}

int main(int argc, char **argv) {
    const long nrandom = argc > 1 ? atol(argv[1]) : 10000;
    g_rng = 0x9E3779B97F4A7C15ull;
    long crafted = 0;
    // crafted: a token of interest (at about byte 300) between plain tokens, every
    // segment position in steps of 7 bytes (the token in the pre-roll, first and
    // last in its segment, its exit in the next lane), then truncated inside
    // each of its fields and the 40 bytes after it (edge, n - 4, n - 18 ...)
    const std::vector<std::vector<uint8_t>> mexts = {{254}, {255, 0}, {255, 255, 7}, {255, 255, 255, 200}, {0}, {255, 254}};
    for (int litmode = 0; litmode < 3; litmode += 2) {  // random literals; mostly 255s
        for (size_t m = 0; m <= mexts.size() + 4; ++m) {
            for (uint32_t ll : {0u, 3u, 15u + 40u, 15u + 255u}) {
                std::vector<uint8_t> s;
                filler(s, 290 + rnd() % 16, litmode);
                const size_t at = s.size();
                if (m < mexts.size()) {
                    token(s, ll, 0, &mexts[m], litmode);
                } else if (m == mexts.size()) {  // no extension, the next token byte is 255
                    token(s, ll, 7, nullptr, litmode);
                    token(s, 15 + 2, 15 + 3, nullptr, litmode);
                } else if (m == mexts.size() + 1) {  // two slow tokens in a row
                    token(s, ll, 0, &mexts[1], litmode);
                    token(s, 2, 0, &mexts[2], litmode);
                } else if (m == mexts.size() + 2) {  // three, the middle one by its literal length
                    token(s, ll, 0, &mexts[2], litmode);
                    token(s, 15 + 255 + 4, 3, nullptr, litmode);
                    token(s, 0, 0, &mexts[1], litmode);
                } else if (m == mexts.size() + 3) {  // a slow token right behind a one-byte literal extension
                    token(s, 15 + 9, 0, &mexts[2], litmode);
                    token(s, ll, 0, &mexts[1], litmode);
                } else {  // a long run of 255 extension bytes (past KEXT)
                    std::vector<uint8_t> e(70, 255);
                    e.push_back(1);
                    token(s, ll, 0, &e, litmode);
                }
                const size_t end = s.size();
                filler(s, end + 400, litmode);
                check_stream(s, (int32_t)s.size(), 7);
                crafted++;
                for (size_t n = at + 1; n <= end + 40; ++n) {
                    const uint8_t *b0 = s.data();
                    uint8_t *b = (uint8_t *)malloc(n);
                    memcpy(b, b0, n);
                    for (int32_t plo = (int32_t)at - 140; plo <= (int32_t)n; plo += 37) check_segment(b, (int32_t)n, plo < 0 ? 0 : plo);
                    free(b);
                    crafted++;
                }
            }
        }
    }
    // seeded random token streams of 300..20,000 bytes: three segments each
    // (one anywhere, one at the stream's end, lane 0's)
    std::vector<uint8_t> s;
    for (long i = 0; i < nrandom; ++i) {
        const uint32_t len = i % 50 == 0 ? 20000 - rnd() % 64 : 300 + rnd() % (i % 7 == 0 ? 19700 : 1500);
        random_stream(s, len);
        uint8_t *b = (uint8_t *)malloc(len);
        memcpy(b, s.data(), len);
        check_segment(b, (int32_t)len, (int32_t)(rnd() % len));
        check_segment(b, (int32_t)len, (int32_t)len - 20 - (int32_t)(rnd() % 150));
        check_segment(b, (int32_t)len, 0);
        free(b);
    }
    printf("crafted=%ld random=%ld walks=%ld fixups=%ld redone=%ld arrived=%ld oob=%ld bad=%ld\n", crafted, nrandom, g_walks, g_fix,
           g_redone, g_arrived, g_oob, g_bad);
    return g_bad || g_oob ? 1 : 0;
}
