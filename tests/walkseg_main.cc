// Host driver for juicefs_amd/csrc/lz4_walkstep.h (tests/test_lz4_walk_seg.py):
// for segments of 128 and of 256 bytes, the deferred-check walks the kernel's
// SegWalk runs (ws_spec_iter, ws_fix_iter on BitSet<SEG>; the fix-up walk
// records into vt, there is no third set) against plain walks that ask
// ws_next_exact at every position, over the same bytes, from every entry of a
// 32-byte pre-roll + segment.  Compared: the visited positions, the exit, STOP
// results; every fetch index must lie in [0, n).  And BitSet<SEG> itself
// against std::bitset for every (d, on).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <bitset>
#include <vector>

#include "lz4_walkstep.h"

using namespace jfs::lz4d;

static constexpr int SPRE = 32;
static long g_oob = 0, g_bad = 0, g_walks = 0, g_redone = 0, g_arrived = 0, g_fix = 0, g_setops = 0, g_straddle = 0;

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

struct Lane {  // the scalar fields of SegWalk the iterations use
    int32_t plo, phi, q;
    uint32_t sx, ex, pe2;
    bool mv, pend;
};

template <int SEG>
struct Res {
    BitSet<SEG> v;
    uint32_t exit;
    bool operator==(const Res &o) const { return memcmp(v.w, o.v.w, sizeof(v.w)) == 0 && exit == o.exit; }
};

template <int SEG>
static void fail(const char *what, int32_t n, int32_t plo, int32_t e, const Res<SEG> &a, const Res<SEG> &b) {
    if (g_bad++ < 10) {
        printf("MISMATCH SEG=%d %s n=%d plo=%d entry=%d: deferred", SEG, what, n, plo, e);
        for (int i = 0; i < SEG / 64; i++) printf(" %016llx", (unsigned long long)a.v.w[i]);
        printf(" exit %08x, plain", a.exit);
        for (int i = 0; i < SEG / 64; i++) printf(" %016llx", (unsigned long long)b.v.w[i]);
        printf(" exit %08x\n", b.exit);
    }
}

static void count(int kind) {
    g_redone += kind == WS_REDONE;
    g_arrived += kind == WS_ARRIVED;
}

template <int SEG>
struct Walks {
    using Set = BitSet<SEG>;
    using R = Res<SEG>;

    // speculative walk from entry e: plain
    static R spec_plain(const Fetch &f, int32_t plo, int32_t e) {
        R r;
        r.v.clear();
        r.exit = 0;
        const int32_t phi = plo + SEG;
        int32_t q = e;
        for (;;) {
            const uint32_t x = ws_next_exact(f, f.n, q);
            const bool stop = (x & WS_STOP) != 0;
            if (!stop && q >= plo) {
                r.v.put((uint32_t)(q - plo), true);
                // a token whose bytes lie on both sides of a word of the set
                if (!((uint32_t)(q - plo) % 64u < 60u) && (int32_t)x - plo >= (q - plo) / 64 * 64 + 64) g_straddle++;
            }
            if (stop || (int32_t)x >= phi) {
                r.exit = x;
                return r;
            }
            q = (int32_t)x;
        }
    }

    static R spec_deferred(const Fetch &f, int32_t plo, int32_t e, Lane *keep) {
        Lane w;
        memset(&w, 0, sizeof(w));
        Set vs;
        vs.clear();
        w.plo = plo;
        w.phi = plo + SEG;
        w.q = e;
        w.mv = true;
        const auto exact = [&](int32_t p) { return ws_next_exact(f, f.n, p); };
        int it = 0;
        while (w.mv) {
            count(ws_spec_iter(w, vs, f, exact, f.n));
            if (++it > SEG + SPRE) {  // the bound SegWalk::advance holds the walk to
                g_bad++;
                printf("SEG=%d speculative walk does not end: n=%d plo=%d entry=%d\n", SEG, f.n, plo, e);
                break;
            }
        }
        if (w.pend) {
            g_bad++;
            printf("SEG=%d a finished lane still owes a test: n=%d plo=%d entry=%d\n", SEG, f.n, plo, e);
        }
        if (keep) *keep = w;
        return R{vs, w.sx};
    }

    // fix-up walk from the true entry in (in [plo, phi), off the chain vs): plain
    static R fix_plain(const Fetch &f, int32_t plo, const Set &vs, uint32_t sx, int32_t in) {
        const int32_t phi = plo + SEG;
        R r;
        r.v.clear();
        int32_t q = in;
        for (;;) {
            const uint32_t d = (uint32_t)(q - plo);
            if (vs.test(d)) {
                for (uint32_t k = d; k < (uint32_t)SEG; k++)
                    if (vs.test(k)) r.v.put(k, true);
                r.exit = sx;
                return r;
            }
            const uint32_t x = ws_next_exact(f, f.n, q);
            const bool stop = (x & WS_STOP) != 0;
            if (!stop) r.v.put(d, true);
            if (stop || (int32_t)x >= phi) {
                r.exit = x;
                return r;
            }
            q = (int32_t)x;
        }
    }

    static R fix_deferred(const Fetch &f, Lane w, const Set &vs, int32_t in) {
        // the state SegWalk::advance sets up for a lane whose entry changed to
        // `in`: vt cleared, it takes the walk's positions
        Set vt;
        vt.clear();
        w.q = in;
        w.mv = true;
        const auto exact = [&](int32_t p) { return ws_next_exact(f, f.n, p); };
        int it = 0;
        while (w.mv) {
            count(ws_fix_iter(w, vs, vt, f, exact, f.n));
            if (++it > SEG + 1) {
                g_bad++;
                printf("SEG=%d fix-up walk does not end: n=%d plo=%d entry=%d\n", SEG, f.n, w.plo, in);
                break;
            }
        }
        if (w.pend) {
            g_bad++;
            printf("SEG=%d a finished fix-up lane still owes a test: n=%d plo=%d entry=%d\n", SEG, f.n, w.plo, in);
        }
        return R{vt, w.ex};
    }

    // every entry of the pre-roll + segment at plo; the fix-up walks against the
    // chain the kernel's lane would hold (entry plo - SPRE, or plo for lane 0)
    static void check_segment(const uint8_t *b, int32_t n, int32_t plo) {
        const Fetch f{b, n};
        const int32_t lo = plo - SPRE < 0 ? 0 : plo - SPRE;
        for (int32_t e = lo; e < plo + SEG; ++e) {
            const R a = spec_deferred(f, plo, e, nullptr), p = spec_plain(f, plo, e);
            g_walks++;
            if (!(a == p)) fail("speculative", n, plo, e, a, p);
        }
        for (int lane0 = 0; lane0 < 2; ++lane0) {
            Lane w;
            const R sp = spec_deferred(f, plo, lane0 ? plo : lo, &w);
            for (int32_t in = plo; in < plo + SEG; ++in) {
                if (sp.v.test((uint32_t)(in - plo))) continue;
                const R a = fix_deferred(f, w, sp.v, in), p = fix_plain(f, plo, sp.v, sp.exit, in);
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

    // BitSet<SEG> against std::bitset: every (d, on), and from / and_from / any /
    // first_from / test of the result for every d
    static void check_sets(uint64_t seed) {
        uint64_t x = seed;
        const auto rnd = [&]() {
            x ^= x << 13;
            x ^= x >> 7;
            x ^= x << 17;
            return x;
        };
        const auto same = [](const Set &a, const std::bitset<SEG> &b) {
            for (int k = 0; k < SEG; k++)
                if (((a.w[k / 64] >> (k % 64)) & 1ull) != (uint64_t)b[(size_t)k]) return false;
            return true;
        };
        const auto bad = [](const char *what, uint32_t d) {
            if (g_bad++ < 10) printf("BitSet<%d>::%s differs from std::bitset at d=%u\n", SEG, what, d);
        };
        for (int fill = 0; fill < 4; fill++) {  // empty, full, random, sparse
            Set a;
            std::bitset<SEG> b;
            a.clear();
            if (!same(a, b) || a.any()) bad("clear", 0);
            for (int k = 0; k < SEG; k++) {
                const bool on = fill == 1 || (fill == 2 && (rnd() & 1)) || (fill == 3 && rnd() % 37 == 0);
                a.put((uint32_t)k, on);
                b[(size_t)k] = on;
            }
            if (!same(a, b)) bad("put (fill)", 0);
            for (uint32_t d = 0; d < (uint32_t)SEG; d++) {
                for (int on = 0; on < 2; on++) {
                    Set c = a;
                    std::bitset<SEG> e = b;
                    c.put(d, on != 0);
                    e[d] = on != 0;
                    if (!same(c, e)) bad("put", d);
                    if (c.test(d) != (on != 0)) bad("test", d);
                    if (c.any() != e.any()) bad("any", d);
                    g_setops += 3;
                }
                if (a.test(d) != b[d]) bad("test", d);
                std::bitset<SEG> fr;
                for (uint32_t k = d; k < (uint32_t)SEG; k++) fr[k] = true;
                if (!same(Set::from(d), fr)) bad("from", d);
                const std::bitset<SEG> af = b & fr;
                if (!same(a.and_from(d), af)) bad("and_from", d);
                if (a.and_from(d).any() != af.any()) bad("any", d);
                uint32_t first = (uint32_t)SEG;
                for (uint32_t k = (uint32_t)SEG; k-- > d;)
                    if (b[k]) first = k;
                if (a.first_from(d) != first) bad("first_from", d);
                Set o = a.and_from(d);
                Set acc;
                acc.clear();
                acc.put(d / 2, true);
                acc.or_in(o);
                std::bitset<SEG> accb = af;
                accb[d / 2] = true;
                if (!same(acc, accb)) bad("or_in", d);
                g_setops += 7;
            }
            // d = SEG: nothing at or past it
            if (Set::from((uint32_t)SEG).any() || a.and_from((uint32_t)SEG).any() || a.first_from((uint32_t)SEG) != (uint32_t)SEG)
                bad("from(SEG)", (uint32_t)SEG);
        }
    }
};

// ---- streams --------------------------------------------------------------
static uint64_t g_rng;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 11);
}

// one token: ll literals, offset bytes, match-length code mlc (match length -
// 4) with explicit extension bytes when mext is given
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
        if (r < longp) mlc = 15 + rnd() % 700;
        else if (r < 2 * longp) mlc = 15 + 255 * (1 + rnd() % 3) + (rnd() % 4 ? rnd() % 255 : 0);
        if (rnd() % 100 < longp / 2) ll = 15 + rnd() % 600;
        else if (rnd() % 40 == 0) ll = 15 + 255;
        token(s, ll, mlc, nullptr, rnd() % 5 == 0 ? 2 : 0);
    }
    s.resize(len);
}

// the token of interest of crafted case m (the kinds of tests/walkstep_main.cc)
static const std::vector<std::vector<uint8_t>> g_mexts = {{254}, {255, 0}, {255, 255, 7}, {255, 255, 255, 200}, {0}, {255, 254}};
static constexpr size_t NKIND = 6 + 5;
static void kind_token(std::vector<uint8_t> &s, size_t m, uint32_t ll, int litmode) {
    const size_t k = g_mexts.size();
    if (m < k) {
        token(s, ll, 0, &g_mexts[m], litmode);
    } else if (m == k) {  // no extension, the next token byte is 255
        token(s, ll, 7, nullptr, litmode);
        token(s, 15 + 2, 15 + 3, nullptr, litmode);
    } else if (m == k + 1) {  // two slow tokens in a row
        token(s, ll, 0, &g_mexts[1], litmode);
        token(s, 2, 0, &g_mexts[2], litmode);
    } else if (m == k + 2) {  // three, the middle one by its literal length
        token(s, ll, 0, &g_mexts[2], litmode);
        token(s, 15 + 255 + 4, 3, nullptr, litmode);
        token(s, 0, 0, &g_mexts[1], litmode);
    } else if (m == k + 3) {  // a slow token right behind a one-byte literal extension
        token(s, 15 + 9, 0, &g_mexts[2], litmode);
        token(s, ll, 0, &g_mexts[1], litmode);
    } else {  // a long run of 255 extension bytes (past KEXT)
        std::vector<uint8_t> e(70, 255);
        e.push_back(1);
        token(s, ll, 0, &e, litmode);
    }
}

template <int SEG>
static long run(long nrandom) {
    using Wk = Walks<SEG>;
    long crafted = 0;
    Wk::check_sets(0x2545F4914F6CDD1Dull + SEG);
    // crafted: a token of interest (at about byte 300) between plain tokens, every
    // segment position in steps of 7 bytes, then truncated inside each of its
    // fields and the 40 bytes after it
    for (int litmode = 0; litmode < 3; litmode += 2) {
        for (size_t m = 0; m < NKIND; ++m) {
            for (uint32_t ll : {0u, 3u, 15u + 40u, 15u + 255u}) {
                std::vector<uint8_t> s;
                filler(s, 290 + rnd() % 16, litmode);
                const size_t at = s.size();
                kind_token(s, m, ll, litmode);
                const size_t end = s.size();
                filler(s, end + 400 + SEG, litmode);
                Wk::check_stream(s, (int32_t)s.size(), 7);
                crafted++;
                for (size_t n = at + 1; n <= end + 40; n += (SEG == 128 ? 1 : 3)) {
                    uint8_t *b = (uint8_t *)malloc(n);
                    memcpy(b, s.data(), n);
                    for (int32_t plo = (int32_t)at - SEG - 12; plo <= (int32_t)n; plo += 37) Wk::check_segment(b, (int32_t)n, plo < 0 ? 0 : plo);
                    free(b);
                    crafted++;
                }
            }
        }
    }
    // a token of each kind that starts in the last 3 bytes before, or the first
    // 3 bytes after, bit 64, 128 and 192 of its segment (at 128: 64 and the
    // segment's end), so that its fields straddle a word of the set: the
    // segment is placed so that the token's position is plo + edge + k
    for (size_t m = 0; m < NKIND; ++m) {
        for (uint32_t ll : {0u, 3u, 15u + 40u}) {
            std::vector<uint8_t> s;
            filler(s, 600 + rnd() % 16, 0);
            const int32_t at = (int32_t)s.size();
            kind_token(s, m, ll, 0);
            filler(s, s.size() + 400 + SEG, 0);
            uint8_t *b = (uint8_t *)malloc(s.size());
            memcpy(b, s.data(), s.size());
            for (int edge = 64; edge <= SEG; edge += 64)
                for (int k = -3; k <= 2; ++k) {
                    Wk::check_segment(b, (int32_t)s.size(), at - edge - k);
                    crafted++;
                }
            free(b);
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
        Wk::check_segment(b, (int32_t)len, (int32_t)(rnd() % len));
        Wk::check_segment(b, (int32_t)len, (int32_t)len - 20 - (int32_t)(rnd() % (SEG + 22)));
        Wk::check_segment(b, (int32_t)len, 0);
        free(b);
    }
    return crafted;
}

int main(int argc, char **argv) {
    const long nrandom = argc > 1 ? atol(argv[1]) : 3000;
    for (int seg : {128, 256}) {
        g_rng = 0x9E3779B97F4A7C15ull;
        g_walks = g_redone = g_arrived = g_fix = g_setops = g_straddle = 0;
        const long crafted = seg == 128 ? run<128>(nrandom) : run<256>(nrandom);
        printf("seg=%d crafted=%ld random=%ld walks=%ld fixups=%ld redone=%ld arrived=%ld straddle=%ld setops=%ld oob=%ld bad=%ld\n", seg,
               crafted, nrandom, g_walks, g_fix, g_redone, g_arrived, g_straddle, g_setops, g_oob, g_bad);
    }
    return g_bad || g_oob ? 1 : 0;
}
