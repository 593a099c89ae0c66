// Stand-alone check of the placement rule of juicefs_amd/csrc/zstd_seek.h
// (Rounds / rounds_build / place_frame), built with
// AddressSanitizer + UBSan by tests/test_zstd_seek_place.py.  The kernels of
// zstd_seek.hip place the j-th selected frame with place_frame from the record
// their scan leaves; here the record comes from rounds_build, and every
// placement must be the frame the serial selectors name: the run of
// seek_select and of table_select, the sequence ranges_select emits.  Tables of
// both entry sizes, hand-built, in buffers of exactly their length; the fetch
// counts every index outside them.
//   zstd_seek_place_main N    the fixed cases, then N seeded random ones; prints
//                             "cases=.. placed=.. oob=.. bad=.." and exits 1 unless oob = bad = 0
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "zstd_seek.h"

namespace zs = jfs::zseek;

static long g_oob = 0, g_bad = 0, g_cases = 0, g_placed = 0;
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

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

static void fail(const char *what, int nf, int wide, int j) {
    if (g_bad++ < 20) printf("FAIL %s nf=%d wide=%d j=%d\n", what, nf, wide, j);
}

struct Object {
    int nf, wide, entry, tpos;
    std::vector<uint32_t> c, d;
    std::vector<uint64_t> C, D;  // the sums in front of frame k; [nf]: of all
    std::vector<uint8_t> bytes;  // the frames' bytes (never read) and the table
    CountingFetch whole() const { return CountingFetch{bytes.data(), (int64_t)bytes.size()}; }
};

static Object build(int nf, int wide, std::vector<uint32_t> c, std::vector<uint32_t> d) {
    Object o;
    o.nf = nf; o.wide = wide; o.entry = wide ? zs::ENTRY_CSUM : zs::ENTRY;
    o.c = std::move(c); o.d = std::move(d);
    o.C.assign(nf + 1, 0); o.D.assign(nf + 1, 0);
    for (int k = 0; k < nf; k++) {
        o.C[k + 1] = o.C[k] + o.c[k];
        o.D[k + 1] = o.D[k] + o.d[k];
    }
    o.tpos = (int)o.C[nf];
    o.bytes.assign((size_t)o.tpos, 0x28);
    auto put = [&](uint32_t v) { for (int j = 0; j < 4; j++) o.bytes.push_back((uint8_t)(v >> (8 * j))); };
    put(zs::SKIP_MAGIC);
    put((uint32_t)(o.entry * nf + 9));
    for (int k = 0; k < nf; k++) {
        put(o.c[k]);
        put(o.d[k]);
        if (wide) put(0x9E3779B9u * (uint32_t)(k + 1));
    }
    put((uint32_t)nf);
    o.bytes.push_back(wide ? 0x80 : 0);
    put(zs::SEEK_MAGIC);
    return o;
}

// every j of a record against the frames `want` names, and no frame past them
template <class F>
static void check_places(const Object &o, F fetch, int32_t tpos, const zs::Rounds &R, int32_t cnt,
                         const std::vector<int32_t> &want, const char *what) {
    if (cnt != (int32_t)want.size()) return fail(what, o.nf, o.wide, -1);
    for (int32_t j = 0; j < cnt; j++, g_placed++) {
        int32_t k = -1;
        uint32_t coff = 0, doff = 0;
        if (!zs::place_frame(fetch, tpos, o.entry, o.nf, R, j, &k, &coff, &doff) || k != want[j] ||
            coff != (uint32_t)o.C[want[j]] || doff != (uint32_t)o.D[want[j]])
            fail(what, o.nf, o.wide, j);
    }
    int32_t k = 0;
    uint32_t coff = 0, doff = 0;
    if (zs::place_frame(fetch, tpos, o.entry, o.nf, R, cnt, &k, &coff, &doff)) fail("one past the selection", o.nf, o.wide, cnt);
    if (zs::place_frame(fetch, tpos, o.entry, o.nf, R, -1, &k, &coff, &doff)) fail("j = -1", o.nf, o.wide, -1);
}

// one range lo' < hi': the run of seek_select (8-byte tables) and of table_select
static void check_run(const Object &o, int32_t cap, int32_t lo, int32_t hi) {
    g_cases++;
    const int32_t l = zs::range_lo(lo), h = zs::range_hi(hi, cap);
    if (h <= l) return;  // the calls answer 0 in front of the selection
    static zs::Rounds R;
    const auto run = [&](int32_t, uint64_t d0, uint32_t d) { return zs::frame_in_run(d0, d, l, h); };
    std::vector<int32_t> want;
    if (!o.wide) {
        int32_t nf = 0, tpos = 0, entry = 0;
        if (!zs::seek_table(o.whole(), (int64_t)o.bytes.size(), false, false, &nf, &tpos, &entry) || nf != o.nf ||
            tpos != o.tpos || entry != o.entry)
            return fail("seek_table", o.nf, o.wide, -1);
        const zs::Sel s = zs::seek_select(o.whole(), (int32_t)o.bytes.size(), cap, lo, hi);
        if (!s.table) return fail("seek_select", o.nf, o.wide, -1);
        for (int32_t j = 0; j < s.count; j++) want.push_back(s.first + j);
        if (s.count > 0 && (s.coff != (uint32_t)o.C[s.first] || s.doff != (uint32_t)o.D[s.first]))
            fail("seek_select offsets", o.nf, o.wide, -1);
        const int32_t cnt = zs::rounds_build(o.whole(), tpos, entry, nf, run, &R);
        check_places(o, o.whole(), tpos, R, cnt, want, "run of seek_select");
    }
    // the table alone, either layout
    const std::vector<uint8_t> t(o.bytes.begin() + o.tpos, o.bytes.end());
    const CountingFetch tf{t.data(), (int64_t)t.size()};
    const zs::TableSel s = zs::table_select(tf, (int64_t)t.size(), (int64_t)o.bytes.size(), cap, lo, hi);
    if (!s.table || s.nf != o.nf) return fail("table_select", o.nf, o.wide, -1);
    want.clear();
    for (int32_t j = 0; j < s.count; j++) want.push_back(s.first + j);
    if (s.count > 0 && (s.coff != o.C[s.first] || s.doff != o.D[s.first] || s.cend != o.C[s.first + s.count]))
        fail("table_select offsets", o.nf, o.wide, -1);
    const int32_t cnt = zs::rounds_build(tf, 0, o.entry, o.nf, run, &R);
    check_places(o, tf, 0, R, cnt, want, "run of table_select");
}

// a list: the sequence ranges_select emits
static void check_list(const Object &o, int32_t cap, const std::vector<Range> &rng) {
    g_cases++;
    static zs::Rounds R;
    std::vector<int32_t> want;
    bool same = true;
    const zs::RangesSel s = zs::ranges_select(o.whole(), (int32_t)o.bytes.size(), cap, rng.data(), (int32_t)rng.size(),
                                              [&](int32_t k, uint32_t coff, uint32_t doff, uint32_t c, uint32_t d, uint32_t) {
                                                  want.push_back(k);
                                                  same = same && coff == (uint32_t)o.C[k] && doff == (uint32_t)o.D[k] &&
                                                         c == o.c[k] && d == o.d[k];
                                              });
    if (s.bad) return;
    if (!s.table || !same) return fail("ranges_select", o.nf, o.wide, -1);
    if (s.live == 0) return;  // the call answers 0 in front of the selection
    const int32_t cnt = zs::rounds_build(o.whole(), o.tpos, o.entry, o.nf, [&](int32_t, uint64_t d0, uint32_t d) {
        return zs::frame_in_ranges(rng.data(), (int32_t)rng.size(), cap, d0, d);
    }, &R);
    check_places(o, o.whole(), o.tpos, R, cnt, want, "sequence of ranges_select");
}

static void fixed_cases() {
    const int counts[] = {1, 63, 64, 65, 128, 129, zs::MAX_FRAMES};
    for (int nf : counts)
        for (int wide = 0; wide < 2; wide++) {
            std::vector<uint32_t> c(nf), d(nf);
            for (int k = 0; k < nf; k++) {
                c[k] = 1 + (uint32_t)(k * 5) % 3;
                d[k] = (uint32_t)(k * 7 + 3) % 5;  // 3 0 2 4 1 ...: frames without content among them
            }
            const Object o = build(nf, wide, c, d);
            const int32_t total = (int32_t)o.D[nf], cap = total + 5;
            auto at = [&](int k) { return (int32_t)o.D[k < nf ? k : nf]; };
            // (lo, hi): from lane 0 of a round, from lane 63, across three rounds, the last frame, nothing, everything
            const int32_t runs[][2] = {{at(64), at(64) + 1}, {at(0), at(2)}, {at(63), at(63) + 1}, {at(63), at(66)},
                                       {at(60), at(130)}, {at(1), at(200)}, {total - 1, total}, {total, total + 5},
                                       {7, 7}, {0, total}, {-9, 1 << 30}, {at(128), at(129)}, {at(127), total}};
            for (const auto &r : runs) {
                check_run(o, cap, r[0], r[1]);
                check_list(o, cap, {Range{r[0], r[1]}});
            }
            std::vector<Range> other, ends;  // every other frame; the first and the last one
            for (int k = 0; k < nf; k += 2)
                if (d[k] > 0) other.push_back(Range{at(k), at(k) + 1});
            check_list(o, cap, other);
            ends = {Range{0, 1}, Range{total - 1, total}};
            check_list(o, cap, ends);
            check_list(o, cap, {});
            check_list(o, cap, {Range{3, 3}, Range{total, total + 9}});
        }
}

static void random_cases(long n) {
    for (long i = 0; i < n; i++) {
        const int pick = (int)(rnd() % 10);
        const int nf = pick < 6 ? 1 + (int)(rnd() % 200) : pick < 9 ? 60 + (int)(rnd() % 12) + 64 * (int)(rnd() % 3) : 1 + (int)(rnd() % 1500);
        const int wide = (int)(rnd() & 1);
        std::vector<uint32_t> c(nf), d(nf);
        for (int k = 0; k < nf; k++) {
            c[k] = 1 + rnd() % 4;
            d[k] = (rnd() % 3) ? rnd() % 9 : 0;
        }
        const Object o = build(nf, wide, c, d);
        const int32_t total = (int32_t)o.D[nf];
        const int32_t cap = (rnd() & 3) ? total + (int32_t)(rnd() % 4) : 1 << 30;
        auto point = [&]() { return (rnd() & 1) ? (int32_t)o.D[rnd() % (nf + 1)] + (int32_t)(rnd() % 3) - 1 : (int32_t)(rnd() % (total + 8)) - 3; };
        if (rnd() & 1) {
            const int32_t a = point(), b = point();
            check_run(o, cap, a < b ? a : b, a < b ? b : a);
        } else {
            std::vector<int32_t> pts(2 * (rnd() % 9));
            for (auto &p : pts) p = point();
            for (size_t a = 1; a < pts.size(); a++)  // ascending
                for (size_t b = a; b > 0 && pts[b - 1] > pts[b]; b--) std::swap(pts[b - 1], pts[b]);
            std::vector<Range> rng;
            for (size_t q = 0; q + 1 < pts.size(); q += 2) rng.push_back(Range{pts[q], pts[q + 1]});
            check_list(o, cap, rng);
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    fixed_cases();
    random_cases(atol(argv[1]));
    printf("cases=%ld placed=%ld oob=%ld bad=%ld\n", g_cases, g_placed, g_oob, g_bad);
    return (g_oob || g_bad) ? 1 : 0;
}
