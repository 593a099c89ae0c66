// Checks the read calls' sparse-mode planning in juicefs_amd/csrc/chain_plan.h
// on a CPU: chain_ranges (the lists of ranges per decoded source: clamped,
// sorted, merged where they overlap or touch, holes and unreferenced sources
// left out, the running sums), and that the list's area of ChainLayout takes
// no byte of a call that does not use it and keeps to itself in one that does.
// Built and run by tests/test_chain_plan_ranges.py under ASan + UBSan.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../juicefs_amd/csrc/chain_plan.h"
#include "../juicefs_amd/csrc/zstd_seek.h"

using namespace jfs_plan;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            g_fail++;                                      \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
            if (g_fail > 20) exit(1);                      \
        }                                                  \
    } while (0)

typedef std::vector<jfs_range> List;

static bool same(const ChainRanges &r, int k, const List &want) {
    if (r.first[k + 1] - r.first[k] != (int32_t)want.size()) return false;
    for (size_t q = 0; q < want.size(); q++)
        if (r.rng[r.first[k] + q].lo != want[q].lo || r.rng[r.first[k] + q].hi != want[q].hi) return false;
    return true;
}

static void lists() {
    // five objects; 1 is answered on the host (not staged), 3 is referenced by nothing
    const int nsrc = 5;
    const std::vector<ChainSrc> st = {
        {0, 0, 0, 100, 1000, false, 0}, {2, 0, 0, 100, 500, false, 0}, {3, 0, 0, 100, 700, false, 0},
        {4, 0, 0, 100, 64, false, 0},   {1, 0, 0, 100, 0, true, 7},  // (behind ns: staged for its checksum only)
    };
    const int ns = 4;
    // {src, src_off, dst_off, len}
    const std::vector<jfs_compact_seg> seg = {
        // read 0: out of order on source 0, a hole, source 2 beyond its capacity
        {0, 900, 0, 50}, {-1, 12345, 50, 33}, {0, 10, 83, 20}, {2, 450, 103, 100},
        // read 1: touching (30 = 10 + 20) and overlapping ranges of source 0, a range inside another
        {0, 30, 0, 5}, {0, 33, 5, 10}, {0, 920, 15, 10}, {0, 500, 25, 1},
        // read 2: source 2 wholly beyond its capacity (dropped), source 4 clamped to it, source 1 (not staged)
        {2, 500, 0, 10}, {2, 600, 10, 10}, {4, 60, 20, 10}, {1, 0, 30, 5},
        // read 3: source 0's last byte and one past it
        {0, 999, 0, 1}, {0, 1000, 1, 4},
        // read 4: only a hole
        {-1, 0, 0, 9},
    };
    const std::vector<int32_t> seg_first = {0, 4, 8, 12, 14, 15};
    const ChainRanges r = chain_ranges(nsrc, 5, seg_first.data(), seg.data(), st, ns);
    CHECK(r.first.size() == (size_t)ns + 1, "first has ns + 1 entries");
    CHECK(r.first[0] == 0 && r.first[ns] == (int32_t)r.rng.size(), "running sums");
    CHECK(same(r, 0, List{{10, 43}, {500, 501}, {900, 950}, {999, 1000}}), "source 0: %d ranges", r.first[1] - r.first[0]);
    CHECK(same(r, 1, List{{450, 500}}), "source 2: clamped to its capacity, what lies beyond dropped");
    CHECK(same(r, 2, List{}), "source 3: nothing references it");
    CHECK(same(r, 3, List{{60, 64}}), "source 4");
    CHECK(r.first[1] == 4 && r.first[2] == 5 && r.first[3] == 5 && r.first[4] == 6, "running sums");
    for (int k = 0; k < ns; k++) {
        const int32_t n = r.first[k + 1] - r.first[k];
        CHECK(jfs::zseek::ranges_ok(r.rng.data() + r.first[k], n), "list %d is ascending and disjoint", k);
        for (int32_t q = 0; q < n; q++) {
            const jfs_range &x = r.rng[r.first[k] + q];
            CHECK(jfs::zseek::range_live(x, (int32_t)st[k].cap), "list %d range %d is live", k, q);
            CHECK(q == 0 || r.rng[r.first[k] + q - 1].hi < x.lo, "list %d: touching ranges are merged", k);
        }
    }
    // the union of the lists is what chain_from / chain_need span
    const std::vector<int64_t> need = chain_need(nsrc, 5, seg_first.data(), seg.data());
    const std::vector<int64_t> from = chain_from(nsrc, 5, seg_first.data(), seg.data());
    CHECK(from[0] == r.rng[r.first[0]].lo && std::min<int64_t>(need[0], 1000) == r.rng[r.first[1] - 1].hi, "hull of source 0");
    // no outputs, no sources
    const ChainRanges none = chain_ranges(0, 0, seg_first.data(), nullptr, {}, 0);
    CHECK(none.first.size() == 1 && none.first[0] == 0 && none.rng.empty(), "empty call");
    // many segments of one source in reverse order, every second one touching the next
    std::vector<jfs_compact_seg> many;
    for (int k = 99; k >= 0; k--) many.push_back({0, 10 * k, 0, k % 2 ? 10 : 5});
    const std::vector<int32_t> mf = {0, 100};
    const std::vector<ChainSrc> one = {{0, 0, 0, 1, 100000, false, 0}};
    const ChainRanges m = chain_ranges(1, 1, mf.data(), many.data(), one, 1);
    CHECK(m.rng.size() == 51, "%zu ranges", m.rng.size());
    CHECK(m.rng[0].lo == 0 && m.rng[0].hi == 5 && m.rng[1].lo == 10 && m.rng[1].hi == 25 && m.rng[50].hi == 1000, "merged runs");
}

static void layout() {
    const int64_t tin = 1000, ns = 3, n = 4, no = 5, nseg = 9, npiece = 6, nrange = 7;
    for (int mask = 0; mask < 128; mask++) {
        const ChainFlags f{(mask & 1) != 0, (mask & 2) != 0, (mask & 4) != 0, (mask & 8) != 0,
                           (mask & 16) != 0, (mask & 32) != 0, (mask & 64) != 0};
        const ChainLayout a(tin, ns, n, no, nseg, f, npiece), b(tin, ns, n, no, nseg, f, npiece, nrange);
        ChainFlags g = f;
        g.sparse = true;
        const ChainLayout c(tin, ns, n, no, nseg, g, npiece, nrange);
        // a call without lists: nothing moves, with or without a count
        CHECK(a.h2d == b.h2d && a.out == b.out && a.srcn == b.srcn && a.from == b.from && a.csum == b.csum, "mask %d", mask);
        CHECK(b.rf == b.srcn && b.rng == b.srcn, "mask %d: an unused area has no bytes", mask);
        // with lists: the two areas lie between `from` and the source lengths, inside the H2D copy
        const int64_t rf_bytes = align16((ns + 1) * 4), rng_bytes = align16(nrange * (int64_t)sizeof(jfs_range));
        CHECK(c.rf == a.srcn && c.rng == c.rf + rf_bytes && c.srcn == c.rng + rng_bytes, "mask %d", mask);
        CHECK(c.from + (f.seek ? align16(ns * 4) : 0) == c.rf, "mask %d: beside from", mask);
        CHECK(c.h2d == a.h2d + rf_bytes + rng_bytes && c.out == a.out + rf_bytes + rng_bytes, "mask %d", mask);
        CHECK(c.rng + rng_bytes <= c.h2d && c.results == c.srcn, "mask %d", mask);
        CHECK(c.rf % 16 == 0 && c.rng % 16 == 0, "mask %d: alignment", mask);
    }
    CHECK(sizeof(jfs_range) == 8, "jfs_range is two int32");
}

int main() {
    lists();
    layout();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("chain plan ranges check OK\n");
    return 0;
}
