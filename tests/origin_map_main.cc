// Host driver of juicefs_amd/csrc/origin_map.h (tests/test_origin_map.py builds
// it with AddressSanitizer and UBSan): the header's entry writers, jump step
// and gather step against a serial LZ interpreter over (ll, ml, off)
// sequences and a literal buffer.
//
// The jump rounds run in the SYNCHRONOUS model: every hop of a round reads a
// snapshot taken before the round, so no thread ever profits from another
// one's update -- the slowest schedule a GPU can produce, and the one the
// round rule is proved for.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "origin_map.h"

namespace om = jfs::om;

struct Seq {
    int64_t ll, ml;
    uint32_t off;
};

static int g_bad = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (g_bad++ < 20) {                         \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                    \
                printf("\n");                           \
            }                                           \
        }                                               \
    } while (0)

// the serial decode: per sequence its literals, then its match byte by byte;
// the literals left over follow the last sequence
static std::vector<uint8_t> serial(const std::vector<Seq> &seqs, const std::vector<uint8_t> &lits) {
    std::vector<uint8_t> out;
    size_t lp = 0;
    for (const Seq &s : seqs) {
        for (int64_t i = 0; i < s.ll; i++) out.push_back(lits.at(lp++));
        for (int64_t i = 0; i < s.ml; i++) out.push_back(out.at(out.size() - s.off));
    }
    while (lp < lits.size()) out.push_back(lits[lp++]);
    return out;
}

constexpr uint32_t POISON = 0x7FFFFF00u;  // a pointer far outside every map
constexpr uint8_t GUARD = 0xEE;

// The map of the first `want` output bytes (the runs clamped as the LZ4 prefix
// emit clamps them), in round4(want) entries + one quad, all poisoned first.
template <class P>
static std::vector<uint32_t> fill_map(const std::vector<Seq> &seqs, int64_t nlits, int64_t want) {
    std::vector<uint32_t> org((size_t)(((want + 3) & ~3ll) + 4));
    for (size_t i = 0; i < org.size(); i++) org[i] = POISON + (uint32_t)(i & 0xFF);
    P pos = 0, lp = 0;
    auto room = [&](int64_t len) { return (P)(len < want - pos ? len : want - pos); };
    for (const Seq &s : seqs) {
        if (pos >= want) break;
        om::put_lits<P>(org.data(), pos, room(s.ll), om::lit_entry(lp));
        pos += (P)s.ll;
        lp += (P)s.ll;
        if (pos >= want) break;
        om::put_match<P>(org.data(), pos, room(s.ml), s.off);
        pos += (P)s.ml;
    }
    if (pos < want) om::put_lits<P>(org.data(), pos, room(nlits - lp), om::lit_entry(lp));
    return org;
}

static void check_poison(const std::vector<uint32_t> &org, int64_t total, const char *what) {
    for (size_t i = (size_t)total; i < org.size(); i++)
        CHECK(org[i] == POISON + (uint32_t)(i & 0xFF), "%s: entry %zu at or above total %lld changed", what, i, (long long)total);
}

// one synchronous round over `threads` strided walkers; returns "something changed"
static bool jump_round(std::vector<uint32_t> &org, int64_t total, int threads) {
    const std::vector<uint32_t> snap(org);
    bool any = false;
    for (int t = 0; t < threads; t++)
        any |= om::jump_walk(org.data(), total, (int64_t)t * 4, (int64_t)threads * 4, [&](int32_t o) -> uint32_t {
            CHECK(o >= 0 && o < total, "hop to %d outside [0, %lld)", o, (long long)total);
            return o >= 0 && o < total ? snap[(size_t)o] : om::lit_entry(0);
        });
    check_poison(org, total, "jump");
    return any;
}

static bool settled(const std::vector<uint32_t> &org, int64_t total) {
    for (int64_t i = 0; i < total; i++)
        if (!om::is_lit(org[(size_t)i])) return false;
    return true;
}

// Gathers [0, total) into a dst misaligned by `mis` bytes; returns the quads
// reported unsettled.  Checks: a reported quad wrote nothing, no byte outside
// [0, total) was written, and every other byte equals want_out.
static int gather(const std::vector<uint32_t> &org, const std::vector<uint8_t> &lits, int64_t total, int mis,
                  const std::vector<uint8_t> &want_out) {
    std::vector<uint8_t> buf((size_t)(16 + total + 16), GUARD);
    CHECK(((uintptr_t)buf.data() & 3u) == 0, "allocator alignment");
    uint8_t *dst = buf.data() + 16 + mis;
    int unsettled = 0;
    for (int64_t p = 0; p < total; p += 4) {
        const bool ok = om::gather_quad(org.data(), lits.data(), dst, p, total);
        bool all_lit = true;
        for (int64_t i = p; i < p + 4 && i < total; i++) all_lit &= om::is_lit(org[(size_t)i]);
        CHECK(ok == all_lit, "gather_quad(%lld) = %d, entries literal = %d", (long long)p, ok, all_lit);
        if (ok) continue;
        unsettled++;
        for (int64_t i = p; i < p + 4 && i < total; i++) CHECK(dst[i] == GUARD, "unsettled quad %lld was written", (long long)p);
        for (int64_t i = p; i < p + 4 && i < total; i++) dst[i] = want_out[(size_t)i];  // (for the compare below)
    }
    for (uint8_t *q = buf.data(); q < dst; q++) CHECK(*q == GUARD, "byte before dst written");
    for (uint8_t *q = dst + total; q < buf.data() + buf.size(); q++) CHECK(*q == GUARD, "byte at or above total written");
    CHECK(total == 0 || memcmp(dst, want_out.data(), (size_t)total) == 0, "gather differs from the serial decode (total %lld, mis %d)",
          (long long)total, mis);
    return unsettled;
}

static int g_cases = 0, g_residue[4] = {0, 0, 0, 0};

// fill, jump to the fixed point (at most max_rounds rounds), gather at the
// four dst alignments, compare; with both position types
template <class P>
static void run_case(const std::vector<Seq> &seqs, const std::vector<uint8_t> &lits, int64_t want, int max_rounds, int threads) {
    const std::vector<uint8_t> ref = serial(seqs, lits);
    const int64_t total = want < (int64_t)ref.size() ? want : (int64_t)ref.size();
    std::vector<uint32_t> org = fill_map<P>(seqs, (int64_t)lits.size(), total);
    check_poison(org, total, "fill");
    for (int r = 0; r < max_rounds && jump_round(org, total, threads); r++) {
    }
    CHECK(settled(org, total), "not settled after %d rounds (total %lld)", max_rounds, (long long)total);
    for (int mis = 0; mis < 4; mis++) CHECK(gather(org, lits, total, mis, ref) == 0, "settled map, unsettled gather");
    g_cases++;
    g_residue[total & 3]++;
}

// Every match copies the same byte of the sequence before: unit literals, then
// (ll 0, ml unit, off unit) up to nbytes, then the 0..unit-1 literals left.
static void flat_chain(int64_t nbytes, int unit, std::vector<Seq> &seqs, std::vector<uint8_t> &lits) {
    const int64_t m = (nbytes - unit) / unit, tail = nbytes - unit - unit * m;
    seqs.assign((size_t)m, Seq{0, unit, (uint32_t)unit});
    seqs[0].ll = unit;
    lits.clear();
    for (int64_t i = 0; i < unit + tail; i++) lits.push_back((uint8_t)(0x61 + i));
}

static int64_t ipow(int64_t b, int k) {
    int64_t r = 1;
    while (k-- > 0) r *= b;
    return r;
}
// tests/split_streams.py bound_edge_sizes
static void bound_edge_sizes(int k, int unit, int64_t out[3]) {
    const int64_t h = ipow(om::HOPS, k);
    out[0] = unit * h - unit - 1;
    out[1] = unit * (h - 2);
    out[2] = unit * (h - 1);
}

int main() {
    std::vector<Seq> seqs;
    std::vector<uint8_t> lits;

    // flat chains at the round rule's edges: settled after exactly the rule's
    // count of synchronous rounds
    for (int unit = 3; unit <= 4; unit++)
        for (int k = 1; k <= 3; k++) {
            int64_t sz[3];
            bound_edge_sizes(k, unit, sz);
            for (int64_t n : sz) {
                flat_chain(n, unit, seqs, lits);
                const std::vector<uint8_t> ref = serial(seqs, lits);
                CHECK((int64_t)ref.size() == n, "flat chain of %lld bytes decodes to %zu", (long long)n, ref.size());
                std::vector<uint32_t> org = fill_map<int64_t>(seqs, (int64_t)lits.size(), n);
                const int jr = om::rounds(n, unit);
                for (int r = 0; r < jr; r++) jump_round(org, n, 3);
                CHECK(settled(org, n), "flat chain %lld / %d not settled after rounds() = %d", (long long)n, unit, jr);
                for (int mis = 0; mis < 4; mis++) CHECK(gather(org, lits, n, mis, ref) == 0, "flat chain gather");
                run_case<int32_t>(seqs, lits, n, jr, 1);
            }
        }

    // one round on the k = 3 flat chain leaves pointers: the gather reports
    // them and writes nothing there
    int unsettled_quads = 0;
    {
        int64_t sz[3];
        bound_edge_sizes(3, 4, sz);
        flat_chain(sz[2], 4, seqs, lits);
        const std::vector<uint8_t> ref = serial(seqs, lits);
        std::vector<uint32_t> org = fill_map<int32_t>(seqs, (int64_t)lits.size(), sz[2]);
        jump_round(org, sz[2], 2);
        CHECK(!settled(org, sz[2]), "k = 3 flat chain settled after one round");
        for (int mis = 0; mis < 4; mis++) unsettled_quads = gather(org, lits, sz[2], mis, ref);
        CHECK(unsettled_quads > 0, "no unsettled quad reported");
    }

    // overlapped matches (off < ml) starting at each residue of p & 3, runs of
    // every short length (scalar head, 4-wide body, scalar tail of both
    // writers), whole and cut at each of the last few bytes (partial quads,
    // runs that stop short)
    const uint32_t offs[] = {1, 2, 3, 5};
    for (int r = 0; r < 4; r++)
        for (uint32_t off : offs)
            for (int64_t ml = off + 1; ml <= off + 14; ml++)
                for (int64_t ll2 = 0; ll2 <= 5; ll2++) {
                    seqs = {Seq{8 + r, ml, off}, Seq{ll2, ml + 3, off}};
                    lits.clear();
                    for (int64_t i = 0; i < 8 + r + ll2 + 3; i++) lits.push_back((uint8_t)(0x30 + 7 * i));
                    const int64_t n = 8 + r + ml + ll2 + ml + 3 + 3;
                    run_case<int32_t>(seqs, lits, n, om::MAX_ROUNDS, 2);
                    run_case<int64_t>(seqs, lits, n, om::MAX_ROUNDS, 3);
                    if (ll2 == 0 || ll2 == 5)
                        for (int64_t cut = 1; cut <= 7; cut++) {
                            run_case<int32_t>(seqs, lits, n - cut, om::MAX_ROUNDS, 1);
                            run_case<int32_t>(seqs, lits, n - cut - ml, om::MAX_ROUNDS, 1);
                        }
                }
    for (int i = 0; i < 4; i++) CHECK(g_residue[i] > 0, "no case with total & 3 == %d", i);

    // the round rule, for the Python mirror (tests/split_streams.py jump_rounds)
    for (int unit = 3; unit <= 4; unit++) {
        for (int k = 1; k <= 7; k++) {
            int64_t sz[3];
            bound_edge_sizes(k, unit, sz);
            for (int64_t n : sz) printf("rounds %lld %d %d\n", (long long)n, unit, om::rounds(n, unit));
        }
        const int64_t more[] = {0, 1, 16, 65536, 4ll << 20, (4ll << 20) + 1, 64ll << 20, 1ll << 30, (1ll << 31) - 1};
        for (int64_t n : more) printf("rounds %lld %d %d\n", (long long)n, unit, om::rounds(n, unit));
    }
    printf("cases=%d unsettled_quads=%d residues=%d,%d,%d,%d bad=%d\n", g_cases, unsettled_quads, g_residue[0], g_residue[1],
           g_residue[2], g_residue[3], g_bad);
    return g_bad ? 1 : 0;
}
