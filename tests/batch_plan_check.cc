// Checks juicefs_amd/csrc/batch_plan.h (the host batch pipeline's planning
// arithmetic) on a CPU: fixed chunk tables derived from the code before the
// planner was split out of run_batch, then invariants over seeded random block
// lists.  Built and run by tests/test_batch_plan.py under ASan + UBSan.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../juicefs_amd/csrc/batch_plan.h"

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

static const int64_t MiB = 1 << 20;
// the tables' parameters: limit 16 MiB, ramp length 3, first-big 192, 3 slots
static PlanParams params(bool ramp_ok, int max_chunk_blocks = 0) { return {16 * MiB, max_chunk_blocks, ramp_ok, 3, 192, 3}; }

static void expect_chunks(const char *what, const Plan &pl, const std::vector<Chunk> &want) {
    CHECK(pl.ch.size() == want.size(), "%s: %zu chunks, want %zu", what, pl.ch.size(), want.size());
    for (size_t k = 0; k < want.size() && k < pl.ch.size(); k++) {
        const Chunk &a = pl.ch[k], &b = want[k];
        CHECK(a.s == b.s && a.e == b.e && a.slot == b.slot && a.tin == b.tin && a.tout == b.tout,
              "%s chunk %zu: [%d,%d) %d %lld %lld, want [%d,%d) %d %lld %lld", what, k, a.s, a.e, a.slot,
              (long long)a.tin, (long long)a.tout, b.s, b.e, b.slot, (long long)b.tin, (long long)b.tout);
    }
}

static void fixed_tables() {
    {
        std::vector<Block> b(10, Block{100, 1000});
        const Plan pl = plan_chunks(b.data(), 10, params(true));
        expect_chunks("10 small", pl, {{0, 10, 0, 1120, 10080}});
        for (int i = 0; i < 10; i++)
            CHECK(pl.in_off[i] == 112 * i && pl.out_off[i] == 1008 * i, "10 small: offsets of block %d", i);
    }
    const std::vector<Chunk> ramp6 = {{0, 32, 0, 524288, 1572864},     {32, 96, 1, 1048576, 3145728},
                                      {96, 224, 2, 2097152, 6291456},  {224, 416, 0, 3145728, 9437184},
                                      {416, 672, 1, 4194304, 12582912}, {672, 928, 2, 4194304, 12582912}};
    {
        std::vector<Block> b(1000, Block{16384, 49152});
        std::vector<Chunk> want = ramp6;
        want.push_back({928, 1000, 0, 1179648, 3538944});
        expect_chunks("1000 ramp", plan_chunks(b.data(), 1000, params(true)), want);
    }
    {
        std::vector<Block> b(1100, Block{16384, 49152});
        std::vector<Chunk> want = ramp6;
        want.push_back({928, 972, 0, 720896, 2162688});
        want.push_back({972, 1100, 1, 2097152, 6291456});
        const Plan pl = plan_chunks(b.data(), 1100, params(true));
        expect_chunks("1100 ramp", pl, want);
        CHECK(pl.in_off[972] == 0, "1100 ramp: in_off[972] = %lld", (long long)pl.in_off[972]);
        CHECK(pl.out_off[971] == 43 * 49152, "1100 ramp: out_off[971] = %lld", (long long)pl.out_off[971]);
        expect_chunks("1100 no ramp", plan_chunks(b.data(), 1100, params(false)),
                      {{0, 256, 0, 4194304, 12582912},
                       {256, 512, 1, 4194304, 12582912},
                       {512, 768, 2, 4194304, 12582912},
                       {768, 1024, 0, 4194304, 12582912},
                       {1024, 1100, 1, 1245184, 3735552}});
    }
    {
        std::vector<Block> b(40, Block{1000, 4096});
        expect_chunks("40 capped", plan_chunks(b.data(), 40, params(false, 16)),
                      {{0, 16, 0, 16128, 65536}, {16, 32, 1, 16128, 65536}, {32, 40, 2, 8064, 32768}});
    }
    {
        const std::vector<Block> b = {{100, 100}, {20 * MiB, 20 * MiB}, {100, 100}};
        for (const bool ramp_ok : {false, true})
            expect_chunks("oversize", plan_chunks(b.data(), 3, params(ramp_ok)),
                          {{0, 1, 0, 112, 112}, {1, 2, 1, 20 * MiB, 20 * MiB}, {2, 3, 2, 112, 112}});
    }
    CHECK(plan_chunks(nullptr, 0, params(true)).ch.empty(), "an empty batch has no chunks");
}

// the staging size as run_batch summed it before ChunkLayout (chunk_bytes)
static int64_t old_chunk_bytes(int64_t nb, int64_t tin, int64_t tout, int64_t zib, bool aead, bool crc, bool csum,
                               int64_t csum_area) {
    const int64_t aead_bytes =
        aead ? align16(nb * (int64_t)sizeof(jfs_aead_block)) + align16(nb * 4) + align16(nb * 64) : 0;
    const int64_t crc_bytes = crc ? align16(nb * (int64_t)sizeof(jfs_dev_block)) + 2 * align16(nb * 4) : 0;
    return tin + tout + align16(nb * (int64_t)sizeof(jfs_dev_block)) + align16(nb * 4) + align16(nb * zib) + aead_bytes +
           crc_bytes + (csum ? align16(nb * (int64_t)sizeof(jfs_dev_block)) + csum_area : 0);
}

static void check_layout(const Chunk &c, int64_t zib, bool aead, bool crc, bool csum, int64_t csum_area) {
    const int64_t nb = c.e - c.s, nd = nb * (int64_t)sizeof(jfs_dev_block);
    const ChunkLayout L(nb, c.tin, c.tout, zib, aead, crc, csum, csum_area);
    // every area in order with the bytes it must hold (0: absent)
    const struct {
        const char *name;
        int64_t off, bytes;
    } area[] = {{"in", L.in, c.tin},
                {"out", L.out, c.tout},
                {"desc", L.desc, nd},
                {"ret", L.ret, nb * 4},
                {"zinfo", L.zinfo, nb * zib},
                {"aead_desc", L.aead_desc, aead ? nb * (int64_t)sizeof(jfs_aead_block) : 0},
                {"aead_ret", L.aead_ret, aead ? nb * 4 : 0},
                {"aead_kn", L.aead_kn, aead ? nb * 64 : 0},
                {"crc_desc", L.crc_desc, crc ? nd : 0},
                {"crc_seed", L.crc_seed, crc ? nb * 4 : 0},
                {"crc", L.crc, crc ? nb * 4 : 0},
                {"csum_desc", L.csum_desc, csum ? nd : 0},
                {"csum", L.csum, csum ? csum_area : 0}};
    int64_t end = 0;  // of the areas so far
    for (const auto &a : area) {
        CHECK(a.off % 16 == 0, "%s at %lld is not 16-aligned", a.name, (long long)a.off);
        CHECK(a.off >= end, "%s at %lld overlaps the area before it (ends %lld)", a.name, (long long)a.off, (long long)end);
        CHECK(a.off - end < 16, "%s at %lld leaves a gap after %lld", a.name, (long long)a.off, (long long)end);
        end = a.off + a.bytes;
        CHECK(end <= L.total, "%s ends at %lld, past total %lld", a.name, (long long)end, (long long)L.total);
    }
    CHECK(L.in == 0, "the input area starts the slot");
    CHECK(L.total == old_chunk_bytes(nb, c.tin, c.tout, zib, aead, crc, csum, csum_area), "total %lld != chunk_bytes %lld",
          (long long)L.total, (long long)old_chunk_bytes(nb, c.tin, c.tout, zib, aead, crc, csum, csum_area));
    CHECK(L.aead_bytes == L.crc_desc - L.aead_desc && L.csum_bytes == L.total - L.csum, "area sizes");
    uint8_t base[1];
    CHECK(ChunkLayout::at<uint8_t>(base, 0) == base, "the accessor applies an offset to a base");
}

static void check_pieces(const Chunk &c, const Plan &pl, int max_npiece, int byte_np) {
    const Pieces pc{max_npiece, byte_np};
    const int np = pc.npiece(c), inp = pc.in_npiece(c), n = c.e - c.s;
    CHECK(np >= 1 && np <= std::max(max_npiece, byte_np) && inp >= 1 && inp <= max_npiece, "piece counts %d %d", np, inp);
    CHECK(pc.byte_pieces(c) == (n == 1 && byte_np > 1), "byte pieces are for one-block chunks");
    CHECK(np == (pc.byte_pieces(c) ? byte_np : n >= 64 ? std::min(max_npiece, n) : 1), "npiece %d", np);
    CHECK(pc.piece_o(c, 0, pl.out_off.data()) == 0, "the first piece starts the output area");
    for (int p = 0; p <= np + 1; p++) {
        const int64_t o = pc.piece_o(c, p, pl.out_off.data());
        if (p >= np) CHECK(o == c.tout, "piece %d of %d ends the output area", p, np);
        if (p < np) {
            CHECK(o <= pc.piece_o(c, p + 1, pl.out_off.data()) && o % 16 == 0, "piece_o is monotone and aligned");
            const int b0 = pc.piece_b(c, p), b1 = pc.piece_b(c, p + 1);
            CHECK(b0 >= c.s && b0 <= b1 && b1 <= c.e, "piece_b %d..%d of [%d,%d)", b0, b1, c.s, c.e);
            if (!pc.byte_pieces(c)) CHECK(b0 < c.e && o == pl.out_off[b0], "a block piece starts at its first block");
        }
    }
    CHECK(pc.in_piece_b(c, 0) == c.s && pc.in_piece_b(c, inp) == c.e, "input pieces cover the chunk");
    for (int p = 0; p < inp; p++) CHECK(pc.in_piece_b(c, p) < pc.in_piece_b(c, p + 1), "input pieces are not empty");
    if (!pc.byte_pieces(c)) CHECK(pc.piece_b(c, 0) == c.s && pc.piece_b(c, np) == c.e, "output pieces cover the chunk");
}

static void random_plans() {
    std::mt19937_64 rng(20240607);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    for (int iter = 0; iter < 400; iter++) {
        const int n = (int)pick(1, iter % 8 == 0 ? 1500 : 300);
        const int64_t big = iter % 3 == 0 ? 64 << 10 : 4 * MiB;
        std::vector<Block> b(n);
        for (Block &x : b) {
            x.in = pick(0, 9) == 0 ? 0 : pick(1, big);
            x.cap = pick(0, 9) == 0 ? 0 : pick(1, 3 * big);
            if (pick(0, 199) == 0) x.cap = 40 * MiB;  // larger than the limit
        }
        // (as run_batch calls it: a ramp only without a block cap)
        const int max_blocks = pick(0, 2) == 0 ? (int)pick(1, 40) : 0;
        const PlanParams p{pick(16, 64) * MiB, max_blocks, max_blocks == 0 && pick(0, 1) == 1, (int)pick(0, 8),
                           pick(0, 3) == 0 ? 0 : (int)pick(1, 300), 3};
        const Plan pl = plan_chunks(b.data(), n, p);
        int64_t total = 0;
        for (const Block &x : b) total += align16(x.in) + align16(x.cap);
        const bool ramp = p.ramp_ok && p.ramp_len > 0 && total > 2 * p.limit;
        int at = 0;
        for (size_t k = 0; k < pl.ch.size(); k++) {
            const Chunk &c = pl.ch[k];
            CHECK(c.s == at && c.e > c.s && c.e <= n, "chunk %zu [%d,%d) does not follow %d", k, c.s, c.e, at);
            CHECK(c.slot == (int)(k % 3), "chunk %zu on slot %d", k, c.slot);
            if (c.e - c.s > 1) {
                CHECK(c.tin + c.tout <= p.limit, "chunk %zu holds %lld bytes", k, (long long)(c.tin + c.tout));
                // block cap: 32, 64, 128, 128.. in the ramp, first_big in the chunk after it
                const int ki = (int)k;
                const int cap = ramp && ki < p.ramp_len                       ? std::min(32 << ki, 128)
                                : ramp && ki == p.ramp_len && p.first_big > 0 ? p.first_big
                                                                              : p.max_chunk_blocks;
                if (cap > 0) CHECK(c.e - c.s <= cap, "chunk %zu holds %d blocks, cap %d", k, c.e - c.s, cap);
            }
            int64_t tin = 0, tout = 0;
            for (int i = c.s; i < c.e; i++) {
                CHECK(pl.in_off[i] == tin && pl.out_off[i] == tout && tin % 16 == 0 && tout % 16 == 0,
                      "offsets of block %d in chunk %zu", i, k);
                tin += align16(b[i].in);
                tout += align16(b[i].cap);
            }
            CHECK(c.tin == tin && c.tout == tout, "totals of chunk %zu", k);
            at = c.e;
            for (int mask = 0; mask < 16; mask++) {
                int64_t csum_area = 0;
                for (int i = c.s; i < c.e; i++) csum_area += align16(4 * (b[i].cap > 0 ? (b[i].cap - 1) / (32 << 10) + 1 : 1));
                check_layout(c, mask & 1 ? 72 : 0, mask & 2, mask & 4, mask & 8, csum_area);
            }
            for (const int bnp : {0, 1, 2, 4}) check_pieces(c, pl, 4, bnp);
            check_pieces(c, pl, 3, 3);
        }
        CHECK(at == n, "chunks end at %d of %d", at, n);
        if (ramp && pl.ch.size() > 4)  // ramp down
            CHECK(pl.ch.back().e - pl.ch.back().s <= 128, "a ramped batch ends with %d blocks", pl.ch.back().e - pl.ch.back().s);
    }
}

static void split_geom() {
    std::mt19937_64 rng(7);
    for (int iter = 0; iter < 200; iter++) {
        const int n = (int)(rng() % 200);
        std::vector<int32_t> lens(n), caps(n);
        int64_t nseg = 0, max_cap = 0, norg = 0;
        for (int k = 0; k < n; k++) {
            lens[k] = (int32_t)(rng() % (8 << 20)) - (rng() % 16 == 0 ? 100 : 0);
            caps[k] = rng() % 32 == 0 ? INT32_MAX : (int32_t)(rng() % (8 << 20)) - (rng() % 16 == 0 ? 100 : 0);
            const int64_t len = lens[k] > 0 ? lens[k] : 0, cap = caps[k] > 0 ? caps[k] : 0;
            nseg += (len + 255) / 256;
            if (caps[k] > max_cap) max_cap = caps[k];
            norg += (cap + 3) / 4 * 4;
        }
        const Lz4SplitGeom g = lz4_split_geom(n, lens.data(), caps.data());
        CHECK(g.nseg == nseg && g.max_cap == max_cap && g.norg == norg, "geometry of %d blocks", n);
    }
}

int main() {
    fixed_tables();
    random_plans();
    split_geom();
    if (g_fail) {
        fprintf(stderr, "batch plan check: %d failure(s)\n", g_fail);
        return 1;
    }
    printf("batch plan check OK\n");
    return 0;
}
