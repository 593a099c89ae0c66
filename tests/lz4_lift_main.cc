// Host driver of the LZ4 lift's rules (juicefs_amd/csrc/lz4_lift.h), built with
// AddressSanitizer and UBSan by tests/test_lz4_lift.py.
//
//   lz4_lift_main CASES
//
// CASES: little-endian records, each [u32 kind] and then
//   1  [u32 n][i32 chunk][n bytes]       a stored LZ4 block and a chunk of it
//   2  [u32 n][n bytes A][n bytes B]     two blocks to encode, B an overwrite of A
//   3  [u32 nout][u32 nsrc][i32 cap * nsrc] then per output
//      [i32 total][u32 nseg][{src, src_off, dst_off, len} * nseg]   a compaction plan
//   4  [u32 n][u32 nsrc] then per source [i32 len][i32 cap][len bytes], then
//      [n bytes G][{i32 src, i32 src_chunk} * chunks of n]   a gathered block, the
//      stored sources and their decode capacities, and a candidate per chunk
// and one line per record:
//   lift I total T ok L nrec R tail X lit0 Y body B first P:M:O:L valid V
//      the serial restatement's answer (lift_host); first = record 0's pos, mlen,
//      off, lit; valid = an independent check of the records against the bytes a
//      serial LZ interpreter decodes: every match copies what stands at its
//      place, the literals between the matches tile the chunk, and nrec, tail,
//      lit0 and body are parse_kernel's formulas over them
//   det I n N chunks C lifted K refused R same S
//      A and B encoded by the fast encoder's host twin; B encoded again by
//      jfs_test_lz4_fast_lift_host with every interior chunk that A and B share
//      a candidate from A's stream; same = the two encodings of B are equal
//   plan I cand b:j:src:i,... srcs a,b,... per_out x,y,...
//      lift_plan's candidates ("-": none)
//   emit I n N size S crc C lifted K valid V nrec r,r,...
//      jfs_test_lz4_fast_lift_host over G: the block's size, zlib's CRC-32 of its
//      bytes, the chunks lifted, valid = the serial interpreter decodes the block
//      to G, and per chunk the lifted records' count or -1 for a parsed chunk
// The last line checks the switch's row of host_modes.h.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "host_modes.h"
#include "lz4_fast_host.cc"  // the host twin and its lift form
#include "lz4_lift.h"

namespace lz4l = jfs::lz4l;

// plain LZ4 block decoding with every bound checked; returns the bytes it could define
static std::vector<uint8_t> interpret(const uint8_t *s, int64_t n) {
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

static bool records_valid(const lz4l::Lifted &r, const std::vector<uint8_t> &bytes, int32_t chunk) {
    const int64_t F = (int64_t)chunk * kChunk;
    if ((int64_t)bytes.size() < F + kChunk) return false;
    const uint8_t *c = bytes.data() + F;
    int64_t anchor = 0;
    uint32_t body = 0;
    for (int32_t k = 0; k < r.nrec; k++) {
        const int64_t pos = r.x[k] & 0xffff, ml = r.x[k] >> 16, off = r.y[k] & 0xffff, lit = r.y[k] >> 16;
        if (pos - lit != anchor || ml < kMinMatch || off < 1 || pos - off < 0 || pos + ml > kChunk) return false;
        for (int64_t q = 0; q < ml; q++)
            if (c[pos + q] != c[pos + q - off]) return false;
        body += (uint32_t)(1 + lit + 2 + len_bytes(ml - kMinMatch) + (k ? len_bytes(lit) : 0));
        anchor = pos + ml;
    }
    return r.tail == kChunk - anchor && body == r.body && r.lit0 == (r.nrec ? (int32_t)(r.y[0] >> 16) : 0) &&
           r.nrec == (int32_t)r.x.size() && r.nrec <= kMaxRec;
}

static std::vector<uint8_t> twin(const std::vector<uint8_t> &src) {
    std::vector<uint8_t> dst(src.size() + src.size() / 255 + 64);
    const int64_t r = jfs_test_lz4_fast_host(dst.data(), (int64_t)dst.size(), src.data(), (int64_t)src.size());
    dst.resize((size_t)r);
    return dst;
}

// zlib's CRC-32 (reflected 0xedb88320), bit by bit
static uint32_t crc32(const uint8_t *p, int64_t n) {
    uint32_t c = 0xffffffffu;
    for (int64_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1)));
    }
    return ~c;
}

static int check_mode_row() {
    using namespace jfs_host;
    const ModeDesc &d = MODE_COMPACT_LZ4_LIFT;
    int bad = 0;
    bad += strcmp(d.env, "JFS_COMPACT_LZ4_LIFT") != 0;
    bad += d.def != JFS_COMPACT_LZ4_LIFT_OFF || d.set_max != JFS_COMPACT_LZ4_LIFT_ON || d.ext_max != JFS_COMPACT_LZ4_LIFT_ON;
    const struct {
        const char *s;
        int v;
    } rows[] = {{nullptr, 0}, {"", 0}, {"on", 1}, {"ON", 1}, {"oN", 1}, {"off", 0}, {"OFF", 0}, {"oFf", 0},
                {"onx", 0},   {" on", 0}, {"on ", 0}, {"1", 0}, {"all", 0}, {"bogus", 0}, {"o", 0}};
    for (const auto &r : rows) bad += mode_parse(d, r.s) != r.v;
    return bad;
}

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int cases = 0;
    for (;; cases++) {
        uint32_t kind = 0, n = 0;
        if (fread(&kind, 4, 1, f) != 1) break;
        if (kind == 1) {
            int32_t chunk = 0;
            if (!rd(f, &n, 4) || !rd(f, &chunk, 4) || n > (1u << 28)) return 2;
            std::vector<uint8_t> s(n);
            if (!rd(f, s.data(), n)) return 2;
            const lz4l::Lifted r = lz4l::lift_host(s.data(), (int32_t)n, chunk);
            const bool valid = r.ok && records_valid(r, interpret(s.data(), n), chunk);
            const uint32_t x0 = r.ok && r.nrec ? r.x[0] : 0, y0 = r.ok && r.nrec ? r.y[0] : 0;
            printf("lift %d total %lld ok %d nrec %d tail %d lit0 %d body %u first %u:%u:%u:%u valid %d\n", cases,
                   (long long)r.total, (int)r.ok, r.nrec, r.tail, r.lit0, r.body, x0 & 0xffff, x0 >> 16, y0 & 0xffff, y0 >> 16,
                   (int)valid);
        } else if (kind == 2) {
            if (!rd(f, &n, 4) || n > (1u << 28)) return 2;
            std::vector<uint8_t> A(n), B(n);
            if (!rd(f, A.data(), n) || !rd(f, B.data(), n)) return 2;
            const std::vector<uint8_t> ea = twin(A), eb = twin(B);
            // the candidates: every interior chunk that A and B share, from A's stream
            std::vector<int32_t> lift;
            int64_t cand = 0, chunks = 0;
            for (int64_t cbase = 0; cbase < n; cbase += kChunk, chunks++) {
                const int64_t c = cbase >> kChunkLog;
                const bool take = lz4l::interior(c, n) && memcmp(A.data() + cbase, B.data() + cbase, (size_t)kChunk) == 0;
                lift.push_back(take ? 0 : -1);
                lift.push_back(take ? (int32_t)c : 0);
                cand += take;
            }
            const uint8_t *stream = ea.data();
            const int32_t slen = (int32_t)ea.size(), cap = (int32_t)n;
            int32_t lifted = 0;
            std::vector<uint8_t> out(eb.size() + 64);
            const int64_t got = jfs_test_lz4_fast_lift_host(out.data(), (int64_t)out.size(), B.data(), n, lift.data(), 1, &stream,
                                                            &slen, &cap, &lifted, nullptr);
            const int64_t refused = cand - lifted;
            const bool same = got == (int64_t)eb.size() && memcmp(out.data(), eb.data(), eb.size()) == 0;
            printf("det %d n %u chunks %lld lifted %lld refused %lld same %d\n", cases, n, (long long)chunks,
                   (long long)lifted, (long long)refused, (int)same);
        } else if (kind == 3) {
            uint32_t nout = 0, nsrc = 0;
            if (!rd(f, &nout, 4) || !rd(f, &nsrc, 4) || nout > 4096 || nsrc > 4096) return 2;
            std::vector<int32_t> cap(nsrc), total(nout), first(1, 0);
            std::vector<jfs_compact_seg> seg;
            if (!rd(f, cap.data(), 4 * (size_t)nsrc)) return 2;
            for (uint32_t k = 0; k < nout; k++) {
                uint32_t ns = 0;
                if (!rd(f, &total[k], 4) || !rd(f, &ns, 4) || ns > 4096) return 2;
                seg.resize(seg.size() + ns);
                if (!rd(f, seg.data() + first.back(), sizeof(jfs_compact_seg) * (size_t)ns)) return 2;
                first.push_back((int32_t)seg.size());
            }
            const lz4l::LiftPlan P = lz4l::lift_plan((int)nout, first.data(), seg.data(), total.data(), (int)nsrc, cap.data());
            printf("plan %d cand ", cases);
            int64_t g = 0, shown = 0, sum = 0;
            for (uint32_t k = 0; k < nout; k++) {
                sum += P.per_out[k];
                for (int64_t j = 0; j < nchunks(total[k]); j++, g++)
                    if (P.chunk[g].src >= 0)
                        printf("%s%u:%lld:%d:%d", shown++ ? "," : "", k, (long long)j, P.chunk[g].src, P.chunk[g].src_chunk);
            }
            if (g != (int64_t)P.chunk.size() || shown != P.candidates || sum != P.candidates) return 3;
            printf("%s srcs ", shown ? "" : "-");
            for (size_t q = 0; q < P.srcs.size(); q++) printf("%s%d", q ? "," : "", P.srcs[q]);
            printf("%s per_out ", P.srcs.empty() ? "-" : "");
            for (uint32_t k = 0; k < nout; k++) printf("%s%d", k ? "," : "", P.per_out[k]);
            printf("\n");
        } else if (kind == 4) {
            uint32_t nsrc = 0;
            if (!rd(f, &n, 4) || !rd(f, &nsrc, 4) || n > (1u << 28) || nsrc > 4096) return 2;
            std::vector<int32_t> slen(nsrc), cap(nsrc);
            std::vector<std::vector<uint8_t>> streams(nsrc);
            std::vector<const uint8_t *> ptr(nsrc);
            for (uint32_t i = 0; i < nsrc; i++) {
                if (!rd(f, &slen[i], 4) || !rd(f, &cap[i], 4) || slen[i] < 0 || slen[i] > (1 << 28)) return 2;
                streams[i].resize((size_t)slen[i]);
                if (!rd(f, streams[i].data(), (size_t)slen[i])) return 2;
                ptr[i] = streams[i].data();
            }
            const int64_t nc = nchunks(n);
            std::vector<uint8_t> G(n);
            std::vector<int32_t> lift(2 * (size_t)nc), nrec((size_t)nc, -2);
            if (!rd(f, G.data(), n) || !rd(f, lift.data(), 8 * (size_t)nc)) return 2;
            std::vector<uint8_t> out((size_t)n + n / 255 + 64);
            int32_t lifted = -1;
            const int64_t got = jfs_test_lz4_fast_lift_host(out.data(), (int64_t)out.size(), G.data(), n, lift.data(), (int)nsrc,
                                                            ptr.data(), slen.data(), cap.data(), &lifted, nrec.data());
            // the block is a block of G, whatever was lifted
            const std::vector<uint8_t> back = interpret(out.data(), got);
            const bool valid = got > 0 && back == G;
            printf("emit %d n %u size %lld crc %u lifted %d valid %d nrec ", cases, n, (long long)got, crc32(out.data(), got),
                   lifted, (int)valid);
            for (int64_t j = 0; j < nc; j++) printf("%s%d", j ? "," : "", nrec[(size_t)j]);
            printf("%s\n", nc ? "" : "-");
        } else {
            return 2;
        }
    }
    fclose(f);
    printf("cases=%d modes_bad=%d\n", cases, check_mode_row());
    return 0;
}
