// Stand-alone driver for tests/test_compact_splice_seal_plan.py, built with
// AddressSanitizer + UBSan: the spliced compaction's rule fed from packed seek
// tables (juicefs_amd/csrc/splice_plan.h, PackedTables -- what the sealed call
// has on the host) against the same rule fed from the whole objects.  Reads
// tests/splice_plan_main.cc's case format.  Per case it packs every source's
// table as the kernel of zstd_seek_tables.hip does -- zstd_seek.h's table_at_end
// on the object, the slot splice_slot_bytes gives its capacity, nothing copied
// for a table that does not fit -- into a buffer of exactly the slots' bytes,
// plans both ways, and prints one JSON object:
//   same     1 when the two SplicePlans agree field for field
//   fit      per source: 1 when it has a table and the table fits its slot, 0 when
//            it has none, -1 when it has one that does not fit
//   tab      per source, from the packed tables: valid, entry, nf, D
//   outside  fetches the rule made of a packed source outside its table
//   counts   the packed plan's counters
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "splice_plan.h"

using namespace jfs_plan;

static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

static bool same_seg(const jfs_compact_seg &a, const jfs_compact_seg &b) {
    return a.src == b.src && a.src_off == b.src_off && a.dst_off == b.dst_off && a.len == b.len;
}

static bool same_plan(const SplicePlan &a, const SplicePlan &b) {
    if (a.tab.size() != b.tab.size() || a.frame_first != b.frame_first || a.frames.size() != b.frames.size() ||
        a.units.size() != b.units.size() || a.seg_first != b.seg_first || a.seg.size() != b.seg.size() || a.outs != b.outs ||
        a.passed != b.passed || a.fresh != b.fresh || a.passed_bytes != b.passed_bytes)
        return false;
    for (size_t i = 0; i < a.tab.size(); i++) {
        const SpliceTable &x = a.tab[i], &y = b.tab[i];
        if (x.valid != y.valid || x.entry != y.entry || x.nf != y.nf || x.total != y.total || x.c != y.c || x.d != y.d ||
            x.x != y.x || x.coff != y.coff || x.doff != y.doff)
            return false;
    }
    for (size_t q = 0; q < a.frames.size(); q++) {
        const SpliceFrame &x = a.frames[q], &y = b.frames[q];
        if (x.src != y.src || x.k != y.k || x.coff != y.coff || x.c != y.c || x.d != y.d || x.x != y.x || x.unit != y.unit)
            return false;
    }
    for (size_t u = 0; u < a.units.size(); u++)
        if (a.units[u].out != b.units[u].out || a.units[u].piece != b.units[u].piece || a.units[u].total != b.units[u].total)
            return false;
    for (size_t q = 0; q < a.seg.size(); q++)
        if (!same_seg(a.seg[q], b.seg[q])) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t nsrc = 0;
    while (rd(f, &nsrc, 4)) {
        std::vector<std::vector<uint8_t>> obj(nsrc);
        std::vector<int64_t> len(nsrc), cap(nsrc);
        for (int i = 0; i < nsrc; i++) {
            int32_t n = 0;
            if (!rd(f, &cap[i], 8) || !rd(f, &n, 4)) return 3;
            obj[i].resize(n);
            if (n > 0 && !rd(f, obj[i].data(), n)) return 3;
            len[i] = n;
        }
        int32_t nout = 0, csum_out = 0;
        if (!rd(f, &nout, 4) || !rd(f, &csum_out, 4)) return 3;
        std::vector<uint8_t> use(nout);
        std::vector<int32_t> seg_first(nout + 1);
        if (nout > 0 && !rd(f, use.data(), nout)) return 3;
        if (!rd(f, seg_first.data(), 4 * (size_t)(nout + 1))) return 3;
        std::vector<jfs_compact_seg> seg(seg_first[nout]);
        if (!seg.empty() && !rd(f, seg.data(), sizeof(jfs_compact_seg) * seg.size())) return 3;
        std::vector<int64_t> total(nout, 0);
        for (int j = 0; j < nout; j++)
            for (int k = seg_first[j]; k < seg_first[j + 1]; k++) total[j] += seg[k].len;
        const SplicePlan whole = splice_plan([&](int i, int32_t p) -> uint8_t { return obj[i][p]; }, nsrc, len.data(),
                                             cap.data(), nout, seg_first.data(), seg.data(), total.data(), use.data(),
                                             csum_out != 0);
        // the packed buffer: exactly the slots, so that ASan sees a byte past any of them
        std::vector<int64_t> at(nsrc + 1, 0);
        for (int i = 0; i < nsrc; i++) at[i + 1] = at[i] + splice_slot_bytes(cap[i]);
        std::vector<uint8_t> tab((size_t)at[nsrc]);
        std::vector<int32_t> tlen(nsrc, 0), fit(nsrc, 0);
        for (int i = 0; i < nsrc; i++) {
            const int32_t T = jfs::zseek::table_at_end([&](int32_t p) { return obj[i][p]; }, len[i]);
            fit[i] = T == 0 ? 0 : T <= at[i + 1] - at[i] ? 1 : -1;
            if (fit[i] == 1) {
                tlen[i] = T;
                memcpy(tab.data() + at[i], obj[i].data() + (len[i] - T), (size_t)T);
            }
        }
        uint64_t outside = 0;
        const PackedTables packed{tab.data(), at.data(), tlen.data(), len.data(), &outside};
        std::vector<int64_t> plen(nsrc);
        for (int i = 0; i < nsrc; i++) plen[i] = packed.src_len(i);
        const SplicePlan P = splice_plan(packed, nsrc, plen.data(), cap.data(), nout, seg_first.data(), seg.data(),
                                         total.data(), use.data(), csum_out != 0);
        std::string s = "{\"same\":";
        s += same_plan(whole, P) ? "1" : "0";
        s += ",\"fit\":[";
        char b[256];
        for (int i = 0; i < nsrc; i++) {
            snprintf(b, sizeof b, "%s%d", i ? "," : "", fit[i]);
            s += b;
        }
        s += "],\"tab\":[";
        for (int i = 0; i < nsrc; i++) {
            snprintf(b, sizeof b, "%s[%d,%d,%d,%u]", i ? "," : "", P.tab[i].valid, P.tab[i].entry, P.tab[i].nf, P.tab[i].total);
            s += b;
        }
        snprintf(b, sizeof b, "],\"outside\":%llu,\"counts\":[%llu,%llu,%llu,%llu]}", (unsigned long long)outside,
                 (unsigned long long)P.outs, (unsigned long long)P.passed, (unsigned long long)P.fresh,
                 (unsigned long long)P.passed_bytes);
        s += b;
        puts(s.c_str());
    }
    fclose(f);
    return 0;
}
