// Stand-alone driver of juicefs_amd/csrc/splice_plan.h for tests/test_splice_plan.py,
// built with AddressSanitizer + UBSan.  Reads cases from a file, all fields
// little-endian:
//   i32 nsrc | nsrc x (i64 cap, i32 len, len bytes)
//   i32 nout | i32 csum_out | nout bytes `use` | (nout + 1) x i32 seg_first | nseg x 4 x i32
// and prints one JSON object per case: the tables, the frames of every spliced
// output, the units and segments of the derived plan, the lists of ranges per
// source, the counters, and `oob`, the fetches outside any object (the fetch
// handed to the rule counts them and answers 0).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "splice_plan.h"

static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

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
        long oob = 0;
        auto fetch = [&](int i, int32_t p) -> uint8_t {
            if (i < 0 || i >= nsrc || p < 0 || p >= (int32_t)obj[i].size()) {
                oob++;
                return 0;
            }
            return obj[i][p];
        };
        const jfs_plan::SplicePlan P = jfs_plan::splice_plan(fetch, nsrc, len.data(), cap.data(), nout, seg_first.data(),
                                                             seg.data(), total.data(), use.data(), csum_out != 0);
        // the decoded sources as the call stages them: every object that has bytes
        std::vector<jfs_plan::ChainSrc> st;
        for (int i = 0; i < nsrc; i++)
            if (len[i] > 0) st.push_back(jfs_plan::ChainSrc{i, 0, 0, len[i], cap[i], false, 0});
        const jfs_plan::ChainRanges R = jfs_plan::splice_ranges(P, nsrc, st, (int)st.size());
        std::string s = "{\"tab\":[";
        char b[256];
        for (int i = 0; i < nsrc; i++) {
            snprintf(b, sizeof b, "%s[%d,%d,%d,%u]", i ? "," : "", P.tab[i].valid, P.tab[i].entry, P.tab[i].nf, P.tab[i].total);
            s += b;
        }
        s += "],\"frame_first\":[";
        for (int j = 0; j <= nout; j++) {
            snprintf(b, sizeof b, "%s%d", j ? "," : "", P.frame_first[j]);
            s += b;
        }
        s += "],\"frames\":[";
        for (size_t q = 0; q < P.frames.size(); q++) {
            const jfs_plan::SpliceFrame &x = P.frames[q];
            snprintf(b, sizeof b, "%s[%d,%d,%u,%u,%u,%u,%d]", q ? "," : "", x.src, x.k, x.coff, x.c, x.d, x.x, x.unit);
            s += b;
        }
        s += "],\"units\":[";
        for (size_t u = 0; u < P.units.size(); u++) {
            snprintf(b, sizeof b, "%s[%d,%d,%d,%d,%d]", u ? "," : "", P.units[u].out, P.units[u].piece, P.units[u].total,
                     P.seg_first[u], P.seg_first[u + 1]);
            s += b;
        }
        s += "],\"seg\":[";
        for (size_t q = 0; q < P.seg.size(); q++) {
            snprintf(b, sizeof b, "%s[%d,%d,%d,%d]", q ? "," : "", P.seg[q].src, P.seg[q].src_off, P.seg[q].dst_off, P.seg[q].len);
            s += b;
        }
        s += "],\"ranges\":{";
        for (size_t k = 0; k < st.size(); k++) {
            snprintf(b, sizeof b, "%s\"%d\":[", k ? "," : "", st[k].idx);
            s += b;
            for (int32_t q = R.first[k]; q < R.first[k + 1]; q++) {
                snprintf(b, sizeof b, "%s[%d,%d]", q > R.first[k] ? "," : "", R.rng[q].lo, R.rng[q].hi);
                s += b;
            }
            s += "]";
        }
        snprintf(b, sizeof b, "},\"counts\":[%llu,%llu,%llu,%llu],\"oob\":%ld}", (unsigned long long)P.outs,
                 (unsigned long long)P.passed, (unsigned long long)P.fresh, (unsigned long long)P.passed_bytes, oob);
        s += b;
        puts(s.c_str());
    }
    fclose(f);
    return 0;
}
