// Stand-alone check of tail_pack (juicefs_amd/csrc/lz4_tailpack.h) over its
// whole stated range: ds, ss in 0..4095, rem in 1..64.  For every triple the
// fields must unpack to what was packed, and the direct bit must be set
// exactly when the byte-wise definition of wave_near (chunks of min(D, 64)
// bytes, slots taken mod 4096) makes one chunk in which no source or
// destination slot wraps; D = (ds - ss) mod 4096 as the kernel's general path
// derives it (D = 0 is no match distance and is skipped).  Built and run by
// test_lz4_tailpack.py.
#include <stdint.h>
#include <stdio.h>

#include "lz4_tailpack.h"

int main() {
    using namespace jfs::lz4d;
    long cases = 0, bad = 0;
    for (uint32_t ds = 0; ds < TP_RING; ++ds) {
        for (uint32_t ss = 0; ss < TP_RING; ++ss) {
            const uint32_t D = (ds - ss) & (TP_RING - 1u);
            if (D == 0) continue;
            for (uint32_t rem = 1; rem <= TP_LEN_MAX; ++rem) {
                const uint32_t w = tail_pack(ds, ss, rem, D);
                const uint32_t step = D < 64u ? D : 64u;
                // byte-wise: one chunk, and the last byte's slots are the unmasked sums
                const bool one = rem <= step;
                const bool flat = ((ss + rem - 1u) & (TP_RING - 1u)) == ss + rem - 1u &&
                                  ((ds + rem - 1u) & (TP_RING - 1u)) == ds + rem - 1u;
                const bool ok = tail_ds(w) == ds && tail_ss(w) == ss && tail_rem(w) == rem &&
                                tail_direct(w) == (one && flat) && ((tail_ds(w) - tail_ss(w)) & (TP_RING - 1u)) == D;
                if (!ok && bad++ < 10) printf("ds=%u ss=%u rem=%u: w=%08x\n", ds, ss, rem, w);
                cases++;
            }
        }
    }
    printf("cases=%ld bad=%ld\n", cases, bad);
    return bad ? 1 : 0;
}
