// Stand-alone check of put16_masks (juicefs_amd/csrc/lz4_put16.h) against the
// byte-wise definition, for every ha in 0..3 and m in 1..16: byte b of the 20
// is written iff ha <= b < ha + m.  Built and run by test_lz4_put16_masks.py.
#include <stdint.h>
#include <stdio.h>

#include "lz4_put16.h"

int main() {
    int cases = 0, bad = 0;
    for (uint32_t ha = 0; ha < 4; ++ha) {
        for (uint32_t m = 1; m <= 16; ++m) {
            const jfs::lz4d::Put16Masks got = jfs::lz4d::put16_masks(ha, m);
            for (int j = 0; j < 5; ++j) {
                uint32_t want = 0;
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint32_t pos = 4u * (uint32_t)j + b;
                    if (pos >= ha && pos < ha + m) want |= 0xFFu << (8 * b);
                }
                if (got.k[j] != want) {
                    printf("ha=%u m=%u dword %d: got %08x want %08x\n", ha, m, j, got.k[j], want);
                    bad++;
                }
            }
            cases++;
        }
    }
    printf("cases=%d bad=%d\n", cases, bad);
    return bad ? 1 : 0;
}
