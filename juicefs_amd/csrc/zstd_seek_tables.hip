// Seek tables out of device-resident objects into one packed buffer (DESIGN 11e;
// the contract is jfs_zstd_seek_tables_device's in the header): what the sealed
// spliced compaction brings to the host of every opened source, instead of the
// source.  One kernel:
//   zseek_tables  one wave per input: the 9-byte footer at its end, the skippable
//                 header where the footer says the table starts, and then the
//                 table's T bytes to the input's slot.
// Only the placement is checked here -- the footer's magic, descriptor and frame
// count, and the header's magic and size word.  What the entries add up to is
// zstd_seek.h's parser's on the host, over the copied bytes.  No LDS; everything
// is written with plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "copy_any.cuh"
#include "jfs_internal.h"
#include "wave.cuh"
#include "zstd_seek.h"

namespace jfs {
namespace zseek {

typedef JFS_GLOBAL const int32_t gc_i32;

__global__ __launch_bounds__(64) void zseek_tables(const jfs_dev_block *__restrict__ blocks,
                                                   const int32_t *__restrict__ len, int nblk,
                                                   const int32_t *__restrict__ slot_first, uint8_t *__restrict__ tables,
                                                   int32_t *__restrict__ table_len) {
    const int i = (int)blockIdx.x, lane = lane_id();
    if (i >= nblk) return;
    gc_u8 *src = (gc_u8 *)((gc_blk *)blocks)[i].src;
    const int32_t n = ((gc_i32 *)len)[i];
    const int32_t s0 = ((gc_i32 *)slot_first)[i], s1 = ((gc_i32 *)slot_first)[i + 1];
    // every lane reads the same 17 bytes: the verdict is the wave's without a broadcast
    int32_t T = src ? table_at_end([src](int32_t p) { return src[p]; }, (int64_t)n) : 0;
    if (s0 < 0 || s1 < s0 || T > s1 - s0) T = 0;  // a table that does not fit its slot is no table
    if (lane == 0) ((JFS_GLOBAL int32_t *)table_len)[i] = T;
    if (T > 0) copy_any<64>((g_u8 *)tables + s0, src + (n - T), T, lane);
}

}  // namespace zseek
}  // namespace jfs

extern "C" int jfs_launch_zstd_seek_tables(const jfs_dev_block *d_blocks, const int32_t *d_len, int nblk,
                                           const int32_t *d_slot_first, uint8_t *d_tables, int32_t *d_table_len,
                                           hipStream_t stream) {
    if (nblk <= 0) return 0;
    hipLaunchKernelGGL(jfs::zseek::zseek_tables, dim3((unsigned)nblk), dim3(64), 0, stream, d_blocks, d_len, nblk,
                       d_slot_first, d_tables, d_table_len);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
