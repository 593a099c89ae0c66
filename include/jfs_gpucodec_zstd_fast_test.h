/*
 * jfs_gpucodec_zstd_fast_test.h -- the test hooks of the fast Zstd encoder
 * (DESIGN 4f), exported by libjfsgpu.so for its own test suite
 * (tests/test_zstd_fast.py, tests/test_zstd_fast_gpu.py).  NOT part of the
 * drop-in ABI of jfs_gpucodec.h: the Go adapter never binds
 * them.  They have a header of their own because jfs_gpucodec_test.h's list of
 * hooks is pinned by tests/test_capi.py.
 *
 * Both hooks return the sequence records the entropy stage reads, for every
 * 128 KiB block of the frame of src[0, n) in block order: block k's records
 * follow block k - 1's in out_u64 (ll | (ml - 3) << 17 | Offset_Value << 34),
 * ns_per_block[k] is their count and nl_per_block[k] the block's literal count
 * (trailing literals included).  ns_per_block and nl_per_block hold
 * (n + 131071) / 131072 entries.  The return value is the total record count,
 * or -1 when n is out of range, cap records do not hold them, or (device) a
 * HIP call failed; nothing is written then.
 */
#ifndef JFS_GPUCODEC_ZSTD_FAST_TEST_H
#define JFS_GPUCODEC_ZSTD_FAST_TEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no GPU: the host twin of the fast parse (zfast_parse and
 * zfast_seq restated tile by tile in plain C++).  Not a fallback: no product
 * entry point calls it. */
int64_t jfs_test_zstd_fast_host_seqs(const uint8_t *src, int64_t n, uint64_t *out_u64, int64_t cap,
                                     int32_t *ns_per_block, int32_t *nl_per_block);

/* The two kernels on the current device: d_src is device memory, the outputs
 * are host memory.  Host-synchronous. */
int64_t jfs_test_zstd_fast_seqs_device(const uint8_t *d_src, int64_t n, uint64_t *out_u64, int64_t cap,
                                       int32_t *ns_per_block, int32_t *nl_per_block);

#ifdef __cplusplus
}
#endif
#endif /* JFS_GPUCODEC_ZSTD_FAST_TEST_H */
