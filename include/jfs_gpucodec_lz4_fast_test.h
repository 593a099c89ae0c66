/*
 * jfs_gpucodec_lz4_fast_test.h -- the test hook of the fast LZ4 encoder
 * (DESIGN 4e), exported by libjfsgpu.so for its own test suite
 * (tests/test_lz4_fast.py, tests/test_lz4_fast_gpu.py).  NOT part of the
 * drop-in ABI of jfs_gpucodec.h: the Go adapter never binds it.
 * It has a header of its own because jfs_gpucodec_test.h's list of hooks is
 * pinned by tests/test_capi.py.
 */
#ifndef JFS_GPUCODEC_LZ4_FAST_TEST_H
#define JFS_GPUCODEC_LZ4_FAST_TEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, no GPU: the host twin of jfs_lz4_compress_fast_device.  It restates
 * the kernels' parse tile by tile and returns the same value and writes the
 * same bytes (0, and not a byte, when the block does not fit dst_cap).  Not a
 * fallback: no product entry point calls it. */
int64_t jfs_test_lz4_fast_host(uint8_t *dst, int64_t dst_cap, const uint8_t *src, int64_t n);
/* Chunks per launch group of the fast encoder (default 8,192; 0 restores it), so
 * that a test reaches several groups with small blocks.  Returns the previous
 * value.  Process-wide; not for use while a call is in flight. */
int jfs_test_set_lz4_fast_group_chunks(int chunks);

#ifdef __cplusplus
}
#endif
#endif /* JFS_GPUCODEC_LZ4_FAST_TEST_H */
