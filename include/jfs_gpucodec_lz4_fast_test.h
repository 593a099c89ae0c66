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
/* Host only, no GPU: what jfs_lz4_compress_fast_lift_device writes for the
 * gathered block src[0, n) -- the twin above, with the records of every chunk
 * the lift takes read from its source's stored stream instead of parsed.
 * lift: one {src, src_chunk} pair of int32 per 64 KiB chunk of the block
 * (src < 0: no candidate).  Source i is the stored LZ4 block stream[i][0,
 * stream_len[i]), decoded into src_cap[i] bytes; the streams are well-formed
 * (the device asks their decode's result, this function only counts their
 * output).  A chunk is lifted iff it is interior in n, its source is one of
 * nsrc, the source's chunk is interior in src_cap[src], the source's output
 * fits src_cap[src], and the serial rule (lz4_lift.h, lift_host) accepts it;
 * every other chunk is parsed.  *lifted (may be null): the chunks lifted.
 * chunk_nrec (may be null): per chunk, a lifted chunk's count of records, or -1
 * for a parsed one.  Returns the block's size (0, and not a byte, when it does
 * not fit dst_cap or an argument is out of range).  Not a fallback: no product
 * entry point calls it. */
int64_t jfs_test_lz4_fast_lift_host(uint8_t *dst, int64_t dst_cap, const uint8_t *src, int64_t n, const int32_t *lift,
                                    int nsrc, const uint8_t *const *stream, const int32_t *stream_len,
                                    const int32_t *src_cap, int32_t *lifted, int32_t *chunk_nrec);

#ifdef __cplusplus
}
#endif
#endif /* JFS_GPUCODEC_LZ4_FAST_TEST_H */
