/*
 * jfs_gpucodec.h -- C ABI of libjfsgpu.so, the MI355X block-compression engine
 * that drops in under JuiceFS's pkg/compress.
 *
 * Plain C types only (pointers + sizes); no torch / HIP types in signatures.
 * A stream argument is a hipStream_t passed as void* (0 = the library's own
 * per-device stream).
 *
 * Reference interface replaced (file:line in /root/reference):
 *   pkg/compress/compress.go:31-36   type Compressor interface {Name, CompressBound, Compress, Decompress}
 *   pkg/compress/compress.go:39-49   func NewCompressor(algr string) Compressor
 *   pkg/compress/compress.go:51-68   noOp            (Name "Noop")
 *   pkg/compress/compress.go:70-103  ZStandard{1}    (Name "Zstd", level ZSTD_LEVEL=1 :28)
 *   pkg/compress/compress.go:105-125 LZ4             (Name "LZ4")
 * Callers: pkg/chunk/cached_store.go:359,372 (upload), :764,814 (load),
 *          :827,846 (NewCachedStore), cmd/format.go:445 (validation).
 * The cgo binding a maintainer adds on the Go side is shown in INTEGRATION.md.
 */
#ifndef JFS_GPUCODEC_H
#define JFS_GPUCODEC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Codec ids (the three values NewCompressor can return). */
#define JFS_ALGO_NONE 0 /* noOp       compress.go:51  */
#define JFS_ALGO_LZ4 1  /* LZ4{}      compress.go:106 */
#define JFS_ALGO_ZSTD 2 /* ZStandard  compress.go:71  */

/* Status codes returned by the library (int64, all <= JFS_ERR_BASE).  LZ4
 * decompression failures return the raw LZ4_decompress_safe value instead (a
 * negative int32), because lz4.DecompressSafe passes it through to the Go
 * caller (compress.go:124); the two ranges never overlap. */
#define JFS_OK 0
#define JFS_ERR_BASE (-(1LL << 40))
#define JFS_ERR_SHORT_BUFFER (JFS_ERR_BASE - 1)  /* "buffer too short: %d < %d"   compress.go:57,64,88,100 */
#define JFS_ERR_EMPTY_INPUT (JFS_ERR_BASE - 2)   /* "decompress an empty input"   compress.go:122 / zstd ErrEmptySlice */
#define JFS_ERR_CORRUPT (JFS_ERR_BASE - 3)       /* malformed Zstd frame (ZSTD_decompress error) */
#define JFS_ERR_COMPRESS_FAIL (JFS_ERR_BASE - 4) /* LZ4_compress_default returned 0 */
#define JFS_ERR_UNSUPPORTED (JFS_ERR_BASE - 5)   /* operation not available in this build */
#define JFS_ERR_NO_DEVICE (JFS_ERR_BASE - 6)     /* no usable gfx950 device; the library never falls back to CPU */
#define JFS_ERR_INVALID (JFS_ERR_BASE - 7)       /* bad argument (unknown algo, negative size, ...) */
#define JFS_ERR_HIP (JFS_ERR_BASE - 8)           /* HIP runtime failure */
#define JFS_ERR_NO_MEMORY (JFS_ERR_BASE - 9)     /* pinned/HBM staging for this block could not be allocated */
#define JFS_ERR_AUTH (JFS_ERR_BASE - 10)         /* "cipher: message authentication failed" (aead.Open, encrypt.go:283) */
#define JFS_ERR_CHECKSUM (JFS_ERR_BASE - 11)     /* "verify checksum failed: %d != %d" (checksum.go:68) */

/* ---- Compressor surface (one synchronous call per block) ---------------- */

/* NewCompressor(algr): case-insensitive "zstd" | "lz4" | "none" | "" -> algo id,
 * anything else -> -1 (the Go factory's nil).                 compress.go:39-49 */
int jfs_codec_from_name(const char *name);

/* Name(): "Noop" / "LZ4" / "Zstd"; NULL for an unknown id.
 *                                                compress.go:53,76,109 */
const char *jfs_codec_name(int algo);

/* CompressBound(n).  LZ4: n>0x7E000000 ? 0 : n + n/255 + 16 (compress.go:112);
 * Zstd: n + n>>8 + (n < 128K ? (128K-n)>>11 : 0) (compress.go:79); none: n. */
int64_t jfs_compress_bound(int algo, int64_t n);

/* Compress(dst, src) -> bytes written (>=0) or a JFS_ERR_* code.
 * dst_cap is len(dst) for LZ4/none and cap(dst) for Zstd (DataDog/zstd writes
 * into dst[:cap]; compress.go:83-89).  LZ4 output is byte-identical to
 * LZ4_compress_default; a dst smaller than the compressed size fails
 * (JFS_ERR_COMPRESS_FAIL), like lz4.CompressDefault returning 0.  Zstd: one
 * RFC 8878 frame (FCS present, no checksum), never larger than
 * CompressBound; dst_cap < CompressBound(n) -> JFS_ERR_SHORT_BUFFER, the
 * "buffer too short" of compress.go:86-89. */
int64_t jfs_compress(int algo, uint8_t *dst, int64_t dst_cap, const uint8_t *src, int64_t n);

/* Decompress(dst, src) -> bytes written (>=0) or <0.
 * LZ4: empty src -> JFS_ERR_EMPTY_INPUT (compress.go:121-123); otherwise the
 * exact LZ4_decompress_safe(src, dst, n, dst_cap) result.
 * Zstd: empty src -> JFS_ERR_EMPTY_INPUT; frame(s) larger than dst_cap ->
 * JFS_ERR_SHORT_BUFFER (compress.go:99-101); malformed -> JFS_ERR_CORRUPT. */
int64_t jfs_decompress(int algo, uint8_t *dst, int64_t dst_cap, const uint8_t *src, int64_t n);

/* ---- Batch surface (host buffers; FillCache / compaction / aggregator) ----
 * Blocks are independent; they are dealt round-robin over the devices in
 * device_mask (bit d = device d; 0 = all visible devices) and staged through
 * pinned host memory with async copies.  out_n[i] receives what the
 * single-block call would have returned for block i.  Errors are per block: a
 * batch that fails as a whole (staging allocation, copy or launch failure) is
 * re-run block by block, so only the blocks that fail on their own report
 * JFS_ERR_NO_MEMORY / JFS_ERR_HIP.  Returns JFS_OK, or JFS_ERR_INVALID /
 * JFS_ERR_NO_DEVICE for a call that cannot run at all.  The calling thread's
 * current HIP device is unchanged on return. */
typedef struct jfs_iov {
    const uint8_t *src;
    int64_t src_len;
    uint8_t *dst;
    int64_t dst_cap;
} jfs_iov;

int64_t jfs_compress_batch(int algo, int nblk, const jfs_iov *iov, int64_t *out_n, uint32_t device_mask);
/* jfs_compress_batch plus crc[i] = crc32.Update(0, crc32c, dst[0:out_n[i]]) -- the
 * object checksum generateChecksum attaches to the PUT (pkg/object/checksum.go:
 * 30-45) -- computed on the GPU over the compressed payload before it leaves
 * HBM (0 for a block that failed).  For "none" the payload is the block itself. */
int64_t jfs_compress_batch_crc(int algo, int nblk, const jfs_iov *iov, int64_t *out_n, uint32_t *crc,
                               uint32_t device_mask);
int64_t jfs_decompress_batch(int algo, int nblk, const jfs_iov *iov, int64_t *out_n, uint32_t device_mask);
/* Mixed-codec batches (algo[i] per block: a chunk store reading objects written
 * under different codecs).  Each codec's blocks form
 * one jfs_{de,}compress_batch call; decode calls run at once, so the codecs
 * share every device's lanes instead of queueing behind one another (encode
 * calls run in turn: the encoders slow each other down).  Per-block
 * results as jfs_{de,}compress_batch (JFS_ERR_INVALID for an unknown algo[i]);
 * returns JFS_OK or the first failing codec call's whole-call error, which is
 * then also written to out_n[i] of every block of that codec. */
int64_t jfs_compress_batch_mixed(const int32_t *algo, int nblk, const jfs_iov *iov, int64_t *out_n,
                                 uint32_t device_mask);
int64_t jfs_decompress_batch_mixed(const int32_t *algo, int nblk, const jfs_iov *iov, int64_t *out_n,
                                   uint32_t device_mask);
/* jfs_decompress_batch plus, for each block with csum[i] != NULL, the disk-cache
 * checksum of the decoded block -- what cacheStore.add writes beside it
 * (pkg/chunk/disk_cache.go:536-537, checksum() of disk_cache_file.go:139-152):
 * the big-endian CRC-32C of every 32 KiB piece, ((n-1)/32768+1)*4 bytes for
 * n = out_n[i] decoded bytes (4 zero bytes for n = 0), computed on the GPU
 * before the block leaves HBM.  csum[i] must hold ((dst_cap-1)/32768+1)*4
 * bytes; nothing is written for a block that fails. */
int64_t jfs_decompress_batch_csum(int algo, int nblk, const jfs_iov *iov, int64_t *out_n, uint8_t *const *csum,
                                  uint32_t device_mask);
/* The batch calls' device dealing policy, exposed for
 * schedulers and tests: out_dev[i] in [0, ndev) for blocks of cost[i] (the
 * library uses src_len + dst_cap + 4096): longest-first greedy onto the least
 * loaded device, so no device ends more than one block above another. */
void jfs_deal_plan(const int64_t *cost, int n, int ndev, int32_t *out_dev);

/* ---- Encrypted objects (host buffers): compress + seal, open + decompress --
 * The PUT path of an encrypted volume is Compress (cached_store.go:372) and
 * then dataEncryptor.Encrypt (pkg/object/encrypt.go:226-257), which writes
 *     be16(len(wrapped)) | u8(len(nonce)) | wrapped key | nonce | sealed
 * with sealed = aead.Seal(nonce, compressed, nil) = ciphertext || 16-byte tag.
 * jfs_compress_seal_batch does both on the GPU per block: iov[i].src is the raw
 * block, iov[i].dst receives the whole envelope (dst_cap must be at least
 * jfs_envelope_bound), out_n[i] = envelope bytes or the codec's error.  The
 * random data key and nonce and the key wrap (RSA / SM2, keyEncryptor) are
 * the caller's: p[i] carries them.  algo may be JFS_ALGO_NONE (encryption
 * without compression).
 * The GET path is Decrypt (:259-284) then Decompress (:814):
 * jfs_open_decompress_batch takes the envelope in iov[i].src and the data key
 * the caller unwrapped from its header (jfs_envelope_parse) in keys[i], and
 * writes the block to iov[i].dst: out_n[i] = what jfs_decompress returns, or
 * JFS_ERR_AUTH when the tag does not verify, or JFS_ERR_CORRUPT for a
 * malformed header.  Errors are per block; the call returns JFS_OK,
 * JFS_ERR_INVALID or JFS_ERR_NO_DEVICE like the plain batch calls. */
typedef struct jfs_seal_param {
    const uint8_t *key;     /* data key, jfs_cipher_key_size(cipher) bytes */
    const uint8_t *nonce;   /* 12 bytes */
    const uint8_t *wrapped; /* keyEncryptor.Encrypt(key) (encrypt.go:234) */
    int32_t wrapped_len;    /* 0 .. 65535 */
    int32_t reserved;
} jfs_seal_param;

/* 3 + wrapped_len + 12 + CompressBound(n) (n for "none") + 16 */
int64_t jfs_envelope_bound(int algo, int64_t n, int32_t wrapped_len);
/* Decrypt's header checks (encrypt.go:260-267): returns the offset of the sealed
 * payload and the wrapped key / nonce positions, or JFS_ERR_CORRUPT when
 * n < 3 or 3 + wrapped_len + nonce_len >= n. */
int64_t jfs_envelope_parse(const uint8_t *src, int64_t n, int64_t *wrapped_off, int64_t *wrapped_len,
                           int64_t *nonce_off, int64_t *nonce_len);
/* crc (optional, may be NULL): per block the CRC-32C of the whole envelope
 * (generateChecksum of the PUT payload), computed on the GPU. */
int64_t jfs_compress_seal_batch(int algo, int cipher, int nblk, const jfs_iov *iov, const jfs_seal_param *p,
                                int64_t *out_n, uint32_t *crc, uint32_t device_mask);
int64_t jfs_open_decompress_batch(int algo, int cipher, int nblk, const jfs_iov *iov, const uint8_t *const *keys,
                                  int64_t *out_n, uint32_t device_mask);
/* jfs_open_decompress_batch plus the disk-cache checksum of every opened and
 * decoded block, with jfs_decompress_batch_csum's contract for csum (NULL with
 * nblk > 0: JFS_ERR_INVALID; csum[i] may be NULL; csum[i] must hold
 * ((dst_cap-1)/32768+1)*4 bytes; nothing is written for a block that fails, a
 * block whose tag does not verify included): the warm-up path
 * (pkg/vfs/fill.go:93) of an encrypted volume.  Everything else is
 * jfs_open_decompress_batch's. */
int64_t jfs_open_decompress_batch_csum(int algo, int cipher, int nblk, const jfs_iov *iov, const uint8_t *const *keys,
                                       int64_t *out_n, uint8_t *const *csum, uint32_t device_mask);

/* ---- Device-resident surface (inputs/outputs already in HBM) ------------
 * One descriptor per block; all pointers are device pointers on the calling
 * thread's current device, which must be a device this library selected
 * (gfx950, in JFS_GPU_DEVICES; else JFS_ERR_NO_DEVICE), and `stream`
 * (0 = the null stream) belongs to it.  ret[i] is written with the
 * single-block result -- exactly the value jfs_decompress/jfs_compress's
 * codec call would produce for that block (see each call below); no other
 * value is ever written.  The LZ4 calls only enqueue work on `stream`.
 * jfs_zstd_decompress_device enqueues too, but first waits on the host for
 * its header-scan kernels (microseconds after the work already on `stream`)
 * so it can size its scratch: it never asks the caller to resubmit.
 * jfs_zstd_compress_device is host-synchronous (per-device scratch, locked). */
typedef struct jfs_dev_block {
    const uint8_t *src;
    uint8_t *dst;
    int32_t src_len;
    int32_t dst_cap;
} jfs_dev_block;

/* ret[i] = LZ4_decompress_safe(src, dst, src_len, dst_cap): bytes written, or
 * its negative error value. */
int64_t jfs_lz4_decompress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream);
/* The same result for a FEW blocks at low latency (cachedStore.load decodes one
 * block per cache miss, pkg/chunk/cached_store.go:755-823): every block is
 * spread over the whole GPU instead of one workgroup.  src_len / dst_cap are
 * HOST copies of the descriptors' sizes (they size the launch without a device
 * round trip) and must match d_blocks.  Asynchronous on `stream`; per-device
 * scratch of about 4 bytes per dst_cap byte, reused across calls.  Best below
 * ~128-192 blocks of 4 MiB; jfs_lz4_decompress_device is faster for large batches. */
int64_t jfs_lz4_decompress_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len, const int32_t *dst_cap,
                                        int nblk, int32_t *d_ret, void *stream);
/* Prefix decode: block i is decoded only as far as its first d_want[i] bytes
 * (an LZ4_decompress_safe_partial-style stop; a 128 KiB read out of a 4 MiB
 * block need not pay for 4 MiB of decode).  d_want is a device array of nblk
 * int32.  For a stream let `size` be what jfs_lz4_decompress_device returns
 * for it and q the output position at which the first sequence it rejects
 * begins (q = infinity for a stream it accepts).
 *   Well-formed stream (size >= 0): ret = min(size, want), and dst[0, ret)
 *     equals the first ret bytes of the full decode.
 *   Rejected stream, want > q: ret = size, the same negative value; everything
 *     up to the faulty sequence was decoded identically with the same dst_cap.
 *   Rejected stream, want <= q: ret is either that negative value or want; if
 *     it is want, dst[0, want) holds the bytes the sequences in front of the
 *     fault define.  Which of the two is unspecified (the two paths cut at
 *     different granularity); a caller that needs the whole object validated
 *     uses the CRC-32C check or the full decoders.
 * Bytes of dst[ret, dst_cap) are unspecified; nothing outside dst[0, dst_cap)
 * is ever written; the small-batch call, for a block it decodes itself, writes
 * nothing at or above ret.  want <= 0 gives 0, after the early answers of the
 * full decoders (NULL src, src_len == 0, dst_cap == 0 keep their results);
 * want > dst_cap acts as dst_cap.  Asynchronous on `stream`.  The _small form
 * is jfs_lz4_decompress_device_small's (host copies of the sizes, the same
 * per-device scratch and its rules); jfs_lz4_split_counts counts its blocks. */
int64_t jfs_lz4_decompress_prefix_device(const jfs_dev_block *d_blocks, const int32_t *d_want, int nblk,
                                         int32_t *d_ret, void *stream);
int64_t jfs_lz4_decompress_prefix_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len,
                                               const int32_t *dst_cap, const int32_t *d_want, int nblk,
                                               int32_t *d_ret, void *stream);
/* Zstd prefix decode: input i is decoded only as far as the Zstd block that
 * reaches its first d_want[i] output bytes; the blocks behind it are neither
 * entropy-decoded nor replayed.  d_want is a device array of nblk int32.
 * Result codes, stream behaviour and scratch are jfs_zstd_decompress_device's.
 * Every stage walks the frame with a lower bound `lb` of the output so far
 * (exact for raw and RLE blocks, literals + 3 * sequences for a compressed
 * block) and stops in front of the next block header once lb >= want.  Let
 * `size` be the full decoder's result, S the block boundary at which that rule
 * stops (fixed by the input and want alone, the same on both paths) and B the
 * block that holds output byte want - 1 in the full decode.
 *   The walk ends before the rule fires (a frame whose last block has been
 *     walked ends with its content-size and checksum checks): ret is the full
 *     decoder's result, min(size, want) when size >= 0.
 *   The walk stops and no fault lies in front of S: ret = want and
 *     dst[0, want) is that prefix of the full decode.
 *   A fault in a block in front of B: the full decoder's negative value (the
 *     first error in stream order is the same one).
 *   A fault in a block from B up to S: that value or want (the replay may
 *     leave at want).
 *   A fault at or behind S -- a wrong content size or checksum, trailing
 *     garbage, output past dst_cap included -- is unseen: ret = want.
 * want > dst_cap acts as dst_cap; want <= 0 stops in front of the first block
 * and gives 0 unless the frame header itself is rejected.  Nothing outside
 * dst[0, dst_cap) is written, and nothing at or above the output end of the
 * last walked block; the small-batch path (jfs_zstd_split_counts counts these
 * inputs too), for an input it decodes itself, writes nothing at or above ret.
 * A highly compressible block has a tiny lb, so such frames are walked to
 * their end and only the result is cut. */
int64_t jfs_zstd_decompress_prefix_device(const jfs_dev_block *d_blocks, const int32_t *d_want, int nblk,
                                          int32_t *d_ret, void *stream);
/* Diagnostics for the small-batch path (used by it, by jfs_decompress and by
 * small jfs_decompress_batch calls), six counters: out[0] = blocks it decoded
 * itself, out[1] = blocks it handed to the one-workgroup kernel (inputs outside
 * its proven cases), and why: out[2] the token-chain fix-up did not converge
 * (e.g. literal runs spanning many segments), out[3] the byte-origin pointer
 * jumping did not converge, out[4] a token outside the proven acceptance
 * conditions (malformed or edge-of-buffer), out[5] no final literal run; on
 * the current device since the last reset.  Synchronous; 0 on success. */
int jfs_lz4_split_counts(uint64_t *out, int reset);
/* ret[i] = LZ4_compress_default(src, dst, src_len, dst_cap): compressed size,
 * or 0 when it does not fit dst_cap. */
int64_t jfs_lz4_compress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream);
/* The same bytes as jfs_lz4_compress_device for few blocks (one-call
 * Compress under cachedStore.upload, pkg/chunk/cached_store.go:372): every
 * block is cut into segments that are parsed at once and re-parsed, each from
 * the state the segment before it stopped in, until nothing changes (then the
 * result is the serial parse, byte for byte); blocks that do not settle take
 * the serial kernel.  src_len = HOST copies of the descriptors' src_len.
 * Asynchronous on `stream`; per-device scratch of about 4 bytes per input
 * byte, reused across calls.  jfs_compress / small jfs_compress_batch calls use
 * it below JFS_LZ4E_SEG_MAX blocks (default 256). */
int64_t jfs_lz4_compress_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len, int nblk, int32_t *d_ret,
                                      void *stream);
/* Fast LZ4 encode (throughput mode): ret[i] = size of a valid LZ4 block that
 * LZ4_decompress_safe decodes back to src, or 0 when it does not fit dst_cap
 * or src_len > 0x7E000000 (no byte of that dst is written).  NOT liblz4's
 * bytes: every block is cut into independent 64 KiB chunks that are parsed
 * 64 positions at a time, so no parse chain is longer than a chunk.  The bytes
 * depend on the input bytes alone (not on the batch, the block's index, the
 * device or alignment); the size never exceeds jfs_compress_bound(LZ4, n);
 * src_len == 0 gives the single byte 0x00.  src_len = HOST copies of the
 * descriptors' src_len.  Asynchronous on `stream`; per-device scratch of at
 * most 1 GiB (2 bytes per input byte below that), reused across calls.  Does
 * not consult jfs_lz4_parse_mode. */
int64_t jfs_lz4_compress_fast_device(const jfs_dev_block *d_blocks, const int32_t *src_len, int nblk, int32_t *d_ret,
                                     void *stream);
/* jfs_lz4_compress_fast_device with LIFTED chunks (compaction; juicefs_amd/csrc/
 * lz4_lift.h has the rule).  The blocks of d_blocks were gathered from decoded
 * sources; d_lift[g], one per 64 KiB chunk of the blocks in order (block after
 * block, ceil(src_len / 65536) each, 1 for an empty block, none for a block over
 * 0x7E000000 bytes), names the source chunk whose bytes chunk g is: bytes
 * [src_chunk * 65536, (src_chunk + 1) * 65536) of source `src`.  That is the
 * caller's statement and is not checked.  The sequence records of such a chunk
 * are read back from the source's stored LZ4 stream instead of being parsed
 * again, where the device finds that they are what the parse would leave; every
 * other chunk -- src < 0, src >= nsrc, src_chunk < 0 or past the source's end, a
 * source that failed, a chunk whose stream the rule refuses -- is parsed as
 * without this call, never a fault.  For a source the fast encoder wrote the
 * bytes and d_ret EQUAL jfs_lz4_compress_fast_device's on the same blocks; for
 * any other source they are a valid LZ4 block of the same content.
 * d_src[i]: src / src_len = source i's stored stream, dst_cap = its decode
 * capacity (dst is not read); d_src_n[i] = what it decoded to, as a decoder's
 * d_ret wrote it; src_src_len / src_cap = HOST copies of d_src's src_len and
 * dst_cap (they size the scratch: some 44 bytes per 256 stored bytes beside the
 * fast encoder's).  d_lifted (may be NULL): chunks lifted per block.
 * JFS_ERR_INVALID for a NULL array with a positive count. */
typedef struct jfs_lz4_lift {
    int32_t src;       /* < 0: parse */
    int32_t src_chunk;
} jfs_lz4_lift;
int64_t jfs_lz4_compress_fast_lift_device(const jfs_dev_block *d_blocks, const int32_t *src_len, int nblk,
                                          const jfs_lz4_lift *d_lift, const jfs_dev_block *d_src,
                                          const int32_t *d_src_n, const int32_t *src_src_len, const int32_t *src_cap,
                                          int nsrc, int32_t *d_ret, int32_t *d_lifted, void *stream);
/* Diagnostics of the segment encoder: out[r] (r = 1..16) = blocks whose
 * segments settled after r rounds, out[0] = blocks handed to the serial kernel
 * (not settled within JFS_LZ4E_SEG_ROUNDS, default 8, or a segment with too
 * many sequences); on the current device since the last reset.  Synchronous. */
int jfs_lz4_eseg_counts(uint64_t *out, int reset);
/* ret[i]: decoded bytes, -1 malformed frame (ZSTD error), -2 output larger
 * than dst_cap ("Destination buffer is too small"), -3 src size incorrect
 * (truncated / trailing bytes). */
int64_t jfs_zstd_decompress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream);
/* Batches of at most JFS_ZSTD_SPLIT_MAX inputs (default 128; also the batch
 * ABI's staged chunks and jfs_decompress) decode one workgroup per Zstd block
 * with an origin-map replay; an input outside that path's proven cases (no
 * frame or more frames than jfs_get_zstd_split_frames, a frame with a content
 * checksum, any error) is replayed by the exact one-wave kernel -- same
 * results either way.  Diagnostics: out[0] = inputs the
 * small-batch path replayed itself, out[1] = inputs it handed over; on the
 * current device since the last reset.  Synchronous; 0 on success. */
int jfs_zstd_split_counts(uint64_t *out, int reset);
/* The most frames an input may hold for the small-batch path to replay it
 * itself: concatenated frames from any writer, seekable objects (one frame per
 * 128 KiB; no seek table is read or trusted), skippable frames anywhere.
 * Default JFS_ZSTD_SPLIT_FRAMES_MAX (the seek table's frame limit); 1 hands
 * every multi-frame input to the one-wave kernel, as before the limit existed.
 * The initial value is read once from JFS_ZSTD_SPLIT_FRAMES (a decimal in
 * [1, 16384]; anything else is the default).  Process-wide; a launch takes the
 * value of the moment it is enqueued.  jfs_set_zstd_split_frames returns the
 * previous value, or -1 for a value outside [1, 16384] (nothing changes). */
#define JFS_ZSTD_SPLIT_FRAMES_MAX 16384
int jfs_get_zstd_split_frames(void);
int jfs_set_zstd_split_frames(int max_frames);
/* Of jfs_zstd_split_counts' out[0]: out[0] = the inputs of two frames or more,
 * out[1] = the frames they held; on the current device since the last reset.
 * Synchronous; 0 on success. */
int jfs_zstd_split_frame_counts(uint64_t out[2], int reset);
/* Zstd frame per block; ret[i] = frame size, or -2 when dst_cap < CompressBound(src_len).
 * Synchronous with respect to `stream` (it uses per-device scratch). */
int64_t jfs_zstd_compress_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream);
/* Fast Zstd encode (throughput mode), the contract of jfs_zstd_compress_device:
 * ret[i] = size of a valid RFC 8878 frame (one frame, content size present, no
 * checksum) that ZSTD_decompress decodes back to src, or -2 when dst_cap <
 * CompressBound(src_len) (no byte of that dst is written).  NOT libzstd's
 * bytes: every 128 KiB block is cut into independent 64 KiB chunks that are
 * parsed 64 positions at a time, and repeat-offset codes never reach outside
 * their block, so no parse chain is longer than a chunk and nothing is parsed
 * twice.  The bytes depend on the input bytes alone (not on the batch, the
 * frame's index, the device or alignment); the size never exceeds
 * jfs_compress_bound(ZSTD, n); src_len == 0 gives the exact encoder's frame.
 * Synchronous with respect to `stream` (it uses per-device scratch).  Does not
 * consult jfs_zstd_parse_mode. */
int64_t jfs_zstd_compress_fast_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream);
/* Seekable Zstd encode: jfs_zstd_compress_fast_device's parse, contract and
 * calling rules (host-synchronous, per-device scratch, -2 with no byte written
 * when dst_cap < CompressBound(src_len), bytes that depend on the input bytes
 * alone, never larger than jfs_compress_bound(ZSTD, n)) in a layout that can be
 * decoded from the middle.  src_len <= 131072 gives the fast call's frame, byte
 * for byte.  A longer input becomes nb = ceil(src_len / 131072) frames and a
 * seek table.  Frame k holds bytes [131072 k, min(n, 131072 (k + 1))): header
 * as for an input of that length (single segment, content size, no checksum,
 * no dictionary), then one block with its last-block bit set, which carries no
 * Huffman table over from the frame before and is never an RLE block.  The table is one skippable frame
 * in the Zstandard seekable format, all fields little-endian:
 *     u32 0x184D2A5E | u32 8 nb + 9 | nb x (u32 compressed size of the frame,
 *     u32 decompressed size) | u32 nb | u8 0x00 | u32 0x8F92EAB1
 * To every Zstd reader -- ZSTD_decompress, jfs_decompress, the reference's
 * ZStandard.Decompress -- the object is concatenated frames and a frame to
 * skip.  Does not consult jfs_zstd_parse_mode. */
int64_t jfs_zstd_compress_seekable_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream);
/* Range decode: input i is decoded for its output bytes [d_lo[i], d_hi[i])
 * (device arrays of nblk int32).  The seek table is read on the device and only
 * the frames the range touches are decoded, each as an independent input of
 * jfs_zstd_decompress_prefix_device; result codes, stream behaviour (one wait
 * on the host, for the number of selected frames, in front of that call's own)
 * and scratch are that call's.  Let lo' = max(lo, 0), hi' = min(hi, dst_cap).
 *   NULL src, src_len == 0, dst_cap == 0: the full decoder's answers.
 *   Otherwise hi' <= lo': 0, nothing written.
 *   A valid table (src_len >= 25; the footer magic; descriptor byte 0x00, so no
 *     per-frame checksums and no reserved bit; 1 <= nf <= 16384 frames, the most
 *     the encoder writes, with 8 nf + 17 <= src_len; the skippable magic and
 *     the size 8 nf + 9 at src_len - (8 nf + 17); compressed sizes all >= 1 that add up to exactly that position;
 *     decompressed sizes that add up to D < 2^32): D > dst_cap gives -2.  Else
 *     the frames whose output range [D_k, D_k+1) meets [lo', hi') are decoded,
 *     each into dst[D_k, D_k+1) with that size as its capacity; ret = min(D,
 *     hi') when every one of them returns exactly its table size, else -1.
 *     dst[flo, fhi) -- from the first selected frame's start to the last one's
 *     end -- equals the full decode's bytes, and nothing outside it is written.
 *     A fault in a frame that was not selected, or a table entry that lies
 *     about such a frame, is unseen: a caller that needs the whole object
 *     validated uses the CRC-32C check or the full decoders.
 *   Anything else -- every Zstd object written without a table, a table with
 *     checksums -- is no error: the input is decoded by
 *     jfs_zstd_decompress_prefix_device with want = hi, same result, same bytes. */
int64_t jfs_zstd_decompress_range_device(const jfs_dev_block *d_blocks, const int32_t *d_lo, const int32_t *d_hi,
                                         int nblk, int32_t *d_ret, void *stream);

/* XXH64 of device-resident pieces (the per-frame checksum of the Zstandard
 * seekable format is its low 32 bits).
 * d_hash[i] = XXH64(src[0, src_len), seed 0).  src_len == 0 gives
 * 0xEF46DB3751D8E999 (src may be NULL).  d_ret (may be NULL): 0, or -1 for a bad
 * descriptor (src_len < 0, NULL src with src_len > 0; d_hash[i] is then 0).
 * dst / dst_cap are ignored.  Reads no byte outside src[0, src_len); src may
 * have any alignment.  Asynchronous on `stream`. */
int64_t jfs_xxh64_device(const jfs_dev_block *d_blocks, int nblk, uint64_t *d_hash, int32_t *d_ret, void *stream);

/* Checksummed seekable Zstd encode: the contract and calling rules of
 * jfs_zstd_compress_seekable_device.  src_len <= 131072 gives that call's
 * bytes, with no table (one frame needs no seek, and the object CRC covers
 * it).  A longer input gives the same nb frames, byte for byte, and then the
 * table with per-frame checksums of the Zstandard seekable format:
 *     u32 0x184D2A5E | u32 12 nb + 9 | nb x (u32 compressed size of the frame,
 *     u32 decompressed size, u32 low 32 bits of XXH64 (seed 0) of the frame's
 *     content) | u32 nb | u8 0x80 | u32 0x8F92EAB1
 * so ret is the seekable call's ret + 4 nb, exactly; the worst case n + 25 nb
 * + 17 stays within jfs_compress_bound(ZSTD, n).  jfs_zstd_decompress_range_device
 * and the JFS_READ_SEEK_ON reads take such a table for no table and decode the
 * object as any other; jfs_zstd_decompress_frames_device,
 * jfs_zstd_decompress_ranges_device and the JFS_READ_SEEK_SPARSE reads read it.  Does not
 * consult jfs_zstd_parse_mode or jfs_zstd_seek_csum_mode. */
int64_t jfs_zstd_compress_seekable_csum_device(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *stream);

/* Planning a ranged GET of a seekable object (host only; needs no device).
 * tail = the last tail_len bytes of an object of object_len bytes (object_len
 * <= 0x7FFFFFFF); [lo, hi) = the content range wanted.  A valid table is the
 * one jfs_zstd_decompress_range_device describes, with descriptor byte 0x00
 * (entries of 8 bytes) or 0x80 (entries of 12 bytes, the third word a
 * checksum), read as a table that stands alone: its bytes run from the
 * skippable magic through the footer.  The 9-byte footer is enough to answer
 * JFS_SEEK_PLAN_MORE with the table's position; a footer that is not one, or a
 * table that fails any check, answers JFS_SEEK_PLAN_NONE.  The selection is the
 * range call's with lo' = max(lo, 0) and hi' = min(hi, D).  Returns JFS_OK and
 * fills *out, or JFS_ERR_INVALID (NULL, negative sizes, tail_len > object_len,
 * object_len > 0x7FFFFFFF). */
#define JFS_SEEK_PLAN_OK 0   /* fetch [get_off, get_off + get_len) of the object */
#define JFS_SEEK_PLAN_MORE 1 /* the table is longer than `tail`: fetch [table_off, table_off + table_len) and call again */
#define JFS_SEEK_PLAN_NONE 2 /* no valid table: fetch the whole object, use the ordinary calls */
typedef struct jfs_seek_plan {
    int32_t status, checksums;    /* checksums: 1 for a 12-byte table */
    int32_t nf, first, count;     /* frames; the selected ones (count 0: the range meets none, get_len 0) */
    int32_t reserved;
    int64_t table_off, table_len; /* where the table lies in the object */
    int64_t get_off, get_len;     /* the selected frames' bytes */
    int64_t content;              /* D */
    int64_t first_off;            /* content offset of frame `first` */
} jfs_seek_plan;
int64_t jfs_zstd_seek_plan(const uint8_t *tail, int64_t tail_len, int64_t object_len, int64_t lo, int64_t hi,
                           jfs_seek_plan *out);

/* Decoding a fragment of a seekable object, verified: input i holds the
 * object's table and the bytes [frag_off, frag_off + frag_len) of the object
 * (what jfs_zstd_seek_plan says to fetch), and is decoded for its content bytes
 * [d_lo[i], d_hi[i]).  Let lo' = max(lo, 0), hi' = min(hi, dst_cap).  ret[i],
 * in this order of precedence:
 *   NULL table, frag or dst, or a negative size: -1.
 *   The table is not valid (as for jfs_zstd_seek_plan; there is no whole object
 *     to fall back on): -1.
 *   dst_cap == 0 or hi' <= lo': 0, nothing written.
 *   D > dst_cap: -2.
 *   A selected frame whose bytes do not lie inside the fragment: -3.
 *   Otherwise the selected frames are decoded exactly as
 *     jfs_zstd_decompress_range_device decodes them, each into dst[D_k, D_k+1).
 *     A frame that does not return its table size: -1.  Else, with a 12-byte
 *     table, a frame whose content's XXH64 low word differs from its entry: -4
 *     (only this call returns it).  Else min(D, hi').
 * Nothing outside dst[flo, fhi) is written.  With frag the whole object,
 * frag_off = 0 and table pointing into it, this is the verified range decode of
 * a resident object.  Stream behaviour and scratch are the range call's (one
 * host wait for the number of selected frames; the per-device lock is held
 * across the waits). */
typedef struct jfs_seek_frag {
    const uint8_t *table; int32_t table_len; int32_t object_len; /* the stand-alone table, device memory */
    const uint8_t *frag;  int32_t frag_off;  int32_t frag_len;   /* bytes [frag_off, frag_off + frag_len) of the object */
    uint8_t *dst;         int32_t dst_cap;   int32_t reserved;   /* dst[k] = content byte k, as for the range call */
} jfs_seek_frag;
int64_t jfs_zstd_decompress_frames_device(const jfs_seek_frag *d_frags, const int32_t *d_lo, const int32_t *d_hi,
                                          int nblk, int32_t *d_ret, void *stream);

/* Ranges decode: input i, a whole object, is decoded for the list of byte
 * ranges d_rng[d_rng_first[i] .. d_rng_first[i+1]) of its output (device arrays:
 * nblk + 1 int32, and that many jfs_range).  The seek table is read on the
 * device in either layout -- descriptor byte 0x00 (8-byte entries) or 0x80
 * (12-byte entries, the third word a checksum); any other descriptor is no
 * table -- and exactly the frames some range touches are decoded, each as an
 * independent input of jfs_zstd_decompress_prefix_device.  Let lo'_r = max(lo_r,
 * 0), hi'_r = min(hi_r, dst_cap); a range is live when hi'_r > lo'_r; H = the
 * largest hi'_r of the live ranges.  Frame k, content [D_k, D_k + d_k), is
 * selected iff d_k > 0 and some live range has lo'_r < D_k + d_k and hi'_r >
 * D_k.  ret[i], in this order of precedence:
 *   NULL src, src_len == 0, dst_cap == 0: the full decoder's answers.
 *   A bad list -- d_rng_first[i] < 0, d_rng_first[i+1] < d_rng_first[i], a range
 *     with hi < lo, two ranges out of order or overlapping (the list must be
 *     ascending and disjoint as given, lo_r <= hi_r <= lo_r+1; empty ranges may
 *     stand anywhere): -1, nothing written.
 *   No live range: 0, nothing written.
 *   A valid table (the conditions of jfs_zstd_decompress_range_device, with
 *     entries of 8 or 12 bytes; compressed sizes all >= 1 that add up to exactly
 *     the table's position; D < 2^32): D > dst_cap gives -2.  Else every
 *     selected frame is decoded into dst[D_k, D_k + d_k) with d_k as its
 *     capacity and its want.  A selected frame that does not return exactly
 *     d_k: -1.  Else, with a 12-byte table, a selected frame whose content's
 *     XXH64 (seed 0) low word differs from its entry: -4.  Else min(D, H).  The
 *     bytes of every selected frame equal the full decode's, and no byte of dst
 *     outside the selected frames' spans is written: the frames between two
 *     ranges are neither decoded nor touched.  A fault in a frame that was not
 *     selected, or a table entry that lies about such a frame, is unseen.
 *   Anything else (no valid table) is no error: the input is decoded by
 *     jfs_zstd_decompress_prefix_device with want = H.
 * With exactly one range per input, ret and the written bytes are
 * jfs_zstd_decompress_range_device's for 8-byte tables and for objects without
 * a table.  Stream behaviour and scratch are the range call's (one host wait
 * for the number of selected frames; the per-device scratch and lock are shared
 * with it). */
typedef struct jfs_range { int32_t lo, hi; } jfs_range;
int64_t jfs_zstd_decompress_ranges_device(const jfs_dev_block *d_blocks, const int32_t *d_rng_first,
                                          const jfs_range *d_rng, int nblk, int32_t *d_ret, void *stream);
/* Diagnostics of that call and of the reads in JFS_READ_SEEK_SPARSE: out[0] =
 * inputs decoded through a table, out[1] = frames selected, out[2] = frames
 * whose checksum was compared; on the current device since the last reset;
 * synchronous.  0, or -1. */
int jfs_zstd_sparse_counts(uint64_t out[3], int reset);

/* LZ4 ranges decode by ORIGIN CHASE: block i is decoded for the list of byte
 * ranges d_rng[d_rng_first[i] .. d_rng_first[i+1]) of its output and nothing
 * else.  A raw LZ4 block has no seek table and needs none: the token chain is
 * walked once over the compressed bytes (the small-batch decoder's index: per
 * 256 compressed bytes, the first token and the output offset there), then
 * every requested byte is resolved on its own -- its sequence is found through
 * the index; a literal is copied from src; a match byte steps to the byte it
 * copies, and so on down to a literal.  Work is (compressed bytes, once) +
 * (requested bytes x chain depth) instead of (output bytes up to the last one
 * requested); it works on every LZ4 block already stored.
 * src_len / dst_cap are HOST copies of the descriptors' sizes, as for the
 * _small calls (a block whose device descriptor asks for more is handed over,
 * see below); d_rng_first (nblk + 1 int32) and d_rng are device arrays, as for
 * jfs_zstd_decompress_ranges_device, and so are the list's rules: lo'_r =
 * max(lo_r, 0), hi'_r = min(hi_r, dst_cap); a range is live when hi'_r > lo'_r;
 * H = the largest hi'_r of the live ranges.  Let `size` be what
 * jfs_lz4_decompress_device returns for the block.  ret[i], in this order:
 *   NULL src, src_len == 0, dst_cap == 0: the full decoder's answers.
 *   A bad list (d_rng_first[i] < 0, d_rng_first[i+1] < d_rng_first[i], a range
 *     with hi < lo, two ranges out of order or overlapping; empty ranges may
 *     stand anywhere in an ascending list): -1, nothing written.
 *   No live range: 0, nothing written.
 *   Well-formed stream (size >= 0): ret = min(size, H), and every byte of every
 *     live range below size equals the full decode's.  A block the chase
 *     resolves itself has no byte of dst outside its live ranges written.
 *   A block the chase does not cover -- a chain deeper than 2,048 steps, a
 *     visited token at the edge of the acceptance conditions, a token chain
 *     whose fix-up did not settle, a block over the host's sizes -- is handed,
 *     on the device, to jfs_lz4_decompress_prefix_device with want = H: ret and
 *     bytes are that call's, so dst[0, ret) may be written.
 *   A fault in a sequence no requested byte visits is UNSEEN, as the sparse
 *     Zstd call leaves unselected frames unseen; a caller that needs the whole
 *     object validated uses the CRC-32C check or the full decoders.
 *   Rejected stream (size < 0): ret is that negative value, or min(total, H)
 *     with the bytes the visited sequences define (total = the output the token
 *     chain adds up to) -- the latitude the prefix call documents.
 * Nothing outside dst[0, dst_cap) is ever written.  Asynchronous on `stream`,
 * no host wait; the per-device scratch (some 44 bytes per 256 compressed
 * bytes: no origin area, so no limit on the batch) and its lock are shared with
 * the _small calls.  The requested positions are spread over the GPU one quad
 * per thread; a thread finds its range by walking its block's list, so lists
 * of a few ranges per block are what the call is built for. */
int64_t jfs_lz4_decompress_ranges_device(const jfs_dev_block *d_blocks, const int32_t *src_len, const int32_t *dst_cap,
                                         const int32_t *d_rng_first, const jfs_range *d_rng, int nblk, int32_t *d_ret,
                                         void *stream);
/* Diagnostics of that call and of the reads in JFS_READ_LZ4_CHASE_ON: out[0] =
 * blocks resolved by the chase, out[1] = bytes requested of them, out[2] =
 * chain steps taken, out[3] = blocks handed to the prefix path; on the current
 * device since the last reset; synchronous.  0, or -1. */
int jfs_lz4_chase_counts(uint64_t out[4], int reset);

/* LZ4 WINDOW decode: block i is decoded for its output bytes [d_lo[i], d_hi[i])
 * from the 64 KiB chunk boundary below d_lo[i] instead of from byte 0.  Blocks
 * written by the fast parse (JFS_LZ4_PARSE_FAST) are cut into independent
 * 64 KiB chunks: no match reaches before its chunk's first byte.  Nothing in
 * the stored bytes says which encoder wrote them, so the call checks the
 * property on the device, for the sequences the window visits, and a block
 * that lacks it is decoded from byte 0 as by the prefix call -- it works on
 * every LZ4 block already stored.  The token chain is walked once over the
 * compressed bytes (the small-batch decoder's index), as for the prefix call;
 * what the window saves is the replay of the output in front of it.
 * src_len / dst_cap are HOST copies of the descriptors' sizes, as for the other
 * _small calls; d_lo and d_hi are device arrays of nblk int32.  Let lo' =
 * max(lo, 0), hi' = min(hi, dst_cap), Fc = lo' rounded down to 64 KiB, `size`
 * what jfs_lz4_decompress_device returns for the block, and F the block's
 * FLOOR: Fc where no visited sequence has a match byte at or above Fc that
 * copies from below Fc, else 0.  ret[i], in this order:
 *   NULL src, src_len == 0, dst_cap == 0: the full decoder's answers.
 *   hi' <= lo': 0, nothing written.
 *   Well-formed stream (size >= 0): ret = min(size, hi'), and dst[F, ret)
 *     equals the full decode's bytes.  For a block the path decodes itself no
 *     byte of dst outside [F, ret) is written.
 *   A fault in a sequence wholly in front of F is UNSEEN, as the sparse Zstd
 *     call leaves unselected frames unseen and the chase the sequences no
 *     requested byte visits; a caller that needs the whole object validated
 *     uses the CRC-32C check or the full decoders.
 *   A fault in a visited sequence, at or above F, and every block outside the
 *     small-batch decoder's proven cases (a token at the edge of the acceptance
 *     conditions, a fix-up or jump that did not settle, a block over the host's
 *     sizes): the block is handed, on the device, to
 *     jfs_lz4_decompress_prefix_device with want = hi; ret and bytes are that
 *     call's, with the latitude it documents, so dst[0, ret) may be written.
 * Nothing outside dst[0, dst_cap) is ever written.  Asynchronous on `stream`,
 * no host wait; scratch, its lock and the batch sizes it suits are
 * jfs_lz4_decompress_device_small's, and jfs_lz4_split_counts counts its
 * blocks too. */
int64_t jfs_lz4_decompress_window_device_small(const jfs_dev_block *d_blocks, const int32_t *src_len,
                                               const int32_t *dst_cap, const int32_t *d_lo, const int32_t *d_hi, int nblk,
                                               int32_t *d_ret, void *stream);
/* Diagnostics of that call and of the reads in JFS_READ_LZ4_WINDOW_ON: out[0] =
 * blocks decoded from a floor above 0, out[1] = blocks whose probe sent them to
 * floor 0, out[2] = blocks handed to the exact kernel, out[3] = origin entries
 * written (the bytes of [F, ret) of the blocks the path decoded itself); on the
 * current device since the last reset; synchronous.  0, or -1. */
int jfs_lz4_window_counts(uint64_t out[4], int reset);

/* The same from host buffers: what a loadRange adapter calls after
 * jfs_zstd_seek_plan and the ranged GET.  Read i holds the object's table and
 * the fragment [frag_off, frag_off + frag_len) of the object, and asks for the
 * content bytes [lo, hi).  Let lo' = max(lo, 0), hi' = min(hi, block_size).
 * out_n[i] = the bytes written to dst, min(D, hi') - lo' (0 when that is not
 * positive), which are content [lo', min(D, hi')); or JFS_ERR_CORRUPT (the
 * table is not valid, a frame does not decode to its table size, or a selected
 * frame lies outside the fragment: the device call's -1 and -3),
 * JFS_ERR_SHORT_BUFFER (D > block_size, the device call's -2; or dst_cap below
 * the bytes to write), JFS_ERR_CHECKSUM (-4).  Nothing is written to dst for a
 * failed read.  Only tables and fragments cross the link upwards (a table that
 * several reads share, by pointer and length, once) and only the requested
 * bytes come down; the decoded blocks of block_size bytes are device scratch.
 * Returns JFS_ERR_INVALID before anything else (n < 0, NULL arrays, a NULL
 * table, a NULL frag with frag_len > 0, a NULL dst with dst_cap > 0, a negative
 * size, or table_len, object_len, frag_off, frag_len or block_size beyond
 * int32), then JFS_ERR_NO_DEVICE, else JFS_OK with every out_n[i] set.  One
 * device of device_mask runs the call, the caller's current device is
 * unchanged on return, a read whose staging or scratch cannot be allocated
 * reports JFS_ERR_NO_MEMORY, a HIP failure JFS_ERR_HIP; jfs_stats counts the
 * call under (Zstd, decompress), bytes_in = table + fragment. */
typedef struct jfs_range_read {
    const uint8_t *table; int64_t table_len; int64_t object_len;
    const uint8_t *frag;  int64_t frag_off;  int64_t frag_len;
    int64_t lo, hi;       /* content range asked for */
    int64_t block_size;   /* capacity of the decoded block (device scratch; never crosses the link) */
    uint8_t *dst; int64_t dst_cap; /* receives content [lo', min(D, hi')); needs hi' - lo' bytes at most */
} jfs_range_read;
int64_t jfs_zstd_load_range_batch(int n, const jfs_range_read *r, int64_t *out_n, uint32_t device_mask);

/* CRC-32C (Castagnoli) of device-resident blocks.
 * d_blocks[i].src / src_len: the data.  d_crc[i] (if d_crc != NULL) receives
 * crc32.Update(0, crc32c, data), the object checksum of
 * pkg/object/checksum.go:30-45.  If seg_bytes > 0 (a multiple of 4096; JuiceFS
 * uses 32768), d_blocks[i].dst receives the disk-cache checksum layout of
 * pkg/chunk/disk_cache_file.go:139-152: the big-endian CRC-32C of every
 * seg_bytes piece, ((len-1)/seg_bytes+1)*4 bytes (4 zero bytes for len 0);
 * dst_cap must hold them.  d_ret[i] (if non-NULL) = bytes written to dst, or
 * -1 for a bad descriptor.  Asynchronous on `stream`. */
int64_t jfs_crc32c_device(const jfs_dev_block *d_blocks, int nblk, int32_t seg_bytes, uint32_t *d_crc,
                          int32_t *d_ret, void *stream);

/* AES-256-GCM of device-resident blocks: the AEAD of
 * pkg/object/encrypt.go dataEncryptor for AES256GCM_RSA (aes.NewCipher(key) +
 * cipher.NewGCM, :178-189): 32-byte key, 12-byte nonce, 16-byte tag, no
 * additional data.  Seal (Encrypt :226-257): dst = ciphertext || tag,
 * ret = src_len + 16 (dst_cap must hold it).  Open (Decrypt :259-284):
 * src = ciphertext || tag, dst = plaintext, ret = src_len - 16, or -1 when the
 * tag does not verify ("cipher: message authentication failed"; dst[0, n)
 * is then zeroed, as Go's gcm.Open clears its output).  ret = -2 for a bad descriptor.  The random key/nonce, the
 * RSA wrap of the key and the object header (:230-252) are the caller's.
 * Asynchronous on `stream`; key and nonce are device pointers. */
typedef struct jfs_aead_block {
    const uint8_t *src;
    uint8_t *dst;
    int32_t src_len;
    int32_t dst_cap;
    const uint8_t *key;   /* 32 bytes */
    const uint8_t *nonce; /* 12 bytes */
} jfs_aead_block;

int64_t jfs_aes256gcm_seal_device(const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream);
int64_t jfs_aes256gcm_open_device(const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream);

/* The three data ciphers of NewDataEncryptor (pkg/object/encrypt.go:176-202).
 * Same seal/open contract as above (ret, zeroed dst on a failed open, no
 * additional data); the key is jfs_cipher_key_size(cipher) bytes. */
#define JFS_CIPHER_AES256GCM 0        /* "aes256gcm-rsa" (and ""), encrypt.go:179-188: 32-byte key */
#define JFS_CIPHER_CHACHA20POLY1305 1 /* "chacha20-rsa", encrypt.go:190: 32-byte key (RFC 8439) */
#define JFS_CIPHER_SM4GCM 2           /* "sm4gcm", encrypt.go:192-201: 16-byte key (GB/T 32907 + GCM) */
/* NewDataEncryptor's names -> cipher id, or -1 ("unsupport cipher") */
int jfs_cipher_from_name(const char *name);
/* keyLen of dataEncryptor (32 / 32 / 16), or -1 */
int jfs_cipher_key_size(int cipher);
int64_t jfs_aead_seal_device(int cipher, const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream);
int64_t jfs_aead_open_device(int cipher, const jfs_aead_block *d_blocks, int nblk, int32_t *d_ret, void *stream);

/* Fused object paths (compression runs before encryption on PUT and after
 * decryption on GET, cmd/format.go:289-302, docs internals.md:920), chained on
 * `stream` with no host round trip: the second kernel reads each block's
 * length from the first kernel's results on the device.
 *   compress -> seal: d_comp[i] LZ4-compresses into an intermediate buffer
 *     (d_ret_comp[i] = LZ4 result); d_aead[i].src must be that buffer (its
 *     src_len is ignored) and is sealed into d_aead[i].dst; d_ret[i] = sealed
 *     bytes, or JFS_CHAIN_FAILED (INT32_MIN) when the compression failed.
 *   open -> decompress: d_aead[i] opens into an intermediate buffer
 *     (d_ret_open[i] = plaintext length or -1); d_dec[i].src must be that
 *     buffer (its src_len is ignored); d_ret[i] = the LZ4_decompress_safe
 *     result, or INT32_MIN when the tag did not verify. */
int64_t jfs_lz4_compress_seal_device(const jfs_dev_block *d_comp, const jfs_aead_block *d_aead, int nblk,
                                     int32_t *d_ret_comp, int32_t *d_ret, void *stream);
int64_t jfs_open_lz4_decompress_device(const jfs_aead_block *d_aead, const jfs_dev_block *d_dec, int nblk,
                                       int32_t *d_ret_open, int32_t *d_ret, void *stream);

/* ---- Slice compaction (pkg/vfs/compact.go:54-108) --------------------------
 * Compact reads byte ranges [s.Off, s.Off+s.Len) of N existing slices (zeros
 * for holes, s.Id == 0, :70-77), concatenates them, re-cuts the stream at
 * BlockSize and uploads each new block through Compress; on the read side
 * every touched block is decompressed whole (cached_store.go:177).  These
 * calls do decode -> gather -> re-encode without the decoded bytes leaving
 * HBM.  The plan: every output block is a run of segments that tile
 * [0, total) in order -- seg[k].dst_off == seg[k-1].dst_off + seg[k-1].len,
 * the first 0 (the caller fills dst_off, so the kernel needs no scan). */
typedef struct jfs_compact_seg {
    int32_t src;     /* index of the decoded source block, or -1: `len` zero bytes (a hole) */
    int32_t src_off; /* first byte inside the decoded source block (ignored for src = -1) */
    int32_t dst_off; /* where the bytes go inside the output block */
    int32_t len;     /* > 0 */
} jfs_compact_seg;

typedef struct jfs_compact_out {
    uint8_t *dst;      /* gathered (uncompressed) output block */
    int32_t dst_cap;
    int32_t seg_first; /* this block's segments are seg[seg_first .. seg_first+seg_count) */
    int32_t seg_count; /* 0 is legal: an empty block */
    int32_t reserved;
} jfs_compact_out;

/* The gather alone, device-resident.  d_src[i].dst / d_src_n[i]: decoded source
 * block i and its decoded length as a decoder's d_ret wrote it (negative = that
 * source failed; d_src[i].dst_cap bounds it too).  d_ret[j] = bytes gathered
 * into d_out[j].dst; JFS_CHAIN_FAILED (INT32_MIN) when a segment of block j
 * reads a failed source or reaches past d_src_n[src]; -1 for a bad plan (src
 * outside [-1, nsrc), negative offsets, len <= 0, broken tiling, total >
 * dst_cap; a bad plan wins over a failed source).  Nothing outside
 * dst[0, total) is ever written, and nothing at all for a block that is not
 * gathered.  max_dst_cap: a HOST value >= every d_out[j].dst_cap (it sizes the
 * launch).  Asynchronous on `stream`. */
int64_t jfs_gather_device(const jfs_dev_block *d_src, const int32_t *d_src_n, int nsrc, const jfs_compact_out *d_out,
                          int nout, const jfs_compact_seg *d_seg, int32_t max_dst_cap, int32_t *d_ret, void *stream);

/* decode d_src (LZ4 blocks) -> gather -> LZ4_compress_default of every gathered
 * block, chained on `stream` with no host round trip.  d_src_ret[i] = the
 * LZ4_decompress_safe result; d_gather[j].dst is the intermediate gathered
 * block; d_enc[j].src must be that buffer (its src_len must equal the block's
 * planned total), d_enc[j].dst receives the compressed block.  d_ret[j] =
 * compressed size, 0 when it does not fit, JFS_CHAIN_FAILED / -1 as
 * jfs_gather_device (the encoder may run on a block whose gather failed; its
 * result is replaced by the gather's verdict). */
int64_t jfs_lz4_compact_device(const jfs_dev_block *d_src, int nsrc, int32_t *d_src_ret,
                               const jfs_compact_out *d_gather, const jfs_compact_seg *d_seg,
                               const jfs_dev_block *d_enc, int nout, int32_t max_dst_cap, int32_t *d_ret,
                               void *stream);

/* Host buffers (what a Go Compact adapter calls).  src[i].src/src_len: stored
 * object i; src[i].dst_cap: its block size (src[i].dst is ignored: the decoded
 * block never reaches the host).  out[j].dst/dst_cap receives new stored
 * object j (out[j].src/src_len are ignored); its segments are
 * seg[seg_first[j] .. seg_first[j+1]) (seg_first has nout+1 entries).
 * src_n[i] = what jfs_decompress would have returned for source i; out_n[j] =
 * what jfs_compress would have returned for the gathered bytes of block j,
 * byte for byte (Zstd's dst_cap < CompressBound rule and LZ4's "does not fit"
 * included), or JFS_ERR_CORRUPT when a source feeding block j failed or is
 * shorter than a segment needs (this wins over the block's own codec error);
 * crc (may be NULL) as jfs_compress_batch_crc.  Errors are per block: blocks
 * that depend only on good sources succeed (the reference aborts the whole
 * compaction on any error, compact.go:83-88: that decision stays with the
 * caller), and a plan may hold several independent compactions.  algo: LZ4,
 * Zstd or none (decode is then a copy, the output the gathered bytes).
 * The plan is checked on the host first: bad indices, broken tiling, len <= 0,
 * a non-monotone seg_first, NULL pointers, negative sizes or sizes beyond
 * int32 return JFS_ERR_INVALID; then JFS_ERR_NO_DEVICE without a usable device.
 * One call runs on ONE device of device_mask (a compaction's sources and
 * outputs are coupled, so the call is not dealt across devices; concurrent
 * calls take turns over the devices).  Only compressed bytes cross the host
 * link, in both directions.  If the device scratch for the decoded sources
 * and gathered blocks cannot be allocated every src_n[i] and out_n[j] is
 * JFS_ERR_NO_MEMORY (JFS_ERR_HIP after a runtime failure); the call still
 * returns JFS_OK.  jfs_stats counts the sources under (algo, decompress) and
 * the outputs under (algo, compress).  The calling thread's current HIP
 * device is unchanged on return. */
int64_t jfs_compact_batch(int algo, int nsrc, const jfs_iov *src, int nout, const jfs_iov *out,
                          const int32_t *seg_first /* nout+1 */, const jfs_compact_seg *seg, int64_t *src_n,
                          int64_t *out_n, uint32_t *crc /* may be NULL */, uint32_t device_mask);

/* ---- Spliced compaction of seekable Zstd objects --------------
 * Assembling seekable objects from frames that already exist, device-resident.
 * Output j is frames d_frames[frame_first .. frame_first + frame_count), in
 * order, and then the seek table.  A PASS frame (unit < 0) is the c stored bytes
 * at src, copied; a FRESH frame (unit >= 0) is the first d_unit_len[unit] bytes
 * at src, the buffer encode unit `unit` was written to, so its length is read
 * on the device from the encoder's results.  d = the frame's content bytes and
 * x = its checksum word, which go to the table; for a FRESH frame x is ignored
 * and the low word of d_unit_hash[unit] is written (d_unit_hash == NULL: the
 * 8-byte layout, descriptor 0x00; else the 12-byte layout, descriptor 0x80).
 * `out` = the index j of the output that owns the frame.
 * d_ret[j], in this order of precedence:
 *   a bad record (NULL dst with frames, dst_cap < 0, frame_first < 0,
 *     frame_count outside 1 .. 16384, a frame whose `out` is not j, NULL src, d <
 *     0, a PASS frame with c outside 1 .. 2^24, a FRESH result above 2^24): -1;
 *   a FRESH unit whose result is JFS_CHAIN_FAILED (INT32_MIN: its gather
 *     failed): JFS_CHAIN_FAILED, as the gather's verdict replaces an encoder's;
 *   else a FRESH unit whose result is <= 0: that result, of the first such frame;
 *   the frames and the table take more than dst_cap: 0;
 *   else the object's size, sum of the frames' bytes + E frame_count + 17 with
 *     E = 8 or 12: dst[0, size) holds the frames back to back and the table
 *         u32 0x184D2A5E | u32 E nf + 9 | nf x (u32 c, u32 d[, u32 x]) | u32 nf
 *         | u8 0x00 or 0x80 | u32 0x8F92EAB1,   all little-endian.
 * No byte of dst is written for an output whose d_ret[j] <= 0, and none outside
 * dst[0, size) otherwise; no byte outside a frame's [src, src + length) is read.
 * src and dst may have any alignment.  nframes: a HOST value, the number of
 * records in d_frames (it sizes the launch); every record belongs to one
 * output.  `unit` indexes d_unit_len (and d_unit_hash) unchecked: their length
 * is the caller's.  Asynchronous on `stream` (per-device scratch of 4 bytes per frame,
 * ordered across streams by an event). */
typedef struct jfs_splice_frame {
    const uint8_t *src;
    int32_t c;    /* PASS: stored bytes of the frame */
    int32_t d;    /* content bytes */
    uint32_t x;   /* PASS: checksum word for a 12-byte table */
    int32_t unit; /* < 0: PASS; else FRESH, the index into d_unit_len / d_unit_hash */
    int32_t out;  /* the output this frame belongs to */
    int32_t reserved;
} jfs_splice_frame;
typedef struct jfs_splice_out {
    uint8_t *dst;
    int32_t dst_cap;
    int32_t frame_first, frame_count;
    int32_t reserved;
} jfs_splice_out;
int64_t jfs_zstd_splice_device(const jfs_splice_out *d_out, int nout, const jfs_splice_frame *d_frames, int nframes,
                               const int32_t *d_unit_len, const uint64_t *d_unit_hash /* NULL for the 8-byte layout */,
                               int32_t *d_ret, void *stream);

/* Seek tables out of device-resident objects, what the sealed
 * spliced compaction brings to the host of every opened source.  Input i is the
 * d_len[i] bytes at d_blocks[i].src (dst and dst_cap are ignored); d_len is read
 * on the device -- in the chain it is the AEAD open's result array, the
 * plaintext length, or negative when the tag fails.  d_slot_first (device, nblk
 * + 1 entries, bytes, ascending multiples of 16): input i's slot is d_tables[
 * d_slot_first[i], d_slot_first[i + 1]).
 * One wave per input reads the 9-byte footer at the input's end and checks: the
 * footer magic; the descriptor is 0x00 or 0x80 (E = 8 or 12); 1 <= nf <= 16384; T
 * = E nf + 17 <= d_len[i]; the skippable magic 0x184D2A5E and the size word E nf +
 * 9 stand at d_len[i] - T.  Nothing else: what the entries add up to is the
 * caller's to check on the copied bytes.  If all of it holds and T fits the
 * slot, the T bytes of the table go to the slot's start and d_table_len[i] = T;
 * otherwise d_table_len[i] = 0 and no byte of the slot is written -- also for
 * d_len[i] < 25 (negative included) and a NULL src.
 * No byte outside src[0, d_len[i]) is read and none outside the slot's first T
 * bytes is written.  src may have any alignment (an opened payload lies behind
 * an envelope header of 15 + wrapped_len bytes).  Asynchronous on `stream`. */
int64_t jfs_zstd_seek_tables_device(const jfs_dev_block *d_blocks, const int32_t *d_len, int nblk,
                                    const int32_t *d_slot_first /* nblk + 1, bytes, multiples of 16 */,
                                    uint8_t *d_tables, int32_t *d_table_len, void *stream);

/* Splice switch of jfs_compact_batch.  JFS_COMPACT_SPLICE_OFF (default): nothing
 * changes.  JFS_COMPACT_SPLICE_ON: a call with algo = Zstd, while the Zstd parse
 * mode is JFS_ZSTD_PARSE_SEEKABLE, cuts every output j with total > 131072 into
 * pieces [131072 f, min(131072 (f + 1), total)).  A piece passes when one
 * segment covers it whole, that segment's source has a valid seek table (as for
 * jfs_zstd_decompress_ranges_device, with D <= src[i].dst_cap), the piece is
 * exactly the content of one frame k of it (D_k == src_off + (lo - dst_off),
 * d_k == the piece's bytes > 0), c_k <= d_k + 21, and, with
 * JFS_ZSTD_SEEK_CSUM_ON, the source table has checksums too.  An output with at
 * least one such piece is spliced; a call without one is the switch off.
 *   Spliced out[j]: a Zstd object that ZSTD_decompress, jfs_decompress and every
 *     decoder here decode to the gathered bytes, with a valid seek table of the
 *     current layout (8-byte entries, or 12-byte ones with
 *     JFS_ZSTD_SEEK_CSUM_ON).  Its passing frames are the source's stored bytes
 *     (and table checksum word); every other frame is what
 *     jfs_zstd_compress_seekable_device returns for that piece alone.  out_n[j]
 *     is its size, never above jfs_compress_bound(ZSTD, total).
 *   dst_cap < CompressBound(total) is JFS_ERR_SHORT_BUFFER as before, and the
 *     error codes are today's: JFS_ERR_CORRUPT when a source that a re-encoded
 *     piece needs failed or is too short.
 *   A damaged passing frame is copied and NOT noticed: with the switch on,
 *     compaction does not validate bytes it does not decode.  A caller that
 *     needs every source validated checks the object CRC-32C or leaves the
 *     switch off.
 *   Unspliced out[j] of such a call: byte-identical to the switch off.
 *   src_n[i]: only the frames the re-encoded pieces and the unspliced outputs
 *     read are decoded (jfs_zstd_decompress_ranges_device over the merged
 *     ranges, every decoded frame checked against a 12-byte table).  For a
 *     source with a valid table src_n[i] = D, the table's content size, when
 *     every selected frame decoded and verified -- also for a source that is
 *     not decoded at all; else the mapped error, -4 being JFS_ERR_CHECKSUM as
 *     in the JFS_READ_SEEK_SPARSE reads.  For a source without a table it is
 *     what those reads report, min(size, need).
 *   crc, jfs_stats: as before.
 * JFS_COMPACT_SPLICE_ALL: JFS_COMPACT_SPLICE_ON for jfs_compact_batch, and
 * jfs_compact_seal_batch splices too (its own comment has that contract; the
 * tables are ciphertext on the host, so it opens the sources first and pays one
 * more host wait).  With OFF or ON jfs_compact_seal_batch does not consult the
 * switch; LZ4, "none" and the read calls never do.  The initial value is read
 * once from JFS_COMPACT_SPLICE = "off" | "on" | "all" (case-insensitive; anything
 * else, or unset: off).  jfs_set_compact_splice_mode returns the previous
 * value, or -1 for an unknown one (which changes nothing) -- ALL among them, as
 * callers built against two values rely on; jfs_set_compact_splice_mode_ext is
 * the same call for all three.  Both are atomic and apply to calls that start
 * afterwards. */
#define JFS_COMPACT_SPLICE_OFF 0
#define JFS_COMPACT_SPLICE_ON 1
#define JFS_COMPACT_SPLICE_ALL 2
int jfs_compact_splice_mode(void);
int jfs_set_compact_splice_mode(int mode);
int jfs_set_compact_splice_mode_ext(int mode);
/* The LZ4 lift switch of the compaction calls (jfs_compact_batch and
 * jfs_compact_seal_batch with algo = LZ4), a switch of its own: JFS_COMPACT_SPLICE
 * never changes what an LZ4 call does.  JFS_COMPACT_LZ4_LIFT_OFF (default):
 * nothing changes, every call is queued as before.  JFS_COMPACT_LZ4_LIFT_ON: where
 * the LZ4 parse mode is JFS_LZ4_PARSE_FAST and the plan has an output chunk that is
 * one whole 64 KiB chunk of one source (one segment covers it, chunk-aligned in
 * both, not within 12 bytes of either block's end), the encode step is
 * jfs_lz4_compress_fast_lift_device's: such chunks are not parsed again.  out_n,
 * the bytes, crc and src_n are the switch off's ONLY for sources the fast encoder
 * wrote.  For a source of any other encoder the device refuses most candidates
 * (its matches cross chunk boundaries) and parses them, at the cost of the index
 * of their streams; a chunk the rule does accept there -- typically chunk 0, when
 * no match straddles its end -- is emitted from the source's own sequences, so
 * the object is a valid LZ4 block of the same content whose bytes may differ
 * from the switch off's.  Measured: calls of a hundred blocks or more
 * on fast-parse volumes gain a few percent, smaller calls lose.  The initial value is read once from JFS_COMPACT_LZ4_LIFT =
 * "off" | "on" (case-insensitive; anything else, or unset: off).  The setter
 * returns the previous value, or -1 for an unknown one (which changes nothing). */
#define JFS_COMPACT_LZ4_LIFT_OFF 0
#define JFS_COMPACT_LZ4_LIFT_ON 1
int jfs_compact_lz4_lift_mode(void);
int jfs_set_compact_lz4_lift_mode(int mode);
/* Diagnostics of those calls since the last reset, process-wide: out[0] = calls
 * that took the lift, out[1] = candidate chunks planned, out[2] = chunks lifted,
 * out[3] = candidates the device refused and parsed.  0, or -1 (NULL). */
int jfs_compact_lz4_lift_counts(uint64_t out[4], int reset);
/* Diagnostics of the spliced calls since the last reset, process-wide: out[0] =
 * outputs spliced, out[1] = frames passed, out[2] = frames re-encoded inside
 * spliced outputs, out[3] = compressed bytes passed.  0, or -1 (NULL). */
int jfs_compact_splice_counts(uint64_t out[4], int reset);

/* jfs_compact_batch for a volume with object encryption: every stored object
 * is an envelope (see jfs_compress_seal_batch), so the chain is open -> decode
 * -> gather -> encode -> seal, on one device, and only sealed bytes cross the
 * host link.  The plan, the jfs_iov conventions, the per-block error policy,
 * the device choice, the stats and "current device unchanged on return" are
 * jfs_compact_batch's.
 *   src[i].src/src_len is the whole stored envelope, src_keys[i] the data key
 *   the caller unwrapped from its header (as for jfs_open_decompress_batch),
 *   src[i].dst_cap the block size.  src_n[i] = exactly what
 *   jfs_open_decompress_batch(algo, cipher, ..) returns for that envelope and
 *   key: JFS_ERR_CORRUPT for a header jfs_envelope_parse rejects, JFS_ERR_AUTH
 *   when the tag does not verify, else the codec's own result.
 *   out[j].dst/dst_cap receives the whole envelope of new block j, built from
 *   out_p[j] (data key, nonce, wrapped key).  out_n[j] = what
 *   jfs_compress_seal_batch(algo, cipher, ..) returns for the gathered bytes
 *   with the same out_p[j] and dst_cap, byte for byte (its answer to a dst_cap
 *   below jfs_envelope_bound and the current JFS_LZ4_PARSE / JFS_ZSTD_PARSE
 *   mode included), or JFS_ERR_CORRUPT when a source feeding block j failed
 *   (a source that does not authenticate is a failed source) or is shorter
 *   than a segment needs; this wins over the block's own error.  Nothing is
 *   written to out[j].dst for a failed block.  crc[j] (crc may be NULL) = the
 *   CRC-32C of the whole envelope, computed on the GPU; 0 for a failed block.
 * With JFS_COMPACT_SPLICE_ALL, algo = Zstd and the Zstd parse mode
 * JFS_ZSTD_PARSE_SEEKABLE, a call of which at least one output survives the
 * host checks splices as jfs_compact_batch does with JFS_COMPACT_SPLICE_ON (the
 * rule is stated there).  The sources are opened on the device, their seek tables alone
 * come to the host (jfs_zstd_seek_tables_device), the rule runs on those, and
 * the call waits once more than with the switch off.  A source's table counts
 * only if it fits 12 ceil(dst_cap / 131072) + 17 bytes rounded up to 16 -- what
 * the seekable encoder and this path write for a block of dst_cap bytes; a
 * longer one is "no table" here, where jfs_compact_batch accepts up to 16,384
 * frames.  If no piece passes, src_n, out_n, the bytes and crc are the switch
 * off's exactly.  Otherwise:
 *   Spliced out[j]: an envelope whose opened payload is byte-identical to what
 *     jfs_compact_batch writes with JFS_COMPACT_SPLICE_ON and the same Zstd
 *     switches for the same plan over the sources' plaintext payloads; its
 *     header is jfs_compress_seal_batch's for out_p[j], and out_n[j] is never
 *     above jfs_envelope_bound(ZSTD, total, wrapped_len).  Unspliced out[j]:
 *     byte-identical to the switch off.
 *   src_n[i], in this order: JFS_ERR_CORRUPT for a header jfs_envelope_parse
 *     rejects; JFS_ERR_AUTH for a tag that does not verify -- such a source has
 *     no table, passes no frame, and every output it feeds is JFS_ERR_CORRUPT as
 *     before; else the spliced jfs_compact_batch's rule: D for a valid table,
 *     else the mapped decoder result, -4 being JFS_ERR_CHECKSUM.
 *   Every passing frame comes from a payload whose tag verified, so "a damaged
 *     passing frame is copied and NOT noticed" shrinks to damage from before the
 *     source was sealed.
 *   An output's own errors (JFS_ERR_SHORT_BUFFER below the envelope bound,
 *     JFS_ERR_INVALID), "a failed source wins", crc and jfs_stats are unchanged;
 *     jfs_compact_splice_counts counts these calls as the plain ones.
 * A FRESH data key / nonce pair per output is the caller's duty, as on the PUT
 * path (encrypt.go:230-243): sealing two blocks under one key and nonce breaks
 * the AEAD; never reuse a source's.
 * Checked on the host first (JFS_ERR_INVALID): everything jfs_compact_batch
 * rejects, an unknown cipher, a NULL src_keys / out_p with nsrc / nout > 0, a
 * NULL src_keys[i], a NULL out_p[j].key or nonce, wrapped_len outside
 * 0..65535, wrapped NULL with wrapped_len > 0; then JFS_ERR_NO_DEVICE. */
int64_t jfs_compact_seal_batch(int algo, int cipher, int nsrc, const jfs_iov *src, const uint8_t *const *src_keys,
                               int nout, const jfs_iov *out, const jfs_seal_param *out_p,
                               const int32_t *seg_first /* nout+1 */, const jfs_compact_seg *seg, int64_t *src_n,
                               int64_t *out_n, uint32_t *crc /* may be NULL */, uint32_t device_mask);

/* ---- Read assembly (pkg/vfs/reader.go:813-879, pkg/object/checksum.go:55-85) --
 * dataReader.Read fills a page from byte ranges of stored slices (zeros for
 * s.Id == 0 and for the tail); on a compressed volume every range costs a whole
 * decoded block (cached_store.go:162-178).  These calls are the GET-side mirror
 * of the compaction calls: stored objects go up, are checked against their
 * CRC-32C, opened, decoded and gathered on the device, and only the requested
 * bytes come down.  The plan is compaction's (jfs_compact_seg, seg_first):
 * read j is the run of segments seg[seg_first[j] .. seg_first[j+1]), a hole is
 * src = -1 (the zero tail of a page is a hole segment), seg_count == 0 is an
 * empty read. */

/* The gather alone, device-resident: jfs_gather_device's contract (verdicts in
 * d_ret, nothing written outside dst[0, total) or for a read that is not
 * gathered) on a one-dimensional grid over the outputs' own tile counts, for
 * batches whose outputs differ widely in size.  dst_cap: a HOST copy of every
 * d_out[j].dst_cap (nout entries; it sizes the launch, a smaller value than the
 * device's leaves that output's tail unwritten).  Asynchronous on `stream`. */
int64_t jfs_read_gather_device(const jfs_dev_block *d_src, const int32_t *d_src_n, int nsrc, const jfs_compact_out *d_out,
                               const int32_t *dst_cap, int nout, const jfs_compact_seg *d_seg, int32_t *d_ret,
                               void *stream);

/* The disk-cache checksums of gathered reads, device-resident: behind
 * jfs_read_gather_device on the same stream, for every read j whose verdict
 * d_ret[j] is its d_out[j].dst_cap (> 0), the big-endian CRC-32C of every
 * 32 KiB piece of d_out[j].dst[0, dst_cap), one piece per workgroup on a
 * one-dimensional grid.  d_piece_first (device, nout + 1 entries) is the
 * running sum of the reads' piece counts, (dst_cap-1)/32768+1, or 0 for a read
 * that wants no checksum; npiece is its last entry, a HOST value (it sizes the
 * launch).  Piece p of the call writes d_csum[4p .. 4p+4) (d_csum 4-byte
 * aligned, 4 npiece bytes), so read j's checksum starts at
 * 4 d_piece_first[j]; nothing is written for any other read.  Asynchronous on
 * `stream`. */
int64_t jfs_read_csum_device(const jfs_compact_out *d_out, const int32_t *d_ret, int nout, const int32_t *d_piece_first,
                             int64_t npiece, uint8_t *d_csum, void *stream);

/* Host buffers (what a Go dataReader.Read adapter calls).  Sources as for
 * jfs_compact_batch: src[i].src/src_len the stored object, src[i].dst_cap its
 * block size, src[i].dst ignored.  out[j].dst/dst_cap receives the raw
 * gathered bytes of read j; out_n[j] = their count, or JFS_ERR_CORRUPT when a
 * source feeding read j failed or is shorter than a segment needs.  Nothing is
 * written to out[j].dst for a failed read; errors are per read (the
 * all-or-nothing choice of reader.go:875-877 stays with the caller).
 * src_n[i] = exactly what jfs_decompress_batch returns for that object, unless
 * its checksum fails: src_crc[i] (src_crc may be NULL) is -1 for "no checksum"
 * (verifyChecksum with ""), else the expected CRC-32C of the whole stored
 * object in its low 32 bits.  It is computed on the device in front of
 * everything else; on a mismatch src_n[i] = JFS_ERR_CHECKSUM, which wins over
 * every other error of that source, and the source counts as failed.
 * crc_got[i] (crc_got may be NULL) = the computed CRC of every source that had
 * an expected value, 0 otherwise.
 * Checked on the host first (JFS_ERR_INVALID): everything jfs_compact_batch
 * rejects, a read whose total exceeds out[j].dst_cap, a src_crc[i] outside
 * -1 .. 0xFFFFFFFF; then JFS_ERR_NO_DEVICE.  One device per call, the scratch
 * failure policy (every src_n[i] / out_n[j] of the call JFS_ERR_NO_MEMORY or
 * JFS_ERR_HIP, return JFS_OK) and "current device unchanged on return" are
 * jfs_compact_batch's.  jfs_stats counts the sources under (algo, decompress),
 * bytes_out being the decoded size; nothing is counted under compress. */
int64_t jfs_read_batch(int algo, int nsrc, const jfs_iov *src, const int64_t *src_crc /* may be NULL */, int nout,
                       const jfs_iov *out, const int32_t *seg_first /* nout+1 */, const jfs_compact_seg *seg,
                       int64_t *src_n, int64_t *out_n, uint32_t *crc_got /* nsrc, may be NULL */,
                       uint32_t device_mask);

/* jfs_read_batch for a volume with object encryption: src[i] is the whole
 * envelope and src_keys[i] its unwrapped data key, as for
 * jfs_compact_seal_batch.  src_n[i] = exactly what jfs_open_decompress_batch
 * returns, unless the checksum fails; the checksum covers the whole envelope
 * and wins over JFS_ERR_CORRUPT and JFS_ERR_AUTH too.  Also JFS_ERR_INVALID: an
 * unknown cipher, a NULL src_keys with nsrc > 0, a NULL src_keys[i]. */
int64_t jfs_read_open_batch(int algo, int cipher, int nsrc, const jfs_iov *src, const uint8_t *const *src_keys,
                            const int64_t *src_crc /* may be NULL */, int nout, const jfs_iov *out,
                            const int32_t *seg_first /* nout+1 */, const jfs_compact_seg *seg, int64_t *src_n,
                            int64_t *out_n, uint32_t *crc_got /* nsrc, may be NULL */, uint32_t device_mask);

/* jfs_read_batch / jfs_read_open_batch plus, for every read j with
 * csum[j] != NULL, the disk-cache checksum of its gathered bytes (holes
 * included) -- what cachedStore.load hands to the block cache with a decoded
 * block (cached_store.go:819-821, disk_cache.go:536-537): the big-endian
 * CRC-32C of every 32 KiB piece, ((n-1)/32768+1)*4 bytes for n = out_n[j]
 * (4 zero bytes for n = 0), computed on the device behind the gather and
 * returned in the same copy as the reads.  For a read that is one whole block
 * (src_off = 0, len = the block's size) these are the bytes
 * jfs_decompress_batch_csum writes for that block, so one call serves the
 * reads and fills the cache.  csum has nout entries; csum[j] must hold that
 * many bytes for the read's planned total; nothing is written for a failed
 * read (out_n[j] < 0) or a NULL entry.  A NULL csum with nout > 0 is
 * JFS_ERR_INVALID.  Everything else -- src_n, out_n, crc_got, the bytes, the
 * precedence of verdicts, the decode mode, jfs_stats, the device choice and the
 * scratch failure policy -- is the call's without _csum. */
int64_t jfs_read_batch_csum(int algo, int nsrc, const jfs_iov *src, const int64_t *src_crc /* may be NULL */, int nout,
                            const jfs_iov *out, const int32_t *seg_first /* nout+1 */, const jfs_compact_seg *seg,
                            int64_t *src_n, int64_t *out_n, uint32_t *crc_got /* nsrc, may be NULL */,
                            uint8_t *const *csum /* nout */, uint32_t device_mask);
int64_t jfs_read_open_batch_csum(int algo, int cipher, int nsrc, const jfs_iov *src, const uint8_t *const *src_keys,
                                 const int64_t *src_crc /* may be NULL */, int nout, const jfs_iov *out,
                                 const int32_t *seg_first /* nout+1 */, const jfs_compact_seg *seg, int64_t *src_n,
                                 int64_t *out_n, uint32_t *crc_got /* nsrc, may be NULL */,
                                 uint8_t *const *csum /* nout */, uint32_t device_mask);

/* Decode mode of jfs_read_batch and jfs_read_open_batch.  JFS_READ_DECODE_FULL
 * (default) decodes every source whole: the calls are what they were before
 * the mode existed, byte for byte and result for result.
 * JFS_READ_DECODE_PREFIX stops each LZ4 decode at the last byte a read needs:
 * per source, need = max(src_off + len) over the segments that reference it
 * (0 for a source nothing references), clamped to its dst_cap, is passed to
 * the prefix decoders above as `want`.  Then, for LZ4, src_n[i] = min(size,
 * need), or the error as the prefix decoders define it (a fault behind `need`
 * may go unseen); the checksum, open and host-answered verdicts keep their
 * precedence, out_n and the output bytes are those of full mode for every read
 * whose sources are well-formed, and a source too short for a segment still
 * fails that read (JFS_ERR_CORRUPT).  A call in which every source is needed to
 * its dst_cap takes the full decoders.  Zstd and "none" decode whole in these
 * two modes, with full mode's src_n.
 * JFS_READ_DECODE_PREFIX_ALL is JFS_READ_DECODE_PREFIX for LZ4 and also stops
 * each Zstd decode at the Zstd block a read ends in: the same `need` is the
 * `want` of jfs_zstd_decompress_prefix_device, whose contract gives src_n[i]
 * (min(size, need) for a well-formed source); everything else is as above.
 * "none" stays whole.  jfs_stats' bytes_out counts src_n.  The compaction calls
 * do not consult the mode.
 * The initial value is read once from JFS_READ_DECODE = "full" | "prefix" |
 * "prefix-all" (case-insensitive; anything else, or unset: full).
 * jfs_set_read_decode_mode returns the previous mode, or -1 for an unknown
 * value (which changes nothing); it is atomic and applies to calls that start
 * afterwards. */
#define JFS_READ_DECODE_FULL 0
#define JFS_READ_DECODE_PREFIX 1
#define JFS_READ_DECODE_PREFIX_ALL 2 /* JFS_READ_DECODE=prefix-all */
int jfs_read_decode_mode(void);
int jfs_set_read_decode_mode(int mode);
/* jfs_set_read_decode_mode knows the two modes it was introduced with and keeps
 * answering -1 for any other value, JFS_READ_DECODE_PREFIX_ALL included.
 * jfs_set_read_decode_mode_ext is the same call for all three modes. */
int jfs_set_read_decode_mode_ext(int mode);

/* Seek switch of the same calls, beside the decode mode.  JFS_READ_SEEK_OFF
 * (default): nothing changes.  JFS_READ_SEEK_ON: in every decode mode each Zstd
 * source is decoded by jfs_zstd_decompress_range_device for [from, need), need
 * as above and from = the smallest src_off of the segments that reference the
 * source (both 0 for a source nothing references), so a read from the middle of
 * a seekable object pays for the frames it touches and any other object is
 * prefix-decoded to `need`.  src_n[i] = min(size, need) for a well-formed
 * source; out_n, the gathered bytes, the checksums and the precedence of
 * verdicts are those of the switch being off for every read whose sources are
 * well-formed.  LZ4 and "none" are untouched; the compaction calls do not
 * consult the switch.  The initial value is read once from JFS_READ_SEEK =
 * "off" | "on" | "sparse" (case-insensitive; anything else, or unset: off).
 * jfs_set_read_seek_mode returns the previous value, or -1 for an unknown one
 * (which changes nothing); it is atomic and applies to calls that start
 * afterwards. */
#define JFS_READ_SEEK_OFF 0
#define JFS_READ_SEEK_ON 1
int jfs_read_seek_mode(void);
int jfs_set_read_seek_mode(int mode);
/* JFS_READ_SEEK_SPARSE (JFS_READ_SEEK = "sparse"): as JFS_READ_SEEK_ON, but each
 * Zstd source is decoded by jfs_zstd_decompress_ranges_device for the list of
 * ranges [src_off, src_off + len) of the segments that reference it (clamped
 * to its capacity, sorted, the ones that overlap or touch merged; a source
 * nothing references has none), so two reads at the two ends of a seekable
 * object pay for two frames, and an object written with JFS_ZSTD_SEEK_CSUM=on
 * is range-decoded too, every decoded frame checked against its table
 * checksum: a mismatch gives src_n[i] = JFS_ERR_CHECKSUM, behind the object
 * CRC-32C verdict and the open's, and the reads that use the source fail with
 * JFS_ERR_CORRUPT like those of any failed source.  src_n, out_n, the gathered
 * bytes, crc_got, the disk-cache checksums and the jfs_stats accounting are
 * those of JFS_READ_SEEK_ON for well-formed sources; a fault in a frame no
 * read touches goes unseen unless the object CRC-32C is checked.
 * jfs_set_read_seek_mode knows the two values it was introduced with and keeps
 * answering -1 for any other, JFS_READ_SEEK_SPARSE included;
 * jfs_set_read_seek_mode_ext is the same call for all three. */
#define JFS_READ_SEEK_SPARSE 2
int jfs_set_read_seek_mode_ext(int mode);

/* LZ4 chase switch of the same calls (and their _csum forms), beside the decode
 * mode.  JFS_READ_LZ4_CHASE_OFF (default): nothing changes.
 * JFS_READ_LZ4_CHASE_ON: in every decode mode, an LZ4 source whose reads ask
 * for at least one and at most JFS_LZ4_CHASE_MAX bytes in all (the list of
 * ranges [src_off, src_off + len) of the segments that reference it, clamped
 * to its capacity, the ones that overlap or touch merged) is decoded by
 * jfs_lz4_decompress_ranges_device for that list; every other source is decoded
 * as with the switch off.  src_n[i] of such a source is min(size, need), as in
 * JFS_READ_DECODE_PREFIX; out_n, the gathered bytes, crc_got, the disk-cache
 * checksums and the precedence of verdicts are those of the switch being off
 * for every read whose sources are well-formed (the gather and the checksum
 * kernels read only bytes inside the reads).  A fault in a sequence no read
 * visits goes unseen unless the object CRC-32C is checked.  The compaction
 * calls do not consult the switch.
 * JFS_LZ4_CHASE_MAX (environment, bytes, read once; default 0) is the largest
 * request per source that takes the chase.  The default comes from the
 * measurement in DESIGN 12h: on 4 MiB text blocks the chase was slower than the
 * prefix decode at every read size measured, so nothing is chased until a
 * deployment sets a threshold of its own.
 * The initial value is read once from JFS_READ_LZ4_CHASE = "off" | "on"
 * (case-insensitive; anything else, or unset: off).
 * jfs_set_read_lz4_chase_mode returns the previous value, or -1 for an unknown
 * one (which changes nothing); it is atomic and applies to calls that start
 * afterwards. */
#define JFS_READ_LZ4_CHASE_OFF 0
#define JFS_READ_LZ4_CHASE_ON 1
int jfs_read_lz4_chase_mode(void);
int jfs_set_read_lz4_chase_mode(int mode);
/* The threshold in force, and a new one (0 .. 2^31 - 1 bytes; returns the
 * previous value, or -1 and no change for anything else).  Atomic; applies to
 * calls that start afterwards. */
int64_t jfs_lz4_chase_max(void);
int64_t jfs_set_lz4_chase_max(int64_t bytes);

/* LZ4 window switch of the same calls (and their _csum forms), beside the
 * decode mode and the chase switch.  JFS_READ_LZ4_WINDOW_OFF (default): nothing
 * changes.  JFS_READ_LZ4_WINDOW_ON: in every decode mode, the LZ4 sources that
 * the chase does not take and that would take the small-batch decoder (at most
 * JFS_LZ4_SPLIT_MAX of them) are decoded by
 * jfs_lz4_decompress_window_device_small for [from, need): the first and the
 * last byte a segment asks of the source, clamped to its capacity.  src_n[i]
 * of such a source is min(size, need), as in JFS_READ_DECODE_PREFIX; out_n, the
 * gathered bytes, crc_got, the disk-cache checksums and the precedence of
 * verdicts are those of the switch being off for every read whose sources are
 * well-formed.  A call in which every such source is read from its first 64 KiB
 * (from < 65536), and a call with more such sources than the small-batch
 * decoder takes, is queued exactly as with the switch off.  A fault in a
 * sequence in front of the chunk a source's reads start in goes unseen unless
 * the object CRC-32C is checked.  The compaction calls do not consult the
 * switch.
 * The initial value is read once from JFS_READ_LZ4_WINDOW = "off" | "on"
 * (case-insensitive; anything else, or unset: off).
 * jfs_set_read_lz4_window_mode returns the previous value, or -1 for an unknown
 * one (which changes nothing); it is atomic and applies to calls that start
 * afterwards. */
#define JFS_READ_LZ4_WINDOW_OFF 0
#define JFS_READ_LZ4_WINDOW_ON 1
int jfs_read_lz4_window_mode(void);
int jfs_set_read_lz4_window_mode(int mode);

/* ---- Runtime / utilities ------------------------------------------------- */

/* Number of usable gfx950 devices (0 when none; never an error).  Only the
 * devices JFS_GPU_DEVICES selects count (a comma list of ordinals such as
 * "0,2,5", a mask such as "0x25", or "all" = the default). */
int jfs_device_count(void);

/* Codec selector, read once from JFS_GPU_CODEC:
 *   "off"   -> JFS_MODE_OFF: the library reports no device; every GPU entry
 *              point returns JFS_ERR_NO_DEVICE and the Go adapter keeps the
 *              CPU codecs of compress.go (NewCompressor unchanged);
 *   "auto"  -> JFS_MODE_AUTO (default, also for unknown values): the adapter
 *              uses this library when jfs_device_count() > 0, else the CPU
 *              codecs;
 *   "force" -> JFS_MODE_FORCE: the adapter must use this library and fail at
 *              start-up when jfs_device_count() == 0.
 * The library itself never runs a CPU codec in any mode. */
#define JFS_MODE_OFF 0
#define JFS_MODE_AUTO 1
#define JFS_MODE_FORCE 2
int jfs_gpu_mode(void);

/* LZ4 parse of the HOST-buffer compress calls (jfs_compress and its
 * coalescer, jfs_compress_batch / _crc / _mixed, jfs_compress_seal_batch, the
 * encode step of jfs_compact_batch / jfs_compact_seal_batch): JFS_LZ4_PARSE_EXACT (default) writes
 * LZ4_compress_default's bytes, JFS_LZ4_PARSE_FAST the blocks of
 * jfs_lz4_compress_fast_device -- ordinary LZ4 blocks to every reader, and
 * per-block results keep their meaning (JFS_ERR_COMPRESS_FAIL when a block
 * does not fit).  The device-resident entry points above do what their
 * comments say in either mode.  The initial value is read once from
 * JFS_LZ4_PARSE = "exact" | "fast" (case-insensitive, like JFS_GPU_CODEC;
 * anything else, or unset: exact).  jfs_set_lz4_parse_mode returns the
 * previous mode, or -1 for an unknown value (which changes nothing); it is
 * atomic and applies to calls that start afterwards. */
#define JFS_LZ4_PARSE_EXACT 0
#define JFS_LZ4_PARSE_FAST 1
int jfs_lz4_parse_mode(void);
int jfs_set_lz4_parse_mode(int mode);

/* Zstd parse of the same HOST-buffer compress calls: JFS_ZSTD_PARSE_EXACT
 * (default) writes ZSTD_compress(level 1)'s bytes, JFS_ZSTD_PARSE_FAST the
 * frames of jfs_zstd_compress_fast_device -- ordinary Zstd frames to every
 * reader, and per-block results keep their meaning.  The device-resident entry
 * points above do what their comments say in either mode.  The initial value
 * is read once from JFS_ZSTD_PARSE = "exact" | "fast" (case-insensitive;
 * anything else, or unset: exact).  jfs_set_zstd_parse_mode returns the
 * previous mode, or -1 for an unknown value (which changes nothing); it is
 * atomic and applies to calls that start afterwards. */
#define JFS_ZSTD_PARSE_EXACT 0
#define JFS_ZSTD_PARSE_FAST 1
#define JFS_ZSTD_PARSE_SEEKABLE 2 /* JFS_ZSTD_PARSE=seekable */
int jfs_zstd_parse_mode(void);
int jfs_set_zstd_parse_mode(int mode);
/* JFS_ZSTD_PARSE_SEEKABLE makes the same calls write the objects of
 * jfs_zstd_compress_seekable_device: the fast parse, one frame per 128 KiB
 * block and a seek table.  jfs_set_zstd_parse_mode knows the two modes it was
 * introduced with and keeps answering -1 for any other value;
 * jfs_set_zstd_parse_mode_ext is the same call for all three modes. */
int jfs_set_zstd_parse_mode_ext(int mode);
/* Checksum switch of the seekable mode.  JFS_ZSTD_SEEK_CSUM_OFF (default):
 * nothing changes.  JFS_ZSTD_SEEK_CSUM_ON: while the Zstd parse mode is
 * JFS_ZSTD_PARSE_SEEKABLE, every host-buffer compress call (jfs_compress, the
 * batch calls and their _crc and _mixed forms, jfs_compress_seal_batch, the
 * encode step of the compaction calls) writes the objects of
 * jfs_zstd_compress_seekable_csum_device; in any other parse mode the switch
 * has no effect.  The initial value is read once from JFS_ZSTD_SEEK_CSUM =
 * "off" | "on" (case-insensitive; anything else, or unset: off).
 * jfs_set_zstd_seek_csum_mode returns the previous value, or -1 for an unknown
 * one (which changes nothing); it is atomic and applies to calls that start
 * afterwards. */
#define JFS_ZSTD_SEEK_CSUM_OFF 0
#define JFS_ZSTD_SEEK_CSUM_ON 1
int jfs_zstd_seek_csum_mode(void);
int jfs_set_zstd_seek_csum_mode(int mode);

/* Per-codec counters (the data behind cachedStore's object_request_data_bytes
 * and block-size metrics, cached_store.go:931-974).  Index algo * 2 + dir,
 * dir 0 = compress, 1 = decompress; 6 entries.  Host-path calls (one-call and
 * batch) count blocks, bytes and errors per block; device-resident launches
 * count only calls and blocks (their results stay in HBM). */
typedef struct jfs_op_stats {
    uint64_t calls;     /* API calls */
    uint64_t blocks;    /* blocks submitted */
    uint64_t bytes_in;  /* input bytes of host-path blocks that succeeded */
    uint64_t bytes_out; /* output bytes of host-path blocks that succeeded */
    uint64_t errors;    /* host-path blocks that returned an error code */
    uint64_t nanos;     /* wall time spent inside host-path calls */
    uint64_t batches;   /* device batches the host path ran (coalesced one-call
                           batches, or per-device parts of a jfs_*_batch call) */
} jfs_op_stats;
#define JFS_STATS_N 6
/* Copy min(n, JFS_STATS_N) entries to out; returns JFS_STATS_N. */
int jfs_stats(jfs_op_stats *out, int n);
void jfs_stats_reset(void);  /* also zeroes the per-device counters below */
/* Per-device host-path counters (where the round-robin deal put
 * the blocks): one entry per usable device, in jfs_device_count() order. */
typedef struct jfs_device_stat {
    int32_t device;   /* HIP device ordinal */
    int32_t pad_;
    uint64_t batches; /* device batches run */
    uint64_t blocks;  /* blocks in them */
} jfs_device_stat;
/* Copy min(n, devices) entries to out; returns the number of devices. */
int jfs_device_stats(jfs_device_stat *out, int n);
/* Free the batch path's pinned host + HBM staging now (it is also released
 * after JFS_STAGING_IDLE_MS, default 15000, of no batch activity). */
void jfs_release_staging(void);
/* Library version string. */
const char *jfs_version(void);

/* Synthetic benchmark input: block i of class cls
 * ('T','Z','R') with seed base+i, each `block_bytes` long, written
 * back-to-back at d_dst (device pointer) on `stream`.  Host twin below. */
int64_t jfs_gen_blocks_device(uint8_t *d_dst, int nblk, int64_t block_bytes, char cls, uint64_t seed_base,
                              void *stream);
void jfs_gen_block_host(uint8_t *dst, int64_t n, char cls, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* JFS_GPUCODEC_H */
