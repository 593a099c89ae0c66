// Internal declarations shared by the HIP translation units of libjfsgpu.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jfs_gpucodec.h"

// Explicit global (address space 1) pointer types: generic pointers compile to
// flat_* instructions, which count on both vmcnt and lgkmcnt and force the
// compiler to drain LDS traffic around every HBM access.
// (The host compilation pass of the same source sees plain types.)
#if defined(__HIP_DEVICE_COMPILE__)
#define JFS_GLOBAL __attribute__((address_space(1)))
#else
#define JFS_GLOBAL
#endif
typedef JFS_GLOBAL uint8_t g_u8;
typedef JFS_GLOBAL const uint8_t gc_u8;
typedef JFS_GLOBAL uint32_t g_u32;
typedef JFS_GLOBAL const uint32_t gc_u32;
typedef JFS_GLOBAL uint4 g_u4;
typedef JFS_GLOBAL const uint4 gc_u4;
typedef JFS_GLOBAL const uint2 gc_u2;
typedef JFS_GLOBAL const jfs_dev_block gc_blk;

extern "C" {
int jfs_launch_lz4_decode(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, hipStream_t stream);
int jfs_launch_lz4_encode(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, hipStream_t stream);
// segment-parallel LZ4 encode (same bytes as jfs_launch_lz4_encode); lens = the
// blocks' src_len on the host; scratch of jfs_lz4_eseg_scratch_bytes
int64_t jfs_lz4_eseg_scratch_bytes(int nblk, const int32_t *lens);
int jfs_launch_lz4_encode_seg(const jfs_dev_block *d_blocks, int nblk, const int32_t *lens, int32_t *d_ret,
                              void *scratch, int64_t scratch_cap, hipStream_t stream);
// fast LZ4 encode (lz4_fast.hip): independent 64 KiB chunks, not liblz4's bytes;
// lens = the blocks' src_len on the host; scratch of jfs_lz4_fast_scratch_bytes
int64_t jfs_lz4_fast_scratch_bytes(int nblk, const int32_t *lens);
int jfs_launch_lz4_fast(const jfs_dev_block *d_blocks, int nblk, const int32_t *lens, int32_t *d_ret, void *scratch,
                        int64_t scratch_cap, hipStream_t stream);
// The fast encode with LIFTED chunks (lz4_lift.h): d_lift[g] names, per output chunk in the flat
// order of the launch groups, the source chunk its records are read back from (src < 0: parse).  The sources'
// stored streams are indexed once (lz4_lift.hip), then every group runs plan, lift, parse (which skips the
// lifted chunks), stitch and emit.  S: the sources; d_lifted (may be null): chunks lifted per output block.
struct jfs_lz4_lift_srcs {
    const jfs_dev_block *d_src;  // [nsrc] src / src_len: the stored stream; dst_cap: its decode capacity
    const int32_t *d_src_n;      // [nsrc] what each source decoded to (negative: it failed)
    int nsrc;
    const int32_t *d_sel;        // [nsel] the sources to index (device), or null: all of them, nsel = nsrc
    int nsel;
    const int32_t *sel_len, *sel_cap;  // [nsel] the host's copies of their descriptors' src_len and dst_cap
};
int64_t jfs_lz4_fast_lift_scratch_bytes(int nblk, const int32_t *lens, int nsrc, int nsel, const int32_t *sel_len);
int jfs_launch_lz4_fast_lift(const jfs_dev_block *d_blocks, int nblk, const int32_t *lens, const jfs_lz4_lift *d_lift,
                             const jfs_lz4_lift_srcs *S, int32_t *d_ret, int32_t *d_lifted, void *scratch,
                             int64_t scratch_cap, hipStream_t stream);
// its parts in lz4_lift.hip: the index areas' bytes, the index launch (once per call, into d_scratch) and the
// lift of one launch group (grp: where lz4_fast.hip keeps the group's parse results)
struct jfs_lz4_lift_group {
    int nblk, ncand;  // ncand: the chunks the host counted for the group, which d_lift holds
    const int32_t *cfirst;
    int32_t *nrec, *tail, *lit0, *body, *lifted;
    uint2 *recs;
};
int64_t jfs_lz4_lift_index_bytes(int nsrc, int nsel, const int32_t *sel_len);
int jfs_launch_lz4_lift_index(const jfs_lz4_lift_srcs *S, void *d_scratch, hipStream_t stream);
int jfs_launch_lz4_lift(const jfs_dev_block *d_blocks, const jfs_lz4_lift_group *grp, int chunks,
                        const jfs_lz4_lift *d_lift, const jfs_lz4_lift_srcs *S, void *d_scratch, int32_t *d_lifted,
                        hipStream_t stream);
// test hook (include/jfs_gpucodec_lz4_fast_test.h): chunks per launch group, 0 = the default
int jfs_test_set_lz4_fast_group_chunks(int chunks);
// parse_mode: JFS_ZSTD_PARSE_EXACT (libzstd's bytes), JFS_ZSTD_PARSE_FAST (zstd_fast.hip: valid frames, not libzstd's
// bytes) or JFS_ZSTD_PARSE_SEEKABLE (the fast parse, one frame per 128 KiB block and a seek table)
int jfs_launch_zstd_encode(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, hipStream_t stream,
                           int parse_mode);
int jfs_launch_zstd_decode(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, uint8_t *d_scratch,
                           hipStream_t stream);
// d_split: the small-batch path's scratch (jfs_zstd_split_bytes), or null;
// tot: jfs_zstd_plan_host's six totals
int jfs_launch_zstd_decode_planned(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, void *d_info,
                                   uint8_t *d_lit, uint16_t *d_tabs, void *d_items, void *d_split,
                                   const uint64_t *tot, hipStream_t stream);
size_t jfs_zstd_info_bytes(void);
// totals[6]: items, literal bytes, table cells, blocks, origin entries, largest dst_cap
void jfs_zstd_plan_host(const uint8_t *const *srcs, const int32_t *lens, const int32_t *caps, int nblk, void *info_out,
                        uint64_t *totals);
// prefix decode (zstd_decode_prefix.hip): input b stops at the block that
// reaches d_want[b] output bytes (<= 0: in front of the first block, above
// dst_cap: dst_cap); jfs_launch_zstd_decode's scratch and stream behaviour
int jfs_launch_zstd_decode_prefix(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, const int32_t *d_want,
                                  hipStream_t stream);
// range decode (zstd_seek.hip): input b is decoded for its output bytes
// [d_lo[b], d_hi[b]) through its seek table, frame by frame, or as a prefix
// decode with want = d_hi[b] when it has none; waits once on the host for the
// number of selected frames, then jfs_launch_zstd_decode_prefix's behaviour
int jfs_launch_zstd_decode_range(const jfs_dev_block *d_blocks, const int32_t *d_lo, const int32_t *d_hi, int nblk,
                                 int32_t *d_ret, hipStream_t stream);
// XXH64, seed 0, of d_blocks[i].src[0, src_len) (xxh64.hip); d_ret may be null
int jfs_launch_xxh64(const jfs_dev_block *d_blocks, int nblk, uint64_t *d_hash, int32_t *d_ret, hipStream_t stream);
// the seekable encode with per-frame checksums in its table (zstd_seek_csum.hip)
int jfs_launch_zstd_encode_seek_csum(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, hipStream_t stream);
// fragment decode (zstd_seek.hip): the range decode from a stand-alone table and
// a fragment of the object's frames, every decoded frame checked against its
// table checksum where the table has them
int jfs_launch_zstd_decode_frames(const jfs_seek_frag *d_frags, const int32_t *d_lo, const int32_t *d_hi, int nblk,
                                  int32_t *d_ret, hipStream_t stream);
// ranges decode (zstd_seek.hip): a whole object decoded for a list of ranges, exactly the frames some range
// touches, through a table of either layout; input i owns d_rng[d_rng_first[i] .. d_rng_first[i + 1])
int jfs_launch_zstd_decode_ranges(const jfs_dev_block *d_blocks, const int32_t *d_rng_first, const jfs_range *d_rng,
                                  int nblk, int32_t *d_ret, hipStream_t stream);
// spliced objects (zstd_splice.hip; jfs_zstd_splice_device's contract): the scan (verdicts into d_ret, every
// frame's place into d_off, nframes words of scratch, and the seek tables) and the copy of the frames
int jfs_launch_zstd_splice(const jfs_splice_out *d_out, int nout, const jfs_splice_frame *d_frames, int nframes,
                           const int32_t *d_unit_len, const uint64_t *d_unit_hash, uint32_t *d_off, int32_t *d_ret,
                           hipStream_t stream);
// seek tables out of device-resident objects (zstd_seek_tables.hip; jfs_zstd_seek_tables_device's contract)
int jfs_launch_zstd_seek_tables(const jfs_dev_block *d_blocks, const int32_t *d_len, int nblk, const int32_t *d_slot_first,
                                uint8_t *d_tables, int32_t *d_table_len, hipStream_t stream);
// jfs_zstd_load_range_batch: the bytes src[0, len) of a decoded block go to dst
// where the fragment decode of that read answered `expect`
struct jfs_range_pack {
    const uint8_t *src;
    uint8_t *dst;
    int32_t len, expect;
};
int jfs_launch_range_pack(const jfs_range_pack *d_pack, int n, int32_t max_len, const int32_t *d_ret,
                          hipStream_t stream);
// jfs_zstd_plan_host of such a decode; totals[5] is the largest clamped want
void jfs_zstd_plan_host_prefix(const uint8_t *const *srcs, const int32_t *lens, const int32_t *caps,
                               const int32_t *wants, int nblk, void *info_out, uint64_t *totals);
int jfs_zstd_split_ok(int nblk, const uint64_t *tot);  // the small-batch path takes this batch
int64_t jfs_zstd_split_bytes(int nblk, const uint64_t *tot);
int jfs_launch_crc32c(const jfs_dev_block *d_blocks, int nblk, int32_t seg_bytes, uint32_t *d_crc, int32_t *d_ret,
                      hipStream_t stream);
int jfs_launch_crc32c_lens(const jfs_dev_block *d_blocks, int nblk, const int32_t *d_lens, const uint32_t *d_seeds,
                           uint32_t *d_crc, hipStream_t stream);
// per-seg_bytes checksums (jfs_crc32c_device's dst layout) of device blocks
// whose length the previous kernel wrote (lens; < 0: it failed, nothing written)
int jfs_launch_crc32c_segs_lens(const jfs_dev_block *d_blocks, int nblk, int32_t seg_bytes, const int32_t *d_lens,
                                hipStream_t stream);
int jfs_launch_aes256gcm(const jfs_aead_block *d_blocks, int nblk, int mode, int32_t *d_ret, const int32_t *d_lens,
                         hipStream_t stream);
int jfs_launch_aead(int cipher, const jfs_aead_block *d_blocks, int nblk, int mode, int32_t *d_ret,
                    const int32_t *d_lens, hipStream_t stream);
int jfs_launch_lz4_decode_lens(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, const int32_t *d_lens,
                               hipStream_t stream);
int jfs_launch_lz4_decode_todo(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, const int32_t *d_todo,
                               hipStream_t stream);
// the decode of block b stops at d_want[b] output bytes (lz4_decode_prefix.hip;
// <= 0: the result is 0, above dst_cap: dst_cap); d_todo may be null
int jfs_launch_lz4_decode_prefix(const jfs_dev_block *d_blocks, int nblk, int32_t *d_ret, const int32_t *d_want,
                                 const int32_t *d_todo, hipStream_t stream);
// small-batch LZ4 decode (lz4_split.hip): compressed bytes per segment (one
// lane each), scratch bytes for these blocks, and
// the launch (nseg_all = sum of ceil(src_len / 256), max_cap = largest dst_cap,
// norg_all = sum of dst_cap rounded up to 4: the host sizes the scratch with them)
#define JFS_LZ4_SPLIT_SEG 256
int64_t jfs_lz4_split_scratch_bytes(int nb, const int32_t *src_len, const int32_t *cap);
int jfs_launch_lz4_split(const jfs_dev_block *d_desc, int nb, int32_t *d_ret, void *d_scratch, int64_t nseg_all,
                         int64_t max_cap, int64_t norg_all, hipStream_t st);
// the same with per-block d_want (as above); max_want: a host-side upper bound
// of them, at most max_cap (max_cap where the host does not know them)
int jfs_launch_lz4_split_prefix(const jfs_dev_block *d_desc, int nb, int32_t *d_ret, const int32_t *d_want,
                                void *d_scratch, int64_t nseg_all, int64_t max_cap, int64_t norg_all, int64_t max_want,
                                hipStream_t st);
// the window decode (lz4_window.h): block b for its output bytes [d_lo[b], d_hi[b]), from the 64 KiB chunk
// boundary below d_lo[b] where the probe proves that enough, else as the prefix launch with want = d_hi[b];
// max_want: a host-side upper bound of the d_hi, as above
int jfs_launch_lz4_split_window(const jfs_dev_block *d_desc, int nb, int32_t *d_ret, const int32_t *d_lo,
                                const int32_t *d_hi, void *d_scratch, int64_t nseg_all, int64_t max_cap,
                                int64_t norg_all, int64_t max_want, hipStream_t st);
// ranges decode by origin chase (lz4_chase.hip): block i is decoded for the ranges d_rng[d_rng_first[i] ..
// d_rng_first[i + 1]) of its output.  src_len / cap: the host's copies of the descriptors' sizes, which size the
// scratch (jfs_lz4_chase_scratch_bytes) and the index grids; max_quads: a host-side upper bound of the 4-byte
// groups the lists touch, or < 0 where the host does not know the lists (it only sizes the grid)
int64_t jfs_lz4_chase_scratch_bytes(int nb, const int32_t *src_len);
int jfs_launch_lz4_chase(const jfs_dev_block *d_desc, const int32_t *src_len, const int32_t *cap, const int32_t *d_rf,
                         const jfs_range *d_rng, int nb, int32_t *d_ret, void *d_scratch, int64_t max_quads,
                         hipStream_t st);
// ret value of a fused chain's second step when its first step failed
#define JFS_CHAIN_FAILED (-2147483647 - 1)
// compaction gather (compact.hip): verdicts into d_ret and the copy; merge != 0:
// only the verdicts, written over d_ret[j] where negative (after an encoder)
int jfs_launch_gather(const jfs_dev_block *d_src, const int32_t *d_src_n, int nsrc, const jfs_compact_out *d_out,
                      int nout, const jfs_compact_seg *d_seg, int32_t max_dst_cap, int32_t *d_ret, int merge,
                      hipStream_t stream);
// sealed compaction: d_src_n[i] = d_open_ret[i] where the AEAD open of source i
// failed (d_open_ret[i] < 0), so the gather counts it as a failed source
int jfs_launch_chain_merge(const int32_t *d_open_ret, int nsrc, int32_t *d_src_n, hipStream_t stream);
// spliced compaction: d_out[k] = d_a[d_idx[k]] for d_idx[k] >= 0, else d_b[~d_idx[k]] (the payload length of
// output k: its whole encode unit's result, or the splice scan's verdict)
int jfs_launch_chain_pick(const int32_t *d_idx, int n, const int32_t *d_a, const int32_t *d_b, int32_t *d_out,
                          hipStream_t stream);
// src_n value of a read source whose CRC-32C did not match (compact.hip, verify_gate_kernel)
#define JFS_CHECKSUM_FAILED (-2147483647)
// the read path's gather (compact.hip): verdicts and the copy on a one-dimensional
// grid over d_tile_first, the running sum of jfs_gather_tiles(dst_cap) (nout + 1
// entries; ntiles = its last entry on the host).  jfs_launch_gather_prefix
// builds it on the device from d_out.
int64_t jfs_gather_tiles(int64_t cap);
int jfs_launch_gather_prefix(const jfs_compact_out *d_out, int nout, int32_t *d_tile_first, hipStream_t stream);
int jfs_launch_gather_flat(const jfs_dev_block *d_src, const int32_t *d_src_n, int nsrc, const jfs_compact_out *d_out,
                           int nout, const jfs_compact_seg *d_seg, int32_t *d_ret, const int32_t *d_tile_first,
                           int64_t ntiles, hipStream_t stream);
// read path: d_crc_got[i] = d_crc[i] where d_lens[i] > 0 (an expected CRC exists) else 0;
// a mismatch with d_expect[i] writes JFS_CHECKSUM_FAILED over d_src_n[i] (i < ndec)
int jfs_launch_verify_gate(const uint32_t *d_crc, const int32_t *d_lens, const uint32_t *d_expect, int n, int ndec,
                           int32_t *d_src_n, uint32_t *d_crc_got, hipStream_t stream);
// read path: the disk-cache checksums of the gathered reads (crc32c.hip,
// read_csum_flat_kernel) on a one-dimensional grid over d_piece_first, the
// running sum of the reads' 32 KiB piece counts (nout + 1 entries; npiece = its
// last entry on the host); piece p's big-endian CRC-32C goes to d_csum[p].
// Nothing is written for a read whose verdict d_ret[j] is not d_out[j].dst_cap.
int jfs_launch_read_csum_flat(const jfs_compact_out *d_out, int nout, const int32_t *d_ret,
                              const int32_t *d_piece_first, int64_t npiece, uint32_t *d_csum, hipStream_t stream);
int jfs_launch_gen(uint8_t *d_dst, int nblk, int64_t block_bytes, char cls, uint64_t seed_base,
                   const uint8_t *d_vocab, hipStream_t stream);
}
